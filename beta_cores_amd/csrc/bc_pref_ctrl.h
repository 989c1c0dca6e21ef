/* bc_pref_ctrl.h -- the pre-filter's control block: 256 bytes of device memory (bc_pref::ctrl, zeroed at creation) that the
 * sweep kernels, the rescoring stage and the host share.  Every access names its word here; the diagnostic seam copies the
 * block out whole as "ctrl" (include/beta_cores_prefdiag.h: 64 ints).  Plain C: tests/pref_ctrl_harness.c compiles it for
 * the host.  A field is an int (one word) or a u64 (two words, the first of them even). */
#ifndef BC_PREF_CTRL_H
#define BC_PREF_CTRL_H

#define BC_PCTL_BYTES 256
#define BC_PCTL_INTS 64

/* word index                  width  written by                                              read by */
#define BC_PCTL_OVERFLOWED 1  /* int: the rescoring stage (bc_rescore_block, bc_bb_pick): 1 if this launch overflowed; the "ctrl" copy only */
#define BC_PCTL_OVERFLOWS 3   /* int: the rescoring stage, +1 per overflow since creation; bc_pref_read_counters */
#define BC_PCTL_SWEEPS 4      /* u64: the rescoring stage, +1 per launch that was not skipped; bc_pref_read_counters */
#define BC_PCTL_RESCORED 6    /* u64: the rescoring stage, + the rows it rescored; bc_pref_read_counters */
#define BC_PCTL_RING_POS 9    /* int: bc_rescore_block, two-level form: where the seeds' ring is written next; bc_rescore_block */
#define BC_PCTL_L1_PASSED 12  /* u64: k_sweep_i4, + the rows its first level passed on; bc_pref_adapt, bc_pref_read_counters */
#define BC_PCTL_SPILL_N 14    /* int: k_sweep_i4, + the pairs it appends to the spill list; bc_rescore_block, which resets it */
#define BC_PCTL_BB_THETA 16   /* u64: k_sweep_i8_bb, the branch-and-bound form's shared bound (bc_pref::bb_theta); k_sweep_i8_bb */

#ifdef __cplusplus
#define BC_PCTL_CHECK(cond, msg) static_assert(cond, msg)
#else
#define BC_PCTL_CHECK(cond, msg) _Static_assert(cond, msg)
#endif
BC_PCTL_CHECK(BC_PCTL_INTS * 4 == BC_PCTL_BYTES, "the block is BC_PCTL_INTS 4-byte words");
BC_PCTL_CHECK(BC_PCTL_SWEEPS % 2 == 0 && BC_PCTL_RESCORED % 2 == 0 && BC_PCTL_L1_PASSED % 2 == 0 && BC_PCTL_BB_THETA % 2 == 0,
              "a u64 field starts on an even word");
/* in ascending order every field ends where the next begins or before it, and the last one inside the block */
BC_PCTL_CHECK(0 <= BC_PCTL_OVERFLOWED && BC_PCTL_OVERFLOWED + 1 <= BC_PCTL_OVERFLOWS && BC_PCTL_OVERFLOWS + 1 <= BC_PCTL_SWEEPS &&
                  BC_PCTL_SWEEPS + 2 <= BC_PCTL_RESCORED && BC_PCTL_RESCORED + 2 <= BC_PCTL_RING_POS &&
                  BC_PCTL_RING_POS + 1 <= BC_PCTL_L1_PASSED && BC_PCTL_L1_PASSED + 2 <= BC_PCTL_SPILL_N &&
                  BC_PCTL_SPILL_N + 1 <= BC_PCTL_BB_THETA && BC_PCTL_BB_THETA + 2 <= BC_PCTL_INTS,
              "the fields are disjoint and lie inside the block");

#endif /* BC_PREF_CTRL_H */
