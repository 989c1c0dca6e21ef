/*
 * beta_cores_prefdiag.h -- C ABI of a read-only diagnostic seam into the sweep's reduced-precision pre-filter (K3', K3''':
 * csrc/bc_prefilter.hip, bc_prefilter_i8.h, bc_prefilter_i4.h) in libbeta_cores.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers borrowed
 * for the call); kept in a header of its own so that the ABI of the existing headers stays as it is.
 * Bound in Python by beta_cores_amd/_native.py (_PREFDIAG_SIGNATURES).
 *
 * TEST AIDS.  The product calls none of the three entry points.  They exist so that the chain of inequalities behind "the
 * pre-filtered sweep selects what the fp64 sweep selects" can be checked link by link on the device
 * (tests/test_gpu_pref_bounds.py against the reference of tests/pref_cases.py): the mirrors the builders wrote, the digit
 * records of the sweep vectors, and the interval [L_i, U_i] the sweep kernels computed for EVERY row -- which the product never
 * stores.  Each call synchronises the context's stream; no sweep may be run while a step is in flight (between
 * bc_snnls_step_local and bc_snnls_step_finish; bc_snnls_prefdiag_copy only reads and may be called there).
 */
#ifndef BETA_CORES_PREFDIAG_H
#define BETA_CORES_PREFDIAG_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

/* indices into the array bc_snnls_prefdiag_info fills */
#define BC_PREFDIAG_PREC 0        /* storage precision of the mirror: 8 / 16 / 32 (0: the solver has no pre-filter; all else 0) */
#define BC_PREFDIAG_PTILE 1       /* rows per mirror tile: 256 (int8, fp32) or 512 (fp16) */
#define BC_PREFDIAG_PTILES 2      /* mirror tiles; every per-row buffer holds ptiles * ptile rows */
#define BC_PREFDIAG_SP 3          /* fp16: planes stored per tile (S padded); fp32: S */
#define BC_PREFDIAG_SP4 4         /* int8: k-groups of 4 stored per tile (also the length of the int8 digit record) */
#define BC_PREFDIAG_SP8 5         /* two-level: k-groups of 8 stored per tile (also the length of the 4-bit digit record) */
#define BC_PREFDIAG_G4 6          /* two-level: ceil(S / 4) */
#define BC_PREFDIAG_RB 7          /* two-level: bytes of a row-major int8 record */
#define BC_PREFDIAG_I4_U 8        /* two-level: loads per batch of the 4-bit sweep (its template instance) */
#define BC_PREFDIAG_GRID 9        /* blocks of the one-level sweep (four waves each; wave w of block b walks tiles 4b+w, +4 grid, ..) */
#define BC_PREFDIAG_GRID1 10      /* blocks of the two-level sweep */
#define BC_PREFDIAG_TWO 11        /* the two-level form exists ... */
#define BC_PREFDIAG_TWO_ACTIVE 12 /* ... and the host's watch has not put it aside */
#define BC_PREFDIAG_IFLUSH 13     /* BC_IFLUSH: tiles a wave of the int8 sweep parks before it writes their results out */
#define BC_PREFDIAG_BLK_NC 14     /* BC_BLK_NC: pairs a block list holds */
#define BC_PREFDIAG_NEXT_FORM 15  /* the form the next sweep takes: 1 one-level, 2 branch-and-bound, 3 two-level */
#define BC_PREFDIAG_QV 16         /* the step kernels keep the int8 digit record of the sweep vectors current */
#define BC_PREFDIAG_SEEDS 17      /* BC_I4_SEEDS and ... */
#define BC_PREFDIAG_HOT 18        /* ... BC_I4_HOT: "hot" holds SEEDS + HOT row numbers */
#define BC_PREFDIAG_SPILL_CAP 19  /* pairs the spill list holds */
#define BC_PREFDIAG_INFO_N 20

/* out[BC_PREFDIAG_INFO_N]: the shape of this solver's pre-filter, see above.  Launches nothing. */
int bc_snnls_prefdiag_info(const bc_snnls* h, int64_t* out);

/* Copies ONE named device buffer to the host, raw, in its device layout (csrc/bc_layout.h, the comments of the bc_pref struct).
 *   mirrors:                  "u32" "u16" "live" | "u8" "rowq" | "u4" "rowq4" "r8"
 *   the last sweep's outputs: "ub" "tile_u" "tile_cand" "tile_ncand" "blk_l" "blk_u" | "l2_blk_l" "l2_blk_u" "l2_blk_cand"
 *                             "l2_blk_nc" "spill" | "ctrl" (64 ints) "hot" (the two-level form's seeds) | "ctrl_swept" (64 ints:
 *                             the control block as the last two-level bc_snnls_prefdiag_sweep left it, before that call
 *                             restored "ctrl" -- word 14 is the number of pairs the sweep appended to "spill", which may
 *                             exceed BC_PREFDIAG_SPILL_CAP: pairs past the cap are not stored; no buffer before the first
 *                             such sweep).  Of a production sweep the same count stands in "ctrl" until the rescoring stage
 *                             clears it: this one call may be made between bc_snnls_step_local and bc_snnls_step_finish.
 *   the solver's current sweep vectors: "v" (GIGA: S pairs (cdir, y^) interleaved; else S doubles), "v_norm" and "post_div"
 *                             (one double each; v_norm is 1 for GIGA), "qv" / "qv4": the int8 / 4-bit digit records
 *                             (csrc/bc_i8_quant.h, bc_i4_quant.h: 4 sp4 / 4 sp8 ints of digits, then 8 header floats)
 * *bytes (if given) receives the buffer's size, also when the call is refused for a short cap_bytes.
 * BC_INVALID_ARGUMENT with a message: an unknown name, a buffer this solver's form does not have, cap_bytes too short. */
int bc_snnls_prefdiag_copy(const bc_snnls* h, const char* which, void* out, int64_t cap_bytes, int64_t* bytes);

/* Runs ONE sweep of the form the solver's next sweep would take (BC_PREFDIAG_NEXT_FORM: the two-level form, else the one-level
 * int8 sweep; other forms are refused) with per-row output and no rescoring.  The values come out of the sweep kernels' own
 * code: k_sweep_i8 / k_sweep_i4 instantiated with DUMP = true, which adds stores and nothing else.
 *   mode: 0 GIGA (two vectors, unit norms), 1 dot (one vector; score u.v / post_div).
 *   v == NULL: the solver's own vectors, ||v|| and digit records -- the production path; mode must be the solver's.
 *   v given (host; S pairs interleaved for mode 0, S doubles for mode 1): uploaded to scratch, where a one-wave kernel
 *     produces both digit records with bc_i8q_wave / bc_i4q_wave, the functions the step kernels use.  GIGA vectors whose
 *     norms differ from 1 by more than 1e-9 are refused (the GIGA sweep takes ||v|| = 1).
 *   self_quantise != 0: the one-level sweep quantises v in its own prologue instead of reading a digit record (refused when
 *     the two-level form would run).
 *   out_ul[2 * rows_cap]: (U, L) of level 1 for rows 0 .. ptiles * 256 - 1 (rows_cap must cover them); dead rows (-inf, -inf).
 *   out_ul8[2 * rows_cap], out_theta0[blocks_cap]: two-level form only (required when it runs): (U8, L8) of every row level 2
 *     re-bounded, NaN for the rest; theta0 of every sweep block (blocks_cap >= BC_PREFDIAG_GRID1).
 *   *form_run: 3 or 1.
 * The solver's skip flag is not consulted.  The call leaves the solver as found: the seeds ("hot") and "ctrl" are put aside and
 * restored and no host-side counter moves, so a build continued afterwards has the trace, weights, prefilter_stats and
 * prefilter_levels of a run without the call.  The buffers listed under "the last sweep's outputs" hold this sweep's results;
 * the two-level form's "spill" is filled with 0xff bytes first, so a slot this sweep did not write reads (-1, -1), and
 * "ctrl_swept" holds the control block as the sweep left it. */
int bc_snnls_prefdiag_sweep(bc_snnls* h, int32_t mode, const double* v, double post_div, int32_t self_quantise, float* out_ul,
                            float* out_ul8, float* out_theta0, int64_t rows_cap, int32_t blocks_cap, int32_t* form_run);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_PREFDIAG_H */
