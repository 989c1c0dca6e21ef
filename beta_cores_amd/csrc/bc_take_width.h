// bc_take_width.h -- how k_take_rows (bc_take.hip) moves a row: the width of one lane's access and which of the kernel's
// two lane mappings serves a row pitch.  Plain C, shared by the launch code and a host harness (tests/take_width_harness.c)
// that checks every combination of base alignment, column count and element size without a GPU.
#ifndef BC_TAKE_WIDTH_H
#define BC_TAKE_WIDTH_H
#include <stdint.h>

#define BC_TAKE_WAVE_BYTES 256      /* rows shorter than this share a wave-instruction through the flat mapping */

/* Bytes one lane moves per access: the widest of 16, 8, 4 that divides the row pitch dz*elem AND both base addresses, so
 * that every word of every row is naturally aligned on both sides.  elem is 8 or 4 and both bases are element-aligned (a
 * borrowed tensor guarantees no more), so float64 rows never go below 8 and float32 rows never below 4.
 * Returns 0 for arguments that break those premises. */
static inline int bc_take_word_bytes(uint64_t src_addr, uint64_t dst_addr, int64_t dz, int elem) {
  if ((elem != 8 && elem != 4) || dz <= 0) return 0;
  const uint64_t pitch = (uint64_t)dz * (uint64_t)elem;
  const uint64_t any = pitch | src_addr | dst_addr;
  if (any & (uint64_t)(elem - 1)) return 0;
  if ((any & 15u) == 0) return 16;
  if ((any & 7u) == 0) return 8;
  return 4;
}

/* 1: rows of this pitch are shorter than one wave-instruction and are copied through the flat word mapping (consecutive
 * lanes take consecutive words of the OUTPUT, crossing row ends); 0: one wave per row, several rows in flight */
static inline int bc_take_flat(int64_t dz, int elem) { return (uint64_t)dz * (uint64_t)elem < BC_TAKE_WAVE_BYTES; }

#endif /* BC_TAKE_WIDTH_H */
