// A cursor over a slab of doubles that is cut into 16-byte aligned pieces: every layout of the chunked runs (bc_viopt.hip,
// bc_hmc.hip, bc_hmc_small.hip) is one walk with it, so that the total and the pieces' offsets cannot disagree.  Host only.
#pragma once
#include <stddef.h>

static inline size_t bc_even(size_t n) { return (n + 1) & ~(size_t)1; }

struct bc_slab {
  size_t total = 0;      // doubles handed out so far: after the walk, the slab's size
  // the offset of a piece of n doubles; the next piece starts 16-byte aligned
  size_t take(size_t n) { return take_unpadded(bc_even(n)); }
  // the same without the rounding: for a slab's last piece, where nothing behind it needs the alignment
  size_t take_unpadded(size_t n) {
    const size_t o = total;
    total += n;
    return o;
  }
};
