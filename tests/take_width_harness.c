/* Host check of beta_cores_amd/csrc/bc_take_width.h, the header k_take_rows' launch code decides its access width with.
 * For every source and destination base offset in 0..63 that is element-aligned, dz in 1..40 and 127..130, and both element
 * sizes: the width is 16, 8 or 4, never below the element size, and the widest that a brute-force walk over the words of
 * the first rows allows -- every word of every row naturally aligned on both sides.  Prints the number of combinations
 * checked; exit status 0 when all agree. */
#include <stdio.h>
#include "bc_take_width.h"

/* 1 if rows of `pitch` bytes starting at src / dst can be moved as w-byte words: w divides the pitch and every word of the
 * first 16 rows (after which the pattern of addresses mod 16 repeats) is w-aligned at its source and at its destination */
static int words_ok(uint64_t src, uint64_t dst, uint64_t pitch, uint64_t w) {
  uint64_t r, c;
  if (pitch % w) return 0;
  for (r = 0; r < 16; ++r)
    for (c = 0; c < pitch; c += w)
      if ((src + r * pitch + c) % w || (dst + r * pitch + c) % w) return 0;
  return 1;
}

int main(void) {
  const uint64_t base = (uint64_t)1 << 40;      /* a 256-aligned allocation */
  long checked = 0;
  int e, dz, so, dso;
  for (e = 4; e <= 8; e += 4)
    for (dz = 1; dz <= 130; dz = (dz == 40 ? 127 : dz + 1))
      for (so = 0; so < 64; so += e)
        for (dso = 0; dso < 64; dso += e) {
          const uint64_t src = base + (uint64_t)so, dst = base + (uint64_t)dso, pitch = (uint64_t)dz * (uint64_t)e;
          const int w = bc_take_word_bytes(src, dst, dz, e);
          int want = 4;
          if (words_ok(src, dst, pitch, 16)) want = 16;
          else if (words_ok(src, dst, pitch, 8)) want = 8;
          if (w != want || w < e || !words_ok(src, dst, pitch, (uint64_t)w)) {
            printf("elem %d dz %d src+%d dst+%d: width %d, expected %d\n", e, dz, so, dso, w, want);
            return 1;
          }
          if (bc_take_flat(dz, e) != (pitch < 256)) { printf("flat(%d, %d)\n", dz, e); return 1; }
          ++checked;
        }
  /* premises broken: an address or pitch that is not element-aligned, an element size the library does not store */
  if (bc_take_word_bytes(base + 4, base, 3, 8) != 0 || bc_take_word_bytes(base, base + 2, 3, 4) != 0) return 2;
  if (bc_take_word_bytes(base, base, 3, 2) != 0 || bc_take_word_bytes(base, base, 0, 8) != 0) return 2;
  printf("%ld combinations\n", checked);
  return 0;
}
