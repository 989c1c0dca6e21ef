// Host program around csrc/bc_slab.h (built with -fsanitize=address,undefined by tests/test_slab_cpu.py).
//
//   slab_harness pieces n0 n1 ... [ints]   walks the cursor over pieces of n0, n1, ... doubles ("ints": the last piece is
//                                          written as ints, the way the runs keep their flags), checks every offset is even,
//                                          that the pieces are disjoint and in order and that the total is the sum of the
//                                          rounded sizes, then writes every piece end to end into a malloc of exactly `total`
//                                          doubles.  Prints "total o0 o1 ...".
//   slab_harness hmc_state c d             bc_hmc's state slab for c chains of d coordinates (layout_state of bc_hmc.hip: five
//                                          [c][d] pieces, three [c], the reduced pass [c][1 + d], the inverse mass [d], two
//                                          doubles of flags) through the same checks.  Prints "total closed_form".
// Exit status 0: every check held.
#include "../beta_cores_amd/csrc/bc_slab.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static size_t even(size_t n) { return (n + 1) & ~(size_t)1; }

static int fail(const char* what, size_t i) {
  fprintf(stderr, "slab_harness: %s (piece %zu)\n", what, i);
  return 1;
}

// walks, checks and writes; offsets and the total come back
static int walk(const std::vector<size_t>& sizes, bool last_as_ints, std::vector<size_t>* offs, size_t* total) {
  bc_slab sl;
  size_t want = 0;
  offs->clear();
  for (size_t i = 0; i < sizes.size(); ++i) {
    const size_t o = sl.take(sizes[i]);
    if (o & 1) return fail("an offset is odd", i);
    if (o != want) return fail("a piece does not start where the one before it ends (rounded)", i);
    if (i > 0 && offs->back() + sizes[i - 1] > o) return fail("two pieces overlap", i);
    want += even(sizes[i]);
    offs->push_back(o);
  }
  if (sl.total != want) return fail("the total is not the sum of the rounded sizes", sizes.size());
  *total = sl.total;
  double* slab = static_cast<double*>(malloc(sl.total * sizeof(double)));      // (exactly the total: an overrun is ASan's to see)
  if (!slab && sl.total) return fail("malloc", 0);
  for (size_t i = 0; i < sizes.size(); ++i) {
    double* p = slab + (*offs)[i];
    if (last_as_ints && i + 1 == sizes.size()) {
      int* q = reinterpret_cast<int*>(p);
      for (size_t k = 0; k < 2 * sizes[i]; ++k) q[k] = (int)k;
    } else {
      for (size_t k = 0; k < sizes[i]; ++k) p[k] = (double)i;
    }
  }
  // every piece still holds what was written into it: nothing was written twice
  for (size_t i = 0; i < sizes.size(); ++i) {
    const double* p = slab + (*offs)[i];
    if (last_as_ints && i + 1 == sizes.size()) {
      const int* q = reinterpret_cast<const int*>(p);
      for (size_t k = 0; k < 2 * sizes[i]; ++k)
        if (q[k] != (int)k) return fail("a piece was overwritten", i);
    } else {
      for (size_t k = 0; k < sizes[i]; ++k)
        if (p[k] != (double)i) return fail("a piece was overwritten", i);
    }
  }
  free(slab);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage", 0);
  std::vector<size_t> sizes, offs;
  size_t total = 0;
  if (!strcmp(argv[1], "pieces")) {
    bool ints = false;
    for (int i = 2; i < argc; ++i) {
      if (!strcmp(argv[i], "ints")) ints = true;
      else sizes.push_back((size_t)strtoull(argv[i], nullptr, 10));
    }
    if (walk(sizes, ints, &offs, &total)) return 1;
    printf("%zu", total);
    for (size_t o : offs) printf(" %zu", o);
    printf("\n");
    return 0;
  }
  if (!strcmp(argv[1], "hmc_state") && argc == 4) {
    const size_t c = (size_t)strtoull(argv[2], nullptr, 10), d = (size_t)strtoull(argv[3], nullptr, 10), cd = c * d;
    sizes = {cd, cd, cd, cd, cd, c, c, c, c * (1 + d), d, 2};
    if (walk(sizes, true, &offs, &total)) return 1;
    printf("%zu %zu\n", total, 5 * even(cd) + 3 * even(c) + even(c * (1 + d)) + even(d) + 2);
    return 0;
  }
  return fail("usage", 0);
}
