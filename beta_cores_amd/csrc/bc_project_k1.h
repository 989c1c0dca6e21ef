// K1 kernels and their launch tables, shared by the two translation units that instantiate them: bc_project.hip (float64
// rows, and everything on the host side of a projection) and bc_project_f32.hip (float32 rows).  Each set of instantiations
// takes about a minute to compile, so they are built side by side.
#pragma once
#include "bc_internal.h"
#include "bc_project_plan.h"
#include "bc_np_exp.h"
#include "bc_np_pow2.h"
#include "bc_layout.h"
#include "bc_k1_math.h"
#include "../../include/beta_cores_betagrad.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double bc_d2v __attribute__((ext_vector_type(2)));
typedef unsigned int bc_u4v __attribute__((ext_vector_type(4)));
typedef unsigned int bc_u2v __attribute__((ext_vector_type(2)));
typedef float bc_f4v __attribute__((ext_vector_type(4)));
// Z is read once and Phi written once per projection; the non-temporal policy on both streams
// (aux = 2 is the `nt` bit of buffer loads on gfx950) was measured and changes nothing here (the kernel
// is MFMA-bound: 3.18 ms vs 3.05-3.11 ms at N=4M, D=128), so it stays off unless built with -DBC_K1_NT.
#ifdef BC_K1_NT
#define BC_K1_Z_AUX 2
__device__ __forceinline__ void bc_store2(double* p, double x, double y) {
  bc_d2v v = {x, y};
  __builtin_nontemporal_store(v, reinterpret_cast<bc_d2v*>(p));
}
#else
#define BC_K1_Z_AUX 0
__device__ __forceinline__ void bc_store2(double* p, double x, double y) { *reinterpret_cast<double2*>(p) = make_double2(x, y); }
#endif

// struct ProjArgs, which the kernels take by value: bc_project_plan.h
#ifdef BC_K1_STAMPS
#define KSTAMP(i) do { if (a.stamps && threadIdx.x == 0) { a.stamps[(size_t)blockIdx.x * 32 + (i)] = __builtin_amdgcn_s_memtime(); \
    if ((i) == 0 || (i) == 24) a.stamps[(size_t)blockIdx.x * 32 + ((i) == 0 ? 30 : 31)] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define KSTAMP(i) do { } while (0)
#endif

// ---- lookup tables of the epilogue's exp / log1p(exp(-a)) bodies (bc_k1_math.h): 578 doubles in global memory, copied
// into LDS by every block of a model that needs them (behind the staging buffers; ~4.6 KB next to the 61 KB those take)
__device__ const unsigned long long g_k1_tab_bits[BC_K1_TAB_DOUBLES] = BC_K1_TABLE_INIT;

template <int MODEL>
constexpr bool bc_model_uses_tables();
// doubles of LDS the tables take: the static ones, plus the per-launch power table of the logistic beta-likelihood
template <int MODEL>
constexpr int bc_model_tab_doubles() { return !bc_model_uses_tables<MODEL>() ? 0 : BC_K1_TAB_DOUBLES + (MODEL == BC_MODEL_LOGISTIC_BETA ? 264 : 0); }
template <int MODEL>
constexpr bool bc_model_uses_tables() {
  return MODEL == BC_MODEL_LINREG_BETA || MODEL == BC_MODEL_LOGISTIC_LL || MODEL == BC_MODEL_LOGISTIC_BETA ||
         MODEL == BC_MODEL_GAUSS_BETA || MODEL == BC_MODEL_GAUSS_BETA_GRAD || MODEL == BC_MODEL_LINREG_BETA_GRAD ||
         MODEL == BC_MODEL_LOGISTIC_BETA_GRAD;
}
// which extras a model's formula takes: the row's y (the column behind the D features), or the Gaussian models' per-row and
// per-sample quadratic forms (the beta-gradients of the regression models, ids 7 and 8, come after the Gaussian block)
template <int MODEL>
constexpr bool bc_model_has_y() { return MODEL == BC_MODEL_LINREG_LL || MODEL == BC_MODEL_LINREG_BETA || MODEL == BC_MODEL_LINREG_BETA_GRAD; }
template <int MODEL>
constexpr bool bc_model_is_gauss() { return MODEL == BC_MODEL_GAUSS_LL || MODEL == BC_MODEL_GAUSS_BETA || MODEL == BC_MODEL_GAUSS_BETA_GRAD; }
// the beta-gradients of the regression models exist as materialising projections only (include/beta_cores_betagrad.h)
template <int MODEL>
constexpr bool bc_model_store_only() { return MODEL == BC_MODEL_LINREG_BETA_GRAD || MODEL == BC_MODEL_LOGISTIC_BETA_GRAD; }

// (the logistic beta-likelihood's body, bc_logistic_beta_value, lives in bc_k1_math.h: compiled for the host too, where
// tests/k1_math_harness.c measures it against 80-bit arithmetic)
// BC_K1_GROUP (build-time): how many elements of a row the epilogue lets the scheduler interleave (see the S = 100
// epilogue); the beta-logistic element is four transcendental bodies by itself
#ifndef BC_K1_GROUP
#define BC_K1_GROUP 2
#endif
template <int MODEL>
__device__ __forceinline__ double bc_model_value(double p, double ra, double sa, const double* c, const double* tab) {
  // every model id has a case of its own: an id without one must not compile (it would compute another model's formula)
  static_assert(MODEL >= BC_MODEL_LINREG_LL && MODEL <= BC_MODEL_LOGISTIC_BETA_GRAD, "bc_model_value: unknown model id");
  switch (MODEL) {
    // (2p)*y is evaluated as p*(2y): doubling is exact, so the product rounds to the same double, and 2y -- like y*y --
    // is a per-row value that stays out of the per-sample code
    case BC_MODEL_LINREG_LL: {            // c0 - c1*(y^2 - 2*p*y + p^2)
      const double q = (ra * ra - p * (2. * ra)) + p * p;
      return c[0] - c[1] * q;
    }
    case BC_MODEL_LINREG_BETA: {          // k0*(k1*exp(k2*q) + k3)
      const double q = (ra * ra - p * (2. * ra)) + p * p;
      return c[0] * (c[1] * bc_exp_tab_nonpos(c[2] * q, tab) + c[3]);
    }
    case BC_MODEL_LOGISTIC_LL: {          // m = -z.th ; m < 100 ? -log1p(exp(m)) : -m ;  log1p(e^m) = max(m, 0) + log1p(e^-|m|)
      const double m = -p;
      // (|m| is bounded for the body: past 800 it returns 0 either way; fmin drops a NaN, which the other branch keeps)
      return (m < 100.) ? -(fmax(m, 0.) + bc_log1p_exp_neg_tab(fmin(fabs(m), 800.), tab)) : -m;
    }
    case BC_MODEL_LOGISTIC_BETA:          // -( (b+1)/b*(1+e^m)^-b - ((1+e^m)^(-b-1) + (1+e^-m)^(-b-1)) ): bc_k1_math.h, the form with the
                                          // per-launch power table behind the static tables (c[1], c[4..7], c[2]: its series)
      return bc_logistic_beta_value_pt(-p, c[0], c[1], c[4], c[5], c[6], c[7], c[2], tab, tab + BC_K1_TAB_DOUBLES);
    case BC_MODEL_GAUSS_LL: {             // cc - 1/2*(xSx + tSt - 2*xSt)
      const double q = (ra + sa) - 2. * p;
      return c[0] - 1. / 2. * q;
    }
    case BC_MODEL_GAUSS_BETA: {           // 1/b*exp(-.5*b*q) - (1+b)^(-.5d-1)
      const double q = (ra + sa) - 2. * p;
      return c[0] * bc_exp_tab_nonpos(c[1] * q, tab) - c[2];
    }
    case BC_MODEL_GAUSS_BETA_GRAD: {      // gaussian.py:46-62
      const double q = (ra + sa) - 2. * p;
      const double gq = bc_exp_tab_nonpos(c[1] * q, tab);
      const double t1 = c[3] * (c[0] * gq - c[2]);
      const double t2 = c[4] * gq;
      const double t3 = c[5] * q * gq;
      return ((t1 - t2) - t3) - c[6];
    }
    case BC_MODEL_LINREG_BETA_GRAD: {     // (k0 + k1*q)*exp(k2*q) - k3: bc_k1_math.h; q in LINREG_BETA's expression order
      const double q = (ra * ra - p * (2. * ra)) + p * p;
      return bc_linreg_beta_grad_value(q, c[0], c[1], c[2], c[3], tab);
    }
    case BC_MODEL_LOGISTIC_BETA_GRAD:     // bc_k1_math.h; static tables only (no per-launch power table)
      return bc_logistic_beta_grad_value(-p, c[0], c[1], c[2], c[3], tab);
    default:
      return 0.;                          // (unreachable: see the static_assert)
  }
}

// exp() carrying NumPy's bits on AVX-512 hosts (bc_np_exp.h) where that routine covers the argument, the ordinary one
// in the far tails (|x| >= 707.7: the results there are below the last bit of anything they are added to)
__device__ __forceinline__ double bc_exp_like_numpy(double x) {
  int covered;
  const double e = bc_np_exp(x, &covered);
  return covered ? e : exp(x);
}

// The model value of a CONSTANT row (all S values equal: a data row with all-zero features) with the reference's bits:
// which of these rows the reference's centring leaves exactly 0 depends on the last bit of the constant (section 7 of
// DESIGN.md, golden F13), so their np.exp() is restated exactly; the formulas without a transcendental are already
// bit-identical; the logistic log-likelihood's log1p(exp(0)) = RN(log 2) matches as it is; the logistic beta-likelihood's
// constant at m = 0 (a data row z = 0: two np.power(2, .) calls, model_lr.py:85) is handed in by the caller as c[3] --
// the host layer evaluates the reference's expression with NumPy itself (likelihoods.LogisticRegression.params) --
// and rows that are constant because every sample saturated (m << 0: -((b+1)/b - 1); m >> 0: 1) need no power at all.
template <int MODEL>
__device__ __forceinline__ double bc_model_value_np(double p, double ra, double sa, const double* c, const double* tab) {
  switch (MODEL) {
    case BC_MODEL_LINREG_BETA: {
      const double q = (ra * ra - p * (2. * ra)) + p * p;
      return c[0] * (c[1] * bc_exp_like_numpy(c[2] * q) + c[3]);
    }
    case BC_MODEL_GAUSS_BETA: {
      const double q = (ra + sa) - 2. * p;
      return c[0] * bc_exp_like_numpy(c[1] * q) - c[2];
    }
    case BC_MODEL_GAUSS_BETA_GRAD: {
      const double q = (ra + sa) - 2. * p;
      const double gq = bc_exp_like_numpy(c[1] * q);
      const double t1 = c[3] * (c[0] * gq - c[2]);
      const double t2 = c[4] * gq;
      const double t3 = c[5] * q * gq;
      return ((t1 - t2) - t3) - c[6];
    }
    case BC_MODEL_LOGISTIC_BETA:
      if (p == 0. && c[3] == c[3]) return c[3];
      return bc_model_value<MODEL>(p, ra, sa, c, tab);
    default:
      return bc_model_value<MODEL>(p, ra, sa, c, tab);
  }
}
template <int MODEL>
constexpr bool bc_model_has_np_exp() { return MODEL == BC_MODEL_LINREG_BETA || MODEL == BC_MODEL_GAUSS_BETA || MODEL == BC_MODEL_GAUSS_BETA_GRAD; }
// models whose constant rows are re-evaluated with the reference's bits (bc_model_value_np)
template <int MODEL>
constexpr bool bc_model_const_fixup() { return bc_model_has_np_exp<MODEL>() || MODEL == BC_MODEL_LOGISTIC_BETA; }

// the constant of a constant row from the contraction value `p` of the lane's first sample: every lane of the row
// evaluates its own (they agree up to the last bit), the lane with g == 0 decides
template <int MODEL>
__device__ __forceinline__ double bc_const_row_value(double devval, double p, double ra, double sa, const double* c, int lane, const double* tab,
                                                     const double* ck = nullptr, const double* cv = nullptr, int nck = 0) {
  if (!bc_model_const_fixup<MODEL>()) return devval;
  double v = bc_model_value_np<MODEL>(p, ra, sa, c, tab);
  if (MODEL == BC_MODEL_LINREG_BETA && nck > 0) {
    // the caller's own evaluation of the reference's expression for rows with all-zero features (their value depends on y
    // alone): binary search on y.  (Rare branch of a rare branch; the value still has to agree with the device's to 1e-13.)
    int lo = 0, hi = nck - 1;
    while (lo <= hi) {
      const int mid = (lo + hi) >> 1;
      const double k = ck[mid];
      if (k == ra) { v = cv[mid]; break; }
      if (k < ra) lo = mid + 1; else hi = mid - 1;
    }
  }
  v = __shfl(v, lane & 15, BC_WAVE);
  // the restated value is the same number as the device's own up to the last bits; anything else means the row is
  // constant for another reason than equal arguments (it then keeps the device's value)
  return (fabs(v - devval) <= 1e-13 * fabs(devval)) ? v : devval;
}

// Row statistics of one wave's accumulators, shared by the staged kernel (k_project) and the Theta-resident one
// (k_project_r): on entry acc / tv hold the contraction values p of the lane's JT data rows (row0 + jt; samples
// 16*st + g + 4*reg, tail sample 16*NT + g); on exit the centred model values.  Writes the row norms (STORE).
// full_tile: every row of the tile is a real one (no masking).
template <int MODEL, int NT, int JT, int TL, bool STORE>
__device__ __forceinline__ void k1_row_stats(double4_t (&acc)[JT][NT], double (&tv)[JT], const double (&ra_pf)[JT], const ProjArgs& a,
                                             const int S, const int lane, const int g, const double* tabl, const long long row0,
                                             const bool full_tile) {
  const int s_tail = NT * 16 + g;
  if (TL > 0) {
    // 96 < S <= 100 (every BASELINE config): all samples of the NT tiles are real ones and every lane holds some, so
    // the `s < S` predicates vanish.  Rows past the end of the shard (last tile only) read as zeros, give finite
    // model values, and are zeroed after the fact under a block-uniform branch instead of a select per element.
    // "All S values of the row are equal" is not tracked per element either: such a row shows up afterwards as a
    // centred row with a vanishing norm and is then examined exactly (below).
    #pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      const double ra = ra_pf[jt];
      const double p00 = acc[jt][0][0];          // the contraction value of the lane's first sample (constant rows, below)
      double sum = 0.;
#pragma unroll
      for (int st = 0; st < NT; ++st) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const double v = bc_model_value<MODEL>(acc[jt][st][reg], ra, bc_model_is_gauss<MODEL>() ? a.saux[16 * st + g + 4 * reg] : 0., a.c, tabl);
          acc[jt][st][reg] = v;
          sum += v;
          // Pin every BC_K1_GROUP elements: left to itself the compiler splits the table-driven bodies in two stages -- index
          // and LDS read of all 25 elements of the row first, polynomials afterwards -- keeps every intermediate alive in
          // between and spills ~900 VGPRs (the beta-logistic instantiation).  The empty asm consumes the finished values
          // (ordering the arithmetic) and its memory clobber keeps the next group's table reads behind it.
          if (bc_model_uses_tables<MODEL>() && ((4 * st + reg + 1) % BC_K1_GROUP) == 0) asm volatile("" : "+v"(acc[jt][st][reg]), "+v"(sum) :: "memory");
        }
      }
      {
        const double v = (s_tail < S) ? bc_model_value<MODEL>(tv[jt], ra, bc_model_is_gauss<MODEL>() ? a.saux[s_tail] : 0., a.c, tabl) : 0.;
        tv[jt] = v;
        sum += v;
      }
      sum += __shfl_xor(sum, 16, BC_WAVE);
      sum += __shfl_xor(sum, 32, BC_WAVE);
      double mean = sum / (double)S;                 // lls.mean(axis=1), tree order
      double sq = 0.;
#pragma unroll
      for (int st = 0; st < NT; ++st)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const double v = acc[jt][st][reg] - mean;
          acc[jt][st][reg] = v;
          sq = fma(v, v, sq);
        }
      {
        const double v = (s_tail < S) ? tv[jt] - mean : 0.;
        tv[jt] = v;
        sq = fma(v, v, sq);
      }
      sq += __shfl_xor(sq, 16, BC_WAVE);
      sq += __shfl_xor(sq, 32, BC_WAVE);
      // A row whose S values are all the same number c (a data row with all-zero features): the reference subtracts
      // NumPy's rounded mean of S copies of c, which is c only for some (c, S) -- otherwise the row keeps a tiny
      // constant residue, a non-zero norm, and is NOT one of the "all-zero rows" dropped at hilbert.py:16.  The
      // tree-order sum above rounds differently and would flip that zero / non-zero status, so such rows are
      // re-centred with NumPy's order.  Every constant row lands here: its centred values are a few ulp of c, i.e.
      // sq <= S*(8 eps c)^2, a thousand times inside the bound below (and NaN rows never do: they stay NaN as in the
      // reference).  Inside the bound each v was within 1e-11 of the mean, so v - mean was exact (Sterbenz) and
      // mean + (v - mean) gives v back exactly: "all v equal" is decided, exactly, on the centred values.
      const double tiny = 1e-12 * mean;
      const bool suspect = sq <= (double)S * (tiny * tiny);
      if (__builtin_amdgcn_ballot_w64(suspect) != 0ull) {
        double d0 = acc[jt][0][0];
        asm volatile("" : "+v"(d0));                 // keeps the 25 compares below out of the straight-line code
        bool same = suspect;
#pragma unroll
        for (int st = 0; st < NT; ++st)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) same &= (acc[jt][st][reg] == d0);
        if (s_tail < S) same &= (tv[jt] == d0);
        int ok = same ? 1 : 0;
        ok &= (d0 == __shfl_xor(d0, 16, BC_WAVE)) ? 1 : 0;
        ok &= __shfl_xor(ok, 16, BC_WAVE);
        ok &= (d0 == __shfl_xor(d0, 32, BC_WAVE)) ? 1 : 0;
        ok &= __shfl_xor(ok, 32, BC_WAVE);
        if (ok) {                                    // the four lanes of a constant row take this together
          const double cval = bc_const_row_value<MODEL>(mean + d0, p00, ra, bc_model_is_gauss<MODEL>() ? a.saux[g] : 0., a.c, lane, tabl, a.ck, a.cv, a.nck);
          mean = bc_np_sum_const_256(cval, S) / (double)S;
          const double v = cval - mean;
          sq = 0.;
#pragma unroll
          for (int st = 0; st < NT; ++st)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              acc[jt][st][reg] = v;
              sq = fma(v, v, sq);
            }
          const double vt = (s_tail < S) ? v : 0.;
          tv[jt] = vt;
          sq = fma(vt, vt, sq);
        }
        // the four lanes of a row agree on `ok`: a recomputed row adds up its four new partial sums, every other
        // row keeps the total it had
        double sq2 = ok ? sq : 0.;
        sq2 += __shfl_xor(sq2, 16, BC_WAVE);
        sq2 += __shfl_xor(sq2, 32, BC_WAVE);
        if (ok) sq = sq2;
      }
      if (!full_tile && !(row0 + jt < a.n_rows)) {
#pragma unroll
        for (int st = 0; st < NT; ++st) acc[jt][st] = (double4_t){0., 0., 0., 0.};
        tv[jt] = 0.;
        sq = 0.;
      }
      if (STORE && g == 0) a.norms[row0 + jt] = sqrt(sq);
    }
  } else {
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
    const long long gr = row0 + jt;
    const bool live = gr < a.n_rows;
    const double ra = ra_pf[jt];
    const double p00 = acc[jt][0][0];            // the contraction value of the lane's first sample (constant rows, below)
    double sum = 0., vmin = INFINITY, vmax = -INFINITY;
    // TL > 0 kernels (96 < S <= 100): every sample of the NT tiles is a real one and every lane holds some, so the
    // `s < S` predicates vanish and "all S values equal" is tracked with compares against the lane's first value
    // (fmin / fmax cost three instructions each with their canonicalisation; a NaN makes the row non-constant,
    // as in the reference, where a NaN row stays NaN).
    double vref = 0.;
    bool differs = false;
#pragma unroll
    for (int st = 0; st < NT; ++st) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int s = 16 * st + g + 4 * reg;
        double v = 0.;
        if (TL > 0) {
          if (live) v = bc_model_value<MODEL>(acc[jt][st][reg], ra, bc_model_is_gauss<MODEL>() ? a.saux[s] : 0., a.c, tabl);
          if (st == 0 && reg == 0) vref = v;
          differs |= (v != vref);
        } else if (s < S && live) {
          v = bc_model_value<MODEL>(acc[jt][st][reg], ra, bc_model_is_gauss<MODEL>() ? a.saux[s] : 0., a.c, tabl);
          vmin = fmin(vmin, v);
          vmax = fmax(vmax, v);
        }
        acc[jt][st][reg] = v;
        sum += v;
      }
      if (bc_model_uses_tables<MODEL>()) asm volatile("" : "+v"(sum) :: "memory");     // see the S = 100 path above
    }
    if (TL > 0) {
      double v = 0.;
      if (s_tail < S && live) {
        v = bc_model_value<MODEL>(tv[jt], ra, bc_model_is_gauss<MODEL>() ? a.saux[s_tail] : 0., a.c, tabl);
        differs |= (v != vref);
      }
      tv[jt] = v;
      sum += v;
    }
    sum += __shfl_xor(sum, 16, BC_WAVE);
    sum += __shfl_xor(sum, 32, BC_WAVE);
    bool constant_row;
    double cval;
    if (TL > 0) {
      int df = differs ? 1 : 0;
      df |= (vref != __shfl_xor(vref, 16, BC_WAVE)) ? 1 : 0;
      df |= __shfl_xor(df, 16, BC_WAVE);
      df |= (vref != __shfl_xor(vref, 32, BC_WAVE)) ? 1 : 0;
      df |= __shfl_xor(df, 32, BC_WAVE);
      constant_row = df == 0;
      cval = vref;
    } else {
      vmin = fmin(vmin, __shfl_xor(vmin, 16, BC_WAVE));
      vmin = fmin(vmin, __shfl_xor(vmin, 32, BC_WAVE));
      vmax = fmax(vmax, __shfl_xor(vmax, 16, BC_WAVE));
      vmax = fmax(vmax, __shfl_xor(vmax, 32, BC_WAVE));
      constant_row = vmin == vmax;
      cval = vmax;
    }
    // a row whose S values are all the same number c (a data row with all-zero features): the reference subtracts
    // NumPy's rounded mean of S copies of c, which is c only for some (c, S) -- otherwise the row keeps a tiny constant
    // residue, a non-zero norm, and is NOT one of the "all-zero rows" dropped at hilbert.py:16.  The tree-order sum
    // above would round differently and flip that zero / non-zero status, so such rows use NumPy's order.
    if (bc_model_const_fixup<MODEL>() && __builtin_amdgcn_ballot_w64(constant_row && live) != 0ull) {
      const double cnp = bc_const_row_value<MODEL>(cval, p00, ra, bc_model_is_gauss<MODEL>() ? a.saux[g] : 0., a.c, lane, tabl, a.ck, a.cv, a.nck);
      if (constant_row && live) {                // the reference's bits for the constant: every element of the row IS it
        cval = cnp;
#pragma unroll
        for (int st = 0; st < NT; ++st)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) acc[jt][st][reg] = cnp;
        if (TL > 0) tv[jt] = cnp;
      }
    }
    const double mean = (constant_row ? bc_np_sum_const_256(cval, S) : sum) / (double)S;   // lls.mean(axis=1)
    double sq = 0.;
#pragma unroll
    for (int st = 0; st < NT; ++st) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int s = 16 * st + g + 4 * reg;
        double v = acc[jt][st][reg];
        v = ((TL > 0 || s < S) && live) ? v - mean : 0.;
        acc[jt][st][reg] = v;
        sq = fma(v, v, sq);
      }
    }
    if (TL > 0) {
      const double v = (s_tail < S && live) ? tv[jt] - mean : 0.;
      tv[jt] = v;
      sq = fma(v, v, sq);
    }
    sq += __shfl_xor(sq, 16, BC_WAVE);
    sq += __shfl_xor(sq, 32, BC_WAVE);
    if (STORE && g == 0) a.norms[row0 + jt] = sqrt(sq);
  }
  }
}

// NT = number of 16-sample accumulator tiles, KC = D-chunk staged per LDS pass,
// JT = 16-row sub-tiles per wave (2 -> 4 waves per 128-row tile, 1 -> 8 waves; the latter keeps
// the accumulators of a 200+-sample projection within the register file).
// TL = 0 or 4 "tail" samples beyond the NT tiles (S <= 16*NT + TL): one sample QUAD contracted with
// v_mfma_f64_4x4x4_4b_f64 (see the loop).  S = 100 (every BASELINE config) thus runs 6 tiles + 1 quad = exactly
// 100 samples instead of 7 tiles with 12 padded ones.
// STORE = false: the store-free mode of the gradient loop (bcores.py:141-146 needs `vecs.sum(axis=0)` only): the same
// contraction, formula, centring and per-tile column partials -- bit for bit -- but neither the tile nor the row norms
// are written; algorithmic traffic 8*128*Dz B per tile.
// ZT = the rows' storage type.  float rows are fetched with 4-byte loads and widened (exactly) on their way into LDS, which keeps
// doubles: everything from the first ds_write on is the same code.
template <int MODEL, int NT, int KC, int JT, bool RAW = false, int TL = 0, bool STORE = true, typename ZT = double>
__global__ __launch_bounds__(128 / (16 * JT) * 64, (JT == 1 && NT <= 8) ? 4 : 2) void k_project(ProjArgs a) {
  constexpr int ZB = (int)sizeof(ZT);             // bytes per stored element
  const ZT* zrows = reinterpret_cast<const ZT*>(a.z);
  static_assert(TL == 0 || (TL == 4 && !RAW), "tail: exactly one extra sample quad");
  static_assert(STORE || !RAW, "the raw passes of S > 256 exist to be stored");
  constexpr int NTHR = 128 / (16 * JT) * 64;
  constexpr int NR = NT * 16 + TL;                // rows of (padded) Theta this kernel contracts with
  constexpr int LDZ = KC + 1;    // odd stride: rows (2j, 2j+1) of a lane pair hit distinct banks
  constexpr int LDT = KC + 2;
  constexpr int ZP = (128 * KC) / NTHR;           // 8-byte loads of Z per thread per chunk
  constexpr int TN = NR * KC / 2;                 // 16-byte loads of Theta per chunk (whole block)
  constexpr int TP = (TN + NTHR - 1) / NTHR;
  extern __shared__ double lds[];
  double* Zl = lds;                    // [128][LDZ]
  double* Tl = lds + 128 * LDZ;        // [NR][LDT]   (reused for the column partials after the loop)
  double* tabl = lds + 128 * LDZ + NR * LDT;      // lookup tables of the epilogue's exp / log bodies (models that have one)
  if (bc_model_uses_tables<MODEL>()) {
    for (int i = threadIdx.x; i < BC_K1_TAB_DOUBLES; i += NTHR) tabl[i] = __builtin_bit_cast(double, g_k1_tab_bits[i]);
    if (MODEL == BC_MODEL_LOGISTIC_BETA)          // the power table of this launch's beta (bc_k1_math.h), from the global tables
      for (int i = threadIdx.x; i < BC_K1_LOG_N; i += NTHR)
        tabl[BC_K1_TAB_DOUBLES + i] = bc_pow_table_entry(i, a.c[1], reinterpret_cast<const double*>(g_k1_tab_bits));
  }                                               // visible after the first barrier of the contraction loop
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const long long tile = blockIdx.x;
  const long long r0 = tile * BC_TILE;
  const int S = a.s;
  const int row_base = (JT == 2) ? 32 * w + 2 * j : 16 * w + j;   // this lane's first data row in the tile

  double4_t acc[JT][NT];     // written by the first k-step
  double tv[JT];

  // Staging through buffer loads: a wave-uniform descriptor per operand (SGPRs), ONE 32-bit
  // per-thread byte offset shared by all passes, and a scalar offset per pass -- no 64-bit
  // address VGPRs.  The Z descriptor covers exactly this tile's valid rows, so rows past the end
  // of the data read as 0 (hardware range check); columns past D are clamped to a valid column
  // and multiply the zero padding of Theta.
  static_assert(NTHR % KC == 0 && NTHR % (KC / 2) == 0 && KC % 8 == 0, "staging map");
  constexpr int ZROWS = NTHR / KC;          // rows of Z covered by one pass
  constexpr int TROWS = NTHR / (KC / 2);    // rows of Theta covered by one pass
  const int zc = tid % KC, zrw = tid / KC;
  const int tc = (tid % (KC / 2)) * 2, trw = tid / (KC / 2);
  const long long rows_here = (a.n_rows - r0) < BC_TILE ? (a.n_rows - r0) : BC_TILE;
  const auto zrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(zrows + (size_t)r0 * a.dz), 0,
                                                       (int)(rows_here * a.dz * ZB), 0x00020000);
  const auto trsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.theta, 0, NR * a.dk * 8, 0x00020000);
  const int toff = (trw * a.dk + tc) * 8;
  ZT zr[ZP];
  double2 tr[TP];
  // Loads of one chunk in NPART slices: the first chunk is requested in one go, every later one in slices spread over
  // the contraction of the chunk before it.  (Issued in one go after the barrier, the 23 loads of a chunk held the
  // wave in the issue stage for 2-4k cycles -- the CU's memory pipeline takes them at ~20 B per cycle -- before its
  // first MFMA of the chunk: 15 % of the tile's time with nothing on the matrix pipe from this wave.)
  constexpr int NPART = KC / 8;                        // pairs of k-steps per chunk
  constexpr int NSL = KC / 4 > 2 ? KC / 4 - 2 : 1;     // slices: one per k-step, none in the chunk's last two (their
                                                       // loads would not be back when the chunk is written to LDS)
  auto load_part = [&](int d0, int part) __attribute__((always_inline)) {
    const int col = min(d0 + zc, a.d - 1);
    const int voff = (zrw * a.dz + col) * ZB;
#pragma unroll
    for (int q = part * ZP / NSL; q < (part + 1) * ZP / NSL; ++q) {
      if constexpr (ZB == 8) zr[q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(zrsrc, voff, q * ZROWS * a.dz * 8, BC_K1_Z_AUX));
      else zr[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(zrsrc, voff, q * ZROWS * a.dz * 4, BC_K1_Z_AUX));
    }
#pragma unroll
    for (int q = part * TP / NSL; q < (part + 1) * TP / NSL; ++q)   // rows past NR are outside the descriptor and read as 0
      tr[q] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(trsrc, toff, (q * TROWS * a.dk + d0) * 8, 0));
  };
  auto store_chunk = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < ZP; ++q) Zl[(q * ZROWS + zrw) * LDZ + zc] = (double)zr[q];
#pragma unroll
    for (int q = 0; q < TP; ++q) {
      const bool ok = (q + 1) * NTHR <= TN || tid + q * NTHR < TN;
      if (ok) *reinterpret_cast<double2*>(Tl + (q * TROWS + trw) * LDT + tc) = tr[q];
    }
  };

  const int nchunks = a.dk / KC;
  KSTAMP(0);
#pragma unroll
  for (int part = 0; part < NSL; ++part) load_part(0, part);
  // per-row extra (y / x^T Siginv x): requested now, consumed in the epilogue (a dependent load there cost its
  // full memory latency per tile)
  double ra_pf[JT];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
    const long long gr = r0 + row_base + jt;
    ra_pf[jt] = 0.;
    if (gr < a.n_rows) {
      if (bc_model_has_y<MODEL>()) ra_pf[jt] = (double)zrows[(size_t)gr * a.dz + a.d];
      else if (bc_model_is_gauss<MODEL>())ra_pf[jt] = a.rowaux[gr];
    }
  }
  const double4_t zero4 = {0., 0., 0., 0.};
  for (int c = 0; c < nchunks; ++c) {
    store_chunk();
    KSTAMP(1 + 5 * c);
    __syncthreads();
    KSTAMP(2 + 5 * c);
    const bool more = c + 1 < nchunks;
    const double* zrow0 = Zl + row_base * LDZ + g;
    const double* trow = Tl + j * LDT + g;
    const double* tquad = Tl + (NT * 16 + (j & 3)) * LDT + g;
    // one k-step (4 features): NT*JT 16x16x4 products + the tail quad.  FIRST: the very first step of the tile starts
    // the accumulators from the instruction's inline-constant 0 (no zero-fill of 100+ VGPRs per tile).
    // (always_inline: left to its heuristics the compiler keeps some of these lambdas out of line in the largest
    // instantiations -- the beta-logistic one -- and the accumulators they capture by reference then live in scratch:
    // 438 scratch stores inside the contraction, 2.35 -> 4.9 ms per 1M rows)
    auto kstep = [&](int kk, auto first) __attribute__((always_inline)) {
      constexpr bool FIRST = decltype(first)::value;
      double bz[JT];
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) bz[jt] = zrow0[jt * LDZ + kk * 4];
#pragma unroll
      for (int st = 0; st < NT; ++st) {
        const double at = trow[st * 16 * LDT + kk * 4];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
          acc[jt][st] = __builtin_amdgcn_mfma_f64_16x16x4f64(at, bz[jt], FIRST ? zero4 : acc[jt][st], 0, 0, 0);
      }
      if (TL > 0) {
        // the 25th sample quad (S in 97..100) on v_mfma_f64_4x4x4_4b_f64: four independent 4x4x4 products per
        // instruction; lane (g, q = 4*blk + t) supplies A_blk[t][g], B_blk[g][t] and receives D_blk[g][t]
        // (tools/mfma_f64_4x4x4_layout.hip).  With the same Theta quad in all four blocks and the sub-tile's 16
        // rows spread over (blk, t), the lane receives, for ITS row, sample 16*NT + g: the accumulator layout of
        // the 16x16x4 tiles, from the B operand they already hold.  (Round 1 contracted these four samples on the
        // vector pipe: 8 v_fma_f64 + 4 operand reads per k-step and 8 shuffles per tile instead of 2 + 1 + 0.)
        const double at = tquad[kk * 4];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) tv[jt] = __builtin_amdgcn_mfma_f64_4x4x4f64(at, bz[jt], FIRST ? 0. : tv[jt], 0, 0, 0);
      }
    };
#pragma unroll
    for (int kp = 0; kp < NPART; ++kp) {
      if (more && 2 * kp < NSL) load_part((c + 1) * KC, 2 * kp);
      if (kp == 0 && c == 0) kstep(0, std::true_type{});
      else kstep(2 * kp, std::false_type{});
      __builtin_amdgcn_sched_barrier(0);     // keeps each slice of loads with its k-step
      if (more && 2 * kp + 1 < NSL) load_part((c + 1) * KC, 2 * kp + 1);
      kstep(2 * kp + 1, std::false_type{});
      __builtin_amdgcn_sched_barrier(0);
    }
    KSTAMP(4 + 5 * c);
    __syncthreads();
    KSTAMP(5 + 5 * c);
  }

  // ---- epilogue: lane holds, for data rows (row_base + jt), samples s = 16*st + g + 4*reg
  if (RAW) {
    // S > 256: write the un-centred model values of this sample range; k_center_tiles finishes the job
    double* rbase = a.tiles + (size_t)tile * a.s_total * BC_TILE + row_base;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      const long long gr = r0 + row_base + jt;
      const bool live = gr < a.n_rows;
      const double ra = ra_pf[jt];
#pragma unroll
      for (int st = 0; st < NT; ++st)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int s = 16 * st + g + 4 * reg;
          if (s < S) {
            const double v = live ? bc_model_value_np<MODEL>(acc[jt][st][reg], ra, bc_model_is_gauss<MODEL>() ? a.saux[s] : 0., a.c, tabl) : 0.;
            rbase[(size_t)(a.s_off + s) * BC_TILE + jt] = v;
          }
        }
    }
    return;
  }
  // column partials reuse the staging LDS (all of it: Zl and Tl are dead after the loop)
  constexpr bool LDSCP = (JT == 2) && (NTHR / 64) * NR * 17 <= 128 * LDZ + NR * LDT;
  double* colpart = LDSCP ? lds : Tl;   // LDSCP: [waves][NR][17], else [waves][NR]
  k1_row_stats<MODEL, NT, JT, TL, STORE>(acc, tv, ra_pf, a, S, lane, g, tabl, r0 + row_base, rows_here == BC_TILE);
  KSTAMP(21);
  // store the tile (JT == 2: two adjacent rows per lane -> 16-byte stores, 256 B contiguous per 16 lanes) through a
  // buffer descriptor of exactly this tile's S*128 doubles: one per-lane byte offset for all stores, the sample's
  // offset as the instruction's scalar operand (no 64-bit address arithmetic per store), samples >= S dropped by the
  // hardware range check.  Column partials: one LDS base per lane, constant offsets.
  const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(a.tiles + (size_t)tile * S * BC_TILE), 0,
                                                       S * BC_TILE * 8, 0x00020000);
  const int woff = (g * BC_TILE + row_base) * 8;
  double* cpl = LDSCP ? colpart + (w * NR + g) * 17 + j : colpart + w * NR + g;
  auto put = [&](int s0, double v0, double v1) __attribute__((always_inline)) {       // sample s0 + g of this lane's row(s)
    double cp;
    if (JT == 2) {
      if (STORE) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bc_u4v, (bc_d2v){v0, v1}), wrsrc, woff, s0 * BC_TILE * 8, BC_K1_Z_AUX);
      cp = v0 + v1;
    } else {
      if (STORE) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(bc_u2v, v0), wrsrc, woff, s0 * BC_TILE * 8, BC_K1_Z_AUX);
      cp = v0;
    }
    // per-tile column partial (K2): sum over the tile's rows.  JT == 2 kernels park each lane's pair sum in LDS
    // ([wave][sample][16 row pairs], rows padded to 17) and let one thread per sample add them up in a fixed
    // order -- a 4-step fp64 shuffle reduction per value cost ~8 % of the kernel (0.25 ms per 4M rows).
    if (LDSCP) {
      cpl[s0 * 17] = cp;
    } else {
      cp += __shfl_xor(cp, 1, BC_WAVE);
      cp += __shfl_xor(cp, 2, BC_WAVE);
      cp += __shfl_xor(cp, 4, BC_WAVE);
      cp += __shfl_xor(cp, 8, BC_WAVE);
      if (j == 0) cpl[s0] = cp;
    }
  };
#pragma unroll
  for (int st = 0; st < NT; ++st)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) put(16 * st + 4 * reg, acc[0][st][reg], acc[JT - 1][st][reg]);
  if (TL > 0) put(NT * 16, tv[0], tv[JT - 1]);
  KSTAMP(22);
  __syncthreads();
  KSTAMP(23);
  constexpr int NW = NTHR / 64;
  for (int s = tid; s < S; s += NTHR) {
    double t = 0.;
    if (LDSCP) {
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) {
        const double* row = colpart + (ww * NR + s) * 17;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) t += row[jj];
      }
    } else {
      t = colpart[s];
#pragma unroll
      for (int ww = 1; ww < NW; ++ww) t += colpart[ww * NR + s];
    }
    a.tile_part[(size_t)tile * S + s] = t;
  }
  KSTAMP(24);
}

// ---------------------------------------------------------------------------------------------
// K1, Theta-RESIDENT formulation (large shards, D <= ~160 at S = 100).
//
// What the staged kernel above pays per 128-row tile besides its MFMAs: the whole of Theta (S x D, 102 KB at the
// headline shape) is re-staged through registers into LDS for EVERY tile, the Z tile is staged the same way, and four
// waves meet at two barriers per D-chunk (profiles/r02_notes.md: staging writes 3.4k, first-chunk wait up to 7.7k of a
// tile's ~38k cycles).  Here:
//   * one 512-thread block per CU keeps Theta in LDS for the whole launch (100 x 130 doubles = 104 KB at D = 128),
//     permuted so that the A-operand reads stay conflict-free (below);
//   * the B operand never touches LDS: lane (j, g) of a wave reads 32 contiguous bytes of ITS data row straight from
//     global memory (two dwordx4 per 16 columns; the four lanes of a row cover one 128-byte line), one 16-column stage
//     ahead of the MFMAs that consume it -- the k index of a 16x16x4 step is lane-group g, so "which column is k" is a free
//     choice as long as Theta uses the same one: k-step (c, t) contracts columns {16c + 4g + t}, and Theta[., 16c + 4g + t]
//     sits at LDS position 16c + 4t + g;
//   * waves are independent: a wave owns 32-row groups (wave id + 8 * gridDim * i), no barrier after the set-up, the
//     next group's first stage and y values are requested before the epilogue of the current one;
//   * column partials (K2) are accumulated per WAVE over all its groups in LDS (one S-vector per wave, written once at
//     the end: tile_part holds gridDim * 8 rows instead of one per tile); assignment of groups to waves is static, so the
//     sums are run-to-run deterministic.
// Same accumulator layout, row statistics (k1_row_stats), Phi layout and norms as the staged kernel.
// a stage of the B operand as doubles: float64 rows are used where they are, float32 rows are widened into `w`
template <int JT>
__device__ __forceinline__ double (&k1_stage_f64(double (&z)[JT][4], double (&)[JT][4]))[JT][4] { return z; }
template <int JT>
__device__ __forceinline__ double (&k1_stage_f64(float (&z)[JT][4], double (&w)[JT][4]))[JT][4] {
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int t = 0; t < 4; ++t) w[jt][t] = (double)z[jt][t];
  return w;
}

// float rows (ZT = float): the lane's four columns of a stage are ONE 16-byte load per row (half the load instructions and half
// the registers in flight), widened by four v_cvt_f64_f32 when the stage is consumed; every byte offset follows the element size.
template <int MODEL, int NT, int TL, bool STORE, typename ZT = double>
__global__ __launch_bounds__(512, 2) void k_project_r(ProjArgs a) {
  constexpr int JT = 2;
  constexpr int ZB = (int)sizeof(ZT);
  const ZT* zrows = reinterpret_cast<const ZT*>(a.z);
  constexpr int NR = NT * 16 + TL;
  constexpr int TRS = 5 * 4 * 17;             // transposition scratch of one wave: 5 values x 4 lane groups x (16 + 1)
  extern __shared__ double lds[];
  const int S = a.s;
  const int dk = a.dk;                        // multiple of 32: an even number of 16-column stages
  const int ldt = dk + 2;
  double* Tl = lds;                           // [NR][ldt], columns permuted inside every block of 16
  double* csum = Tl + NR * ldt;               // [8][NR] per-wave column partials
  double* trs = csum + 8 * NR;                // [8][TRS]
  double* tabl = trs + 8 * TRS;               // lookup tables of the transcendental bodies (models that have one)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;

  // ---- set-up: Theta -> LDS (wave w takes rows w, w + 8, ...), zero the accumulators, tables
  for (int i = w; i < NR; i += 8)
    for (int col = lane; col < dk; col += 64) Tl[i * ldt + (col & ~15) + 4 * (col & 3) + ((col >> 2) & 3)] = a.theta[(size_t)i * dk + col];
  if (a.part_init) {
    // a chunk of a chunked projection: wave (b, w) continues the partial it left in row (8 b + w) of tile_part.  Chunks
    // start at multiples of 8 * gridDim groups, so the wave meets the same groups in the same order as in one launch
    // over all rows and its additions are the same ones.
    for (int i = tid; i < 8 * NR; i += 512) {
      const int ww = i / NR, ss = i - ww * NR;
      csum[i] = ss < S ? a.tile_part[((size_t)blockIdx.x * 8 + ww) * S + ss] : 0.;
    }
  } else {
    for (int i = tid; i < 8 * NR; i += 512) csum[i] = 0.;
  }
  if (bc_model_uses_tables<MODEL>()) {
    for (int i = tid; i < BC_K1_TAB_DOUBLES; i += 512) tabl[i] = __builtin_bit_cast(double, g_k1_tab_bits[i]);
    if (MODEL == BC_MODEL_LOGISTIC_BETA)
      for (int i = tid; i < BC_K1_LOG_N; i += 512)
        tabl[BC_K1_TAB_DOUBLES + i] = bc_pow_table_entry(i, a.c[1], reinterpret_cast<const double*>(g_k1_tab_bits));
  }
  __syncthreads();

  const double* trow = Tl + j * ldt + g;
  const double* tquad = Tl + (NT * 16 + (j & 3)) * ldt + g;
  double* mycs = csum + w * NR;
  double* mytr = trs + w * TRS;
  const long long wstride = (long long)gridDim.x * 8;
  const int nstage = dk >> 4;
  const bool colmask = (a.d & 31) != 0;       // columns in [d, dk) exist: their Z values are zeroed (Theta's are zero already)
  const int voff0 = ((2 * j) * a.dz + 4 * g) * ZB;

  auto rsrc_of = [&](long long grp) __attribute__((always_inline)) {
    const long long row0 = grp * 32;
    long long rows = a.n_rows - row0;
    rows = rows > 32 ? 32 : rows;
    return __builtin_amdgcn_make_buffer_rsrc((void*)(zrows + (size_t)row0 * a.dz), 0, (int)(rows * a.dz * ZB), 0x00020000);
  };
  // one 16-column stage of the lane's two rows: b[jt][t] = Z[row0 + 2j + jt][16c + 4g + t]   (rows past N read as 0)
  // (float rows: the buffer's range check works per dword, so a load that straddles the end of the group's rows returns its
  // in-range floats and zeros behind them; columns >= d -- the y column, the next row -- are zeroed by the column mask below)
  auto issue = [&](auto rs, int c, ZT (&b)[JT][4]) __attribute__((always_inline)) {
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      if constexpr (ZB == 4) {
        const bc_f4v v = __builtin_bit_cast(bc_f4v, __builtin_amdgcn_raw_buffer_load_b128(rs, voff0 + jt * a.dz * 4, c * 64, BC_K1_Z_AUX));
        b[jt][0] = v[0]; b[jt][1] = v[1]; b[jt][2] = v[2]; b[jt][3] = v[3];
      } else {
        const bc_d2v lo = __builtin_bit_cast(bc_d2v, __builtin_amdgcn_raw_buffer_load_b128(rs, voff0 + jt * a.dz * 8, c * 128, BC_K1_Z_AUX));
        const bc_d2v hi = __builtin_bit_cast(bc_d2v, __builtin_amdgcn_raw_buffer_load_b128(rs, voff0 + jt * a.dz * 8 + 16, c * 128, BC_K1_Z_AUX));
        b[jt][0] = lo[0]; b[jt][1] = lo[1]; b[jt][2] = hi[0]; b[jt][3] = hi[1];
      }
    }
  };
  auto load_ra = [&](long long grp, double (&ra)[JT]) __attribute__((always_inline)) {
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      const long long gr = grp * 32 + 2 * j + jt;
      ra[jt] = 0.;
      if (gr < a.n_rows) {
        if (bc_model_has_y<MODEL>()) ra[jt] = (double)zrows[(size_t)gr * a.dz + a.d];
        else if (bc_model_is_gauss<MODEL>())ra[jt] = a.rowaux[gr];
      }
    }
  };

  double4_t acc[JT][NT];
  double tv[JT];
  const double4_t zero4 = {0., 0., 0., 0.};
  // the four k-steps of stage c; FIRST: the accumulators start from the instruction's inline-constant 0
  auto kstage = [&](int c, ZT (&bz)[JT][4], auto first) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first)::value;
    // float rows: the stage is widened here, when it is consumed (until then it waits in four registers per row, not eight)
    double bw[JT][4];
    double (&b)[JT][4] = k1_stage_f64(bz, bw);
    if (colmask && 16 * c + 16 > a.d) {       // wave-uniform: only the last stages of a D that is not a multiple of 32
#pragma unroll
      for (int jt = 0; jt < JT; ++jt)
#pragma unroll
        for (int t = 0; t < 4; ++t) b[jt][t] = (16 * c + 4 * g + t < a.d) ? b[jt][t] : 0.;
    }
    const double* tr0 = trow + 16 * c;
    const double* tq0 = tquad + 16 * c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int st = 0; st < NT; ++st) {
        const double at = tr0[st * 16 * ldt + 4 * t];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
          acc[jt][st] = __builtin_amdgcn_mfma_f64_16x16x4f64(at, b[jt][t], (FIRST && t == 0) ? zero4 : acc[jt][st], 0, 0, 0);
      }
      if (TL > 0) {
        const double at = tq0[4 * t];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) tv[jt] = __builtin_amdgcn_mfma_f64_4x4x4f64(at, b[jt][t], (FIRST && t == 0) ? 0. : tv[jt], 0, 0, 0);
      }
    }
  };

#ifdef BC_K1_STAMPS
  unsigned long long ph[4] = {0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memtime(), tstart = tprev;
#define RSTAMP(i) do { const unsigned long long tn = __builtin_amdgcn_s_memtime(); ph[i] += tn - tprev; tprev = tn; } while (0)
#else
#define RSTAMP(i) do { } while (0)
#endif
  long long grp = (long long)blockIdx.x * 8 + w;
  ZT bA[JT][4], bB[JT][4];
  double ra_next[JT] = {0., 0.};
  if (grp < a.ngroups) {
    issue(rsrc_of(grp), 0, bA);
    load_ra(grp, ra_next);
  }
  while (grp < a.ngroups) {
    const long long nxt = grp + wstride;
    const bool has_next = nxt < a.ngroups;
    const auto rs = rsrc_of(grp);
    double ra_pf[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) ra_pf[jt] = ra_next[jt];
    // ---- contraction: stage c + 1 is in flight while stage c is consumed; the last stage overlaps the NEXT group's first
    issue(rs, 1, bB);
    kstage(0, bA, std::true_type{});
    for (int c = 1; c + 1 < nstage; c += 2) {
      issue(rs, c + 1, bA);
      kstage(c, bB, std::false_type{});
      issue(rs, c + 2, bB);
      kstage(c + 1, bA, std::false_type{});
    }
    if (has_next) {
      issue(rsrc_of(nxt), 0, bA);
      load_ra(nxt, ra_next);
    }
    kstage(nstage - 1, bB, std::false_type{});
    RSTAMP(0);

    // ---- epilogue: model values, centring, norms (shared with the staged kernel)
    const long long row0 = grp * 32 + 2 * j;
    k1_row_stats<MODEL, NT, JT, TL, STORE>(acc, tv, ra_pf, a, S, lane, g, tabl, row0, grp * 32 + 32 <= a.n_rows);
    RSTAMP(1);
    const long long tile = grp >> 2;
    const int row_base = 32 * (int)(grp & 3) + 2 * j;
    const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(a.tiles + (size_t)tile * S * BC_TILE), 0, S * BC_TILE * 8, 0x00020000);
    const int woff = (g * BC_TILE + row_base) * 8;
    // stores + column partials.  The 25 pair sums of a lane go through the wave's transposition scratch five at a time:
    // [value][g][16 row pairs] -> lanes 0..19 add up one (value, g) each in row order and add the total to the wave's
    // running column sum.  LDS operations of one wave execute in issue order: no barrier, only the compiler is held.
    auto flush = [&](int v0idx, int nvals) __attribute__((always_inline)) {
      asm volatile("" ::: "memory");
      if (lane < 4 * nvals) {
        const double* src = mytr + lane * 17;
        double t = 0.;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) t += src[jj];
        const int val = v0idx + (lane >> 2), gg = lane & 3;          // value index 0..24 -> sample
        const int smp = (val < NT * 4) ? 16 * (val >> 2) + 4 * (val & 3) + gg : NT * 16 + gg;
        if (smp < S) mycs[smp] += t;
      }
      asm volatile("" ::: "memory");
    };
    int nq = 0;                                                        // values parked since the last flush
    int vbase = 0;
    auto put = [&](int vidx, int s0, double v0, double v1) __attribute__((always_inline)) {
      if (STORE) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bc_u4v, (bc_d2v){v0, v1}), wrsrc, woff, s0 * BC_TILE * 8, BC_K1_Z_AUX);
      mytr[((vidx - vbase) * 4 + g) * 17 + j] = v0 + v1;
    };
#pragma unroll
    for (int st = 0; st < NT; ++st)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int vidx = 4 * st + reg;
        put(vidx, 16 * st + 4 * reg, acc[0][st][reg], acc[1][st][reg]);
        if (++nq == 5) { flush(vbase, 5); vbase += 5; nq = 0; }
      }
    if (TL > 0) {
      put(4 * NT, NT * 16, tv[0], tv[1]);
      ++nq;
    }
    if (nq > 0) flush(vbase, nq);
    RSTAMP(2);
    grp = nxt;
  }
#ifdef BC_K1_STAMPS
  if (a.stamps && lane == 0) {
    unsigned long long* o = a.stamps + ((size_t)blockIdx.x * 8 + w) * 8;
    o[0] = ph[0]; o[1] = ph[1]; o[2] = ph[2]; o[3] = __builtin_amdgcn_s_memtime() - tstart; o[4] = tstart;
  }
#endif
  // ---- the wave's column sums: row (blockIdx.x * 8 + w) of tile_part
  asm volatile("" ::: "memory");
  double* outp = a.tile_part + ((size_t)blockIdx.x * 8 + w) * S;
  for (int s = lane; s < S; s += 64) outp[s] = mycs[s];
}


template <int MODEL, int NT, int KC, int JT, bool RAW = false, int TL = 0, bool STORE = true, typename ZT = double>
static int launch_project(bc_ctx* ctx, const ProjArgs& a, long long ntiles) {
  size_t lds = (size_t)(128 * (KC + 1) + (NT * 16 + TL) * (KC + 2)) * sizeof(double);
  if (bc_model_uses_tables<MODEL>()) lds += (size_t)bc_model_tab_doubles<MODEL>() * sizeof(double);
#ifdef BC_K1_STAMPS
  if (getenv("BC_K1_EXTRA_LDS")) lds += (size_t)atoi(getenv("BC_K1_EXTRA_LDS"));   // diagnostic: fewer blocks per CU
#endif
  if (lds > (size_t)ctx->max_lds) {
    bc_set_error("bc_project: this instantiation stages %zu bytes of LDS per block, the device allows %d", lds, ctx->max_lds);
    return BC_INVALID_ARGUMENT;
  }
  static unsigned attr_done = 0;            // per instantiation, one bit per device ordinal
  const unsigned bit = 1u << (ctx->device & 31);
  if (!(attr_done & bit) && lds > 64 * 1024) {
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_project<MODEL, NT, KC, JT, RAW, TL, STORE, ZT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_done |= bit;
  }
  hipLaunchKernelGGL((k_project<MODEL, NT, KC, JT, RAW, TL, STORE, ZT>), dim3((unsigned)ntiles), dim3(128 / (16 * JT) * 64), lds, ctx->stream, a);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

// the launch tables below name every model id: one without a case is an error, never another model's formula
static int bc_k1_unknown_model(int model) {
  bc_set_error("bc_project: internal: no kernel for model %d", model);
  return BC_INVALID_ARGUMENT;
}
static int bc_k1_no_store_free(int model) {
  bc_set_error("bc_project_colsum: model %d (a beta-gradient) has no store-free form: project and take bc_phi_colsum", model);
  return BC_INVALID_ARGUMENT;
}

template <int MODEL, bool STORE, typename ZT>
static int launch_project_nt(bc_ctx* ctx, const ProjArgs& a, long long ntiles, int ntsel) {
  if constexpr (!STORE && bc_model_store_only<MODEL>()) return bc_k1_no_store_free(MODEL);      // not instantiated
  else
  switch (ntsel) {
    case 4: return launch_project<MODEL, 4, 32, 2, false, 0, STORE, ZT>(ctx, a, ntiles);
    case 6: return launch_project<MODEL, 6, 32, 2, false, 4, STORE, ZT>(ctx, a, ntiles);      // 96 < S <= 100: 6 tiles + 1 sample quad
    case 7: return launch_project<MODEL, 7, 32, 2, false, 0, STORE, ZT>(ctx, a, ntiles);
    case 13: return launch_project<MODEL, 13, 16, 1, false, 0, STORE, ZT>(ctx, a, ntiles);
    default: return launch_project<MODEL, 16, 16, 1, false, 0, STORE, ZT>(ctx, a, ntiles);
  }
}

template <bool STORE, typename ZT>
static int launch_project_model(bc_ctx* ctx, const ProjArgs& a, long long ntiles, int model, int ntsel) {
  switch (model) {
    case BC_MODEL_LINREG_LL: return launch_project_nt<BC_MODEL_LINREG_LL, STORE, ZT>(ctx, a, ntiles, ntsel);
    case BC_MODEL_LINREG_BETA: return launch_project_nt<BC_MODEL_LINREG_BETA, STORE, ZT>(ctx, a, ntiles, ntsel);
    case BC_MODEL_LOGISTIC_LL: return launch_project_nt<BC_MODEL_LOGISTIC_LL, STORE, ZT>(ctx, a, ntiles, ntsel);
    case BC_MODEL_LOGISTIC_BETA: return launch_project_nt<BC_MODEL_LOGISTIC_BETA, STORE, ZT>(ctx, a, ntiles, ntsel);
    case BC_MODEL_GAUSS_LL: return launch_project_nt<BC_MODEL_GAUSS_LL, STORE, ZT>(ctx, a, ntiles, ntsel);
    case BC_MODEL_GAUSS_BETA: return launch_project_nt<BC_MODEL_GAUSS_BETA, STORE, ZT>(ctx, a, ntiles, ntsel);
    case BC_MODEL_GAUSS_BETA_GRAD: return launch_project_nt<BC_MODEL_GAUSS_BETA_GRAD, STORE, ZT>(ctx, a, ntiles, ntsel);
    case BC_MODEL_LINREG_BETA_GRAD: return launch_project_nt<BC_MODEL_LINREG_BETA_GRAD, STORE, ZT>(ctx, a, ntiles, ntsel);
    case BC_MODEL_LOGISTIC_BETA_GRAD: return launch_project_nt<BC_MODEL_LOGISTIC_BETA_GRAD, STORE, ZT>(ctx, a, ntiles, ntsel);
    default: return bc_k1_unknown_model(model);
  }
}

// ---- Theta-resident kernel: one 512-thread block per CU, LDS = Theta + per-wave column sums + transposition scratch (+ tables)
static size_t project_r_lds_bytes(int nr, int dk, int table_doubles) {
  return ((size_t)nr * (dk + 2) + 8 * (size_t)nr + 8 * (5 * 4 * 17) + (size_t)table_doubles) * sizeof(double);
}

template <int MODEL, int NT, int TL, bool STORE, typename ZT>
static int launch_project_r(bc_ctx* ctx, const ProjArgs& a, int grid) {
  const size_t lds = project_r_lds_bytes(NT * 16 + TL, a.dk, bc_model_tab_doubles<MODEL>());
  static unsigned attr_done = 0;
  const unsigned bit = 1u << (ctx->device & 31);
  if (!(attr_done & bit)) {
    BC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_project_r<MODEL, NT, TL, STORE, ZT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, ctx->max_lds));
    attr_done |= bit;
  }
  hipLaunchKernelGGL((k_project_r<MODEL, NT, TL, STORE, ZT>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, a);
  BC_HIP(hipGetLastError());
  return BC_OK;
}

template <int MODEL, bool STORE, typename ZT>
static int launch_project_r_nt(bc_ctx* ctx, const ProjArgs& a, int grid, int ntsel) {
  if constexpr (!STORE && bc_model_store_only<MODEL>()) return bc_k1_no_store_free(MODEL);      // not instantiated
  else
  switch (ntsel) {
    case 4: return launch_project_r<MODEL, 4, 0, STORE, ZT>(ctx, a, grid);
    case 6: return launch_project_r<MODEL, 6, 4, STORE, ZT>(ctx, a, grid);
    default:
      if constexpr (bc_model_has_np_exp<MODEL>() || bc_model_store_only<MODEL>()) {      // not instantiated (would spill), never selected (project_r_grid)
        bc_set_error("bc_project: internal: no resident kernel for this model at S in 101..112");
        return BC_INVALID_ARGUMENT;
      } else {
        return launch_project_r<MODEL, 7, 0, STORE, ZT>(ctx, a, grid);
      }
  }
}

template <bool STORE, typename ZT>
static int launch_project_r_model(bc_ctx* ctx, const ProjArgs& a, int grid, int model, int ntsel) {
  switch (model) {
    case BC_MODEL_LINREG_LL: return launch_project_r_nt<BC_MODEL_LINREG_LL, STORE, ZT>(ctx, a, grid, ntsel);
    case BC_MODEL_LINREG_BETA: return launch_project_r_nt<BC_MODEL_LINREG_BETA, STORE, ZT>(ctx, a, grid, ntsel);
    case BC_MODEL_LOGISTIC_LL: return launch_project_r_nt<BC_MODEL_LOGISTIC_LL, STORE, ZT>(ctx, a, grid, ntsel);
    case BC_MODEL_LOGISTIC_BETA: return launch_project_r_nt<BC_MODEL_LOGISTIC_BETA, STORE, ZT>(ctx, a, grid, ntsel);
    case BC_MODEL_GAUSS_LL: return launch_project_r_nt<BC_MODEL_GAUSS_LL, STORE, ZT>(ctx, a, grid, ntsel);
    case BC_MODEL_GAUSS_BETA: return launch_project_r_nt<BC_MODEL_GAUSS_BETA, STORE, ZT>(ctx, a, grid, ntsel);
    case BC_MODEL_GAUSS_BETA_GRAD: return launch_project_r_nt<BC_MODEL_GAUSS_BETA_GRAD, STORE, ZT>(ctx, a, grid, ntsel);
    case BC_MODEL_LINREG_BETA_GRAD: return launch_project_r_nt<BC_MODEL_LINREG_BETA_GRAD, STORE, ZT>(ctx, a, grid, ntsel);
    case BC_MODEL_LOGISTIC_BETA_GRAD: return launch_project_r_nt<BC_MODEL_LOGISTIC_BETA_GRAD, STORE, ZT>(ctx, a, grid, ntsel);
    default: return bc_k1_unknown_model(model);
  }
}

template <typename ZT>
static int launch_project_raw(bc_ctx* ctx, const ProjArgs& a, long long ntiles, int model) {
  switch (model) {
    case BC_MODEL_LINREG_LL: return launch_project<BC_MODEL_LINREG_LL, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    case BC_MODEL_LINREG_BETA: return launch_project<BC_MODEL_LINREG_BETA, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    case BC_MODEL_LOGISTIC_LL: return launch_project<BC_MODEL_LOGISTIC_LL, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    case BC_MODEL_LOGISTIC_BETA: return launch_project<BC_MODEL_LOGISTIC_BETA, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    case BC_MODEL_GAUSS_LL: return launch_project<BC_MODEL_GAUSS_LL, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    case BC_MODEL_GAUSS_BETA: return launch_project<BC_MODEL_GAUSS_BETA, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    case BC_MODEL_GAUSS_BETA_GRAD: return launch_project<BC_MODEL_GAUSS_BETA_GRAD, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    case BC_MODEL_LINREG_BETA_GRAD: return launch_project<BC_MODEL_LINREG_BETA_GRAD, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    case BC_MODEL_LOGISTIC_BETA_GRAD: return launch_project<BC_MODEL_LOGISTIC_BETA_GRAD, 16, 16, 1, true, 0, true, ZT>(ctx, a, ntiles);
    default: return bc_k1_unknown_model(model);
  }
}


// which kernel a launch wants (the host side of bc_project.hip decides), and the two tables it is looked up in
enum { BC_K1_STAGED_FULL = 0, BC_K1_STAGED_COLSUM = 1, BC_K1_STAGED_RAW = 2, BC_K1_RESIDENT_FULL = 3, BC_K1_RESIDENT_COLSUM = 4 };

// count: 128-row tiles (staged kernels) or the grid (resident kernel)
template <typename ZT>
static int bc_k1_launch(bc_ctx* ctx, const ProjArgs& a, int kind, long long count, int model, int ntsel) {
  switch (kind) {
    case BC_K1_STAGED_FULL: return launch_project_model<true, ZT>(ctx, a, count, model, ntsel);
    case BC_K1_STAGED_COLSUM: return launch_project_model<false, ZT>(ctx, a, count, model, ntsel);
    case BC_K1_STAGED_RAW: return launch_project_raw<ZT>(ctx, a, count, model);
    case BC_K1_RESIDENT_FULL: return launch_project_r_model<true, ZT>(ctx, a, (int)count, model, ntsel);
    default: return launch_project_r_model<false, ZT>(ctx, a, (int)count, model, ntsel);
  }
}
int bc_k1_launch_f32(bc_ctx* ctx, const ProjArgs& a, int kind, long long count, int model, int ntsel);   // bc_project_f32.hip
