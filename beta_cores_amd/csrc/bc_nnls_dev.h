// Non-negative least squares on the cached columns of the active list, for one thread block.
//
//   min ||sum_j x_j a_j - b||  s.t. x >= 0     over the list entries (a_j = cached fp64 column j, at most BC_NNLS_MAXP)
//
// is solved from the normal equations: G[i][j] = a_i . a_j and c[i] = a_i . b are kept in device memory next to the
// list (bc_nnls_gram_rows extends them when a column is appended), and bc_nnls_solve runs Lawson-Hanson's active-set
// method on (G, c) -- warm-started from the entries that carry a positive weight -- with a Cholesky factor of G_PP
// packed in LDS.  This is orthopursuit.py:37-41 / snnls.py:82-97 (scipy.optimize.nnls on A[:, active]) without the host:
// the result is the NNLS minimiser, not SciPy's bits.
//
// Every loop is written as "element i = tid, tid + nt, ..." with barriers between phases and every reduction is a
// fixed-order scan by thread 0, so (a) a run is bit-reproducible and (b) the same text compiles for the host with
// tid = 0, nt = 1 and an empty barrier (tests/nnls_host_model.cpp checks the algorithm against SciPy without a GPU).
#pragma once
#include <math.h>

#define BC_NNLS_MAXP 128                                              // longest list a refit accepts
#define BC_NNLS_LTRI (BC_NNLS_MAXP * (BC_NNLS_MAXP + 1) / 2)          // packed lower triangle: 66 KB
#define BC_NNLS_NVEC 7                                                // x, z, y, t, c, d, g
#define BC_NNLS_WS_DOUBLES (BC_NNLS_LTRI + BC_NNLS_NVEC * BC_NNLS_MAXP + 4 + (2 * BC_NNLS_MAXP + 8) / 2)      // 74.3 KB of LDS

#ifndef BC_NNLS_FN
#define BC_NNLS_FN __device__
#define BC_NNLS_TID ((int)threadIdx.x)
#define BC_NNLS_NT ((int)blockDim.x)
#define BC_NNLS_SYNC() __syncthreads()
#endif

struct NnlsWs {
  double* L;      // packed factor, by POSITION in the passive order: L[i][k] at i(i+1)/2 + k
  double* x;      // current iterate, by list slot
  double* z;      // least-squares solution on the passive set, by position
  double* y;      // L^-1 c_P, by position (kept across rounds: appending a column adds one element)
  double* t;      // scratch, by position
  double* c;      // LDS copy of c, by slot
  double* d;      // diag(G), by slot
  double* g;      // dual c - G x on the zero set, by slot
  double* sc;     // [4] block-wide scalars
  int* ord;       // position -> slot
  int* st;        // slot -> 0 zero set, 1 passive set, 2 barred for the rest of this refit
  int* ctl;       // [8] block-wide integers
};

BC_NNLS_FN inline NnlsWs bc_nnls_ws(double* base) {
  NnlsWs W;
  W.L = base;
  W.x = W.L + BC_NNLS_LTRI;
  W.z = W.x + BC_NNLS_MAXP;
  W.y = W.z + BC_NNLS_MAXP;
  W.t = W.y + BC_NNLS_MAXP;
  W.c = W.t + BC_NNLS_MAXP;
  W.d = W.c + BC_NNLS_MAXP;
  W.g = W.d + BC_NNLS_MAXP;
  W.sc = W.g + BC_NNLS_MAXP;
  W.ord = reinterpret_cast<int*>(W.sc + 4);
  W.st = W.ord + BC_NNLS_MAXP;
  W.ctl = W.st + BC_NNLS_MAXP;
  return W;
}

BC_NNLS_FN inline int bc_nnls_tri(int i, int k) { return i * (i + 1) / 2 + k; }

// one fixed fma order for every Gram entry, whoever computes it
BC_NNLS_FN inline double bc_nnls_dot(const double* a, const double* b, int s) {
  double acc = 0.0;
  for (int k = 0; k < s; ++k) acc = fma(a[k], b[k], acc);
  return acc;
}

// G[i][j] = G[j][i] = cols[i] . cols[j] for rows i in [r0, r1) against every list entry j < n, and c[i] = cols[i] . b.
// (a pair inside [r0, r1) is computed once, by its lower-triangle owner)
BC_NNLS_FN inline void bc_nnls_gram_rows(const double* cols, int s, const double* b, double* G, double* c, int n, int r0, int r1) {
  const int tid = BC_NNLS_TID, nt = BC_NNLS_NT;
  const int total = (r1 - r0) * n;
  for (int e = tid; e < total; e += nt) {
    const int i = r0 + e / n, j = e - (e / n) * n;
    if (j > i && j >= r0 && j < r1) continue;
    const double v = bc_nnls_dot(cols + (size_t)i * s, cols + (size_t)j * s, s);
    G[(size_t)i * BC_NNLS_MAXP + j] = v;
    G[(size_t)j * BC_NNLS_MAXP + i] = v;
    if (j == i) c[i] = bc_nnls_dot(cols + (size_t)i * s, b, s);
  }
  BC_NNLS_SYNC();
}

// v <- L^-1 v for the leading p x p block (column-oriented forward substitution, one barrier per column)
BC_NNLS_FN inline void bc_nnls_forward(const double* L, double* v, int p) {
  const int tid = BC_NNLS_TID, nt = BC_NNLS_NT;
  for (int k = 0; k < p; ++k) {
    const double vk = v[k] / L[bc_nnls_tri(k, k)];
    for (int i = k + 1 + tid; i < p; i += nt) v[i] = fma(-L[bc_nnls_tri(i, k)], vk, v[i]);
    BC_NNLS_SYNC();
    if (tid == 0) v[k] = vk;
  }
  BC_NNLS_SYNC();
}

// z <- L^-T y
BC_NNLS_FN inline void bc_nnls_backward(const double* L, const double* y, double* z, int p) {
  const int tid = BC_NNLS_TID, nt = BC_NNLS_NT;
  for (int i = tid; i < p; i += nt) z[i] = y[i];
  BC_NNLS_SYNC();
  for (int k = p - 1; k >= 0; --k) {
    const double zk = z[k] / L[bc_nnls_tri(k, k)];
    for (int i = tid; i < k; i += nt) z[i] = fma(-L[bc_nnls_tri(k, i)], zk, z[i]);
    BC_NNLS_SYNC();
    if (tid == 0) z[k] = zk;
  }
  BC_NNLS_SYNC();
}

// Cholesky of G_PP for the passive order W.ord[0..p) into W.L, then W.y = L^-1 c_P.  Returns 1 (block-uniform) when a
// pivot is not above rel * (k + 1) * G_kk: the set is numerically rank deficient.
BC_NNLS_FN inline int bc_nnls_factor(const double* G, NnlsWs& W, int p, double rel) {
  const int tid = BC_NNLS_TID, nt = BC_NNLS_NT;
  for (int e = tid; e < p * BC_NNLS_MAXP; e += nt) {
    const int i = e / BC_NNLS_MAXP, k = e - i * BC_NNLS_MAXP;
    if (k <= i) W.L[bc_nnls_tri(i, k)] = G[(size_t)W.ord[i] * BC_NNLS_MAXP + W.ord[k]];
  }
  for (int i = tid; i < p; i += nt) W.y[i] = W.c[W.ord[i]];
  BC_NNLS_SYNC();
  for (int k = 0; k < p; ++k) {
    // left-looking: thread i finishes element (i, k) from the finished columns < k
    for (int i = k + tid; i < p; i += nt) {
      double sum = W.L[bc_nnls_tri(i, k)];
      const double* ri = W.L + bc_nnls_tri(i, 0);
      const double* rk = W.L + bc_nnls_tri(k, 0);
      for (int m = 0; m < k; ++m) sum = fma(-ri[m], rk[m], sum);
      W.t[i] = sum;
    }
    BC_NNLS_SYNC();
    const double piv = W.t[k];
    if (!(piv > rel * (double)(k + 1) * W.d[W.ord[k]])) return 1;
    const double dd = sqrt(piv);
    for (int i = k + tid; i < p; i += nt) W.L[bc_nnls_tri(i, k)] = (i == k) ? dd : W.t[i] / dd;
    BC_NNLS_SYNC();
  }
  bc_nnls_forward(W.L, W.y, p);
  return 0;
}

// Append list slot j as row p of the factor (it enters LAST in the order).  Returns 0 (block-uniform) when its pivot is
// not above the relative floor: the column is numerically dependent on the passive set and nothing was changed.
BC_NNLS_FN inline int bc_nnls_append(const double* G, NnlsWs& W, int p, int j, double rel) {
  const int tid = BC_NNLS_TID, nt = BC_NNLS_NT;
  for (int i = tid; i < p; i += nt) W.t[i] = G[(size_t)j * BC_NNLS_MAXP + W.ord[i]];
  BC_NNLS_SYNC();
  bc_nnls_forward(W.L, W.t, p);
  if (tid == 0) {
    double piv = W.d[j], yc = W.c[j];
    for (int m = 0; m < p; ++m) {
      piv = fma(-W.t[m], W.t[m], piv);
      yc = fma(-W.t[m], W.y[m], yc);
    }
    const int ok = (piv > rel * (double)(p + 1) * W.d[j]) ? 1 : 0;
    if (ok) {
      const double dd = sqrt(piv);
      W.L[bc_nnls_tri(p, p)] = dd;
      W.y[p] = yc / dd;
      W.ord[p] = j;
      W.st[j] = 1;
    } else {
      W.st[j] = 2;
    }
    W.ctl[1] = ok;
  }
  BC_NNLS_SYNC();
  const int ok = W.ctl[1];
  if (ok)
    for (int i = tid; i < p; i += nt) W.L[bc_nnls_tri(p, i)] = W.t[i];
  BC_NNLS_SYNC();
  return ok;
}

// Lawson-Hanson on (G, c) for the n <= BC_NNLS_MAXP list entries.
//   val      in: the current weights (the passive set starts as {val > 0}, x = val); out, ONLY on success: the minimiser,
//            entries off its support exactly 0.0
//   enter    a slot that may enter although its weight is 0 (the picked column of an OMP step), or -1
//   all      != 0: every zero-weight slot may enter (NNLS over the whole list); 0: only `enter` (the reference refits
//            A[:, w > 0] -- a column whose weight an earlier refit left at 0 is not part of the problem)
//   stats    global {refits, factor-and-solve rounds, rejected columns}, updated by thread 0
// Returns 0, or 1 (block-uniform) when the warm-start set does not factor or more than 3n outer rounds did not converge.
BC_NNLS_FN inline int bc_nnls_solve(const double* G, const double* cg, int n, double* val, int enter, int all, double bnorm,
                                    NnlsWs W, long long* stats) {
  const int tid = BC_NNLS_TID, nt = BC_NNLS_NT;
  const double rel = 64. * 2.220446049250313e-16;
  for (int j = tid; j < n; j += nt) {
    const double v = val[j];
    const bool pos = v > 0.;
    W.st[j] = pos ? 1 : ((all || j == enter) ? 0 : 2);
    W.x[j] = pos ? v : 0.;
    W.c[j] = cg[j];
    W.d[j] = G[(size_t)j * BC_NNLS_MAXP + j];
  }
  BC_NNLS_SYNC();
  if (tid == 0) {
    int q = 0;
    for (int j = 0; j < n; ++j)
      if (W.st[j] == 1) W.ord[q++] = j;
    W.ctl[0] = q;
  }
  BC_NNLS_SYNC();
  int p = W.ctl[0];
  bool refactor = true, do_inner = true;
  int entered = 0;                 // the last position holds a column that entered in this round
  int solves = 0, rejected = 0, status = 0;
  for (int outer = 0;; ++outer) {
    while (do_inner && p > 0) {
      if (refactor) {
        if (bc_nnls_factor(G, W, p, rel)) { status = 1; break; }
        refactor = false;
      }
      bc_nnls_backward(W.L, W.y, W.z, p);
      ++solves;
      if (entered && !(W.z[p - 1] > 0.)) {
        // Lawson-Hanson's rejection: the entering column's own weight is not positive.  Put it back and bar it; x is
        // still the solution on the set without it, and the leading rows of the factor are that set's factor.
        BC_NNLS_SYNC();
        if (tid == 0) W.st[W.ord[p - 1]] = 2;
        --p;
        ++rejected;
        entered = 0;
        BC_NNLS_SYNC();
        break;
      }
      entered = 0;
      if (tid == 0) {
        double amin = INFINITY;
        int kmin = -1;
        for (int k = 0; k < p; ++k) {
          if (!(W.z[k] > 0.)) {
            const double xk = W.x[W.ord[k]];
            const double a = xk / (xk - W.z[k]);
            if (kmin < 0 || a < amin) { amin = a; kmin = k; }
          }
        }
        W.ctl[2] = kmin;
        W.sc[0] = amin;
      }
      BC_NNLS_SYNC();
      const int kmin = W.ctl[2];
      if (kmin < 0) {
        for (int k = tid; k < p; k += nt) W.x[W.ord[k]] = W.z[k];
        BC_NNLS_SYNC();
        break;
      }
      const double alpha = W.sc[0];
      for (int k = tid; k < p; k += nt) {
        const int j = W.ord[k];
        double xn = W.x[j] + alpha * (W.z[k] - W.x[j]);
        if (k == kmin || !(xn > 0.)) {
          xn = 0.;
          W.st[j] = 0;
        }
        W.x[j] = xn;
      }
      BC_NNLS_SYNC();
      if (tid == 0) {
        int q = 0;
        for (int k = 0; k < p; ++k) {
          const int j = W.ord[k];
          if (W.st[j] == 1) W.ord[q++] = j;
        }
        W.ctl[0] = q;
      }
      BC_NNLS_SYNC();
      p = W.ctl[0];
      refactor = true;
    }
    if (status) break;
    if (outer > 3 * n) { status = 1; break; }
    // dual on the zero set; the largest entry enters (ties: lowest slot) unless it is at rounding level
    for (int j = tid; j < n; j += nt) {
      if (W.st[j] != 0) continue;
      double acc = W.c[j];
      const double* gr = G + (size_t)j * BC_NNLS_MAXP;
      for (int k = 0; k < p; ++k) acc = fma(-gr[W.ord[k]], W.x[W.ord[k]], acc);
      W.g[j] = acc;
    }
    BC_NNLS_SYNC();
    if (tid == 0) {
      int best = -1;
      for (int j = 0; j < n; ++j)
        if (W.st[j] == 0 && (best < 0 || W.g[j] > W.g[best])) best = j;
      if (best >= 0 && !(W.g[best] > rel * sqrt(W.d[best]) * bnorm)) best = -1;
      W.ctl[3] = best;
    }
    BC_NNLS_SYNC();
    const int best = W.ctl[3];
    if (best < 0) break;
    if (bc_nnls_append(G, W, p, best, rel)) {
      ++p;
      entered = 1;
      do_inner = true;
    } else {
      ++rejected;
      do_inner = false;
    }
  }
  if (!status)
    for (int j = tid; j < n; j += nt) val[j] = W.x[j];
  if (tid == 0 && stats) {
    stats[0] += 1;
    stats[1] += solves;
    stats[2] += rejected;
  }
  BC_NNLS_SYNC();
  return status;
}
