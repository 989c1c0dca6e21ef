/*
 * beta_cores_laplace.h -- C ABI of the full-data logistic Laplace pass (K5 + K4) of libbeta_cores.
 *
 * An extension of include/beta_cores.h (same library, same conventions: int status, bc_last_error(), host pointers
 * borrowed for the call, IEEE double); kept in a header of its own so that the core ABI of beta_cores.h stays as it is.
 * Bound in Python by beta_cores_amd/_native.py (_EXT_SIGNATURES).
 */
#ifndef BETA_CORES_LAPLACE_H
#define BETA_CORES_LAPLACE_H

#include "beta_cores.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- K5: the logistic log-likelihood of resident rows (full-data Laplace, util/opt.py:10-33) ---------- */
/* rows z = y*x (width D <= 1024, no y column, model_lr.py:29) at theta (host, D doubles), local rows only (the host adds the
 * N(0, I) prior and sums ranks): value = sum_n w_n ll_n, out_grad = its gradient (D), and optionally out_diag = the diagonal
 * (D) and out_hess = the full matrix (D x D row-major) of  sum_n w_n c_n z_n z_n^T  = minus its Hessian, with
 * m = -z.theta, ll = -log1p(e^m) (-m for m >= 100), p = e^m / (1 + e^m) (1 for m >= 100), c = p (1 - p) (0 for m >= 100).
 * w: a bc_data of n_rows x 1 (uploaded once per fit) or NULL = all ones.  NULL out_diag / out_hess skip that part.
 * Bit-reproducible run to run (fixed-order reductions); the Hessian is K4 over the curvature weights w_n c_n. */
int bc_logistic_newton_pass(bc_ctx* ctx, const bc_data* data, const bc_data* w, const double* theta, double* out_value,
                            double* out_grad, double* out_diag, double* out_hess);

#ifdef __cplusplus
}
#endif
#endif /* BETA_CORES_LAPLACE_H */
