// The reflector of gprhip_observe's triangular-pentagonal QR update (observe.hip), in one text for the device kernels and
// for tests/cpp/tp_reflect_check.cpp, which runs it in double against long double on the CPU (as refine_step.h is shared).
//
// [R~' | b'] is the triangular factor of [R~ | b] stacked on [W | eta] (k rows).  Pivot column j sees x = (alpha; w) with
// alpha = R~_jj > 0 and w = W[:, j] as the earlier reflectors left it.  With sigma = |w|^2,
//   mu = sqrt(alpha^2 + sigma)           the new diagonal entry, positive
//   v  = (v1; w),  v1 = alpha - mu = -sigma / (alpha + mu)        (no cancellation)
//   H  = I - beta v v^T,  beta = 2 / (v^T v) = -1 / (mu v1),      H x = (mu; 0)
// sigma == 0 is the identity (v1 = beta = 0): every padded column, where R~ holds its identity block and W is zero.
// A column c right of j (or the b | eta column) with pivot-row entry rho = R~_jc and entries w_c of W:
//   t = beta (v1 rho + w . w_c),   rho' = rho - t v1,   w_c' = w_c - t w
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define TP_HD __host__ __device__
#else
#define TP_HD
#endif

namespace gprhip {

TP_HD inline double tp_sqrt(double x) { return ::sqrt(x); }
TP_HD inline double tp_log1p(double x) { return ::log1p(x); }
TP_HD inline double tp_log(double x) { return ::log(x); }
#if !defined(__HIP_DEVICE_COMPILE__)
inline long double tp_sqrt(long double x) { return ::sqrtl(x); }
inline long double tp_log1p(long double x) { return ::log1pl(x); }
inline long double tp_log(long double x) { return ::logl(x); }
#endif

// the reflector of pivot column j from alpha = R~_jj and sigma = |W[:, j]|^2; returns log(mu / alpha), the column's share of
// the log-determinant ratio
template <typename T>
TP_HD inline T tp_reflector(T alpha, T sigma, T& mu, T& v1, T& beta) {
  // sigma <= 2^-120 alpha^2 is the identity as well: mu rounds to alpha in any format up to 113 bits, the reflector would
  // move a column by at most 2^-60 of its norm, and v1, beta leave the normal range (beta = 2 / sigma overflows) for the
  // entries of W that a squared-exponential kernel gives far from every inducing point (1e-160 and below)
  // (alpha^2 itself underflows below alpha ~ 1e-154, where the threshold is 0 and only sigma == 0 is skipped; R~_jj >= 1
  //  in this library, B~ = I + ...)
  if (!(sigma > T(7.5231638452626401e-37) * alpha * alpha)) {
    mu = alpha;
    v1 = T(0);
    beta = T(0);
    return T(0);
  }
  mu = tp_sqrt(alpha * alpha + sigma);
  v1 = -sigma / (alpha + mu);
  beta = T(-1) / (mu * v1);
  // (log1p keeps the ratio's relative accuracy where sigma is small against alpha^2; a tiny pivot takes the plain form)
  const T q = mu / alpha;
  return q < T(2) ? T(0.5) * tp_log1p(sigma / (alpha * alpha)) : tp_log(q);
}

// t of one column from its pivot-row entry and the dot product w . w_c
template <typename T>
TP_HD inline T tp_factor(T v1, T beta, T rho, T dot) {
  return beta * (v1 * rho + dot);
}

// the whole application to one column: u = the reflector's w (stride us), w = the column's entries (stride ws), k of each
template <typename T>
TP_HD inline void tp_apply_column(int k, T v1, T beta, const T* u, long us, T& rho, T* w, long ws) {
  if (beta == T(0)) return;
  T dot = T(0);
  for (int i = 0; i < k; ++i) dot += u[i * us] * w[i * ws];
  const T t = tp_factor(v1, beta, rho, dot);
  rho -= t * v1;
  for (int i = 0; i < k; ++i) w[i * ws] -= t * u[i * us];
}

// The update as the launches order it, in blocks of nb columns: per block row the reflectors of its nb pivot columns are
// generated and applied inside the block (the b | eta column rides with the LAST block), then applied to every column right of
// the block and to b | eta.  R: row-major mp x mp upper factor (entries on and above the diagonal are read and written), W:
// row-major k x mp, overwritten (column j ends as the w of reflector j); b (mp) / eta (k) may be null.  logdet (may be null)
// receives sum_j log(R'_jj / R_jj), summed in column order.
template <typename T>
inline void tp_update_blocked(int mp, int k, int nb, T* R, T* W, T* b, T* eta, T* logdet) {
  T ld = T(0);
  T* v1 = new T[nb];
  T* beta = new T[nb];
  for (int j0 = 0; j0 < mp; j0 += nb) {
    const int j1 = j0 + nb < mp ? j0 + nb : mp;
    const bool last = j1 == mp;
    for (int j = j0; j < j1; ++j) {  // the diagonal launch
      T sigma = T(0);
      for (int i = 0; i < k; ++i) sigma += W[(long)i * mp + j] * W[(long)i * mp + j];
      T mu;
      ld += tp_reflector(R[(long)j * mp + j], sigma, mu, v1[j - j0], beta[j - j0]);
      R[(long)j * mp + j] = mu;
      for (int c = j + 1; c < j1; ++c)
        tp_apply_column(k, v1[j - j0], beta[j - j0], W + j, mp, R[(long)j * mp + c], W + c, mp);
      if (last && b) tp_apply_column(k, v1[j - j0], beta[j - j0], W + j, mp, b[j], eta, 1);
    }
    if (last) break;
    for (int c = j1; c < mp; ++c)  // the trailing launch: one lane per column
      for (int j = j0; j < j1; ++j) tp_apply_column(k, v1[j - j0], beta[j - j0], W + j, mp, R[(long)j * mp + c], W + c, mp);
    if (b)
      for (int j = j0; j < j1; ++j) tp_apply_column(k, v1[j - j0], beta[j - j0], W + j, mp, b[j], eta, 1);
  }
  if (logdet) *logdet = ld;
  delete[] v1;
  delete[] beta;
}

}  // namespace gprhip
