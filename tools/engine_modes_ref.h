// Host side of tools/engine_modes_check.hip: the description of one engine launch (Spec), the operand fill with its
// poison, the long-double reference of the launch's full formula and the componentwise bound.  Plain C++ (no HIP), so that
// tests/cpp/engine_modes_selftest.cpp can turn the same code on an emulated launch on the CPU.
//
// Bound.  For an entry whose reference formula is a sum of terms t_1 .. t_n (K products, the beta / epilogue terms),
//   |got - ref| <= (K + c) u S,   S = sum |t_i|,   u = 2^-53 (fp64) / 2^-24 (fp32),
// holds to first order for ANY summation order (each product carries one rounding, every term passes through fewer than
// K additions, the epilogue adds c roundings), so no constant here is measured.  c per epilogue, counted from
// mfma_gemm.hip's epilogue() and gemm_body() (one of each is the second-order remainder of the first-order bound):
//   plain store, alpha * acc                                   1 + 1            = 2
//   per-k weights (TN _w / _ws: the weight multiplies A)       + 1
//   alpha * acc + beta * old                                   3 + 1            = 4
//   nt_xt: ra*acc - rb*M - rc*cv, ra rb rc cv rounded to T     5 + 4 + 1        = 10
//   nt_sx: ra*acc - rc*cv, ra rc cv rounded to T               3 + 3 + 1        = 7
//   two-phase nt_sx: f = -num/den (divide, round to T), acc*f  7 + 3            = 10
// Row partials are checked against the device's own C entries (which the entry check has just bounded): 64 squares or
// products summed in double, (64 + 2) 2^-53 of the sum of their absolute values.  Column sums: K products of T values,
// (K + 2) u sum |A w|.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

namespace emc {

constexpr int TILE_ = 128;
enum { NN = 0, NT = 1, TN = 2 };                                                        // GemmOp
enum { T_NONE = 0, T_KHI_BN = 1, T_KLO_BN = 2, T_KLO_BM = 3, T_KLO_MAX = 4, T_KHI_MIN = 5, T_BAND = 6 };  // GemmTri
enum { E_PLAIN = 0, E_XT = 1, E_SX = 2 };

template <typename T> struct Bits;
template <> struct Bits<double> { typedef uint64_t U; static constexpr U POISON = 0x7ff8dead0000beefull; static constexpr double u = 1.0 / 9007199254740992.0; };
template <> struct Bits<float> { typedef uint32_t U; static constexpr U POISON = 0x7fc0dead; static constexpr double u = 1.0 / 16777216.0; };
template <typename T> inline T poison() { typename Bits<T>::U b = Bits<T>::POISON; T v; std::memcpy(&v, &b, sizeof v); return v; }
template <typename T> inline bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Win { int arena = -1; int64_t off = 0, ld = 0; };  // a matrix inside arena `arena`: element (r, c) at off + r*ld + c

template <typename T>
struct Spec {
  std::string name;
  int op = NN, M = 0, N = 0, K = 0;
  std::vector<int> Ms;  // launches that differ in M only share operands and one reference pass (empty: {M})
  Win A, B, C, A2, B2, EM;
  double alpha = 1.0, beta = 0.0;
  int tri = T_NONE, upper = 0, order = 0;
  int nbatch = 1; int64_t batch_a = 0, batch_b = 0, batch_c = 0;
  int kslices = 1; int64_t slice_stride = 0;
  bool weights = false, colsums = false, same_ab = false;
  int epi = E_PLAIN; bool two_phase = false, rp_sumsq = false, rp_dot = false;
  // what launch_gemm's plan says for this launch (the harness fills them from gemm_plan; the self-test by hand)
  int syrk = 0, dslices = 0;
  // expectations on the plan, -1 = not asserted; tail: 1 = tail_panels > 0, 0 = none
  int x_kernel = -1, x_ipw = -1, x_tail = -1, x_desc2 = -1, x_syrk = -1, x_dslices = -1, x_order = -1;
  std::vector<std::vector<T>> ar;  // arenas as they are in front of the launch
  std::vector<T> sk, csw;          // per-k weights, column-sum weights
  std::vector<double> ra, rb, rc, cv, num, den, rpvec;
};

// k-range [lo, hi) of output tile (bm, bn): the union of its k-slices (mfma_gemm.hip, tile_at)
template <typename T>
inline void k_range(const Spec<T>& s, int bm, int bn, int& lo, int& hi) {
  lo = 0; hi = s.K;
  switch (s.tri) {
    case T_KHI_BN: hi = std::min(hi, (bn + 1) * TILE_); break;
    case T_KLO_BN: lo = std::max(lo, bn * TILE_); break;
    case T_KLO_BM: lo = std::max(lo, bm * TILE_); break;
    case T_KLO_MAX: lo = std::max(lo, std::max(bm, bn) * TILE_); break;
    case T_KHI_MIN: hi = std::min(hi, (std::min(bm, bn) + 1) * TILE_); break;
    case T_BAND: lo = std::max(lo, bm * TILE_); hi = std::min(hi, (bn + 1) * TILE_); break;
    default: break;
  }
  if (hi < lo) hi = lo;
}
template <typename T> inline bool tile_runs(const Spec<T>& s, int bm, int bn) { return !s.upper || bm <= bn; }
// k-slices that store tile (bm, bn)
template <typename T> inline int slices_of(const Spec<T>& s, int bm, int bn) {
  if (s.kslices <= 1) return 1;
  return (s.syrk && s.dslices > 0 && bm == bn) ? s.dslices : s.kslices;
}
// entries of a computed tile the launch does not compute: strictly-lower 16 x 16 sub-tiles of the diagonal tiles of a
// SYRK-shaped launch (stored as +0, see check)
template <typename T> inline bool entry_stored(const Spec<T>& s, int i, int j) {
  return !(s.syrk && i / TILE_ == j / TILE_ && j / 16 < i / 16);
}

template <typename T> inline int64_t ia(const Spec<T>& s, const Win& w, int i, int k) { return w.off + (s.op == TN ? (int64_t)k * w.ld + i : (int64_t)i * w.ld + k); }
template <typename T> inline int64_t ib(const Spec<T>& s, const Win& w, int k, int j) { return w.off + (s.op == NT ? (int64_t)j * w.ld + k : (int64_t)k * w.ld + j); }

struct Rng {
  uint64_t x;
  explicit Rng(uint64_t seed) : x(seed * 0x9E3779B97F4A7C15ull + 1) {}
  double next() {  // uniform in [-1, 1) with a full fp64 mantissa (24-bit values would make every fp64 product and sum exact)
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return (double)(x >> 11) / 4503599627370496.0 - 1.0;
  }
};

// Fill the operand windows of every problem of the launch: 128-blocks some computed tile reads get random data (with real
// zeros where the triangular structure of the policy has them), every other byte of every arena stays poison -- the
// blocks the policy skips included.  C gets data on its computed, stored entries when beta != 0.
template <typename T>
void fill_operands(Spec<T>& s, uint64_t seed) {
  Rng rng(seed);
  const int M = s.Ms.empty() ? s.M : *std::max_element(s.Ms.begin(), s.Ms.end());
  const int nbm = M / TILE_, nbn = s.N / TILE_, nkb = (s.K + TILE_ - 1) / TILE_;
  std::vector<char> needA((size_t)nbm * nkb, 0), needB((size_t)nkb * nbn, 0);
  for (int bm = 0; bm < nbm; ++bm)
    for (int bn = 0; bn < nbn; ++bn) {
      if (!tile_runs(s, bm, bn)) continue;
      int lo, hi;
      k_range(s, bm, bn, lo, hi);
      for (int kb = lo / TILE_; kb * TILE_ < hi; ++kb) needA[(size_t)bm * nkb + kb] = needB[(size_t)kb * nbn + bn] = 1;
    }
  const bool azero = s.tri == T_KLO_BM || s.tri == T_KLO_MAX || s.tri == T_BAND;  // A[i][k] = 0 for k < i
  for (int b = 0; b < s.nbatch; ++b) {
    auto fillA = [&](Win w) {
      if (w.arena < 0) return;
      w.off += b * s.batch_a;
      for (int i = 0; i < M; ++i)
        for (int k = 0; k < s.K; ++k)
          if (needA[(size_t)(i / TILE_) * nkb + k / TILE_]) s.ar[w.arena][ia(s, w, i, k)] = (azero && k < i) ? (T)0 : (T)rng.next();
    };
    auto fillB = [&](Win w) {
      if (w.arena < 0) return;
      w.off += b * s.batch_b;
      for (int k = 0; k < s.K; ++k)
        for (int j = 0; j < s.N; ++j)
          if (needB[(size_t)(k / TILE_) * nbn + j / TILE_]) {
            bool z = false;
            if (s.tri == T_KHI_BN || s.tri == T_BAND || s.tri == T_KHI_MIN) z = k > j;
            if (s.tri == T_KLO_BN || s.tri == T_KLO_MAX) z = k < j;
            s.ar[w.arena][ib(s, w, k, j)] = z ? (T)0 : (T)rng.next();
          }
    };
    fillA(s.A); fillA(s.A2);
    if (!s.same_ab) { fillB(s.B); fillB(s.B2); }
    if (s.beta != 0.0 || s.epi == E_XT) {
      Win c = s.C, em = s.EM;
      c.off += b * s.batch_c;
      for (int i = 0; i < M; ++i)
        for (int j = 0; j < s.N; ++j)
          if (tile_runs(s, i / TILE_, j / TILE_) && entry_stored(s, i, j)) {
            if (s.beta != 0.0) s.ar[c.arena][c.off + (int64_t)i * c.ld + j] = (T)rng.next();
            if (s.epi == E_XT) s.ar[em.arena][em.off + (int64_t)i * em.ld + j] = (T)rng.next();
          }
    }
  }
  if (s.weights) { s.sk.resize(s.K); for (auto& v : s.sk) v = (T)(0.75 + 0.25 * rng.next()); }
  if (s.colsums) { s.csw.resize(s.K); for (auto& v : s.csw) v = (T)rng.next(); }
  if (s.epi != E_PLAIN) {
    s.ra.resize(M); s.rb.resize(M); s.rc.resize(M); s.cv.resize(s.N);
    for (int i = 0; i < M; ++i) { s.ra[i] = rng.next() * 1.0000001; s.rb[i] = rng.next() / 3.0; s.rc[i] = rng.next() / 7.0; }  // (not exact in fp32)
    for (auto& v : s.cv) v = rng.next() / 3.0;
  }
  if (s.two_phase) {
    s.num.resize(M); s.den.resize(M);
    for (int i = 0; i < M; ++i) { s.num[i] = rng.next(); s.den[i] = (i % 37 == 5) ? 0.0 : 0.5 + std::fabs(rng.next()); }
  }
  if (s.rp_dot) { s.rpvec.resize(s.N); for (auto& v : s.rpvec) v = rng.next() / 3.0; }
}

// What one launch left behind
template <typename T>
struct Result {
  int M = 0;
  long pre_touched = 0;            // operand arenas the caller compared itself and dropped (left empty in `ar`): changed ones
  std::vector<std::vector<T>> ar;
  std::vector<double> rp_sumsq, rp_dot, cs_out;  // each with RP_PAD poisoned doubles behind its extent
};
constexpr int RP_PAD = 64;

struct Verdict {
  double worst = 0.0;        // largest error / bound over entries, partials and column sums
  long bad_entries = 0;      // entries beyond their bound (or not finite)
  long touched = 0;          // bytes outside the written set that changed
  std::string where;
  bool ok() const { return bad_entries == 0 && touched == 0 && worst <= 1.0; }
};

// Compare every launch of `outs` (one per entry of s.Ms, or one) with the long-double reference, entry by entry, and
// every byte outside the written set with what was there before the launch.
template <typename T>
Verdict check(const Spec<T>& s, const std::vector<Result<T>>& outs, int nthreads = 16) {
  const double u = Bits<T>::u;
  const int Mmax = s.Ms.empty() ? s.M : *std::max_element(s.Ms.begin(), s.Ms.end());
  const int nv = (int)outs.size();
  const int c_epi = (s.epi == E_XT ? 10 : s.epi == E_SX ? (s.two_phase ? 10 : 7) : s.beta != 0.0 ? 4 : 2) + (s.weights ? 1 : 0);
  std::vector<std::vector<std::vector<uint8_t>>> written(nv);
  for (int v = 0; v < nv; ++v) {
    written[v].resize(s.ar.size());
    written[v][s.C.arena].assign(s.ar[s.C.arena].size(), 0);
  }
  nthreads = std::max(1, std::min(nthreads, 16));
  std::vector<Verdict> part(nthreads);
  const int nbn = s.N / TILE_, P = 2;
  auto rows = [&](int tix) {
    Verdict& vd = part[tix];
    for (int b = 0; b < s.nbatch; ++b)
      for (int i = tix; i < Mmax; i += nthreads) {
        Win A = s.A, B = s.same_ab ? s.A : s.B, A2 = s.A2, B2 = s.B2, C = s.C, EM = s.EM;
        A.off += b * s.batch_a; A2.off += b * s.batch_a; B.off += b * s.batch_b; B2.off += b * s.batch_b;
        C.off += b * s.batch_c;
        if (s.same_ab) { B.ld = s.A.ld; }
        const int bm = i / TILE_;
        for (int j = 0; j < s.N; ++j) {
          const int bn = j / TILE_;
          if (!tile_runs(s, bm, bn)) continue;
          if (!entry_stored(s, i, j)) {
            // not computed, stored as +0 in every slice the diagonal tile occupies: the slice sum (finalize.hip) adds up whole
            // diagonal tiles, so these entries may be neither garbage nor left at their fill
            for (int v = 0; v < nv; ++v)
              for (int z = 0; z < slices_of(s, bm, bn) && i < outs[v].M; ++z) {
                const int64_t iz = C.off + (int64_t)i * C.ld + j + (int64_t)z * s.slice_stride;
                written[v][C.arena][iz] = 1;
                if (!same_bits(outs[v].ar[C.arena][iz], (T)0) && vd.bad_entries++ == 0) {
                  char buf[256];
                  snprintf(buf, sizeof buf, "launch %d slice %d C[%d][%d] (lower sub-tile of a SYRK diagonal tile): %.17g, not +0", v, z, i, j, (double)outs[v].ar[C.arena][iz]);
                  vd.where = buf;
                }
              }
            continue;
          }
          int lo, hi;
          k_range(s, bm, bn, lo, hi);
          const T* pa = s.ar[A.arena].data();
          const T* pb = s.ar[B.arena].data();
          long double acc = 0, sab = 0;
          for (int k = lo; k < hi; ++k) {
            long double p = (long double)pa[ia(s, A, i, k)] * (long double)pb[ib(s, B, k, j)];
            if (s.weights) p *= (long double)s.sk[k];
            acc += p; sab += fabsl(p);
          }
          int nterms = hi - lo;
          if (s.two_phase && hi > lo) {  // (an item with an empty k-range runs neither phase)
            const T* pa2 = s.ar[A2.arena].data();
            const T* pb2 = s.ar[B2.arena].data();
            long double acc2 = 0, sab2 = 0;
            for (int k = lo; k < hi; ++k) {
              const long double p = (long double)pa2[ia(s, A2, i, k)] * (long double)pb2[ib(s, B2, k, j)];
              acc2 += p; sab2 += fabsl(p);
            }
            const long double f = s.den[i] != 0.0 ? -(long double)s.num[i] / (long double)s.den[i] : 0.0L;
            acc += f * acc2; sab += fabsl(f) * sab2;
            nterms *= 2;
          }
          long double ref, S;
          const int64_t ic = C.off + (int64_t)i * C.ld + j;
          if (s.epi == E_XT) {
            const long double m = (long double)s.ar[EM.arena][EM.off + (int64_t)i * EM.ld + j];
            ref = (long double)s.ra[i] * acc - (long double)s.rb[i] * m - (long double)s.rc[i] * (long double)s.cv[j];
            S = fabsl((long double)s.ra[i]) * sab + fabsl((long double)s.rb[i] * m) + fabsl((long double)s.rc[i] * (long double)s.cv[j]);
          } else if (s.epi == E_SX) {
            ref = (long double)s.ra[i] * acc - (long double)s.rc[i] * (long double)s.cv[j];
            S = fabsl((long double)s.ra[i]) * sab + fabsl((long double)s.rc[i] * (long double)s.cv[j]);
          } else {
            ref = (long double)s.alpha * acc; S = fabsl((long double)s.alpha) * sab;
            if (s.beta != 0.0) {
              const long double o = (long double)s.beta * (long double)s.ar[C.arena][ic];
              ref += o; S += fabsl(o);
            }
          }
          const long double bound = (long double)(nterms + c_epi) * u * S;
          const int nsl = slices_of(s, bm, bn);
          for (int v = 0; v < nv; ++v) {
            if (i >= outs[v].M) continue;
            long double got = 0;
            for (int z = 0; z < nsl; ++z) {
              const int64_t iz = ic + (int64_t)z * s.slice_stride;
              got += (long double)outs[v].ar[C.arena][iz];
              written[v][C.arena][iz] = 1;
            }
            const long double err = fabsl(got - ref);
            // (an entry all of whose terms are exact zeros must be exactly zero)
            const double ratio = !std::isfinite((double)got) ? INFINITY : bound > 0 ? (double)(err / bound) : (err == 0 ? 0.0 : INFINITY);
            if (ratio > vd.worst) vd.worst = ratio;
            if (!(ratio <= 1.0)) {
              if (vd.bad_entries++ == 0) {
                char buf[256];
                snprintf(buf, sizeof buf, "launch %d batch %d C[%d][%d]: got %.17g ref %.17Lg err %.3Lg bound %.3Lg", v, b, i, j, (double)got, ref, err, bound);
                vd.where = buf;
              }
            }
          }
        }
        // row partials of this row, per 128-column tile and wave column, against the device's own (stored) C entries
        if (s.rp_sumsq)
          for (int v = 0; v < nv; ++v) {
            if (i >= outs[v].M) continue;
            const int64_t Mv = outs[v].M;
            for (int q = 0; q < P * nbn; ++q) {
              const int bn = q / P, wc = q % P;
              long double s2 = 0, sd = 0, ad = 0;
              for (int cc = 0; cc < TILE_; ++cc) {
                if ((cc / 16) % 2 != wc) continue;
                const int j = bn * TILE_ + cc;
                const long double val = (long double)outs[v].ar[C.arena][C.off + (int64_t)i * C.ld + j];
                s2 += val * val;
                if (s.rp_dot) { sd += val * (long double)s.rpvec[j]; ad += fabsl(val * (long double)s.rpvec[j]); }
              }
              const double u64 = Bits<double>::u;
              auto one = [&](double got, long double ref, long double S, const char* what) {
                const long double bound = 66.0L * u64 * S, err = fabsl((long double)got - ref);
                const double ratio = !std::isfinite(got) ? INFINITY : bound > 0 ? (double)(err / bound) : (err == 0 ? 0.0 : INFINITY);
                if (ratio > vd.worst) vd.worst = ratio;
                if (!(ratio <= 1.0) && vd.bad_entries++ == 0) {
                  char buf[256];
                  snprintf(buf, sizeof buf, "launch %d %s[part %d][row %d]: got %.17g ref %.17Lg bound %.3Lg", v, what, q, i, got, ref, bound);
                  vd.where = buf;
                }
              };
              one(outs[v].rp_sumsq[(int64_t)q * Mv + i], s2, s2, "rp_sumsq");
              if (s.rp_dot) one(outs[v].rp_dot[(int64_t)q * Mv + i], sd, ad, "rp_dot");
            }
          }
      }
  };
  {
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) th.emplace_back(rows, t);
    for (auto& t : th) t.join();
  }
  Verdict vd;
  for (auto& p : part) {
    vd.worst = std::max(vd.worst, p.worst);
    if (p.bad_entries && vd.where.empty()) vd.where = p.where;
    vd.bad_entries += p.bad_entries;
  }
  // column sums of the raw A operand: cs_out[z * N + c], stored by the diagonal tiles' slices; summed over the slices
  if (s.colsums)
    for (int v = 0; v < nv; ++v) {
      const int nsl = s.kslices <= 1 ? 1 : (s.dslices > 0 ? s.dslices : s.kslices);
      for (int c = 0; c < s.N; ++c) {
        long double ref = 0, S = 0, got = 0;
        for (int k = 0; k < s.K; ++k) {
          const long double p = (long double)s.ar[s.A.arena][ia(s, s.A, c, k)] * (long double)s.csw[k];
          ref += p; S += fabsl(p);
        }
        for (int z = 0; z < nsl; ++z) got += (long double)outs[v].cs_out[(int64_t)z * s.N + c];
        const long double bound = (long double)(s.K + 2) * u * S, err = fabsl(got - ref);
        const double ratio = !std::isfinite((double)got) ? INFINITY : (double)(err / bound);
        vd.worst = std::max(vd.worst, ratio);
        if (!(ratio <= 1.0) && vd.bad_entries++ == 0) {
          char buf[256];
          snprintf(buf, sizeof buf, "launch %d column sum %d: got %.17Lg ref %.17Lg bound %.3Lg", v, c, got, ref, bound);
          vd.where = buf;
        }
      }
      const double pz = poison<double>();
      for (size_t q = (size_t)nsl * s.N; q < outs[v].cs_out.size(); ++q)
        if (!same_bits(outs[v].cs_out[q], pz)) { if (vd.touched == 0) vd.where += " | cs_out beyond its slices written at " + std::to_string(q); vd.touched += 8; }
    }
  // everything outside the written set: bit for bit as before the launch
  for (int v = 0; v < nv; ++v) {
    if (outs[v].pre_touched) {
      if (vd.touched == 0) vd.where += " | launch " + std::to_string(v) + " changed an operand arena";
      vd.touched += outs[v].pre_touched;
    }
    for (size_t a = 0; a < s.ar.size(); ++a) {
      const bool isC = (int)a == s.C.arena;
      const std::vector<T>& was = s.ar[a];
      const std::vector<T>& now = outs[v].ar[a];
      if (now.empty()) continue;
      for (size_t q = 0; q < was.size(); ++q)
        if (!(isC && written[v][a][q]) && !same_bits(was[q], now[q])) {
          if (vd.touched == 0) vd.where += " | launch " + std::to_string(v) + " changed arena " + std::to_string(a) + " element " + std::to_string(q) + " outside its written set";
          vd.touched += sizeof(T);
        }
    }
    const double pz = poison<double>();
    if (s.rp_sumsq) {
      const size_t ext = (size_t)P * nbn * outs[v].M;
      for (size_t q = ext; q < outs[v].rp_sumsq.size(); ++q) if (!same_bits(outs[v].rp_sumsq[q], pz)) vd.touched += 8;
      for (size_t q = s.rp_dot ? ext : 0; q < outs[v].rp_dot.size(); ++q) if (!same_bits(outs[v].rp_dot[q], pz)) vd.touched += 8;
    }
  }
  return vd;
}

}  // namespace emc
