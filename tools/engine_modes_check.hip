// Every launch mode of the MFMA contraction engine the library issues, entry by entry ("Engine launch modes").
//
//   build/engine_modes_check <group> <f64|f32> [margins file]
//   groups: plain tri batch epilogue syrk paired paired512
//
// Linked against the PRODUCTION engine objects.  Per case: the operands are generated on the host with every byte the launch
// must not read or write poisoned (tools/engine_modes_ref.h), the launch runs through launch_gemm, and every entry is
// compared with the long-double host reference of the launch's full formula under the bound (K + c) u S; every byte
// outside the written set is compared bit for bit.  The plan launch_gemm took (gemm_plan) is printed and asserted.
#include <chrono>
#include <map>
#include "../gpr_amd/csrc/mfma_gemm.h"
#include "engine_modes_ref.h"
using namespace gprhip;
using namespace emc;

#define HIPOK(x)                                                                          \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__);       \
      printf("failed: 1 (aborted)\n");                                                    \
      exit(3);                                                                            \
    }                                                                                     \
  } while (0)

static int g_failed = 0, g_cases = 0;
static FILE* g_margins = nullptr;
static const int FRONT = 256;  // poisoned elements in front of the first window of an arena (keeps 16-byte alignment)

template <typename T> static const char* tname() { return sizeof(T) == 8 ? "f64" : "f32"; }

// sizes the arenas so that every window (all problems, all slices) lies inside with FRONT poisoned elements behind it
template <typename T>
static void alloc_arenas(Spec<T>& s, const std::vector<int64_t>& min_sz = {}) {
  const int M = s.Ms.empty() ? s.M : *std::max_element(s.Ms.begin(), s.Ms.end());
  std::map<int, int64_t> need;
  auto span = [&](const Win& w, int64_t rows, int64_t cols, int64_t batch, int64_t slices) {
    if (w.arena < 0) return;
    const int64_t end = w.off + (s.nbatch - 1) * batch + slices + (rows - 1) * w.ld + cols;
    need[w.arena] = std::max(need[w.arena], end + FRONT);
  };
  const int64_t ar_ = s.op == TN ? s.K : M, ac_ = s.op == TN ? M : s.K;
  const int64_t br_ = s.op == NT ? s.N : s.K, bc_ = s.op == NT ? s.K : s.N;
  span(s.A, ar_, ac_, s.batch_a, 0); span(s.A2, ar_, ac_, s.batch_a, 0);
  if (!s.same_ab) { span(s.B, br_, bc_, s.batch_b, 0); span(s.B2, br_, bc_, s.batch_b, 0); }
  span(s.C, M, s.N, s.batch_c, (int64_t)(std::max(1, s.kslices) - 1) * s.slice_stride);
  span(s.EM, M, s.N, 0, 0);
  int na = 0;
  for (auto& kv : need) na = std::max(na, kv.first + 1);
  s.ar.resize(na);
  for (int a = 0; a < na; ++a) {
    int64_t n = need[a];
    if (a < (int)min_sz.size()) n = std::max(n, min_sz[a]);
    s.ar[a].assign((size_t)n, poison<T>());
  }
}

template <typename T>
static std::string plan_text(const GemmPlan& pl) {
  char buf[320];
  snprintf(buf, sizeof buf, "kernel=%s grid=(%d,%d) work=%d ipw=%d pair_split=%d tail_panels=%d desc2=%d syrk=%d dslices=%d order=%d",
           gemm_kernel_name(pl.kernel, sizeof(T) == 8), pl.grid_x, pl.grid_y, pl.work, pl.ipw, pl.pair_split, pl.tail_panels,
           pl.desc2, pl.syrk, pl.dslices, pl.order);
  return buf;
}

template <typename T>
static T* upload(const std::vector<T>& h) {
  T* d = nullptr;
  HIPOK(hipMalloc(&d, std::max<size_t>(16, h.size() * sizeof(T))));
  if (!h.empty()) HIPOK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

template <typename T>
static void run_case(Spec<T>& s) {
  ++g_cases;
  std::vector<int> Ms = s.Ms.empty() ? std::vector<int>{s.M} : s.Ms;
  const int Mmax = *std::max_element(Ms.begin(), Ms.end());
  std::vector<T*> dar(s.ar.size());
  for (size_t a = 0; a < s.ar.size(); ++a) dar[a] = upload(s.ar[a]);
  T* dsk = s.weights ? upload(s.sk) : nullptr;
  T* dcsw = s.colsums ? upload(s.csw) : nullptr;
  double *dra = s.epi ? upload(s.ra) : nullptr, *drb = s.epi == E_XT ? upload(s.rb) : nullptr, *drc = s.epi ? upload(s.rc) : nullptr;
  double *dcv = s.epi ? upload(s.cv) : nullptr, *dnum = s.two_phase ? upload(s.num) : nullptr, *dden = s.two_phase ? upload(s.den) : nullptr;
  double* drpv = s.rp_dot ? upload(s.rpvec) : nullptr;
  const int nbn = s.N / TILE;
  const size_t rp_n = s.rp_sumsq ? (size_t)2 * nbn * Mmax + RP_PAD : 0;
  const size_t cs_n = s.colsums ? (size_t)((std::max(1, s.kslices) + 7) / 8 * 8) * s.N + RP_PAD : 0;
  const std::vector<double> rp_poison(std::max(rp_n, cs_n), poison<double>());
  double *drp1 = nullptr, *drp2 = nullptr, *dcs = nullptr;
  if (rp_n) { HIPOK(hipMalloc(&drp1, rp_n * 8)); HIPOK(hipMalloc(&drp2, rp_n * 8)); }
  if (cs_n) HIPOK(hipMalloc(&dcs, cs_n * 8));

  bool plan_ok = true;
  std::string plans, err;
  std::vector<Result<T>> outs;
  for (size_t v = 0; v < Ms.size(); ++v) {
    GemmArgsT<T> g;
    g.A = dar[s.A.arena] + s.A.off; g.lda = s.A.ld;
    if (s.same_ab) { g.B = g.A; g.ldb = g.lda; } else { g.B = dar[s.B.arena] + s.B.off; g.ldb = s.B.ld; }
    g.C = dar[s.C.arena] + s.C.off; g.ldc = s.C.ld;
    g.M = Ms[v]; g.N = s.N; g.K = s.K; g.alpha = s.alpha; g.beta = s.beta; g.tri = s.tri; g.upper_only = s.upper; g.order = s.order;
    g.nbatch = s.nbatch; g.batch_a = s.batch_a; g.batch_b = s.batch_b; g.batch_c = s.batch_c;
    g.kslices = s.kslices; g.slice_stride = s.slice_stride;
    g.scale_k = dsk; g.cs_w = dcsw; g.cs_out = dcs;
    if (s.two_phase) { g.A2 = dar[s.A2.arena] + s.A2.off; g.B2 = dar[s.B2.arena] + s.B2.off; g.mid_num = dnum; g.mid_den = dden; }
    if (s.epi) { g.epi_rows_a = dra; g.epi_rows_b = drb; g.epi_rows_c = drc; g.epi_col = dcv; }
    if (s.epi == E_XT) { g.epi_mat = dar[s.EM.arena] + s.EM.off; g.epi_ldm = s.EM.ld; }
    if (s.rp_sumsq) g.rp_sumsq = drp1;
    if (s.rp_dot) { g.rp_dot = drp2; g.rp_vec = drpv; }
    const GemmPlan pl = gemm_plan((GemmOp)s.op, g);
    s.syrk = pl.syrk; s.dslices = pl.dslices;
    const std::string pt = plan_text<T>(pl);
    printf("plan %s %s M=%d N=%d K=%d: %s\n", s.name.c_str(), tname<T>(), Ms[v], s.N, s.K, pt.c_str());
    if (!plans.empty()) plans += " || ";
    plans += "M=" + std::to_string(Ms[v]) + " " + pt;
    // the path the case is named for (with several launches: the expectations of the case's M list, see paired_cases)
    auto want = [&](int x, int got, const char* what) {
      if (x >= 0 && x != got) { plan_ok = false; err += std::string(" plan: ") + what + " = " + std::to_string(got) + ", expected " + std::to_string(x); }
    };
    if (Ms.size() == 1) {
      want(s.x_kernel, pl.kernel, "kernel"); want(s.x_ipw, pl.ipw, "ipw"); want(s.x_desc2, pl.desc2, "desc2");
      want(s.x_syrk, pl.syrk, "syrk"); want(s.x_dslices, pl.dslices, "dslices"); want(s.x_order, pl.order, "order");
      if (s.x_tail >= 0) want(s.x_tail, pl.tail_panels > 0 ? 1 : 0, "tail_panels > 0");
    } else {
      // paired: Ms = {just below the threshold, first paired M, first paired M with a tail}
      want(s.x_kernel, pl.kernel, "kernel");
      want(v == 0 ? 1 : 2, pl.ipw, "ipw");
      want(v == 0 ? 0 : 3, pl.order, "order");
      want(v == 0 ? 0 : s.x_desc2, pl.desc2, "desc2");
      if (v == 2) want(1, pl.tail_panels > 0 ? 1 : 0, "tail_panels > 0");
      if (v == 1 && s.x_tail == 0) want(0, pl.tail_panels, "tail_panels");
    }
    // fresh contents (the previous launch of the list wrote C), poisoned reduction outputs
    if (v > 0) HIPOK(hipMemcpy(dar[s.C.arena], s.ar[s.C.arena].data(), s.ar[s.C.arena].size() * sizeof(T), hipMemcpyHostToDevice));
    if (rp_n) { HIPOK(hipMemcpy(drp1, rp_poison.data(), rp_n * 8, hipMemcpyHostToDevice)); HIPOK(hipMemcpy(drp2, rp_poison.data(), rp_n * 8, hipMemcpyHostToDevice)); }
    if (cs_n) HIPOK(hipMemcpy(dcs, rp_poison.data(), cs_n * 8, hipMemcpyHostToDevice));
    try {
      launch_gemm((GemmOp)s.op, g, 0);
    } catch (const HipFail&) {
      printf("case %s %s: launch_gemm refused the launch FAIL\n", s.name.c_str(), tname<T>());
      ++g_failed;
      return;
    }
    HIPOK(hipDeviceSynchronize());
    Result<T> r;
    r.M = Ms[v];
    r.ar.resize(s.ar.size());
    for (size_t a = 0; a < s.ar.size(); ++a) {
      r.ar[a].resize(s.ar[a].size());
      HIPOK(hipMemcpy(r.ar[a].data(), dar[a], s.ar[a].size() * sizeof(T), hipMemcpyDeviceToHost));
      if ((int)a != s.C.arena && Ms.size() > 1) {  // large operand arenas: compared here, not kept
        if (std::memcmp(r.ar[a].data(), s.ar[a].data(), s.ar[a].size() * sizeof(T)) != 0) r.pre_touched += 1;
        std::vector<T>().swap(r.ar[a]);
      }
    }
    if (rp_n) {
      r.rp_sumsq.resize(rp_n); r.rp_dot.resize(rp_n);
      HIPOK(hipMemcpy(r.rp_sumsq.data(), drp1, rp_n * 8, hipMemcpyDeviceToHost));
      HIPOK(hipMemcpy(r.rp_dot.data(), drp2, rp_n * 8, hipMemcpyDeviceToHost));
      // the extent of this launch: 2 * nbn * M partials; the reference pass expects the pad right behind it
      r.rp_sumsq.erase(r.rp_sumsq.begin() + (size_t)2 * nbn * Ms[v] + RP_PAD, r.rp_sumsq.end());
      r.rp_dot.erase(r.rp_dot.begin() + (size_t)2 * nbn * Ms[v] + RP_PAD, r.rp_dot.end());
    }
    if (cs_n) { r.cs_out.resize(cs_n); HIPOK(hipMemcpy(r.cs_out.data(), dcs, cs_n * 8, hipMemcpyDeviceToHost)); }
    outs.push_back(std::move(r));
  }
  const auto t0 = std::chrono::steady_clock::now();
  const Verdict vd = check(s, outs);
  const double ref_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const bool ok = vd.ok() && plan_ok;
  printf("case %s %s: worst=%.3e bad=%ld touched=%ld ref=%.2fs plan=%s%s%s %s\n", s.name.c_str(), tname<T>(), vd.worst, vd.bad_entries, vd.touched, ref_s,
         plan_ok ? "ok" : "WRONG", err.c_str(), vd.where.empty() ? "" : (" [" + vd.where + "]").c_str(), ok ? "OK" : "FAIL");
  if (g_margins) fprintf(g_margins, "%-34s %s  worst error/bound %.3e  %s\n    %s\n", s.name.c_str(), tname<T>(), vd.worst, ok ? "OK" : "FAIL", plans.c_str());
  if (!ok) ++g_failed;
  for (auto p : dar) HIPOK(hipFree(p));
  for (void* p : {(void*)dsk, (void*)dcsw, (void*)dra, (void*)drb, (void*)drc, (void*)dcv, (void*)dnum, (void*)dden, (void*)drpv, (void*)drp1, (void*)drp2, (void*)dcs})
    if (p) HIPOK(hipFree(p));
}

// ---- case builders
template <typename T>
static Spec<T> dense(const std::string& name, int op, int M, int N, int K, int pad_bytes = 0) {
  Spec<T> s;
  s.name = name; s.op = op; s.M = M; s.N = N; s.K = K;
  const int pad = pad_bytes / (int)sizeof(T);
  s.A = {0, FRONT, (op == TN ? M : K) + pad};
  s.B = {1, FRONT, (op == NT ? K : N) + pad};
  s.C = {2, FRONT, N + pad};
  return s;
}
template <typename T>
static void go(Spec<T>& s, const std::vector<int64_t>& min_sz = {}) {
  static uint64_t seed = 1;
  alloc_arenas(s, min_sz);
  fill_operands(s, ++seed);
  run_case(s);
}
static int mxm_slices(int mp) { return mp >= 3 * TILE ? std::min(4, mp / TILE) : 1; }  // as gprhip.hip

template <typename T>
static void plain_cases() {
  const bool f64 = sizeof(T) == 8;
  const int K1 = f64 ? 48 : 96, K2 = f64 ? 80 : 160;
  const char* opn[3] = {"nn", "nt", "tn"};
  const int shapes[3][2] = {{1, 1}, {2, 3}, {3, 2}};
  const double ab[3][2] = {{1, 0}, {-1, 1}, {1, 1}};
  for (int op = 0; op < 3; ++op)
    for (int sh = 0; sh < 3; ++sh) {
      const int v = (op + sh) % 3;  // every op meets every alpha / beta pair, every shape too
      char nm[96];
      snprintf(nm, sizeof nm, "plain_%s_%dx%d_a%+d_b%d_ld16", opn[op], shapes[sh][0], shapes[sh][1], (int)ab[v][0], (int)ab[v][1]);
      Spec<T> s = dense<T>(nm, op, shapes[sh][0] * TILE, shapes[sh][1] * TILE, sh == 1 ? K2 : K1, 16);
      s.alpha = ab[v][0]; s.beta = ab[v][1];
      s.x_kernel = op == NN ? GK_NN : op == NT ? GK_NT : GK_TN; s.x_ipw = 1; s.x_syrk = 0;
      go(s);
    }
  {  // generic split-K with a slice stride on a launch that is not SYRK-shaped (gemm_splitk's launch shape, no triangle)
    Spec<T> s = dense<T>("plain_nn_2x2_splitk3", NN, 256, 256, f64 ? 112 : 224, 16);  // 7 stages over 3 slices: 3 + 3 + 1
    s.kslices = 3; s.slice_stride = (int64_t)256 * s.C.ld + 32;
    s.x_kernel = GK_NN; s.x_ipw = 1;
    go(s);
  }
  if (f64) {
    // the covariance launches of do_covariances: NT, both operands the same np x mp matrix, C np x np
    const double cab[3][2] = {{-1, 1}, {1, 1}, {1, 0}};
    for (int v = 0; v < 3; ++v) {
      char nm[96];
      snprintf(nm, sizeof nm, "plain_cov_nt_384x384x256_a%+d_b%d", (int)cab[v][0], (int)cab[v][1]);
      Spec<T> s = dense<T>(nm, NT, 384, 384, 256);
      s.same_ab = true; s.alpha = cab[v][0]; s.beta = cab[v][1]; s.x_kernel = GK_NT;
      go(s);
    }
    {  // potrf_upper_n's trailing update: panel and trailing matrix are windows of one 512-wide buffer
      Spec<T> s;
      s.name = "plain_trailing_tn_upper_384_k128"; s.op = TN; s.M = s.N = 384; s.K = 128;
      s.A = {0, FRONT + 128, 512}; s.same_ab = true; s.C = {0, FRONT + 128 * 512 + 128, 512};
      s.alpha = -1; s.beta = 1; s.upper = 1; s.x_kernel = GK_TN; s.x_syrk = 0;
      go(s, {FRONT + 512 * 512 + FRONT});
    }
    {  // ... and its panel solve, in place: C is the B operand (every block reads its whole column tile first)
      Spec<T> s;
      s.name = "plain_panel_tn_inplace_128x384"; s.op = TN; s.M = 128; s.N = 384; s.K = 128;
      s.A = {1, FRONT, 128}; s.B = {0, FRONT + 128, 512}; s.C = s.B; s.x_kernel = GK_TN;
      go(s, {FRONT + 512 * 512 + FRONT});
    }
  }
  {  // argument refusals: thrown on the host in front of any launch
    int refused = 0;
    T* d = nullptr;
    HIPOK(hipMalloc(&d, 1 << 20));
    auto refuses = [&](GemmOp op, GemmArgsT<T> g) {
      try { launch_gemm(op, g, 0); } catch (const HipFail&) { ++refused; }
    };
    GemmArgsT<T> g; g.A = d; g.B = d; g.C = d; g.lda = g.ldb = g.ldc = 128; g.M = g.N = 128; g.K = 64;
    GemmArgsT<T> a = g; a.M = 100; refuses(OP_NN, a);                       // unpadded
    a = g; a.lda = 129; refuses(OP_NN, a);                                 // leading dimension not 16-byte aligned
    a = g; a.kslices = 2; a.beta = 1.0; refuses(OP_NN, a);                  // split-K with beta
    a = g; a.scale_k = d; refuses(OP_NN, a);                               // weights off TN
    a = g; a.epi_rows_a = (const double*)d; refuses(OP_NN, a);             // fused epilogue off NT
    HIPOK(hipDeviceSynchronize());
    HIPOK(hipFree(d));
    ++g_cases;
    printf("case plain_refusals %s: %d of 5 refused %s\n", tname<T>(), refused, refused == 5 ? "OK" : "FAIL");
    if (refused != 5) ++g_failed;
  }
}

template <typename T>
static void tri_cases() {
  const bool f64 = sizeof(T) == 8;
  struct P { const char* n; int op, tri, upper; bool both; };
  const P pol[5] = {{"khi_bn_nn", NN, T_KHI_BN, 0, true}, {"klo_bn_nt", NT, T_KLO_BN, 0, true}, {"klo_bm_nn", NN, T_KLO_BM, 0, false},
                    {"klo_max_nt_upper", NT, T_KLO_MAX, 1, false}, {"band_nn_upper", NN, T_BAND, 1, false}};
  for (const P& p : pol) {
    if (!f64 && !p.both) continue;  // the m x m products of triangular factors are fp64 in the library
    for (int n = 128; n <= 512; n += 128) {
      std::vector<int> ks = {1, 2};
      if (mxm_slices(n) > 2) ks.push_back(mxm_slices(n));
      for (int k : ks) {
        char nm[96];
        snprintf(nm, sizeof nm, "tri_%s_%d_ks%d", p.n, n, k);
        Spec<T> s = dense<T>(nm, p.op, n, n, n);
        s.tri = p.tri; s.upper = p.upper; s.x_kernel = p.op == NN ? GK_NN : GK_NT; s.x_ipw = 1;
        if (k > 1) { s.kslices = k; s.slice_stride = (int64_t)n * n; }
        go(s);
      }
    }
  }
}

// the two joins of trtri_upper as it issues them: windows of sz rows at pair * (mp + 1) strides inside mp x mp buffers
template <typename T>
static void batch_cases() {
  const int shapes[4][3] = {{512, 128, 2}, {768, 128, 3}, {768, 256, 1}, {1024, 256, 2}};  // mp, window, nbatch
  for (auto& sh : shapes)
    for (int ks = 1; ks <= 2; ++ks) {
      const int mp = sh[0], sz = sh[1], nb = sh[2];
      const int64_t mm = (int64_t)mp * mp, stride = (int64_t)2 * sz * (mp + 1);
      char nm[96];
      {  // T = U12 * X22
        snprintf(nm, sizeof nm, "batch_join_a_khi_bn_mp%d_w%d_nb%d_ks%d", mp, sz, nb, ks);
        Spec<T> s;
        s.name = nm; s.op = NN; s.M = s.N = s.K = sz; s.tri = T_KHI_BN;
        s.A = {0, FRONT + sz, mp}; s.B = {1, FRONT + (int64_t)sz * (mp + 1), mp}; s.C = {2, FRONT + sz, mp};
        s.nbatch = nb; s.batch_a = s.batch_b = s.batch_c = stride;
        if (ks > 1) { s.kslices = ks; s.slice_stride = mm; }
        s.x_kernel = GK_NN; s.x_ipw = 1;
        go(s, {FRONT + mm + FRONT, FRONT + mm + FRONT, FRONT + ks * mm + FRONT});
      }
      {  // X12 = -X11 * T: A and (without k-slices) C are windows of the same buffer
        snprintf(nm, sizeof nm, "batch_join_b_klo_bm_mp%d_w%d_nb%d_ks%d", mp, sz, nb, ks);
        Spec<T> s;
        s.name = nm; s.op = NN; s.M = s.N = s.K = sz; s.tri = T_KLO_BM; s.alpha = -1.0;
        s.A = {0, FRONT, mp}; s.B = {1, FRONT + sz, mp}; s.C = {ks > 1 ? 2 : 0, FRONT + sz, mp};
        s.nbatch = nb; s.batch_a = s.batch_b = s.batch_c = stride;
        if (ks > 1) { s.kslices = ks; s.slice_stride = mm; }
        s.x_kernel = GK_NN; s.x_ipw = 1;
        go(s, {FRONT + mm + FRONT, FRONT + mm + FRONT, FRONT + ks * mm + FRONT});
      }
    }
}

template <typename T>
static void epilogue_cases() {
  const int M = 384, N = 256, K = 256;
  {
    Spec<T> s = dense<T>("epi_nt_xt_klo_bn_ldm16", NT, M, N, K);
    s.tri = T_KLO_BN; s.epi = E_XT; s.EM = {3, FRONT, N + 16 / (int)sizeof(T)}; s.x_kernel = GK_NT_XT;
    go(s);
  }
  {
    Spec<T> s = dense<T>("epi_nt_sx_two_phase_den0", NT, M, N, K);
    s.tri = T_KLO_BN; s.epi = E_SX; s.two_phase = true; s.A2 = {3, FRONT, K}; s.B2 = {4, FRONT, K}; s.x_kernel = GK_NT_SX;
    go(s);
  }
  for (int dot = 0; dot < 2; ++dot) {
    Spec<T> s = dense<T>(dot ? "epi_nn_khi_bn_rp_sumsq_dot" : "epi_nn_khi_bn_rp_sumsq", NN, M, N, K);
    s.tri = T_KHI_BN; s.rp_sumsq = true; s.rp_dot = dot != 0; s.x_kernel = GK_NN;
    go(s);
  }
}

template <typename T>
static void syrk_cases() {
  const bool f64 = sizeof(T) == 8;
  const int K = f64 ? 1040 : 1056;  // 65 / 33 stages: no multiple of kslices x stage
  struct C { int n, ks; bool cs; };
  const C cs[] = {{256, 8, false}, {256, 16, false}, {384, 8, false}, {128, 8, true}, {256, 8, true}, {384, 8, true}, {256, 16, true}, {384, 3, true}};
  for (const C& c : cs) {
    char nm[96];
    snprintf(nm, sizeof nm, "syrk_%s_upper_%d_ks%d", c.cs ? "tn_ws" : "tn_w", c.n, c.ks);
    Spec<T> s;
    s.name = nm; s.op = TN; s.M = s.N = c.n; s.K = K; s.upper = 1; s.weights = true; s.colsums = c.cs; s.same_ab = true;
    s.A = {0, FRONT, c.n}; s.C = {1, FRONT, c.n}; s.kslices = c.ks; s.slice_stride = (int64_t)c.n * c.n;
    s.x_kernel = c.cs ? GK_TN_WS : GK_TN_W; s.x_syrk = 1; s.x_ipw = 1;
    s.x_dslices = c.ks % 8 == 0 ? gemm_syrk_diag_slices(c.ks, f64, c.cs) : 0;
    if (c.ks % 8 == 0 && !(s.x_dslices > 0 && s.x_dslices < c.ks)) s.x_dslices = -2;  // the diagonal tiles must get fewer slices: fails the plan check
    go(s);
  }
}

// The paired order (order 3) around its thresholds.  The row counts come from the plan, which takes the slot count from
// the device: M just below the first paired launch (single tiles, order falls back to 0), the first paired M, and the
// first paired M with tail panels -- three launches on the same operands, one reference pass.
template <typename T>
static void paired_cases(int N) {
    for (int two = 0; two < 2; ++two) {
      GemmArgsT<T> g;
      g.N = g.K = N; g.order = 3; g.tri = two ? TRI_KLO_BN : TRI_KHI_BN;
      if (two) { g.A2 = (const T*)16; g.epi_rows_a = (const double*)16; }
      const GemmOp op = two ? OP_NT : OP_NN;
      int first = 0, first_tail = 0, none = 0;
      for (int nbm = 1; nbm <= 16384 && !(first && first_tail && none); ++nbm) {
        g.M = nbm * TILE;
        const GemmPlan pl = gemm_plan(op, g);
        if (pl.ipw == 2 && !first) first = nbm;
        if (pl.ipw == 2 && pl.tail_panels > 0 && !first_tail) first_tail = nbm;
        if (pl.ipw == 2 && pl.tail_panels == 0 && !none) none = nbm;
      }
      char nm[96];
      snprintf(nm, sizeof nm, "paired_%s_N%d", two ? "nt_sx_two_phase_klo_bn" : "nn_khi_bn", N);
      if (!first || !first_tail || !none || first < 2) {
        ++g_cases; ++g_failed;
        printf("case %s %s: no paired row count found (first %d, with tail %d, without %d) FAIL\n", nm, tname<T>(), first, first_tail, none);
        continue;
      }
      Spec<T> s = dense<T>(nm, two ? NT : NN, first_tail * TILE, N, N);
      s.Ms = {(first - 1) * TILE, none * TILE, first_tail * TILE};
      s.order = 3; s.tri = two ? T_KLO_BN : T_KHI_BN; s.x_desc2 = 1; s.x_tail = 0;
      if (two) { s.epi = E_SX; s.two_phase = true; s.A2 = {3, FRONT, N}; s.B2 = {4, FRONT, N}; s.x_kernel = GK_NT_SX; }
      else s.x_kernel = GK_NN;
      go(s);
    }
}

template <typename T>
static void run_group(const std::string& grp) {
  if (grp == "plain") plain_cases<T>();
  else if (grp == "tri") tri_cases<T>();
  else if (grp == "batch") batch_cases<T>();
  else if (grp == "epilogue") epilogue_cases<T>();
  else if (grp == "syrk") syrk_cases<T>();
  else if (grp == "paired") paired_cases<T>(256);
  else if (grp == "paired512") paired_cases<T>(512);  // two pairs per row panel; 6 s of host reference: run by hand, not by the suite
  else { printf("unknown group %s\n", grp.c_str()); exit(2); }
}

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  if (argc < 3) {
    printf("usage: engine_modes_check <plain|tri|batch|epilogue|syrk|paired|paired512> <f64|f32> [margins file]\n");
    return 2;
  }
  const std::string grp = argv[1], ty = argv[2];
  if (argc > 3) g_margins = fopen(argv[3], "a");
  gemm_init();
  printf("engine_modes_check %s %s: %d resident slots\n", grp.c_str(), ty.c_str(), gemm_resident_slots());
  if (ty == "f64") run_group<double>(grp);
  else if (ty == "f32") {
    if (grp == "batch") { printf("the batched joins are fp64 only\n"); return 2; }
    run_group<float>(grp);
  } else return 2;
  if (g_margins) fclose(g_margins);
  printf("cases: %d\nfailed: %d\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
