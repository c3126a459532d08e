// C ABI + orchestration of the two-pass streaming FITC evaluation (see include/gprhip.h).
//
// Whitened formulation (V = K_nm U^-1 with U = chol(K_m + jitter)): every quantity of the reference's
// stacked-QR path is obtained from  B~ = I + V^T diag(1/s) V = R~^T R~  -- no K_m^-1 / B^-1 cancellation,
// QR-grade accuracy from SYRK + potrf.
// Pass 1 (per row chunk):  K = cov(X, Z);  V = K U^-1 (kept in HBM for pass 2);  r, s, 1/s;
//                          B~_part += V^T diag(1/s) V;  c~ += V^T (y/s).
// Exchange 1            :  sum over shards of (B~_part, c~, sum log s, sum y^2/s, sum r/s).
// Middle (m x m)        :  R~ = chol(I + B~_part);  b = R~^-T c~;  t~ = R~^-1 b;  t = U^-1 t~;  R~^-1.
//                          l1, l2 are complete here: evidence-only evaluations stop after this.
// Pass 2 (per row chunk):  Q' = V R~^-1;  q_diag, w, v;  X~ = diag(1/s) Q' R~^-T - diag(v) V - w t~^T
//                          (fused GEMM epilogue);  X = X~ U^-T;  G~_part += V^T diag(v) V;
//                          fused gradient accumulators over E = X .* K_nm.
// Exchange 2            :  sum over shards of (G~_part, gradient column accumulators, scalars).
// Finish                :  W = U^-1 (I - B~^-1 - t~ t~^T - G~) U^-T;  traces;  dl/dsigma2, dl/dtheta.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include <string>
#include "../../include/gprhip.h"
#include "common.h"
#include "kernels.h"
#include "mfma_gemm.h"
#include "predict_plan.h"
#include "problem_internal.h"
#include "sample_paths_host.h"

static_assert(gprhip::PLAN_TILE == gprhip::TILE, "predict_plan.h rounds to the engine's tile");

namespace gprhip {
const std::string& last_error();

// x <- x / |x| over the first n entries (single block); nrm[0] = |x| before the scaling
__global__ __launch_bounds__(256) void normalize_kernel(double* __restrict__ x, int n, double* __restrict__ nrm) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += x[i] * x[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sqrt(red[0]);
  const double inv = r > 0.0 ? 1.0 / r : 0.0;
  for (int i = threadIdx.x; i < n; i += 256) x[i] *= inv;
  if (threadIdx.x == 0) nrm[0] = r;
}

__global__ void copy_diag_kernel(const double* __restrict__ A, int mp, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < mp) out[i] = A[(int64_t)i * (mp + 1)];
}

// dst = I + a on upper tiles, 0 elsewhere; a: packed upper tiles (the exchange-1 buffer)
__global__ void add_identity_upper_kernel(const double* __restrict__ a, int mp, double* __restrict__ dst) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y;
  if (c >= mp) return;
  const int64_t off = (int64_t)r * mp + c;
  dst[off] = (r / TILE <= c / TILE) ? a[packed_upper_off(r, c)] + (r == c ? 1.0 : 0.0) : 0.0;
}

}  // namespace gprhip

using namespace gprhip;

extern "C" int64_t gprhip_ar1_len(const gprhip_problem* p);
extern "C" int64_t gprhip_ar2_len(const gprhip_problem* p);

namespace {

constexpr double LOG_2PI = 1.8378770664093454835606594728112;  // lib/utils.ml:39-40
constexpr int NSCAL = 16;
enum {  // device scalar slots
  SC_LOGDET_B = 0,  // log |B~| = log |B| - log |K_m + jitter|
  SC_BB = 1,        // |b|^2 = |Q_n^T y~|^2
  SC_LMAX = 2,      // power-iteration estimates of lambda_max(K_m + jitter) and lambda_max((K_m + jitter)^-1)
  SC_LMAX_INV = 3,
  SC_A1TAIL = 8,    // 8..11: copy of the reduced exchange-1 tail (single-block problems: written by the fused B~ phase)
};
// tail of the exchange-1 buffer
enum { A1_SUMLOGS = 0, A1_ISY2 = 1, A1_ISR = 2, A1_TAIL = 4 };
// tail of the exchange-2 buffer
enum { A2_SUMV = 0, A2_SUMIS = 1, A2_WRES = 2, A2_SUMV1 = 3, A2_SUME = 4, A2_SUMED = 5, A2_TAIL = 8 };

struct Timer {
  std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> ev;
  bool on = false;       // level 2: an event pair around every stage of the evaluation
  bool kernel = false;   // level 1: one event pair around the dominant kernel alone (the pass-1 SYRK launch)
  hipEvent_t k0 = nullptr, k1 = nullptr;
  bool k_recorded = false;
};

}  // namespace

struct gprhip_problem {
  // A lane of a gprhip_batch (lane_of = the problem the batch was made on): X, y and the stream are that problem's, the
  // parameter block (hy_dev / hy_host) is a slice of the batch's one upload block -- none of them is released with the lane
  gprhip_problem* lane_of = nullptr;
  bool is_lane = false;
  std::vector<gprhip_batch*> batches;  // the batches that borrow this problem (told when it is destroyed)
  int device = 0, kind = 0;
  int64_t n = 0;
  int D = 0, d = 0, m = 0, mp = 0;
  int64_t chunk = 0;
  int nchunks = 0;
  int kslices = 0;   // upper bound on the split-K factor (set at creation from the memory budget)
  hipStream_t stream = nullptr;
  // second stream: the covariance of the first row chunk runs beside the K_m factorisation (do_pass1)
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_rf = nullptr, ev_binv = nullptr;  // pass 2: R^-1 and B~^-1 come from the second stream (do_pass2)
  // GPRHIP_COV_OVERLAP (read at creation): the covariance of row chunk c + 1 is built on the second stream beside the
  // V = K U^-1 product of chunk c (the two chunk buffers alternate in pass 1) instead of in front of its own product
  int cov_overlap = 0;
  hipEvent_t ev_cov[2] = {nullptr, nullptr}, ev_vdone[2] = {nullptr, nullptr};
  // third stream + events: look-ahead of the blocked factorisation (chol.hip, potrf_upper_blocked) -- a stream of its own,
  // because stream2 carries the first row chunk's covariance beside the K_m factorisation
  PotrfAux potrf_aux{};
  std::vector<void*> allocs;
  int64_t alloc_bytes = 0, planned_bytes = 0;  // hipMalloc'ed so far / gprhip_memory_plan's total for this problem

  double *X = nullptr, *y = nullptr, *P = nullptr;
  double *Z = nullptr, *tproj = nullptr;
  double *km = nullptr, *kj = nullptr, *umat = nullptr, *uinv = nullptr;
  double *bmat = nullptr, *rinv = nullptr, *binv = nullptr, *wtil = nullptr, *wmat = nullptr,
         *tmp = nullptr, *dinv = nullptr;
  double *bvec = nullptr, *ttil = nullptr, *tvec = nullptr, *scal = nullptr;
  int* info = nullptr;
  double *r = nullptr, *is = nullptr, *yis = nullptr, *w = nullptr, *v = nullptr, *es = nullptr;
  double* projpart = nullptr;
  double* zshift = nullptr;  // [64] centroid of the inducing points (gradient kernel's expansion offset)
  double *rp1 = nullptr, *rp2 = nullptr;  // per-row partial sums from the GEMM epilogues [parts*mp/128][chunk]
  double *xt = nullptr, *pt = nullptr, *prow = nullptr;  // prediction: test-point chunk, its projection, 3 row vectors
  int64_t xt_rows = 0;                                   // rows they hold
  void *predA = nullptr, *predB = nullptr;               // prediction chunk buffers beyond the training chunk (do_predict)
  int64_t pred_rows = 0;
  bool have_model = false;
  bool have_factors = false;  // U^-1 / R~^-1 valid (false after a means-only gprhip_load_predictor)
  bool have_v = false;        // Vstore / r hold V = K_nm U^-1 of the current kernel and inducing points (reuse_v)
  bool merged_x = false;      // this evaluation forms X by the two-phase product (set in pass 2)
  double cond_km = -1.0;       // 2-norm condition estimate of K_m + jitter of the last evaluation (< 0: not computed yet)
  double f32_coeff_tol = 0.25; // GPRHIP_F32_COEFF_TOL (read at creation): fp32-bulk problems refuse to use their mean
                               // coefficients when cond_km * 2^-24 exceeds it (0 = never refuse).  Measured over d = 1..16,
                               // m = 50..512 (profiles/r04_f32_guard.txt): the coefficients' error is 1/17 .. 1/3600 of that
                               // worst-case bound, i.e. <= ~1.5e-2 at the default threshold (cond ~ 4e6), typically 4e-3
  const void* x_last = nullptr;  // single-chunk gradient evaluations: the chunk buffer that holds X (debug fetch "x_rows")
  bool have_k = false;        // Kstore holds K_nm of the current kernel and inducing points for every chunk
  int k_resident = 1;         // GPRHIP_K_RESIDENT=0 (read at creation): never keep K_nm (ablation)
  // GPRHIP_SMALL_PATH=0 (read at creation): never take the one-kernel passes for at most 64 inducing points (small.hip)
  int small_path = 1;
  // GPRHIP_MID_PATH=0 (read at creation): never take the one-kernel passes for 65 .. 128 inducing points (mid.hip)
  int mid_path = 1;
  double* mid_part = nullptr;    // their per-workgroup partial sums (allocated at first use)
  int mid_gram = 1;              // GPRHIP_MID_GRAM: two tiles -- the Gram accumulations by mid.hip's own launch pair (0: the engine's)
  double* mid_gram_part = nullptr;  // its per-slice partial tiles (allocated at first use)
  int* mid_done = nullptr;       // arrival counter of their last finish launch (its last workgroup ships the results)
  double* small_part = nullptr;  // their per-workgroup partial sums (allocated at first use)
  double* small_k = nullptr;     // K_nm [rows_p][64] of the small pass 1, read back by the small pass 2
  bool small_k_valid = false;    // ... of the current kernel parameters and inducing points (as have_v)
  int w_as_ws = 1;            // GPRHIP_W_AS_WS=0 (read at creation): pass-2 SYRK through the plain weighted kernel (do_pass2)
  // GPRHIP_MERGED_X (read at creation): 0 = X~ and X = X~ U^-T as two launches, as in rounds 1-2 (A/B runs); 1 (default) =
  // the two-phase product for shards large enough to pay for R^-1; 2 = always (parity tests at small sizes)
  int merged_x_mode = 1;
  // GPRHIP_POTRF_ENGINE=1 (read at creation): the round-2 factorisation (engine launches per step) + recursive-doubling inverse
  bool engine_steps = false;
  // GPRHIP_POTRF_CHAIN=1 (read at creation; default 0): factorisation + inverse of matrices of two or more 128-blocks as
  // ONE persistent launch with device-side dependencies (chol.hip, potrf_upper_chain) instead of three launches per step.
  // Built in round 5, bit-identical, and measured 1.4 - 2.8 x SLOWER than the launches: kept for A/B
  int potrf_chain_mode = 0;
#ifdef GPRHIP_LAB
  PotrfChain* chain = nullptr;  // its task list and flag words (created at the first factorisation)
#endif
  // n x m storage: double, or float in the fp32-bulk mode (element size `esz`)
  void *bufA = nullptr, *bufB = nullptr, *Vstore = nullptr;
  // Cov_se_fat with projection hypers: K_nm of all rows, kept from pass 1 for the gradient kernel of pass 2 (which then
  // reads E = X .* K instead of recomputing distances and exp) when the device has room for a second n x m matrix
  void* Kstore = nullptr;
  bool kstore_tried = false;
  float *uinv_f = nullptr, *rinv_f = nullptr;  // fp32 copies of U^-1 / R~^-1 (fp32-bulk mode)
  double* rfinv = nullptr;   // R^-1 = U^-1 R~^-1 (R = R~ U is the reference's r_mat): B operand of the two-phase X product
  float* rfinv_f = nullptr;
  float *is_f = nullptr, *yis_f = nullptr, *v_f = nullptr;  // fp32 copies of the SYRK row weights (fp32-bulk mode)
  int f32 = 0;
  size_t esz = 8;
  void* slices = nullptr;
  int64_t slices_bytes = 0;
  double *rowpart = nullptr, *gemvpart = nullptr, *colpart = nullptr, *scalpart = nullptr,
         *kmpart = nullptr, *kmred = nullptr;
  double *ar1 = nullptr, *ar2 = nullptr;  // internal exchange buffers for single-device eval

  // state of the evaluation in flight
  gprhip_hypers h{};
  CovParams cp{};
  int want_grad = 0;
  int64_t n_total = 0;
  int stage = 0;  // 0 idle, 1 pass1 done, 2 pass2 done
  bool have_inputs = false, have_targets = false;
  // Per-evaluation parameters cross the PCIe link as ONE block: [Z (mp x d) | centroid (64) | tproj (D x d) | het (mp) |
  // multiscales (mp x d)] (the last three for Cov_se_fat), assembled in pinned host memory (hy_host, whose parts the
  // gradient assembly reads again) and copied by one asynchronous transfer of the prefix in use.
  double *hy_dev = nullptr, *hy_host = nullptr;
  int64_t hy_len = 0;
  hipEvent_t ev_hy = nullptr;  // the last upload of hy_host has been consumed
  double *hShift = nullptr, *hZ = nullptr, *hTproj = nullptr, *hHet = nullptr, *hMs = nullptr;  // parts of hy_host
  double* het = nullptr;                  // device copy of hHet
  // Results of an evaluation come back as one block as well: [scalars (NSCAL) | potrf flags (2 ints in one double) |
  // t (mp) | K_m traces (km_rows x mp) | diag W (mp)] = res_dev -> res_host (pinned), plus the tails of the two exchange
  // buffers (ex_host: [A1_TAIL | column block .. end of the exchange-2 buffer]).
  // ex_host / ex_dev lie directly behind the result block (one transfer can bring both).  Since round 6 the transfer is a
  // kernel's stores into res_host (mapped pinned memory) wherever it would exceed 32 KB or take more than one copy:
  // ship_kernel (finalize.hip) on the engine path, the last workgroup of mid_finish2_kernel (mid.hip)
  double *res_dev = nullptr, *res_host = nullptr, *ex_host = nullptr, *ex_dev = nullptr;
  bool a1_in_scal = false;  // this evaluation's exchange-1 tail is in the result block's scalars (SC_A1TAIL)
  int64_t res_len = 0, ex_len = 0;
  double *ms = nullptr, *rowes = nullptr, *es2 = nullptr;  // multiscales [mp][d]; per-row E/ms partials
  double* wdiag = nullptr;  // diag W inside the result block
  Timer timer;
  std::vector<std::string> tnames;
  std::vector<float> tms;

  template <typename T>
  T* alloc(int64_t count) {
    void* ptr = nullptr;
    GPR_HIP(hipMalloc(&ptr, (size_t)std::max<int64_t>(count, 1) * sizeof(T)));
    allocs.push_back(ptr);
    alloc_bytes += std::max<int64_t>(count, 1) * (int64_t)sizeof(T);
    return static_cast<T*>(ptr);
  }
  const double* pts() const { return kind == GPRHIP_COV_SE_FAT && h.tproj ? P : X; }
  int64_t rows_of(int c) const { return std::min<int64_t>(chunk, n - (int64_t)c * chunk); }
  // rows of the resident n x m store: full chunks are contiguous, the last one is padded to the tile
  int64_t rows_total_padded() const {
    return (int64_t)(nchunks - 1) * chunk + round_up(rows_of(nchunks - 1), TILE);
  }
  int ks_used = 8;
  int64_t slice_rows = 8192;  // training points per split-K slice of the SYRK launches (both precisions)
  // training points per workgroup of the gradient kernels (grad_slab_rows: 256 or 1024), halved down to 64 while the launch
  // would leave most of the chip idle (n = 2000, m = 128: 8 workgroups of 256 rows took 30 us; set at creation)
  int grad_slab = 256;
  int tile_order = 3;  // block -> tile order of the chunk GEMMs (mfma_gemm.hip tile_of_block): paired column tiles, XCD-local groups
  int grad_scalar = 0;  // GPRHIP_GRAD_SCALAR: use the scalar gradient kernel even where the MFMA one applies
  // Cov_se_fat `Proj hypers: rows of the exchange-2 column block beyond d+1, and the D x d second term
  int dbig() const { return kind == GPRHIP_COV_SE_FAT ? D : 0; }
  bool has_proj() const { return kind == GPRHIP_COV_SE_FAT && h.tproj != nullptr; }
  bool has_het() const { return kind == GPRHIP_COV_SE_FAT && h.log_hetero_skedasticity != nullptr; }
  bool has_ms() const { return kind == GPRHIP_COV_SE_FAT && h.log_multiscales_m05 != nullptr; }
  int64_t km_rows() const { return d + 2 + (kind == GPRHIP_COV_SE_FAT ? d : 0); }
  // exchange-2 column block: sum E, sum p_k E (d), sum x_big E (D), and for Cov_se_fat sum p_k^2 E (d)
  int64_t col_rows() const { return d + 1 + dbig() + (kind == GPRHIP_COV_SE_FAT ? d : 0); }
  // several target vectors on one model (gprhip_set_targets_many / gprhip_eval_targets, targets.hip)
  int tg_k = 0;               // columns of the target matrix held (0: none)
  int multi = 0;              // the evaluation in flight is one over `multi` target vectors: it takes the engine row path
  bool multi_state = false;   // the completed evaluation was one: t / w are not those of one target vector
  bool tg_coeffs = false;     // T of that evaluation is resident in tg_small (a target matrix of another width re-makes it)
  double *tg_y = nullptr, *tg_w = nullptr;  // Y and W_mat, column-major [k][nchunks * chunk]
  double* tg_small = nullptr;  // [y2 (16) | |b_k|^2 (16) | T | T~ | B | c~ (mp x 16 each)]
  double *tg_part = nullptr, *tg_rowpart = nullptr;  // per-workgroup partials of the tall-skinny products / of the row kernels
  int64_t tg_bytes = 0;
  int64_t npad() const { return (int64_t)nchunks * chunk; }
  double* tg_y2() const { return tg_small; }
  double* tg_bb() const { return tg_small + TG_LD; }
  double* tg_T() const { return tg_small + 2 * TG_LD; }
  double* tg_Tt() const { return tg_T() + (int64_t)mp * TG_LD; }
  double* tg_B() const { return tg_Tt() + (int64_t)mp * TG_LD; }
  double* tg_C() const { return tg_B() + (int64_t)mp * TG_LD; }
  // gprhip_eval_input_grad: the evaluation in flight also writes dl/d(training inputs) (input_grad.hip), per chunk in pass 2,
  // to xg_dst (point-major [n][D]); xg_engine: it takes the engine row path although its shape is one of small.hip / mid.hip
  // (those keep X only for single-chunk problems)
  bool xgrad = false, xg_engine = false;
  double* xg_dst = nullptr;
  double* xg_buf = nullptr;  // the library's own [n][D] destination of host-side callers (allocated at the first such call)
  double* xg_g = nullptr;    // [chunk][d] dl/d(projected points) of one chunk (projection hypers; allocated at first use)
  // gprhip_predict_input_grad: M = U^-1 (I - R~^-1 R~^-T) U^-T (mp x mp, full) of the current model state -- formed at the
  // first call that asks for a variance part, kept until an evaluation or gprhip_load_predictor clears pg_m_valid
  double* pg_m = nullptr;
  bool pg_m_valid = false;
  double* pg_buf = nullptr;  // gradient staging of one chunk: [2][rows][D] for a host destination + [2][rows][d] dp (projection)
  int64_t pg_rows = 0;       // rows it holds
  bool pg_host = false, pg_proj = false;  // ... with those two parts
  // gprhip_acquire_max_value: the extremes of the call on the device and their pinned mirror [GPRHIP_MAX_EXTREMES each]
  double *mv_extremes = nullptr, *mv_host = nullptr;
  // gprhip_acquire's selection: candidate lists of the slabs (device), the block of a piece's k winners [k (D + 2)] on the
  // device and its pinned mirror; made at the first call with top_k > 0
  void* acq_scratch = nullptr;
  double *acq_out = nullptr, *acq_host = nullptr;
  // gprhip_acquire_refine: one arena for the box, the state and trial points of the starts and the staging of host outputs
  // (rf_len doubles; grown when a call needs more), and the pinned count of starts that go on
  double* rf_buf = nullptr;
  int64_t rf_len = 0;
  int* rf_active = nullptr;
  // gprhip_sample_paths: the normal draws Z [mp][64] in pinned host memory that the weight kernel reads, R~^-1 Z and the
  // weights A (2 [mp][64]); F / eps of one chunk ([64][sp_rows] each, made when a call needs them); the selection's
  // candidate lists and the winners' blocks [64][64 (D + 2)] with their pinned mirror
  double *sp_zhost = nullptr, *sp_coef = nullptr;
  int sp_ns_last = 0;  // draws of the weights the second half of sp_coef holds; 0: none of the current model state
  double *sp_f = nullptr, *sp_eps = nullptr;
  int64_t sp_f_rows = 0, sp_eps_rows = 0;
  char* sp_scratch = nullptr;
  int64_t sp_scratch_bytes = 0;
  double *sp_out = nullptr, *sp_host = nullptr;
  // gprhip_observe: have_b -- bvec holds b = R~ (U t) of the current model state (every evaluation leaves it; a loaded predictor
  // forms it once, at the first call); n_observed -- observations folded in since the last evaluation or gprhip_load_predictor;
  // obs_buf -- the scratch of a call (obs_len doubles); post_slot -- gprhip_posterior_save's copy [R~ | R~^-1 | b | t~ | t],
  // released by an evaluation and by gprhip_load_predictor
  bool have_b = false;
  int64_t n_observed = 0;
  double* obs_buf = nullptr;
  int64_t obs_len = 0;
  double* post_slot = nullptr;
  int64_t slot_observed = 0;
  bool slot_have_b = false;
  bool use_small() const {
    return !multi && !xg_engine && small_path && !f32 && !engine_steps && small_path_fits(m, mp, d, has_proj() ? D : 0, n, has_ms());
  }
  // one or two 128-column tiles of inducing points that the small path does not take (65 .. 256 of them, or fewer with more
  // input dimensions than small.hip stages): the row passes and the finish stage of mid.hip
  bool use_mid_gram() const { return mid_gram && n <= MID_GRAM_ROWS; }
  bool use_mid() const {
    return !multi && !xg_engine && mid_path && !f32 && !engine_steps && !use_small() && mid_path_fits(m, mp, d, has_proj() ? D : 0, n, has_ms());
  }
  // two tiles whose Gram accumulations go through mid.hip's own launch pair (else: through the engine's launch)
  bool mid_pair() const { return use_mid() && mp > TILE && use_mid_gram(); }
};

// Several evaluations side by side (gprhip_batch_*): one internal problem per lane on the parent's device and stream, and ONE
// upload block -- per lane [parameter block (upload_hypers' layout) | the argument structs of the lane's eight launches],
// `stride` bytes apiece, so that the lanes in use are one contiguous transfer and lane j's structs lie at a fixed offset
// behind lane 0's (the batched kernels index them with blockIdx.y * stride)
struct gprhip_batch {
  gprhip_problem* parent = nullptr;  // null once the parent has been destroyed
  std::vector<gprhip_problem*> lanes;
  char *up_host = nullptr, *up_dev = nullptr;
  int64_t stride = 0;
  int64_t o_km = 0, o_p1 = 0, o_r1 = 0, o_fuse = 0, o_p2 = 0, o_r2 = 0, o_fin = 0, o_ship = 0;  // byte offsets in a lane's slice
  template <typename T> T* host(int j, int64_t off) const { return reinterpret_cast<T*>(up_host + j * stride + off); }
  template <typename T> const T* dev(int64_t off) const { return reinterpret_cast<const T*>(up_dev + off); }
};

namespace {

void batch_orphan_all(gprhip_problem* p) {
  for (gprhip_batch* b : p->batches) {
    b->parent = nullptr;
    for (gprhip_problem* l : b->lanes) {
      l->stream = nullptr;
      l->X = l->y = nullptr;
      l->have_inputs = l->have_targets = l->have_model = false;
    }
  }
  p->batches.clear();
}

template <typename TS> const TS* inv_u(const gprhip_problem* p);
template <> const double* inv_u<double>(const gprhip_problem* p) { return p->uinv; }
template <> const float* inv_u<float>(const gprhip_problem* p) { return p->uinv_f; }
// per-row weights of the SYRK-shaped launches in the engine's element type
template <typename TS> const TS* row_weights(gprhip_problem* p, const double* w, float* wf);
template <> const double* row_weights<double>(gprhip_problem*, const double* w, float*) { return w; }
template <> const float* row_weights<float>(gprhip_problem* p, const double* w, float* wf) {
  launch_to_float(w, wf, (int64_t)p->nchunks * p->chunk, p->stream);
  return wf;
}
template <typename TS> const TS* inv_r(const gprhip_problem* p);
template <> const double* inv_r<double>(const gprhip_problem* p) { return p->rinv; }
template <> const float* inv_r<float>(const gprhip_problem* p) { return p->rinv_f; }
template <typename TS> const TS* inv_rfull(const gprhip_problem* p);
template <> const double* inv_rfull<double>(const gprhip_problem* p) { return p->rfinv; }
template <> const float* inv_rfull<float>(const gprhip_problem* p) { return p->rfinv_f; }

void need_trustworthy_coeffs(gprhip_problem* p, const char* who);
void need_factors(gprhip_problem* p, const char* who);

template <typename T>
void release_buf(gprhip_problem* p, T*& q);

// a new model state (an evaluation, gprhip_load_predictor): the observations folded into the old one and the saved
// posterior slot of gprhip_posterior_save belong to that old state
void forget_observations(gprhip_problem* p) {
  p->have_b = false;
  p->n_observed = 0;
  release_buf(p, p->post_slot);
}

void tstart(gprhip_problem* p, const char* name) {
  if (!p->timer.on) return;
  hipEvent_t a, b;
  GPR_HIP(hipEventCreate(&a));
  GPR_HIP(hipEventCreate(&b));
  GPR_HIP(hipEventRecord(a, p->stream));
  p->timer.ev.push_back({name, {a, b}});
}
void tstop(gprhip_problem* p) {
  if (!p->timer.on) return;
  GPR_HIP(hipEventRecord(p->timer.ev.back().second.second, p->stream));
}
void tcollect(gprhip_problem* p) {
  p->tnames.clear();
  p->tms.clear();
  if (p->timer.k_recorded) {
    float ms = 0;
    hipEventElapsedTime(&ms, p->timer.k0, p->timer.k1);
    p->tnames.push_back("kernel_p1_syrk_B");
    p->tms.push_back(ms);
    p->timer.k_recorded = false;
  }
  for (auto& e : p->timer.ev) {
    float ms = 0;
    hipEventElapsedTime(&ms, e.second.first, e.second.second);
    bool found = false;
    for (size_t i = 0; i < p->tnames.size(); ++i)
      if (p->tnames[i] == e.first) {
        p->tms[i] += ms;
        found = true;
      }
    if (!found) {
      p->tnames.push_back(e.first);
      p->tms.push_back(ms);
    }
    hipEventDestroy(e.second.first);
    hipEventDestroy(e.second.second);
  }
  p->timer.ev.clear();
}

// Blocked upper Cholesky A = U^T U in place (dpotrf `U; lib/fitc_gp.ml:56) -- diagonal blocks in
// LDS, panel solve and trailing update on the MFMA engine.  dinv receives inv(U_jj) per block.
void potrf_upper_n(hipStream_t s, double* A, int mp, double* dinv, int* info, bool engine_steps, int m_real = 0) {
  // default: the engine-free step kernels of chol.hip (potrf_upper_blocked); engine_steps (GPRHIP_POTRF_ENGINE=1 at
  // problem creation) keeps the round-2 sequence below for A/B timing -- diagonal block with its full inverse, panel
  // and trailing update as engine launches
  if (!engine_steps) {
    potrf_upper_blocked(s, A, mp, dinv, info, nullptr, nullptr, m_real);
    return;
  }
  const int nb = mp / TILE;
  for (int j = 0; j < nb; ++j) {
    double* dj = dinv + (int64_t)j * TILE * TILE;
    launch_potrf_diag(A, mp, j, dj, info, s);
    if (j + 1 < nb) {
      const int rest = (nb - 1 - j) * TILE;
      double* panel = A + (int64_t)j * TILE * mp + (int64_t)(j + 1) * TILE;
      GemmArgs g;  // panel <- inv(U_jj)^T * panel   (in place: a block reads its whole column tile first)
      g.A = dj; g.lda = TILE; g.B = panel; g.ldb = mp; g.C = panel; g.ldc = mp;
      g.M = TILE; g.N = rest; g.K = TILE;
      launch_gemm(OP_TN, g, s);
      GemmArgs u;  // trailing <- trailing - panel^T panel  (upper tiles)
      u.A = panel; u.lda = mp; u.B = panel; u.ldb = mp;
      u.C = A + (int64_t)(j + 1) * TILE * mp + (int64_t)(j + 1) * TILE; u.ldc = mp;
      u.M = rest; u.N = rest; u.K = TILE; u.alpha = -1.0; u.beta = 1.0; u.upper_only = 1;
      launch_gemm(OP_TN, u, s);
    }
  }
}
void potrf_upper(gprhip_problem* p, double* A, int* info) {
  potrf_upper_n(p->stream, A, p->mp, p->dinv, info, p->engine_steps, p->m);
}

// k-slices of an m x m product of triangular factors: few output tiles, each up to m / 128 blocks deep.  From three
// 128-blocks on the k-range is split (slices end on block boundaries) -- at m = 512 the two products of the finish stage
// took 64 and 69 us as 16 workgroups of up to four blocks each (profiles/r05_timeline_n50000_m512.txt).
static int mxm_slices(int mp) { return mp >= 3 * TILE ? std::min(4, mp / TILE) : 1; }

// A non-batched m x m product with few output tiles and a long k-range, split over `ks` k-slices so that the
// launch fills the chip; partial products go to the split-K scratch and are summed in a fixed order.
void gemm_splitk(gprhip_problem* p, GemmOp op, GemmArgs g, int ks) {
  const int64_t mm = (int64_t)p->mp * p->mp;
  if (ks < 2 || (int64_t)ks * mm * 8 > p->slices_bytes || g.ldc != p->mp) {
    launch_gemm(op, g, p->stream);
    return;
  }
  double* const dst = g.C;
  g.C = static_cast<double*>(p->slices);
  g.kslices = ks;
  g.slice_stride = mm;
  launch_gemm(op, g, p->stream);
  launch_sum_slices_rect(static_cast<double*>(p->slices), ks, mm, g.M, g.N, p->mp, 1, 0, dst, p->stream);
}

// inv(U) for the upper-triangular factor by recursive doubling over the 128-blocks:
//   inv([U11 U12; 0 U22]) = [X11, -X11 U12 X22; 0, X22]
// Level s joins neighbouring inverted diagonal blocks of s rows; all joins of a level are independent
// and run as one batched launch (two per level: T = U12 X22, X12 = -X11 T), so the whole inverse is
// 2 log2(mp/128) launches instead of one short GEMM chain per block column.
void trtri_upper(gprhip_problem* p, const double* U, double* X, double* tmp) {
  const int mp = p->mp;
  hipStream_t s = p->stream;
  launch_scatter_diag_blocks(p->dinv, mp, X, s);
  for (int64_t sz = TILE; sz < mp; sz *= 2) {
    const int64_t pair = 2 * sz;
    const int nfull = (int)(mp / pair);                 // pairs with two full halves
    const int64_t rem = mp - (int64_t)nfull * pair;     // a trailing pair with a short second half?
    auto join = [&](int64_t off, int64_t s2, int nb) {
      // The late levels have few output tiles and long k-ranges: split k over up to 8 slices so the launch fills
      // the chip (partial products go to the split-K scratch at the destination's offsets, then a fixed-order sum)
      const int64_t blocks = (int64_t)nb * (sz / TILE) * (s2 / TILE);
      auto slices_for = [&](int64_t kdim) {
        int ks = 1;
        while (ks < 8 && blocks * ks * 2 <= 256 && kdim / (ks * 2) >= 256) ks *= 2;
        return (double*)p->slices && (int64_t)ks * mp * mp * 8 <= p->slices_bytes ? ks : 1;
      };
      double* const sl = static_cast<double*>(p->slices);
      // T = U12 * X22   (X22 upper triangular)
      GemmArgs a;
      a.A = U + off * mp + off + sz; a.lda = mp; a.B = X + (off + sz) * (mp + 1); a.ldb = mp;
      a.C = tmp + off * mp + off + sz; a.ldc = mp;
      a.M = (int)sz; a.N = (int)s2; a.K = (int)s2; a.tri = TRI_KHI_BN;
      a.nbatch = nb; a.batch_a = a.batch_b = a.batch_c = pair * (mp + 1);
      const int ksa = slices_for(s2);
      if (ksa > 1) {
        a.C = sl + off * mp + off + sz; a.kslices = ksa; a.slice_stride = (int64_t)mp * mp;
        launch_gemm(OP_NN, a, s);
        launch_sum_slices_rect(sl + off * mp + off + sz, ksa, (int64_t)mp * mp, (int)sz, (int)s2, mp, nb,
                               pair * (mp + 1), tmp + off * mp + off + sz, s);
      } else {
        launch_gemm(OP_NN, a, s);
      }
      // X12 = -X11 * T  (X11 upper triangular)
      GemmArgs b;
      b.A = X + off * (mp + 1); b.lda = mp; b.B = tmp + off * mp + off + sz; b.ldb = mp;
      b.C = X + off * mp + off + sz; b.ldc = mp;
      b.M = (int)sz; b.N = (int)s2; b.K = (int)sz; b.tri = TRI_KLO_BM; b.alpha = -1.0;
      b.nbatch = nb; b.batch_a = b.batch_b = b.batch_c = pair * (mp + 1);
      const int ksb = slices_for(sz);
      if (ksb > 1) {
        b.C = sl + off * mp + off + sz; b.kslices = ksb; b.slice_stride = (int64_t)mp * mp;
        launch_gemm(OP_NN, b, s);
        launch_sum_slices_rect(sl + off * mp + off + sz, ksb, (int64_t)mp * mp, (int)sz, (int)s2, mp, nb,
                               pair * (mp + 1), X + off * mp + off + sz, s);
      } else {
        launch_gemm(OP_NN, b, s);
      }
    };
    if (nfull > 0) join(0, sz, nfull);
    if (rem > sz) join((int64_t)nfull * pair, rem - sz, 1);
  }
}

// U = chol(A) in place and X = inv(U): one pass of the step kernels with the identity riding along as right-hand side
// (chol.hip); `tmp` is an mp x mp scratch
void potrf_trtri(gprhip_problem* p, double* A, double* X, double* tmp, int* info) {
  if (p->engine_steps) {
    potrf_upper(p, A, info);
    trtri_upper(p, A, X, tmp);
    return;
  }
#ifdef GPRHIP_LAB
  if (p->potrf_chain_mode && p->mp >= 2 * TILE) {
    if (!p->chain) p->chain = potrf_chain_create(p->mp);
    if (p->chain) {
      potrf_upper_chain(p->stream, p->chain, A, p->mp, p->dinv, info, tmp, X, p->m);
      return;
    }
  }
#endif
  potrf_upper_blocked(p->stream, A, p->mp, p->dinv, info, tmp, X, p->m, p->potrf_aux.side ? &p->potrf_aux : nullptr);
}

// C (upper tiles) = X X^T for upper-triangular X: (U^T U)^-1 = U^-1 U^-T   (Utils.ichol, lib/utils.ml:110-113)
void triu_xxt(gprhip_problem* p, const double* X, double* C, hipStream_t st) {
  GemmArgs g;
  g.A = X; g.lda = p->mp; g.B = X; g.ldb = p->mp; g.C = C; g.ldc = p->mp;
  g.M = p->mp; g.N = p->mp; g.K = p->mp; g.tri = TRI_KLO_MAX; g.upper_only = 1;
  // few tiles, long triangular k-ranges: four k-slices (ending on block boundaries) fill the chip
  const int64_t mm = (int64_t)p->mp * p->mp;
  const int ks = (mxm_slices(p->mp) > 1 && 4 * mm * 8 <= p->slices_bytes) ? mxm_slices(p->mp) : 1;
  if (ks > 1) {
    g.C = static_cast<double*>(p->slices);
    g.kslices = ks;
    g.slice_stride = mm;
    launch_gemm(OP_NT, g, st);
    launch_sum_slices<double>(nullptr, static_cast<double*>(p->slices), ks, mm, p->mp, C, st);
  } else {
    launch_gemm(OP_NT, g, st);
  }
}

void check_hypers(const gprhip_problem* p, const gprhip_hypers* h) {
  if (!h || !h->inducing) {
    set_error("gprhip: hypers/inducing pointer is NULL");
    throw HipFail{ST_BAD_ARG};
  }
  if (h->sigma2 < 0.0) {
    set_error("Model.check_sigma2: sigma2 < 0");  // lib/fitc_gp.ml:148-149
    throw HipFail{ST_BAD_ARG};
  }
  if (p->kind == GPRHIP_COV_SE_ISO && h->tproj) {
    set_error("gprhip: tproj given for Cov_se_iso");
    throw HipFail{ST_BAD_ARG};
  }
  if (p->kind == GPRHIP_COV_SE_FAT && !h->tproj && p->D != p->d) {
    set_error("gprhip: Cov_se_fat without tproj needs D == d");
    throw HipFail{ST_BAD_ARG};
  }
  if (p->kind == GPRHIP_COV_SE_ISO && h->log_hetero_skedasticity) {
    set_error("gprhip: log_hetero_skedasticity given for Cov_se_iso");
    throw HipFail{ST_BAD_ARG};
  }
  if (h->log_multiscales_m05 && p->kind == GPRHIP_COV_SE_ISO) {
    set_error("gprhip: log_multiscales_m05 given for Cov_se_iso");
    throw HipFail{ST_BAD_ARG};
  }
}

// the host half of an upload: p->h, p->cp and the pinned parameter block; returns the doubles of the block in use (a prefix)
int64_t stage_hypers(gprhip_problem* p, const gprhip_hypers* h) {
  p->h = *h;                // (after every argument check: a refused call leaves no borrowed pointer behind)
  p->h.inducing = nullptr;  // borrowed; the padded copy lives in hZ
  // the optional arrays are presence flags from here on, pointing at the library's own pinned copies (filled below)
  p->h.tproj = h->tproj ? p->hTproj : nullptr;
  p->h.log_hetero_skedasticity = h->log_hetero_skedasticity ? p->hHet : nullptr;
  p->h.log_multiscales_m05 = h->log_multiscales_m05 ? p->hMs : nullptr;
  int64_t used = (int64_t)p->mp * p->d + 64;  // doubles of the block this evaluation uploads (a prefix)
  if (h->log_hetero_skedasticity) {  // Kernel.create: Vec.map exp, lib/cov_se_fat.ml:63-65
    for (int i = 0; i < p->m; ++i) p->hHet[i] = std::exp(h->log_hetero_skedasticity[i]);
    for (int i = p->m; i < p->mp; ++i) p->hHet[i] = 0.0;
    p->h.log_hetero_skedasticity = p->hHet;  // only used as a presence flag from here on
    used = (p->hHet - p->hy_host) + p->mp;
  }
  if (h->log_multiscales_m05) {
    // Kernel.create: exp v +. 0.5, lib/cov_se_fat.ml:66-69 ; Fortran d x m == [m][d]; padding rows 1
    for (int64_t i = 0; i < (int64_t)p->m * p->d; ++i) p->hMs[i] = std::exp(h->log_multiscales_m05[i]) + 0.5;
    for (int64_t i = (int64_t)p->m * p->d; i < (int64_t)p->mp * p->d; ++i) p->hMs[i] = 1.0;
    p->h.log_multiscales_m05 = p->hMs;  // presence flag from here on
    used = (p->hMs - p->hy_host) + (int64_t)p->mp * p->d;
  }
  CovParams& cp = p->cp;
  cp.kind = p->kind;
  cp.ms = h->log_multiscales_m05 ? p->ms : nullptr;
  cp.log_sf2 = h->log_sf2;
  cp.sf2 = std::exp(h->log_sf2);
  if (p->kind == GPRHIP_COV_SE_ISO) {
    cp.inv_ell2 = std::exp(-2.0 * h->log_ell);  // lib/cov_se_iso.ml:41-44
    cp.inv_ell2_05 = -0.5 * cp.inv_ell2;
  } else {
    cp.inv_ell2 = 1.0;
    cp.inv_ell2_05 = -0.5;
  }
  // inducing: Fortran d x m == point-major [m][d]; pad to mp rows with zeros
  std::memcpy(p->hZ, h->inducing, (size_t)p->m * p->d * sizeof(double));
  std::memset(p->hZ + (size_t)p->m * p->d, 0, (size_t)(p->mp - p->m) * p->d * sizeof(double));
  {  // centroid of the inducing points
    for (int k = 0; k < 64; ++k) p->hShift[k] = 0.0;
    for (int c = 0; c < p->m; ++c)
      for (int k = 0; k < p->d && k < 64; ++k) p->hShift[k] += p->hZ[(size_t)c * p->d + k];
    for (int k = 0; k < 64; ++k) p->hShift[k] /= p->m;
  }
  if (h->tproj) {
    std::memcpy(p->hTproj, h->tproj, (size_t)p->D * p->d * sizeof(double));  // borrowed pointer: copy before returning
    p->h.tproj = p->hTproj;
    used = std::max<int64_t>(used, (p->hTproj - p->hy_host) + (int64_t)p->D * p->d);
  }
  return used;
}

void upload_hypers(gprhip_problem* p, const gprhip_hypers* h) {
  check_hypers(p, h);
  // the pinned block may still be the source of the previous evaluation's transfer (a pass 1 repeated without a finish)
  GPR_HIP(hipEventSynchronize(p->ev_hy));
  const int64_t used = stage_hypers(p, h);
  GPR_HIP(hipMemcpyAsync(p->hy_dev, p->hy_host, (size_t)used * sizeof(double), hipMemcpyHostToDevice, p->stream));
  GPR_HIP(hipEventRecord(p->ev_hy, p->stream));
  if (h->tproj) launch_project(p->X, p->n, p->D, p->d, p->tproj, p->P, p->stream);
}

// Split-K factor of the SYRK-shaped accumulations over training points.  Slices are dealt to the
// 8 XCDs (mfma_gemm.hip), so the factor is a multiple of 8.  Blocks of one slice share their operand
// rows through the XCD's L2 while they run in step.  Measured at n=1M, m=2048 (rocprofv3 FETCH_SIZE per launch,
// against 16.4 GB of V): 60 GB through the fabric for 2k-, 4k- and 8k-row slices alike once every workgroup of the
// launch runs the same loop (mfma_gemm.hip) -- the re-fetch factor is set by the stagger of workgroup start times
// against the L2 window, not by the slice length -- and the step is fastest with 8k..16k-row slices (381.6 ms;
// 385 ms at 4k and at 32k), so slices are kept near `slice_rows`.  Among nearby factors the one whose
// (tiles x slices / 8) fills whole residency rounds of an XCD (32 CUs x 2 blocks) is taken.
int pick_kslices(int mp, int64_t rows_p, int max_slices, int64_t slice_rows, bool f64) {
  const int nt = mp / TILE, tiles = nt * (nt + 1) / 2;
  const int slots = std::max(8, gemm_resident_slots() / 8);  // workgroups one XCD holds at a time (64 on MI355X)
  auto items_of = [&](int ks) {  // items of one XCD: off-diagonal tiles per slice + the diagonal tiles' own slices
    const int ksd = gemm_syrk_diag_slices(ks, f64, true);
    return (tiles - nt) * (ks / 8) + nt * ((ksd + 7) / 8);
  };
  if (rows_p < 32 * slice_rows) {
    // Mid-size shards (round 5): with few tiles (36 at m = 1024, 10 at m = 512) and few `slice_rows`-sized slices the
    // launch is one or two badly filled residency rounds -- 72 items per XCD for 64 slots at n = 100 000, m = 1024, ten
    // items at n = 50 000, m = 512.  Here the factor is chosen over the WHOLE feasible range by the time a launch of that
    // shape takes: residency rounds (the last, partial one at about half price while it leaves every CU a single
    // workgroup) x (fixed cost of an item + its rows at half a CU's matrix rate) + the slice sum that follows.
    const double t_fixed = 10.0, t_row = f64 ? 0.22 : 0.11;  // us per item; us per training point of a 128 x 128 tile item
    int best = 8;
    double best_t = 1e300;
    for (int ks = 8; ks <= max_slices / 8 * 8; ks += 8) {
      if ((int64_t)ks * TILE > rows_p && ks > 8) break;  // at least 128 training points per slice
      const int items = items_of(ks);
      const int full = items / slots, rem = items % slots;
      // a partly filled round behind full ones costs a whole round (the dispatcher refills CUs in pairs of slots as they fall
      // free, so its workgroups still share their CUs: profiles/r05_ts_nn_m1024.txt); a launch that never fills the chip
      // runs one workgroup per CU at nearly twice the speed
      const double rounds = full + (rem == 0 ? 0.0 : (full == 0 && rem <= slots / 2 ? 0.55 : 1.0));
      const double t_item = t_fixed + (double)rows_p / ks * t_row;
      const double t_sum = (double)ks * tiles * TILE * TILE * (f64 ? 8.0 : 4.0) / 3.0e6;  // us at 3 TB/s
      const double t = rounds * t_item + t_sum;
      if (t < best_t - 1e-9) {
        best_t = t;
        best = ks;
      }
    }
    return best;
  }
  int target = (int)((rows_p / slice_rows + 7) / 8 * 8);
  target = std::max(8, std::min(target, max_slices / 8 * 8));
  int best = target;
  double best_eff = 0.0;
  for (int ks = std::max(8, target - 16); ks <= std::min(max_slices / 8 * 8, target + 16); ks += 8) {
    if ((int64_t)ks * BK * 8 > rows_p && ks > 8) continue;
    const int items = items_of(ks);
    const double eff = (double)items / ((double)((items + slots - 1) / slots) * slots);
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = ks;
    }
  }
  return best;
}

// Training points per workgroup of the gradient kernels: grad_slab_rows (256 or 1024 by the accumulator rows), halved down
// to 64 while a launch -- min(n, chunk) rows -- would leave most of the chip idle.  GPRHIP_GRAD_SLAB overrides with one of
// the sizes the kernels and their partial buffers are exercised with: 64, 128, 256, 512, 1024 (anything else is rounded
// down to the next of these).
int pick_grad_slab(int col_rows, int64_t n, int64_t chunk, int mp) {
  int slab = grad_slab_rows(col_rows);
  const int64_t rows = std::min(n, chunk);
  while (slab > 64 && ((rows + slab - 1) / slab) * (int64_t)(mp / TILE) < 256) slab /= 2;
  if (const char* e = getenv("GPRHIP_GRAD_SLAB")) {
    const int want = atoi(e);
    slab = 64;
    while (slab < 1024 && slab * 2 <= want) slab *= 2;
  }
  return slab;
}

// Row chunking and split-K scratch of a problem: one place, used by the creation entry point and by the memory plan.
struct Sizing {
  int64_t chunk = 0, slice_rows = 8192;
  int nchunks = 0, kslices = 8;
};
Sizing problem_sizing(int64_t n, int mp, int64_t chunk_rows, bool f64) {
  Sizing z;
  int64_t chunk = chunk_rows > 0 ? chunk_rows : 131072;
  if (const char* e = getenv("GPRHIP_CHUNK_ROWS")) chunk = atoll(e);
  chunk = round_up(std::min<int64_t>(std::max<int64_t>(chunk, 1), round_up(n, TILE)), TILE);
  z.chunk = chunk;
  z.nchunks = (int)((n + chunk - 1) / chunk);
  // partial-sum buffers of the split-K SYRK launches: one m x m slice per `slice_rows` training points, capped at 40 GB
  // (fp32-bulk mode: fp32 accumulation runs over one slice before the fp64 slice sum.  Measured at config 3 against
  // the fp64 evaluation, tools/lab10.sh: 2048 / 4096 / 8192 / 16384-row slices give the evidence to 7.4e-8 / 7.3e-8 /
  // 5.6e-8 / 2.3e-8 and SYRK launches of 119.9 / 120.3 / 119.0 / 118.9 ms -- no reason for shorter slices than fp64's.)
  if (const char* e = getenv("GPRHIP_SLICE_ROWS")) z.slice_rows = std::max<int64_t>(1024, atoll(e));
  const int64_t mm8 = (int64_t)mp * mp * 8;
  z.kslices = (int)std::max<int64_t>(8, std::min<int64_t>((round_up(n, z.slice_rows) / z.slice_rows + 23) / 8 * 8, (40LL << 30) / mm8 / 8 * 8));
  if (n < 32 * z.slice_rows) {
    // mid-size shards take many short slices: exactly the factor pick_kslices will choose for this shape (it depends on
    // (m, rows, cap) only) within a cap of 128 slices / 2 GB -- not the cap itself, which at n = 100 000, m = 1024 was 1 GB
    // of scratch beside a 0.8 GB V store; the m x m products that borrow the scratch need eight slices
    const int cap = (int)std::max<int64_t>(8, std::min<int64_t>(128, (2LL << 30) / mm8 / 8 * 8));
    const int64_t rows_p = (int64_t)(z.nchunks - 1) * chunk + round_up(n - (int64_t)(z.nchunks - 1) * chunk, TILE);
    z.kslices = std::max(8, pick_kslices(mp, rows_p, cap, z.slice_rows, f64));
  }
  if (const char* e = getenv("GPRHIP_KSLICES")) z.kslices = std::max(8, atoi(e) / 8 * 8);
  return z;
}

// Bytes a problem holds on its device (gprhip_memory_plan).  Everything gprhip_problem_create allocates plus the V store
// the first evaluation adds; the optional copy of K_nm (Cov_se_fat with projection hypers) is listed but not counted -- it
// is only taken while it leaves room.
void memory_plan(int cov_kind, int precision, int64_t n, int D, int d, int m, int64_t chunk_rows, gprhip_memory_plan_t* o) {
  const int mp = (int)round_up(m, TILE);
  const bool f32 = precision == GPRHIP_F32_BULK, fat = cov_kind == GPRHIP_COV_SE_FAT;
  const int64_t esz = f32 ? 4 : 8, mm = (int64_t)mp * mp;
  const Sizing z = problem_sizing(n, mp, chunk_rows, !f32);
  const int64_t npad = (int64_t)z.nchunks * z.chunk;
  std::memset(o, 0, sizeof *o);
  o->chunk_rows = z.chunk;
  o->kslices = z.kslices;
  o->inputs = (n * D + npad + (fat ? n * d : 0)) * 8;
  o->row_vectors = npad * 8 * (5 + (fat ? 1 : 0)) + (f32 ? npad * 4 * 3 : 0);
  o->v_store = npad * mp * esz;
  o->k_store_optional = fat ? npad * mp * esz : 0;
  o->chunk_buffers = 2 * z.chunk * mp * esz + 2 * z.chunk * 4 * (mp / TILE) * 8;
  o->slices = (int64_t)z.kslices * mm * esz + (int64_t)z.kslices * mp * 8;
  o->mxm = 10 * mm * 8 + (f32 ? 3 * mm * 4 : 0) + (int64_t)mp * TILE * 8 + (int64_t)(mp / TILE) * TILE * TILE * 8;
  const int64_t col_rows = d + 1 + (fat ? D + d : 0), km_rows = d + 2 + (fat ? d : 0);
  const int gslab = pick_grad_slab((int)col_rows, n, z.chunk, mp);
  const int64_t nslab = (z.chunk + gslab - 1) / gslab;
  o->rest = (gprhip_exchange_len(cov_kind, D, d, m, 1) + gprhip_exchange_len(cov_kind, D, d, m, 2)) * 8 +
            nslab * col_rows * mp * 8 + (fat ? ((z.chunk + 255) / 256) * (int64_t)D * d * 8 : 0) +
            (int64_t)((m + km_slab_rows(m) - 1) / km_slab_rows(m)) * km_rows * mp * 8 + (int64_t)(8 + km_rows + col_rows) * mp * 8;
  o->total = o->inputs + o->row_vectors + o->v_store + o->chunk_buffers + o->slices + o->mxm + o->rest;
}

template <typename TS>
void cov_chunk(gprhip_problem* p, int c, TS* K, hipStream_t s = nullptr) {
  const int64_t rows = p->rows_of(c);
  const int64_t rows_p = round_up(rows, TILE);
  const double* pts = p->pts() + (int64_t)c * p->chunk * p->d;
  launch_cov_cross<TS>(p->cp, pts, (int)rows, (int)rows_p, p->Z, p->m, p->mp, p->d, K, s ? s : p->stream, p->zshift);
}

// ---- several target vectors (targets.hip): the k-column steps around the model-only engine passes
// Pass 1, after the row vectors: c~ = V^T diag(1/s) Y (m x k) over the resident V, and the k sums y_k^T diag(1/s) y_k
void targets_pass1(gprhip_problem* p) {
  hipStream_t s = p->stream;
  tstart(p, "p1_targets");
  launch_targets_vty(static_cast<const double*>(p->Vstore), p->mp, p->n, p->mp, 0, p->is, p->tg_y, 1, p->npad(), p->multi,
                     p->tg_part, p->tg_C(), s);
  launch_targets_y2(p->tg_y, p->npad(), p->is, p->n, p->multi, p->tg_rowpart, p->tg_y2(), s);
  tstop(p);
}
// Middle: B = R~^-T c~ (column k = Q_n^T y~_k, lib/fitc_gp.ml:285-286), T~ = R~^-1 B, T = U^-1 T~ (:291), |b_k|^2
void targets_middle(gprhip_problem* p) {
  hipStream_t s = p->stream;
  const int mp = p->mp, k = p->multi;
  tstart(p, "mid_targets");
  launch_targets_vty(p->rinv, mp, mp, mp, 1, nullptr, p->tg_C(), TG_LD, 1, k, p->tg_part, p->tg_B(), s);
  launch_targets_colsq(p->tg_B(), mp, p->tg_bb(), s);
  launch_targets_rows(p->rinv, mp, mp, mp, 1, p->tg_B(), k, p->tg_Tt(), TG_LD, 1, s);
  launch_targets_rows(p->uinv, mp, mp, mp, 1, p->tg_Tt(), k, p->tg_T(), TG_LD, 1, s);
  tstop(p);
}
// Pass 2, one row chunk, after the Q' launch and the (model-only) row kernel: W_mat = diag(1/s) (Y - Q' B), then
// v = v1 - mean_k w_k^2 and the row sums of E accordingly
void targets_pass2_rows(gprhip_problem* p, const double* Q, int64_t base, int rows, double* es, double* sumv) {
  hipStream_t s = p->stream;
  tstart(p, "p2_targets");
  launch_targets_rows(Q, p->mp, rows, p->mp, 0, p->tg_B(), p->multi, p->tg_w + base, 1, p->npad(), s);
  launch_targets_p2_rows(p->tg_y + base, p->tg_w + base, p->npad(), p->is + base, p->r + base, p->cp.sf2, rows, p->multi,
                         p->v + base, es, p->tg_rowpart, sumv, s);
  tstop(p);
}
// ... after the X launch (run with w = 0): X -= (1/k) W_mat T^T, the rank-k form of the ger of lib/fitc_gp.ml:1204-1206
void targets_xcorr(gprhip_problem* p, double* X, int64_t base, int rows) {
  tstart(p, "p2_xcorr");
  launch_targets_xcorr(X, rows, p->mp, p->tg_w + base, p->npad(), p->tg_T(), p->multi, p->stream);
  tstop(p);
}

// ---- the two exchange buffers by part (gprhip_exchange_len has the lengths)
// exchange 1: [packed upper tiles of B~_part | c~ (mp) | scalar tail (A1_TAIL)]
template <typename T> struct Ex1 { T *tiles, *c, *tail; };
template <typename T> Ex1<T> ex1_of(const gprhip_problem* p, T* ar1) {
  T* c = ar1 + packed_upper_len(p->mp);
  return {ar1, c, c + p->mp};
}
// exchange 2: [packed upper tiles of G~_part | column block (col_rows x mp) | `Proj second term (D x d) | scalar tail (A2_TAIL)]
// The host mirror (ex_host + A1_TAIL) starts at the column block: ex2_proj_off / ex2_tail_off count from there.
int64_t ex2_proj_off(const gprhip_problem* p) { return p->col_rows() * p->mp; }
int64_t ex2_tail_off(const gprhip_problem* p) { return ex2_proj_off(p) + (int64_t)p->dbig() * p->d; }
template <typename T> struct Ex2 {
  T *tiles, *col, *proj, *tail;
  int64_t len_from_col() const { return (tail + A2_TAIL) - col; }  // what the host assembly reads after a gradient evaluation
};
template <typename T> Ex2<T> ex2_of(const gprhip_problem* p, T* ar2) {
  T* col = ar2 + packed_upper_len(p->mp);
  return {ar2, col, col + ex2_proj_off(p), col + ex2_tail_off(p)};
}

// ---- scratch of an evaluation: everything its path allocates lazily, at the first evaluation that needs it (pass 1, once
// the path is known; pass 2 and the finish stage allocate nothing)
template <typename TS>
void ensure_eval_scratch(gprhip_problem* p, bool small, bool mid, bool reuse) {
  const int mp = p->mp;
  if (!p->Vstore)  // V = K U^-1 for all rows of the shard stays resident (one SYRK launch; pass 2 re-reads it)
    p->Vstore = p->alloc<TS>((int64_t)p->nchunks * p->chunk * mp);
  if (small) {
    if (!p->small_part) p->small_part = p->alloc<double>(small_part_len(p->d, p->D));
    if (!reuse && !p->small_k && p->d <= 8 && !p->has_ms()) p->small_k = p->alloc<double>(round_up(p->n, TILE) * 64);
  }
  if (mid) {
    if (!p->mid_part) p->mid_part = p->alloc<double>(mid_part_len(mp, p->d, p->D));
    if (p->mid_pair() && !p->mid_gram_part) p->mid_gram_part = p->alloc<double>(mid_gram_part_len());
    if (p->want_grad && !p->mid_done) {  // (every finish launch pair leaves the counter at zero again)
      p->mid_done = p->alloc<int>(1);
      GPR_HIP(hipMemsetAsync(p->mid_done, 0, sizeof(int), p->stream));
    }
  }
  if (!small && !mid && p->want_grad && p->has_ms() && p->has_proj() && !p->rowes) {
    const int nslots = 4 * ((mp + 255) / 256);  // (as the gradient kernels of pass 2 lay them out)
    p->rowes = p->alloc<double>(p->chunk * nslots * p->d);
    p->es2 = p->alloc<double>(p->chunk * p->d);
  }
}

// K resident (see Kstore): decided at the first gradient evaluation that can use it, kept for the problem's life.  An
// attempt that finds no room fails silently: the gradient kernel then recomputes K.
template <typename TS>
void try_k_resident(gprhip_problem* p) {
  if (p->Kstore || p->kstore_tried || !p->want_grad || !p->k_resident || !p->has_proj() || p->has_ms() || p->d > 64 || p->D > 64 ||
      p->grad_scalar)
    return;
  p->kstore_tried = true;
  size_t free_b = 0, total_b = 0;
  const size_t need = (size_t)p->nchunks * p->chunk * p->mp * sizeof(TS);
  // taken only while it leaves 4 GB free AND stays below 40 % of the device's memory: the copy is held for the life of
  // the problem, and other problems (fitc_gp caches several per functor; other shards may share the device) must still
  // find room.  GPRHIP_K_RESIDENT=0 never keeps it.
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > need + (size_t(4) << 30) && need <= total_b / 5 * 2) {
    void* ptr = nullptr;
    if (hipMalloc(&ptr, need) == hipSuccess) {
      p->allocs.push_back(ptr);
      p->Kstore = ptr;
    } else {
      (void)hipGetLastError();  // no room after all: the gradient kernel recomputes K
    }
  }
}

// Level-1 timer: an event pair around the dominant kernel alone (the pass-1 Gram launch).
template <typename F>
void kernel_timed(gprhip_problem* p, bool timed, F&& launch) {
  timed = timed && p->timer.kernel;
  if (timed) {
    if (!p->timer.k0) {
      GPR_HIP(hipEventCreate(&p->timer.k0));
      GPR_HIP(hipEventCreate(&p->timer.k1));
    }
    GPR_HIP(hipEventRecord(p->timer.k0, p->stream));
  }
  launch();
  if (timed) {
    GPR_HIP(hipEventRecord(p->timer.k1, p->stream));
    p->timer.k_recorded = true;
  }
}

// The Gram accumulation over all rows of the shard (V is resident), reduced into the packed upper tiles of an exchange
// buffer:
//   pass 1:  B~_part = V^T diag(is) V  (R~^T R~ replaces the stacked QR's R, lib/fitc_gp.ml:170-182) into exchange 1, and
//            c~ = V^T (is .* y) into `csum`;
//   pass 2:  G~_part = V^T diag(v) V  (the two dsyrk of lib/fitc_gp.ml:1198-1203, whitened, in one) into exchange 2.
// mid_pair: by mid.hip's Gram launch pair (two tiles; the engine's SYRK-shaped launch, its column-sum reduction and its
// slice sum cost 45 us at these sizes whatever the row count); else one SYRK-shaped engine launch + its reductions.
template <typename TS>
void gram_over_v(gprhip_problem* p, int pass, bool mid_pair, double* tiles, double* csum) {
  hipStream_t s = p->stream;
  const int mp = p->mp;
  const bool p1 = pass == 1;
  tstart(p, p1 ? "p1_syrk_B" : "p2_syrk_W");
  if (mid_pair) {
    MidGramArgs ga;
    ga.V = static_cast<const double*>(p->Vstore); ga.w = p1 ? p->is : p->v; ga.y = p1 ? p->yis : nullptr; ga.rows = (int)p->n;
    ga.part = p->mid_gram_part;
    // (the level-1 bracket goes around a fresh evaluation's launch; a re-weighted one has never carried it)
    kernel_timed(p, p1 && !p->h.reuse_v, [&] { launch_mid_gram(ga, tiles, p1 ? csum : nullptr, s); });
    tstop(p);
    return;
  }
  const int64_t mm = (int64_t)mp * mp, ktot = p->rows_total_padded();
  TS* const Vstore = static_cast<TS*>(p->Vstore);
  TS* const slices = static_cast<TS*>(p->slices);
  const int ks = p1 ? pick_kslices(mp, ktot, p->kslices, p->slice_rows, !p->f32) : p->ks_used;
  GemmArgsT<TS> g;
  g.A = Vstore; g.lda = mp; g.B = Vstore; g.ldb = mp; g.C = slices; g.ldc = mp;
  g.M = mp; g.N = mp; g.K = (int)ktot; g.beta = 0.0; g.upper_only = 1;
  g.scale_k = p1 ? row_weights<TS>(p, p->is, p->is_f) : row_weights<TS>(p, p->v, p->v_f);
  g.kslices = ks; g.slice_stride = mm;
  // The pass-2 launch goes through the kernel of the pass-1 one (its diagonal tiles then also form column sums nobody
  // reads): measured in round 4, the plain weighted kernel (gemm_*_tn_w) runs this very launch with 172 GB instead of
  // 67 GB through the fabric and 1-2 ms slower on most boxes of the pool -- its workgroups fall out of step from the
  // first residency round on -- while the column-sum kernel does not (tools/lab19.sh, lab20.sh; GPRHIP_W_AS_WS=0 restores
  // the plain kernel).
  const bool colsums = p1 || p->w_as_ws != 0;
  if (colsums) {
    // pass 1: c~ rides along -- the diagonal-tile blocks of every k-slice also sum V[k][c] * (is*y)[k] over their rows
    g.cs_w = p1 ? row_weights<TS>(p, p->yis, p->yis_f) : g.scale_k;
    g.cs_out = p->gemvpart;
  }
  kernel_timed(p, p1, [&] { launch_gemm(OP_TN, g, s); });
  const int ksd = gemm_syrk_diag_slices(ks, !p->f32, colsums);  // the diagonal tiles (which also store the column sums) use fewer, longer slices
  if (p1) launch_reduce_rows(p->gemvpart, ksd, mp, csum, 1, s);
  tstop(p);
  if (p1) p->ks_used = ks;
  launch_sum_slices<TS>(nullptr, slices, ks, mm, mp, tiles, s, 1, ksd);
}

// ---- pass 1
// K_nm of the first chunk does not depend on U: it is built on the second stream while the (latency-bound, few-CU)
// factorisation and inversion of K_m run -- 0.4 ms of every evaluation, which is what a chunk's builder takes.
// (Not under the per-stage timer, whose events sit on the main stream.)
template <typename TS>
void fork_first_cov(gprhip_problem* p) {
  GPR_HIP(hipEventRecord(p->ev_fork, p->stream));  // hypers, inducing points and projections are enqueued on the main stream
  GPR_HIP(hipStreamWaitEvent(p->stream2, p->ev_fork, 0));
  cov_chunk<TS>(p, 0, static_cast<TS*>(p->Kstore ? p->Kstore : p->bufA), p->stream2);
  GPR_HIP(hipEventRecord(p->ev_join, p->stream2));
}

// U = chol(K_m + jitter) and U^-1.  clear_c: c~ and the tail of exchange 1 are accumulated into by this evaluation's row
// pass (the small and the one-tile passes write them outright)
void pass1_km_chol(gprhip_problem* p, const Ex1<double>& ex, bool clear_c) {
  hipStream_t s = p->stream;
  const int mp = p->mp;
  tstart(p, "km_chol");
  // the scalars and the two potrf flags behind them (single-block problems: every slot an evaluation reads is written by
  // the factorisation kernels themselves, flags included), and the accumulators of the exchange-1 tail (the small row pass
  // writes them outright)
  if (mp != TILE || p->engine_steps) GPR_HIP(hipMemsetAsync(p->scal, 0, (NSCAL + 2) * sizeof(double), s));
  // (the one-tile passes write c~ and the tail outright; with two tiles c~ still comes from the Gram launch, accumulated)
  if (clear_c) GPR_HIP(hipMemsetAsync(ex.c, 0, (size_t)(mp + A1_TAIL) * sizeof(double), s));
  // K_m + (hetero) + jitter goes straight into the factor's buffer (kj is scratch of the finish stage only)
  // (tried for 65 .. 128 inducing points too, round 6: 16 384 entries on ONE CU cost 20 us at d = 8 where the cov_upper launch
  //  spread over the chip costs 4 + its 4 us gap -- K_m phase 45 -> 68 us; it stays a launch of its own above 64)
  if (mp == TILE && p->m <= 64 && p->d <= 16 && !p->engine_steps && !p->has_ms() && p->small_path) {
    PotrfKm g;  // few inducing points: the covariance is built inside the factorisation kernel (chol.hip, MODE 2)
    g.cp = p->cp; g.Z = p->Z; g.m = p->m; g.d = p->d; g.jitter = p->h.jitter;
    g.het = p->has_het() ? p->het : nullptr; g.km = p->km;
    launch_potrf_km(g, p->umat, p->uinv, p->info, s);
  } else {
    launch_cov_upper(p->cp, p->Z, p->m, mp, p->d, p->h.jitter, p->has_het() ? p->het : nullptr, p->km, p->umat, s);
    potrf_trtri(p, p->umat, p->uinv, p->wmat, p->info);  // U = chol(K_m + jitter), lib/fitc_gp.ml:53-57, and U^-1
  }
  if (p->f32) launch_to_float(p->uinv, p->uinv_f, (int64_t)mp * mp, s);
  tstop(p);
}

// the fields the one-kernel row passes of small.hip and mid.hip share
template <typename Args>
void fill_row_pass1(const gprhip_problem* p, Args& a) {
  a.cp = p->cp; a.pts = p->pts(); a.Z = p->Z; a.uinv = p->uinv; a.y = p->h.model_only ? nullptr : p->y;
  a.rows = (int)p->n; a.rows_p = (int)round_up(p->n, TILE); a.m = p->m; a.mp = p->mp; a.d = p->d;
  a.sigma2 = p->h.sigma2;
  a.V = static_cast<double*>(p->Vstore); a.r = p->r; a.is = p->is; a.yis = p->yis;
}

// at most 64 inducing points: covariance, V, the row quantities and both accumulations in one kernel + one reduction
// (small.hip)
void pass1_small(gprhip_problem* p, const Ex1<double>& ex) {
  tstart(p, "p1_small");
  SmallPass1Args a;
  fill_row_pass1(p, a);
  a.part = p->small_part;
  a.Kout = (p->d <= 8 && !p->has_ms()) ? p->small_k : nullptr;
  launch_small_pass1(a, ex.tiles, ex.c, ex.tail, p->stream);
  p->small_k_valid = a.Kout != nullptr;
  tstop(p);
  p->have_k = false;
}

// one or two 128-column tiles of inducing points: the same in one kernel per row block with the triangular operand
// streamed from memory (mid.hip).  One tile: that kernel accumulates B~ and c~ as well.  Two tiles: mid rows, then the Gram
// accumulation -- by mid.hip's launch pair, or by the engine's launch (GPRHIP_MID_GRAM=0, shards above MID_GRAM_ROWS)
void pass1_mid(gprhip_problem* p, const Ex1<double>& ex) {
  tstart(p, "p1_mid");
  MidPass1Args a;
  fill_row_pass1(p, a);
  a.part = p->mid_part;
  launch_mid_pass1(a, ex.tiles, ex.c, ex.tail, p->stream);
  tstop(p);
  if (p->mp > TILE) gram_over_v<double>(p, 1, p->mid_pair(), ex.tiles, ex.c);
  p->have_k = false;
}

// the chunked engine path: per row chunk K, V = K U^-1 and the row quantities (reuse: the row quantities alone, from the
// resident V and r), then one Gram accumulation over all rows.  Re-weighted evaluations (reuse_v) of every path come here.
template <typename TS>
void pass1_engine(gprhip_problem* p, const Ex1<double>& ex, bool reuse, bool cov0_ahead) {
  hipStream_t s = p->stream;
  const int mp = p->mp;
  TS* const Vstore = static_cast<TS*>(p->Vstore);
  TS* const Kstore = static_cast<TS*>(p->Kstore);
  TS* const bufA = static_cast<TS*>(p->bufA);
  // Overlap (GPRHIP_COV_OVERLAP=1): chunk c + 1's covariance goes out on the second stream just before chunk c's V product
  // goes out on the main one, into the other chunk buffer (pass 1 uses one of the two at a time) -- it waits only for the V
  // product that last read that buffer, i.e. it runs beside V(c).
#ifdef GPRHIP_LAB
  const bool overlap = p->cov_overlap && cov0_ahead && p->nchunks >= 2;
#else
  constexpr bool overlap = false;  // (measured: no gain, profiles/r05_lab_cov_overlap.txt -- lab build only)
#endif
  TS* const bufB1 = static_cast<TS*>(p->bufB);
  auto kbuf = [&](int c) -> TS* {
    if (Kstore) return Kstore + (int64_t)c * p->chunk * mp;
    return (overlap && (c & 1)) ? bufB1 : bufA;
  };
  for (int c = 0; c < p->nchunks; ++c) {
    const int64_t rows = p->rows_of(c);
    const int rows_p = (int)round_up(rows, TILE);
    const int64_t base = (int64_t)c * p->chunk;
    TS* V = Vstore + base * mp;
    TS* const Kc = kbuf(c);  // this chunk's K_nm: kept, or in a chunk buffer
    if (!reuse) {
      tstart(p, "p1_cov");
      if (overlap) {
        if (c + 1 < p->nchunks) {
          if (c >= 1 && !Kstore) GPR_HIP(hipStreamWaitEvent(p->stream2, p->ev_vdone[(c - 1) & 1], 0));
          cov_chunk<TS>(p, c + 1, kbuf(c + 1), p->stream2);
          GPR_HIP(hipEventRecord(p->ev_cov[(c + 1) & 1], p->stream2));
        }
        GPR_HIP(hipStreamWaitEvent(s, c == 0 ? p->ev_join : p->ev_cov[c & 1], 0));
      } else if (c == 0 && cov0_ahead) GPR_HIP(hipStreamWaitEvent(s, p->ev_join, 0));
      else cov_chunk<TS>(p, c, Kc);
      tstop(p);
      tstart(p, "p1_trmm_V");
      GemmArgsT<TS> g;  // V = K U^-1   (dtrsm `R, lib/fitc_gp.ml:226-227)
      g.A = Kc; g.lda = mp; g.B = inv_u<TS>(p); g.ldb = mp; g.C = V; g.ldc = mp;
      g.M = rows_p; g.N = mp; g.K = mp; g.tri = TRI_KHI_BN; g.order = p->tile_order;
      g.rp_sumsq = p->rp1;  // r = k_diag - rowsum(V.^2) comes out of the epilogue (Mat.syrk_diag, :222-223)
      launch_gemm(OP_NN, g, s);
      if (overlap) GPR_HIP(hipEventRecord(p->ev_vdone[c & 1], s));
      tstop(p);
    }
    tstart(p, "p1_rows");
    Pass1RowArgs ra;
    ra.part = reuse ? nullptr : p->rp1; ra.npart = gemm_row_parts_per_tile() * (mp / TILE); ra.ld = rows_p;
    ra.y = p->h.model_only ? nullptr : p->y + base; ra.rows = (int)rows;
    ra.sf2 = p->cp.sf2; ra.sigma2 = p->h.sigma2;
    ra.r = p->r + base; ra.is = p->is + base; ra.yis = p->yis + base; ra.partial = p->rowpart;
    launch_pass1_rows(ra, s);
    launch_reduce_rows(p->rowpart, pass1_row_blocks(rows_p), 4, ex.tail, 1, s);
    tstop(p);
  }
  // Model.update_sigma2 on a two-tile problem whose fresh evaluations accumulate B~ with mid.hip's launch pair: the same
  // pair here, so that the re-weighted evaluation returns the very numbers a fresh one would
  // (test_update_sigma2_reuses_resident_v)
  gram_over_v<TS>(p, 1, reuse && p->mid_pair(), ex.tiles, ex.c);
  if (!reuse) p->have_k = Kstore != nullptr;
}

template <typename TS>
void do_pass1(gprhip_problem* p, const gprhip_hypers* h, int want_grad, int64_t n_total, double* ar1) {
  if (!h || !h->inducing) {
    set_error("gprhip: hypers/inducing pointer is NULL");
    throw HipFail{ST_BAD_ARG};
  }
  if (!p->have_inputs || (!p->have_targets && !h->model_only)) {
    set_error("gprhip: inputs/targets not set");
    throw HipFail{ST_STATE};
  }
  GPR_HIP(hipSetDevice(p->device));
  // the state of the previous evaluation is void from here on; finish() re-validates it
  p->have_model = p->have_factors = false;
  p->multi_state = false;
  p->tg_coeffs = false;
  p->stage = 0;
  p->x_last = nullptr;
  p->cond_km = -1.0;
  p->pg_m_valid = false;
  p->sp_ns_last = 0;
  forget_observations(p);
  upload_hypers(p, h);
  p->want_grad = want_grad;
  p->n_total = n_total;
  const bool reuse = h->reuse_v != 0;
  // the path of this evaluation.  A re-weighted one (reuse_v) has V and r already: whichever path made them, its rows go
  // through the engine's row kernel
  const bool small = p->use_small(), mid = p->use_mid();
  ensure_eval_scratch<TS>(p, small, mid, reuse);
  if (!small && !mid) try_k_resident<TS>(p);
  if (reuse && !p->have_v) {
    set_error("gprhip: reuse_v set but this problem holds no V of a previous evaluation");
    throw HipFail{ST_STATE};
  }
  p->have_v = false;
  if (!reuse) p->have_k = p->small_k_valid = false;
  const Ex1<double> ex = ex1_of(p, ar1);
  const bool cov0_ahead = !reuse && !p->timer.on && !small && !mid;
  if (cov0_ahead) fork_first_cov<TS>(p);
  pass1_km_chol(p, ex, !(small || (mid && p->mp == TILE)) || reuse);
  if (small && !reuse) pass1_small(p, ex);
  else if (mid && !reuse) pass1_mid(p, ex);
  else pass1_engine<TS>(p, ex, reuse, cov0_ahead);
  p->stage = 1;
  p->have_v = true;  // (revoked by finish() if the factorisation of K_m turns out to have failed)
}

// ---- pass 2
// B~ = I + sum of shard parts; R~ = chol(B~): R = R~ U is the reference's r_mat (lib/fitc_gp.ml:181); R~^-1 and the m-vectors
void pass2_b_chol(gprhip_problem* p, const Ex1<const double>& ex) {
  hipStream_t s = p->stream;
  const int mp = p->mp;
  tstart(p, "b_chol");
  const bool fused_b = mp == TILE && !p->engine_steps;
  p->a1_in_scal = fused_b;
  if (fused_b) {
    // a single block: I + the accumulation, the factorisation, the inverse and the m-vectors below in one kernel
    PotrfFuse f;
    f.src = ex.tiles; f.cvec = ex.c;
    f.tail_in = ex.tail; f.tail_out = p->scal + SC_A1TAIL;
    f.uinv = p->uinv; f.bvec = p->bvec; f.ttil = p->ttil; f.tvec = p->tvec;
    f.logdet = p->scal + SC_LOGDET_B; f.bb = p->scal + SC_BB;
    launch_potrf_fused(f, p->bmat, p->rinv, p->info + 1, p->m, s);
  } else {
    hipLaunchKernelGGL(add_identity_upper_kernel, dim3((mp + 255) / 256, mp), dim3(256), 0, s, ex.tiles, mp,
                       p->bmat);
    potrf_trtri(p, p->bmat, p->rinv, p->wmat, p->info + 1);
  }
  if (p->f32) launch_to_float(p->rinv, p->rinv_f, (int64_t)mp * mp, s);
  // b = R~^-T c~ (= Q_n^T y~, lib/fitc_gp.ml:285-286);  t~ = R~^-1 b;  t = U^-1 t~ (trsv, :291 / :1167)
  if (!fused_b) {
    // (log|B~| and |b|^2 ride on the first two launches: two launches less on the chain)
    launch_triu_matvec_rider(p->rinv, mp, ex.c, p->bvec, 1, 1, p->bmat, mp, p->scal + SC_LOGDET_B, s);
    launch_triu_matvec_rider(p->rinv, mp, p->bvec, p->ttil, 0, 2, p->bvec, mp, p->scal + SC_BB, s);
    launch_triu_matvec(p->uinv, mp, p->ttil, p->tvec, 0, s);
  }
  tstop(p);
}

// the fields the one-kernel row passes of small.hip and mid.hip share
template <typename Args>
void fill_row_pass2(const gprhip_problem* p, Args& a) {
  const bool proj = p->has_proj();
  a.cp = p->cp; a.pts = p->pts(); a.Z = p->Z; a.rinv = p->rinv; a.bvec = p->bvec; a.ttil = p->ttil;
  a.V = static_cast<const double*>(p->Vstore); a.y = p->h.model_only ? nullptr : p->y; a.is = p->is; a.r = p->r;
  a.big = proj ? p->X : nullptr; a.D = proj ? p->D : 0;
  a.rows = (int)p->n; a.rows_p = (int)round_up(p->n, TILE); a.m = p->m; a.mp = p->mp; a.d = p->d;
  a.variational = p->h.variational;
  // (X itself is only kept for the debug fetch "x_rows", which wants all rows in one chunk buffer)
  a.w = p->w; a.v = p->v; a.es = proj ? p->es : nullptr; a.X = p->nchunks == 1 ? static_cast<double*>(p->bufB) : nullptr;
}

// gprhip_eval_input_grad: dl/d(training inputs) of one row chunk from its X (input_grad.hip), written to the destination at
// the chunk's row offset; K: K_nm of the chunk in memory, or null (recomputed)
void input_grad_chunk(gprhip_problem* p, const double* Xc, const double* K, int64_t base, int64_t rows) {
  hipStream_t s = p->stream;
  const bool proj = p->has_proj();
  tstart(p, "p2_xgrad");
  InputGradArgs a;
  a.X = Xc; a.K = K; a.pts = p->pts() + base * p->d; a.Z = p->Z;
  a.shift = p->d <= 64 ? p->zshift : p->Z;  // (the centroid is kept for 64 dimensions: beyond, the first inducing point)
  a.rows = (int)rows; a.m = p->m; a.mp = p->mp; a.d = p->d;
  a.log_sf2 = p->cp.log_sf2; a.inv_ell2_05 = p->cp.inv_ell2_05;
  a.G = proj ? p->xg_g : p->xg_dst + base * p->D; a.ldg = p->d;
  launch_input_grad(a, s);
  if (proj) launch_input_grad_project(p->xg_g, rows, p->d, p->D, p->tproj, p->xg_dst + base * p->D, p->D, s);
  tstop(p);
}

// at most 64 inducing points: Q', the row quantities, X~, X, the column sums of E = X .* K and G~ in one kernel (small.hip);
// B~^-1 is formed by the finish kernel, R^-1 is not needed
void pass2_small(gprhip_problem* p, const Ex2<double>& ex) {
  tstart(p, "p2_small");
  p->merged_x = false;
  SmallPass2Args a;
  fill_row_pass2(p, a);
  a.uinv = p->uinv;
  a.Kin = (p->small_k_valid && p->d <= 8 && !p->has_ms()) ? p->small_k : nullptr;
  a.part = p->small_part;
  launch_small_pass2(a, (int)p->col_rows(), ex.tiles, ex.col, ex.proj, ex.tail, p->stream);
  p->x_last = a.X;
  tstop(p);
  if (p->xgrad) input_grad_chunk(p, a.X, nullptr, 0, p->n);
}

// one or two 128-column tiles: Q', the row quantities, X~, X, E = X .* K with its moments (and, one tile, G~) in one
// kernel (mid.hip); B~^-1 is formed by the finish kernels, R^-1 is not needed.  Two tiles: mid rows, then the Gram
// accumulation G~_part = V^T diag(v) V -- by mid.hip's launch pair or by the engine's launch, as in pass 1
void pass2_mid(gprhip_problem* p, const Ex2<double>& ex) {
  hipStream_t s = p->stream;
  tstart(p, "p2_mid");
  p->merged_x = false;
  // (U^-T and R~^-T for the "times B^T" products and the finish stage: W~'s and B~^-1's buffers are free on this path)
  launch_mid_transposes(p->uinv, p->rinv, p->mp, p->wtil, p->binv, s);
  MidPass2Args a;
  fill_row_pass2(p, a);
  a.uinvT = p->wtil; a.rinvT = p->binv; a.shift = p->zshift;
  a.part = p->mid_part;
  launch_mid_pass2(a, (int)p->col_rows(), ex.tiles, ex.col, ex.proj, ex.tail, s);
  p->x_last = a.X;
  if (p->has_proj()) {  // second term of the `Proj derivative from the per-row sums of E the kernel left (as the engine path)
    for (int c = 0; c < p->nchunks; ++c) {
      const int64_t rows = p->rows_of(c), base = (int64_t)c * p->chunk;
      launch_proj_term2(p->X + base * p->D, p->P + base * p->d, p->es + base, 1, (int)rows, p->D, p->d, p->projpart, s);
      launch_reduce_rows(p->projpart, (int)((rows + 255) / 256), p->D * p->d, ex.proj, 1, s);
    }
  }
  tstop(p);
  if (p->xgrad) input_grad_chunk(p, a.X, nullptr, 0, p->n);
  if (p->mp > TILE) gram_over_v<double>(p, 2, p->mid_pair(), ex.tiles, nullptr);
}

// the chunked engine path: the m x m inverses beside the first chunk, per row chunk Q', the row quantities, X and the
// gradient accumulators, then one Gram accumulation over all rows
template <typename TS>
void pass2_engine(gprhip_problem* p, const Ex2<double>& ex) {
  hipStream_t s = p->stream;
  const int mp = p->mp;
  const int64_t mm = (int64_t)mp * mp;
  const bool mo = p->h.model_only != 0;
  const bool proj = p->has_proj();
  TS* const Vstore = static_cast<TS*>(p->Vstore);
  TS* const bufA = static_cast<TS*>(p->bufA);
  TS* const bufB = static_cast<TS*>(p->bufB);
  // B~^-1 = R~^-1 R~^-T (needed by the finish stage only) and R^-1 = U^-1 R~^-1 (needed by the first X product) do not
  // belong on the chain between the factorisation and the Q' products: they go to the second stream and run beside
  // the first chunk's Q' launch (0.28 ms of every gradient evaluation at m = 2048).  Both use the split-K scratch,
  // which the main stream touches next in the pass-2 SYRK -- it waits for ev_binv before that.  (Under the per-stage
  // timer everything stays on the main stream, so that "inverses" keeps its meaning.)
  const bool side = !p->timer.on;
  hipStream_t si = side ? p->stream2 : s;
  if (side) {
    GPR_HIP(hipEventRecord(p->ev_fork, s));  // R~^-1 (and its fp32 copy), t~, t are enqueued on s
    GPR_HIP(hipStreamWaitEvent(p->stream2, p->ev_fork, 0));
  }
  tstart(p, "inverses");
  // The two-phase X product (below) needs R^-1 = U^-1 R~^-1, one more m x m product (0.14 ms at m = 2048, 0.8 ms at
  // m = 4096), and saves 2.5 us per 1000 training points at m = 2048 (6 us at m = 4096): taken from 48 m training
  // points per shard on.
  p->merged_x = p->merged_x_mode == 2 || (p->merged_x_mode == 1 && p->n >= 48 * (int64_t)p->m);
  if (p->merged_x) {
    GemmArgs rf;  // R^-1 = U^-1 R~^-1, both upper triangular
    rf.A = p->uinv; rf.lda = mp; rf.B = p->rinv; rf.ldb = mp; rf.C = p->rfinv; rf.ldc = mp;
    rf.M = mp; rf.N = mp; rf.K = mp; rf.tri = TRI_BAND; rf.upper_only = 1;
    // the corner tile's k-range is the whole of m: eight k-slices keep the launch from waiting on it
    const int rks = (mp >= 1024 && 8 * mm * 8 <= p->slices_bytes) ? 8 : 1;
    if (rks > 1) {
      rf.C = static_cast<double*>(p->slices);
      rf.kslices = rks;
      rf.slice_stride = mm;
      launch_gemm(OP_NN, rf, si);
      launch_sum_slices<double>(nullptr, static_cast<double*>(p->slices), rks, mm, mp, p->rfinv, si);
    } else {
      launch_gemm(OP_NN, rf, si);
    }
    if (p->f32) launch_to_float(p->rfinv, p->rfinv_f, mm, si);
  }
  if (side) GPR_HIP(hipEventRecord(p->ev_rf, si));
  triu_xxt(p, p->rinv, p->binv, si);  // B~^-1 (upper tiles)
  if (side) GPR_HIP(hipEventRecord(p->ev_binv, si));
  tstop(p);
  bool derive_inducing = false;
  for (int c = 0; c < p->nchunks; ++c) {
    const int64_t rows = p->rows_of(c);
    const int rows_p = (int)round_up(rows, TILE);
    const int64_t base = (int64_t)c * p->chunk;
    const TS* V = Vstore + base * mp;
    tstart(p, "p2_trmm_Q");
    GemmArgsT<TS> q;  // Q' = V R~^-1 = K R^-1  (Q_n = diag(sqrt is) Q', lib/fitc_gp.ml:176-182)
    q.A = V; q.lda = mp; q.B = inv_r<TS>(p); q.ldb = mp; q.C = bufA; q.ldc = mp;
    q.M = rows_p; q.N = mp; q.K = mp; q.tri = TRI_KHI_BN; q.order = p->tile_order;
    q.rp_sumsq = p->rp1; q.rp_dot = p->rp2; q.rp_vec = p->bvec;  // q_diag and Q'b from the epilogue
    launch_gemm(OP_NN, q, s);
    tstop(p);
    tstart(p, "p2_rows");
    Pass2RowArgs ra;
    ra.part_sq = p->rp1; ra.part_dot = p->rp2; ra.npart = gemm_row_parts_per_tile() * (mp / TILE); ra.ld = rows_p;
    ra.y = mo ? nullptr : p->y + base; ra.is = p->is + base; ra.r = p->r + base;
    ra.rows = (int)rows; ra.variational = p->h.variational;
    ra.sf2 = p->cp.sf2; ra.es = proj ? p->es + base : nullptr;
    ra.w = p->w + base; ra.v = p->v + base; ra.partial = p->rowpart;
    launch_pass2_rows(ra, s);
    launch_reduce_rows(p->rowpart, pass1_row_blocks(rows_p), 4, ex.tail, 1, s);
    tstop(p);
    if constexpr (std::is_same<TS, double>::value)
      if (p->multi) targets_pass2_rows(p, bufA, base, (int)rows, proj ? p->es + base : nullptr, ex.tail + A2_SUMV);
    const TS* Xc;  // X of this chunk
    if (p->merged_x) {
      // X = diag(is) Q' R^-T - diag(v) V U^-T - w t^T  (S, U_mat and the ger of lib/fitc_gp.ml:931-939, :1204-1206) as
      // one launch of two-phase items: acc = V U^-T, rows scaled by -v/is, acc += Q' R^-T, epilogue is*acc - w t^T --
      // one epilogue per tile instead of two, no X~ round trip, no operand read in the epilogue
      if (side && c == 0) GPR_HIP(hipStreamWaitEvent(s, p->ev_rf, 0));
      tstart(p, "p2_trmm_SX");
      GemmArgsT<TS> xg;
      xg.A = bufA; xg.lda = mp; xg.B = inv_rfull<TS>(p); xg.ldb = mp; xg.C = bufB; xg.ldc = mp;
      xg.A2 = V; xg.B2 = inv_u<TS>(p); xg.mid_num = p->v + base; xg.mid_den = p->is + base;
      xg.M = rows_p; xg.N = mp; xg.K = mp; xg.tri = TRI_KLO_BN; xg.order = p->tile_order;
      xg.epi_rows_a = p->is + base; xg.epi_rows_c = p->w + base; xg.epi_col = p->tvec;
      launch_gemm(OP_NT, xg, s);
      tstop(p);
      Xc = bufB;
    } else {
      tstart(p, "p2_trmm_S");
      GemmArgsT<TS> sg;  // X~ = diag(is) Q' R~^-T - diag(v) V - w t~^T   (S, U_mat and the ger of :936-938, :1204-1206)
      sg.A = bufA; sg.lda = mp; sg.B = inv_r<TS>(p); sg.ldb = mp; sg.C = bufB; sg.ldc = mp;
      sg.M = rows_p; sg.N = mp; sg.K = mp; sg.tri = TRI_KLO_BN; sg.order = p->tile_order;
      sg.epi_rows_a = p->is + base; sg.epi_rows_b = p->v + base; sg.epi_rows_c = p->w + base;
      sg.epi_col = p->ttil; sg.epi_mat = V; sg.epi_ldm = mp;
      launch_gemm(OP_NT, sg, s);
      tstop(p);
      tstart(p, "p2_trmm_X");
      GemmArgsT<TS> xg;  // X = X~ U^-T
      xg.A = bufB; xg.lda = mp; xg.B = inv_u<TS>(p); xg.ldb = mp; xg.C = bufA; xg.ldc = mp;
      xg.M = rows_p; xg.N = mp; xg.K = mp; xg.tri = TRI_KLO_BN; xg.order = p->tile_order;
      launch_gemm(OP_NT, xg, s);
      tstop(p);
      Xc = bufA;
    }
    p->x_last = (p->nchunks == 1) ? static_cast<const void*>(Xc) : nullptr;
    if constexpr (std::is_same<TS, double>::value)
      if (p->multi) targets_xcorr(p, const_cast<double*>(Xc), base, (int)rows);
    tstart(p, "p2_grad");
    GradArgs<TS> ga;
    ga.X = Xc; ga.pts = p->pts() + base * p->d; ga.Z = p->Z;
    ga.rows = (int)rows; ga.rows_p = rows_p; ga.m = p->m; ga.mp = mp; ga.d = p->d;
    ga.log_sf2 = p->cp.log_sf2; ga.inv_ell2_05 = p->cp.inv_ell2_05;
    ga.colpart = p->colpart; ga.scalpart = p->scalpart;
    ga.big = proj ? p->X + base * p->D : nullptr; ga.D = proj ? p->D : 0;
    ga.ms = p->cp.ms; ga.shift = p->zshift;
    ga.K = (p->Kstore && p->have_k && proj && !ga.ms) ? static_cast<const TS*>(p->Kstore) + base * mp : nullptr;
    ga.col_rows = p->d + 1 + ga.D + (ga.ms ? p->d : 0);  // rows this launch produces (tightly packed)
    ga.slab = p->grad_slab;
    const int nslots = 4 * ((mp + 255) / 256);
    ga.rowes = (ga.ms && proj) ? p->rowes : nullptr;
    // matrix-core version unless multiscales (or > 64 dimensions) need the scalar kernel; GPRHIP_GRAD_SCALAR=1
    // forces the scalar one (parity tests run both)
    int nbx = p->grad_scalar ? 0 : grad_mfma_col_blocks(ga);
    const TS* Kc = ga.K;  // K_nm of this chunk in memory, if any
    if (p->d > 64 || ga.D > 64) {
      // wide points: K of the chunk is rebuilt into the chunk buffer that does not hold X, and E = X .* K read from memory
      TS* const Kw = (Xc == bufA) ? bufB : bufA;
      cov_chunk<TS>(p, c, Kw);
      launch_grad_wide(ga, static_cast<const TS*>(Kw), s);
      Kc = Kw;
      nbx = (mp + 255) / 256;
    } else if (nbx > 0) {
      launch_grad_mfma(ga, s);
      derive_inducing = proj;  // that kernel accumulates only the projection-gradient sums (grad_mfma.hip)
    } else {
      launch_grad_fused(ga, s);
      nbx = (mp + 255) / 256;
    }
    const int nslabs = (int)((rows + ga.slab - 1) / ga.slab);
    launch_reduce_rows(p->colpart, nslabs, ga.col_rows * mp, ex.col, 1, s);
    if (proj) {
      if (ga.ms) {
        launch_reduce_rowes(p->rowes, (int)rows, nslots, p->d, p->es2, s);
        launch_proj_term2(p->X + base * p->D, p->P + base * p->d, p->es2, p->d, (int)rows, p->D, p->d,
                          p->projpart, s);
      } else {
        launch_proj_term2(p->X + base * p->D, p->P + base * p->d, p->es + base, 1, (int)rows, p->D, p->d,
                          p->projpart, s);
      }
      launch_reduce_rows(p->projpart, (int)((rows + 255) / 256), p->D * p->d, ex.proj, 1, s);
    }
    launch_reduce_rows(p->scalpart, nslabs * nbx, 2, ex.tail + A2_SUME, 1, s);
    tstop(p);
    if constexpr (std::is_same<TS, double>::value)
      if (p->xgrad) input_grad_chunk(p, Xc, Kc, base, rows);
  }
  if (derive_inducing) launch_proj_inducing_grad(ex.col, mp, p->d, p->D, p->tproj, s);
  if (side) GPR_HIP(hipStreamWaitEvent(s, p->ev_binv, 0));  // B~^-1 done: the split-K scratch is free again
  gram_over_v<TS>(p, 2, false, ex.tiles, nullptr);
}

template <typename TS>
void do_pass2(gprhip_problem* p, const double* ar1, double* ar2) {
  if (p->stage != 1) {
    set_error("gprhip: eval_pass2 called before eval_pass1");
    throw HipFail{ST_STATE};
  }
  GPR_HIP(hipSetDevice(p->device));
  pass2_b_chol(p, ex1_of(p, ar1));
  if (p->multi) targets_middle(p);  // (c~, b, t~, t above are those of no target: zero)
  const Ex2<double> ex = ex2_of(p, ar2);
  const bool small = p->use_small(), mid = p->use_mid();
  // evidence-only evaluations (multim_f) carry nothing in the second exchange buffer: only its scalar tail is cleared,
  // and the caller need not reduce it.  The reductions of the small and the mid pass write every entry of the buffer
  // (two tiles through mid.hip: its reduction writes everything behind the packed tiles, the Gram accumulation the tiles)
  if (!p->want_grad) GPR_HIP(hipMemsetAsync(ex.tail, 0, (size_t)A2_TAIL * sizeof(double), p->stream));
  else if (small) pass2_small(p, ex);
  else if (mid) pass2_mid(p, ex);
  else {
    GPR_HIP(hipMemsetAsync(ar2, 0, (size_t)gprhip_ar2_len(p) * sizeof(double), p->stream));
    pass2_engine<TS>(p, ex);
  }
  p->stage = 2;
}

// ---- finish stage, first half, per path
bool wants_wdiag(const gprhip_problem* p) { return p->want_grad && (p->has_het() || p->has_ms()); }

// at most 64 inducing points: the m x m work in one workgroup, which also gathers the exchange-2 tail behind the
// result block
void finish_small(gprhip_problem* p, const Ex2<const double>& ex) {
  hipStream_t s = p->stream;
  const int d = p->d;
  tstart(p, "finish");
  SmallFinishArgs a;
  a.uinv = p->uinv; a.rinv = p->rinv; a.ttil = p->ttil; a.km = p->km; a.Z = p->Z; a.g = ex.tiles;
  a.ms = p->has_ms() ? p->ms : nullptr;
  a.m = p->m; a.mp = p->mp; a.d = d; a.km_rows = p->has_ms() ? 2 * d + 2 : d + 2;
  a.wmat = p->wmat; a.kmred = p->kmred; a.wdiag = wants_wdiag(p) ? p->wdiag : nullptr;
  a.gather_from = ex.col; a.n_gather = ex.len_from_col(); a.ex = p->ex_dev + A1_TAIL;
  launch_small_finish(a, s);
  tstop(p);
  const int64_t n_res = p->res_len + A1_TAIL + ex.len_from_col();
  if (n_res * (int64_t)sizeof(double) > 32768) {  // (d > 8 or so: above 32 KB a copy starts 17 us late, a kernel at once)
    ShipArgs sh;
    sh.src[0] = p->res_dev; sh.dst[0] = p->res_host; sh.n[0] = n_res;
    launch_ship(sh, s);
  } else {
    GPR_HIP(hipMemcpyAsync(p->res_host, p->res_dev, (size_t)n_res * sizeof(double), hipMemcpyDeviceToHost, s));
  }
}

// one or two 128-blocks: the m x m work in two launches of one workgroup per 16 rows (mid.hip), the first of which also
// gathers the exchange-2 tail behind the result block
void finish_mid(gprhip_problem* p, const Ex2<const double>& ex) {
  tstart(p, "finish");
  MidFinishArgs a;
  a.uinv = p->uinv; a.rinv = p->rinv; a.uinvT = p->wtil; a.rinvT = p->binv; a.ttil = p->ttil; a.km = p->km; a.Z = p->Z;
  a.g = ex.tiles;
  a.m = p->m; a.mp = p->mp; a.d = p->d; a.km_rows = p->d + 2;
  a.wmat = p->wmat; a.kmred = p->kmred; a.wdiag = wants_wdiag(p) ? p->wdiag : nullptr;
  a.ybuf = p->kj;  // (free after the factorisation of K_m)
  a.gather_from = ex.col; a.n_gather = ex.len_from_col(); a.ex = p->ex_dev + A1_TAIL;
  // the kernels' last workgroup writes the result block (and, two tiles, the exchange-1 tail) into the pinned mirror itself
  a.res_dev = p->res_dev; a.res_host = p->res_host; a.res_total = p->res_len + A1_TAIL + ex.len_from_col();
  a.done_ctr = p->mid_done;
  if (!p->a1_in_scal) {  // (two tiles: the B~ phase is not the fused single-block kernel that leaves the tail in the result block)
    a.a1_tail = ex1_of(p, p->ar1).tail;
    a.a1_host = p->ex_host;
  }
  launch_mid_finish(a, p->stream);
  tstop(p);
}

// the engine path, and every evidence-only evaluation: the m x m products of W as engine launches, then one launch that
// ships the results
void finish_engine(gprhip_problem* p, const Ex2<const double>& ex) {
  hipStream_t s = p->stream;
  const int mp = p->mp, m = p->m, d = p->d;
  const bool wdiag = wants_wdiag(p);
  if (p->want_grad) {
    const int nkslab = (m + km_slab_rows(m) - 1) / km_slab_rows(m);
    tstart(p, "finish");
    launch_build_w(p->binv, p->ttil, ex.tiles, mp, p->wtil, s);
    if (p->multi) launch_targets_w_rankk(p->wtil, mp, p->tg_Tt(), p->multi, s);  // (1/k) T~ T~^T in place of t~ t~^T (zero here)
    GemmArgs y;  // Y = W~ U^-T
    y.A = p->wtil; y.lda = mp; y.B = p->uinv; y.ldb = mp; y.C = p->kj; y.ldc = mp;  // kj is free after potrf; R~ stays in bmat
    y.M = mp; y.N = mp; y.K = mp; y.tri = TRI_KLO_BN;
    const int wks = ((int64_t)(mp / TILE) * (mp / TILE) <= 256) ? mxm_slices(mp) : 1;
    gemm_splitk(p, OP_NT, y, wks);
    GemmArgs w;  // W = U^-1 Y   (lib/fitc_gp.ml:1196-1203)
    w.A = p->uinv; w.lda = mp; w.B = p->kj; w.ldb = mp; w.C = p->wmat; w.ldc = mp;
    w.M = mp; w.N = mp; w.K = mp; w.tri = TRI_KLO_BM;
    gemm_splitk(p, OP_NN, w, wks);
    if (p->has_ms()) {
      launch_km_traces_ms(p->wmat, p->km, p->Z, p->ms, m, mp, d, p->kmpart, s);
      launch_reduce_rows(p->kmpart, nkslab, (2 * d + 2) * mp, p->kmred, 0, s);
    } else {
      launch_km_traces(p->wmat, p->km, p->Z, m, mp, d, p->kmpart, p->cp, s);
      launch_reduce_rows(p->kmpart, nkslab, (d + 2) * mp, p->kmred, 0, s);
    }
    // W_ii for the `Diag_vec / multiscale diagonal terms, into the result block
    if (wdiag) hipLaunchKernelGGL(copy_diag_kernel, dim3((mp + 255) / 256), dim3(256), 0, s, p->wmat, mp, p->wdiag);
    tstop(p);
  }
  // three transfers into pinned memory bring everything the host assembly needs: the result block (its K_m-trace and
  // diag-W parts only after a gradient evaluation), the scalar tail of the reduced exchange-1 buffer (kept in p->ar1 by
  // pass 2), and the exchange-2 buffer from its column block on (its scalar tail only after an evidence-only evaluation)
  const int64_t res_used = NSCAL + 2 + mp + (p->want_grad ? p->km_rows() * mp + (wdiag ? mp : 0) : 0);
  // -- by one launch of ship_kernel (finalize.hip): three hipMemcpyAsync calls cost 17-18 us of idle stream before them
  ShipArgs sh;
  sh.src[0] = p->res_dev; sh.dst[0] = p->res_host; sh.n[0] = res_used;
  if (!p->a1_in_scal) {
    sh.src[1] = ex1_of(p, p->ar1).tail; sh.dst[1] = p->ex_host; sh.n[1] = A1_TAIL;
  }
  if (p->want_grad) {  // (an evidence-only evaluation reads nothing of the exchange-2 buffer)
    sh.src[2] = ex.col; sh.dst[2] = p->ex_host + A1_TAIL; sh.n[2] = ex.len_from_col();
  }
  launch_ship(sh, s);
}

// Finish stage, first half: the m x m work of the gradient (W, traces) and the asynchronous copies of everything the
// host assembly needs, all on the problem's stream; nothing blocks.  `light` (shards of a multi-device context other
// than the first): only the factorisation flags are fetched -- the reduced buffers are identical on every device, and
// one device's assembly serves the caller.
void do_finish_enqueue(gprhip_problem* p, const double* ar2, bool light = false) {
  if (p->stage != 2) {
    set_error("gprhip: eval_finish called before eval_pass2");
    throw HipFail{ST_STATE};
  }
  GPR_HIP(hipSetDevice(p->device));
  p->stage = 3;
  if (light) {
    GPR_HIP(hipMemcpyAsync(p->res_host + NSCAL, p->info, 2 * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    return;
  }
  const Ex2<const double> ex = ex2_of(p, ar2);
  if (p->want_grad && p->use_small()) finish_small(p, ex);
  else if (p->want_grad && p->use_mid()) finish_mid(p, ex);
  else finish_engine(p, ex);
}

// Finish stage, second half: wait for the stream, check the factorisations, assemble l1, l2, dl/dsigma2 and the gradient
// in the reference's Hyper.get_all order on the host.  light: flags and state only (see do_finish_enqueue).
void do_finish_collect(gprhip_problem* p, gprhip_result* res, double* grad, double* coeffs, bool light = false) {
  if (p->stage != 3) {
    set_error("gprhip: finish collected before it was enqueued");
    throw HipFail{ST_STATE};
  }
  GPR_HIP(hipSetDevice(p->device));
  const int mp = p->mp, m = p->m, d = p->d;
  GPR_HIP(hipStreamSynchronize(p->stream));
  p->stage = 0;
  if (p->timer.on || p->timer.kernel) tcollect(p);
  const double* const hscal = p->res_host;
  int hinfo[2];
  std::memcpy(hinfo, p->res_host + NSCAL, sizeof hinfo);
  const double* const ht = p->res_host + NSCAL + 2;
  const double* const hkm = ht + mp;
  const double* const hwdiag = hkm + p->km_rows() * mp;
  const double* const ha1tail = p->a1_in_scal ? hscal + SC_A1TAIL : p->ex_host;
  const double* const hcol = p->ex_host + A1_TAIL;  // column block + Proj second term + scalar tail of exchange 2
  const double* const htail = hcol + ex2_tail_off(p);
  if (hinfo[0] == POTRF_CHAIN_ABORT_CODE || hinfo[1] == POTRF_CHAIN_ABORT_CODE) {
    p->have_v = p->have_k = false;
    set_error("gprhip: internal error: a dependency wait of the one-launch factorisation ran into its bound "
              "(GPRHIP_POTRF_CHAIN=0 selects the step-by-step launches)");
    throw HipFail{ST_HIP_ERROR};
  }
  if (hinfo[0] != 0 || hinfo[1] != 0) {
    p->have_v = p->have_k = false;  // V came out of a failed factor
    char buf[160];
    snprintf(buf, sizeof buf,
             "Lacaml.D.potrf: leading minor of order %d of %s is not positive definite",
             hinfo[0] ? hinfo[0] : hinfo[1], hinfo[0] ? "K_m + jitter" : "B~ = I + V^T S^-1 V");
    set_error(buf);
    throw HipFail{ST_NOT_POSDEF};
  }
  p->have_model = true;
  p->have_factors = true;
  p->have_b = true;  // (pass2_b_chol left b = R~^-T c~ in bvec)
  if (light) return;
  const bool mo = p->h.model_only != 0;
  const double sum_log_s = ha1tail[A1_SUMLOGS], sum_isr = ha1tail[A1_ISR], sum_isy2 = ha1tail[A1_ISY2];
  // l1: lib/fitc_gp.ml:204-208 with log|R^T R| - log|K_m| = log|B~| ; variational: :262-263
  double l1 = -0.5 * (hscal[SC_LOGDET_B] + sum_log_s + (double)p->n_total * LOG_2PI);
  if (p->h.variational) l1 += -0.5 * sum_isr;
  // l2 = -1/2 (|y~|^2 - |Q_n^T y~|^2), lib/fitc_gp.ml:290
  double l2 = mo ? 0.0 : -0.5 * (sum_isy2 - hscal[SC_BB]);
  res->l1 = l1;
  res->l2 = l2;
  res->l = l1 + l2;
  res->dl_dsigma2 = 0.0;
  res->n_hypers = 0;
  if (coeffs) std::memcpy(coeffs, ht, (size_t)m * sizeof(double));
  if (!p->want_grad) return;
  // dl/dsigma2: lib/fitc_gp.ml:1112-1119, :1187-1188
  double sumv = htail[A2_SUMV];
  res->dl_dsigma2 = -0.5 * (p->h.variational ? (sumv - htail[A2_SUMIS]) : sumv);
  // per-hyper evidence derivative, lib/fitc_gp.ml:1005-1021:
  //   dl = -1/2 (dkn_diag_term - dkm_term) - dknm_term
  double tr_wk = 0.0, tr_wkd = 0.0;
  for (int c = 0; c < m; ++c) {
    tr_wk += hkm[c];
    tr_wkd += hkm[(size_t)mp + c];
  }
  const double sumE = htail[A2_SUME], sumED = htail[A2_SUMED];
  const double scale = p->cp.inv_ell2;
  // Log_sf2: `Factor 1. on all three (lib/cov_se_iso.ml:248, :298, :302)
  const double g_sf2 = -0.5 * (p->cp.sf2 * sumv - tr_wk) - sumE;
  int64_t pos = 0;
  if (p->kind == GPRHIP_COV_SE_ISO) {
    // Log_ell: dkn_diag `Const 0.; dkm `Dense K.*D/ell^2 (diag 0); dknm `Dense (lib/cov_se_iso.ml:249-260, :303-314)
    grad[pos++] = 0.5 * scale * tr_wkd - scale * sumED;
    grad[pos++] = g_sf2;
  } else {
    grad[pos++] = g_sf2;
  }
  // Inducing_hyper {ind; dim}: dkm `Sparse_rows -> 2*scale*sum_{r!=c} W_rc K_rc (z_kr - z_kc)
  // (lib/utils.ml:196-220); dknm `Sparse_cols -> scale*sum_r (x_kr - z_kc) E_rc.  With multiscales the
  // row entries carry 1/(ms_kr + ms_kc - 1) (already inside the trace kernel) and the column 1/ms_kc
  // (lib/cov_se_fat.ml:501-513, :633-638).
  const bool msm = p->has_ms();
  const int Dp = p->has_proj() ? p->D : 0;
  for (int c = 0; c < m; ++c) {
    for (int k = 0; k < d; ++k) {
      const double zk = p->hZ[(size_t)c * d + k];
      const double dkm_half = scale * hkm[(size_t)(2 + k) * mp + c];
      double dknm = scale * (hcol[(size_t)(k + 1) * mp + c] - zk * hcol[c]);
      if (msm) dknm /= p->hMs[(size_t)c * d + k];
      grad[pos++] = dkm_half - dknm;
    }
  }
  // Proj {big_dim; small_dim} (lib/cov_se_fat.ml:429, :531, :570-596): dkm, dkn_diag `Const 0.;
  // dknm `Dense x_big,r (z_small,c - p_small,r) [/ ms_small,c] K_rc
  if (p->has_proj()) {
    const int D = p->D;
    const double* m1 = hcol + (size_t)(d + 1) * mp;       // [big][c] = sum_r x_big,r E_rc
    const double* term2 = hcol + ex2_proj_off(p);  // [big][small]
    for (int big = 0; big < D; ++big) {
      for (int small = 0; small < d; ++small) {
        double term1 = 0.0;
        for (int c = 0; c < m; ++c) {
          double zz = p->hZ[(size_t)c * d + small];
          if (msm) zz /= p->hMs[(size_t)c * d + small];
          term1 += zz * m1[(size_t)big * mp + c];
        }
        grad[pos++] = -(term1 - term2[(size_t)big * d + small]);
      }
    }
  }
  // Log_hetero_skedasticity i (lib/cov_se_fat.ml:430-440): dkm `Diag_vec het_i e_i, the other two `Const 0.
  //   -> dl = 1/2 het_i W_ii   (lib/fitc_gp.ml:962-967)
  if (p->has_het())
    for (int i = 0; i < m; ++i) grad[pos++] = 0.5 * p->hHet[i] * hwdiag[i];
  // Log_multiscale_m05 {ind; dim} (lib/cov_se_fat.ml:441-485, :598-622), theta = log(ms - 1/2):
  //   dkm `Sparse_rows: inner_i K_i,ind for i != ind, (1/2 - ms)/(2 ms - 1) K_ind,ind on the diagonal
  //   dknm `Sparse_cols: inner_r K_r,ind with inner = (1/ms - ((p_kr - z_kc)/ms)^2) * (1/2)(1/2 - ms)
  if (msm) {
    const double* gxx = hcol + (size_t)(d + 1 + Dp) * mp;   // [k][c] = sum_r p_kr^2 E_rc
    for (int c = 0; c < m; ++c) {
      double lsum = 0.0;  // K_cc without heteroskedastic noise: exp(log_sf2 - 1/2 sum log(2 ms - 1))
      for (int k = 0; k < d; ++k) lsum += std::log(2.0 * p->hMs[(size_t)c * d + k] - 1.0);
      const double kcc = std::exp(p->cp.log_sf2 - 0.5 * lsum);
      for (int k = 0; k < d; ++k) {
        const double msk = p->hMs[(size_t)c * d + k], zk = p->hZ[(size_t)c * d + k];
        const double mh = 0.5 - msk, factor = 0.5 * mh;
        const double dkm = 2.0 * factor * hkm[(size_t)(2 + d + k) * mp + c] + hwdiag[c] * mh / (2.0 * msk - 1.0) * kcc;
        const double colE = hcol[c], gx = hcol[(size_t)(k + 1) * mp + c], g2 = gxx[(size_t)k * mp + c];
        const double dknm = factor * (colE / msk - (g2 - 2.0 * zk * gx + zk * zk * colE) / (msk * msk));
        grad[pos++] = 0.5 * dkm - dknm;
      }
    }
  }
  res->n_hypers = pos;
}

// ---- several hyper-parameter sets in one pass (gprhip_batch_eval): the small path's chain, each launch once for all lanes
// Bytes one lane adds to the device: a problem's resident set without the inputs and targets it borrows, plus what the small
// path otherwise allocates at its first evaluation (the V store is in the plan; the partial sums and the K read-back are not)
int64_t batch_lane_bytes(const gprhip_problem* p) {
  gprhip_memory_plan_t plan;
  memory_plan(p->kind, GPRHIP_F64, p->n, p->D, p->d, p->m, p->chunk, &plan);
  const int64_t npad = (int64_t)p->nchunks * p->chunk;
  return plan.total - (p->n * p->D + npad) * 8 + small_part_len(p->d, p->D) * 8 + round_up(p->n, TILE) * 64 * 8;
}

// everything gprhip_batch_eval refuses, before anything is staged or enqueued
void batch_check(const gprhip_batch* b, int count, const gprhip_hypers* h, const gprhip_result* res, const double* grad,
                 int64_t ldg, int want_grad, const int* status) {
  if (!b || !h || !res || !status || count < 1 || count > (int)b->lanes.size()) {
    set_error("gprhip_batch_eval: invalid arguments (need 1 <= count <= the batch's lanes, h, res and status for every lane)");
    throw HipFail{ST_BAD_ARG};
  }
  const gprhip_problem* p = b->parent;
  if (!p) {
    set_error("gprhip_batch_eval: the problem this batch was made on has been destroyed");
    throw HipFail{ST_STATE};
  }
  for (int j = 0; j < count; ++j) {
    check_hypers(b->lanes[j], &h[j]);
    if (h[j].reuse_v) {
      set_error("gprhip_batch_eval: reuse_v is not available inside a batch");
      throw HipFail{ST_BAD_ARG};
    }
    if ((h[j].tproj != nullptr) != (h[0].tproj != nullptr) ||
        (h[j].log_hetero_skedasticity != nullptr) != (h[0].log_hetero_skedasticity != nullptr) ||
        (h[j].log_multiscales_m05 != nullptr) != (h[0].log_multiscales_m05 != nullptr) ||
        (h[j].variational != 0) != (h[0].variational != 0) || (h[j].model_only != 0) != (h[0].model_only != 0)) {
      set_error("gprhip_batch_eval: the lanes of one call must share their option shape (tproj, log_hetero_skedasticity, "
                "log_multiscales_m05 each given for all or none; variational and model_only equal)");
      throw HipFail{ST_BAD_ARG};
    }
  }
  if (!small_path_fits(p->m, p->mp, p->d, h[0].tproj ? p->D : 0, p->n, h[0].log_multiscales_m05 != nullptr)) {
    set_error("gprhip_batch_eval: these hypers are outside the small path (at most 64 input dimensions in front of a "
              "projection, multiscales with d <= 8): evaluate them one by one with gprhip_eval");
    throw HipFail{ST_BAD_ARG};
  }
  if (want_grad) {
    const gprhip_problem* l = b->lanes[0];
    const int64_t nh = gprhip_n_hypers(l, (h[0].tproj ? 1 : 0) | (h[0].log_hetero_skedasticity ? 2 : 0) |
                                              (h[0].log_multiscales_m05 ? 4 : 0));
    if (!grad || ldg < nh) {
      set_error("gprhip_batch_eval: want_grad needs grad with ldg >= the number of hyper-parameters");
      throw HipFail{ST_BAD_ARG};
    }
  }
  if (!p->have_inputs || (!p->have_targets && !h[0].model_only)) {
    set_error("gprhip: inputs/targets not set");
    throw HipFail{ST_STATE};
  }
}

// Lane l's part of the upload block and its state for this evaluation: what do_pass1 / do_pass2 / do_finish_enqueue decide on
// the host for a small-path evaluation, with every launch's arguments written into the lane's structs instead of launched
void batch_stage_lane(gprhip_batch* b, int j, const gprhip_hypers* h, int want_grad) {
  gprhip_problem* l = b->lanes[j];
  const gprhip_problem* p = b->parent;
  l->have_inputs = p->have_inputs;
  l->have_targets = p->have_targets;
  // (as do_pass1) the state of the lane's previous evaluation is void from here on
  l->have_model = l->have_factors = false;
  l->multi_state = false;
  l->tg_coeffs = false;
  l->x_last = nullptr;
  l->cond_km = -1.0;
  l->pg_m_valid = false;
  l->sp_ns_last = 0;
  forget_observations(l);
  l->have_v = l->have_k = l->small_k_valid = false;
  stage_hypers(l, h);
  l->want_grad = want_grad;
  l->n_total = l->n;
  const Ex1<double> e1 = ex1_of(l, l->ar1);
  const Ex2<double> e2 = ex2_of(l, l->ar2);
  {  // K_m and its factor (pass1_km_chol; with multiscales the lane takes the single evaluation's launches instead)
    PotrfKmLane& k = *b->host<PotrfKmLane>(j, b->o_km);
    k = PotrfKmLane{};
    k.g.cp = l->cp; k.g.Z = l->Z; k.g.m = l->m; k.g.d = l->d; k.g.jitter = l->h.jitter;
    k.g.het = l->has_het() ? l->het : nullptr; k.g.km = l->km;
    k.A = l->umat; k.Xinv = l->uinv; k.info = l->info;
  }
  {  // pass 1 and its reduction (pass1_small)
    SmallPass1Args& a = *b->host<SmallPass1Args>(j, b->o_p1);
    fill_row_pass1(l, a);
    a.part = l->small_part;
    a.Kout = (l->d <= 8 && !l->has_ms()) ? l->small_k : nullptr;
    l->small_k_valid = a.Kout != nullptr;
    SmallReduce1Args& r = *b->host<SmallReduce1Args>(j, b->o_r1);
    r.part = a.part; r.ng = small_pass1_groups(a.rows_p); r.mp = a.mp; r.tile = e1.tiles; r.cvec = e1.c; r.tail = e1.tail;
  }
  {  // B~, its factor and the m-vectors (pass2_b_chol, single block)
    l->a1_in_scal = true;
    PotrfFuseLane& f = *b->host<PotrfFuseLane>(j, b->o_fuse);
    f = PotrfFuseLane{};
    f.f.src = e1.tiles; f.f.cvec = e1.c; f.f.tail_in = e1.tail; f.f.tail_out = l->scal + SC_A1TAIL;
    f.f.uinv = l->uinv; f.f.bvec = l->bvec; f.f.ttil = l->ttil; f.f.tvec = l->tvec;
    f.f.logdet = l->scal + SC_LOGDET_B; f.f.bb = l->scal + SC_BB;
    f.A = l->bmat; f.Xinv = l->rinv; f.info = l->info + 1; f.m_real = l->m;
  }
  ShipArgs& sh = *b->host<ShipArgs>(j, b->o_ship);
  sh = ShipArgs{};
  sh.src[0] = l->res_dev; sh.dst[0] = l->res_host;
  if (want_grad) {
    l->merged_x = false;
    SmallPass2Args& a = *b->host<SmallPass2Args>(j, b->o_p2);  // pass 2 and its reduction (pass2_small)
    fill_row_pass2(l, a);
    a.uinv = l->uinv;
    a.Kin = (l->small_k_valid && l->d <= 8 && !l->has_ms()) ? l->small_k : nullptr;
    a.part = l->small_part;
    l->x_last = a.X;
    SmallReduce2Args& r = *b->host<SmallReduce2Args>(j, b->o_r2);
    r.part = a.part; r.ng = small_pass2_groups(a.rows_p); r.mp = a.mp; r.d = a.d; r.D = a.D; r.ms = l->has_ms() ? 1 : 0;
    r.col_rows = (int)l->col_rows(); r.tile = e2.tiles; r.colblk = e2.col; r.proj = e2.proj; r.tail = e2.tail;
    SmallFinishArgs& fa = *b->host<SmallFinishArgs>(j, b->o_fin);  // finish_small
    fa.uinv = l->uinv; fa.rinv = l->rinv; fa.ttil = l->ttil; fa.km = l->km; fa.Z = l->Z; fa.g = e2.tiles;
    fa.ms = l->has_ms() ? l->ms : nullptr;
    fa.m = l->m; fa.mp = l->mp; fa.d = l->d; fa.km_rows = l->has_ms() ? 2 * l->d + 2 : l->d + 2;
    fa.wmat = l->wmat; fa.kmred = l->kmred; fa.wdiag = wants_wdiag(l) ? l->wdiag : nullptr;
    fa.gather_from = e2.col; fa.n_gather = e2.len_from_col(); fa.ex = l->ex_dev + A1_TAIL;
    sh.n[0] = l->res_len + A1_TAIL + e2.len_from_col();  // (the lane's own pinned block, written by the ship launch)
  } else {
    sh.n[0] = NSCAL + 2 + l->mp;  // (finish_engine's evidence-only block: scalars, flags, t)
  }
}

void batch_eval(gprhip_batch* b, int count, const gprhip_hypers* h, int want_grad, gprhip_result* res, double* grad,
                int64_t ldg, double* coeffs, int* status) {
  batch_check(b, count, h, res, grad, ldg, want_grad, status);
  gprhip_problem* const p = b->parent;
  gprhip_problem* const l0 = b->lanes[0];  // (its timer carries the batched stages)
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  want_grad = want_grad != 0;
  for (int j = 0; j < count; ++j) batch_stage_lane(b, j, &h[j], want_grad);
  // one transfer: the parameter blocks and the argument structs of the lanes in use (the previous batch evaluation ended
  // in a wait for the stream, so the pinned block is free)
  GPR_HIP(hipMemcpyAsync(b->up_dev, b->up_host, (size_t)(b->stride * count), hipMemcpyHostToDevice, s));
  if (l0->has_proj())
    for (int j = 0; j < count; ++j) {
      gprhip_problem* l = b->lanes[j];
      launch_project(l->X, l->n, l->D, l->d, l->tproj, l->P, s);
    }
  const int64_t st = b->stride;
  tstart(l0, "batch_km_chol");
  if (l0->has_ms()) {  // (K_m with multiscales is built by the launch the single evaluation uses, lane by lane)
    for (int j = 0; j < count; ++j) {
      gprhip_problem* l = b->lanes[j];
      launch_cov_upper(l->cp, l->Z, l->m, l->mp, l->d, l->h.jitter, l->has_het() ? l->het : nullptr, l->km, l->umat, s);
      potrf_trtri(l, l->umat, l->uinv, l->wmat, l->info);
    }
  } else {
    launch_potrf_km_batch(b->dev<PotrfKmLane>(b->o_km), count, st, s);
  }
  tstop(l0);
  tstart(l0, "batch_p1");
  launch_small_pass1_batch(*b->host<SmallPass1Args>(0, b->o_p1), b->dev<SmallPass1Args>(b->o_p1),
                           b->dev<SmallReduce1Args>(b->o_r1), count, st, s);
  tstop(l0);
  tstart(l0, "batch_b_chol");
  launch_potrf_fused_batch(b->dev<PotrfFuseLane>(b->o_fuse), count, st, s);
  tstop(l0);
  if (want_grad) {
    tstart(l0, "batch_p2");
    launch_small_pass2_batch(*b->host<SmallPass2Args>(0, b->o_p2), (int)l0->col_rows(), b->dev<SmallPass2Args>(b->o_p2),
                             b->dev<SmallReduce2Args>(b->o_r2), count, st, s);
    tstop(l0);
    tstart(l0, "batch_finish");
    launch_small_finish_batch(*b->host<SmallFinishArgs>(0, b->o_fin), b->dev<SmallFinishArgs>(b->o_fin), count, st, s);
  } else {
    tstart(l0, "batch_finish");
  }
  // every lane's results into its own pinned block by one launch, whatever their size
  launch_ship_batch(b->dev<ShipArgs>(b->o_ship), count, st, b->host<ShipArgs>(0, b->o_ship)->n[0], s);
  tstop(l0);
  for (int j = 0; j < count; ++j) {
    b->lanes[j]->stage = 3;
    b->lanes[j]->have_v = true;  // (revoked by the collect if the lane's factorisation was refused)
  }
  GPR_HIP(hipStreamSynchronize(s));  // the one wait of the batch
  std::string first_error;
  for (int j = 0; j < count; ++j) {
    try {
      do_finish_collect(b->lanes[j], &res[j], grad ? grad + (int64_t)j * ldg : nullptr,
                        coeffs ? coeffs + (int64_t)j * p->m : nullptr);
      status[j] = GPRHIP_OK;
    } catch (const HipFail& e) {
      if (e.status != ST_NOT_POSDEF) throw;
      status[j] = GPRHIP_ENOTPOSDEF;
      if (first_error.empty()) first_error = last_error();
    }
  }
  if (!first_error.empty()) set_error(first_error);
}

// a buffer of the problem that is being regrown: freed now, not at problem destruction
template <typename T>
void release_buf(gprhip_problem* p, T*& q) {
  if (!q) return;
  auto it = std::find(p->allocs.begin(), p->allocs.end(), static_cast<void*>(q));
  if (it != p->allocs.end()) p->allocs.erase(it);
  (void)hipFree(q);
  q = nullptr;
}

// a buffer of the problem that a call needs `need` elements of (`have`: what it holds): regrown once the stream has drained;
// the recorded size is zero while there is no buffer
template <typename T>
void grow_buf(gprhip_problem* p, T*& q, int64_t& have, int64_t need) {
  if (have >= need) return;
  GPR_HIP(hipStreamSynchronize(p->stream));
  release_buf(p, q);
  have = 0;
  q = p->alloc<T>(need);
  have = need;
}

// prediction scratch for chunks of `chunk` test points: the points, their projection and three row vectors
void ensure_predict_scratch(gprhip_problem* p, int64_t chunk) {
  if (p->xt && p->xt_rows >= chunk) return;
  GPR_HIP(hipStreamSynchronize(p->stream));
  release_buf(p, p->xt);
  release_buf(p, p->pt);
  release_buf(p, p->prow);
  p->xt_rows = 0;
  p->xt = p->alloc<double>(chunk * p->D);
  p->pt = p->alloc<double>(chunk * p->d);
  p->prow = p->alloc<double>(3 * chunk);
  p->xt_rows = chunk;
}

// The calls that evaluate the model at test points share three steps ("Calls at test points"): a plan of the
// chunk and of what must grow (predict_plan.h: nothing is allocated), its allocation, and a walk over the chunks.

// few inducing points: a chunk of test points is one kernel (small.hip / predict_grad.hip) that keeps its n x m tiles in LDS
bool one_kernel_path(const gprhip_problem* p) {
  return p->small_path && !p->f32 && p->m <= 64 && p->mp == TILE && p->d <= 16 && !p->has_ms();
}

ChunkPlan chunk_plan(const gprhip_problem* p, int64_t nt, bool mats) {
  return predict_plan(p->chunk, nt, mats, p->pred_rows, p->xt_rows);
}

// carries out a plan: predA / predB and the xt / pt / prow scratch, as far as they must grow
void chunk_alloc(gprhip_problem* p, const ChunkPlan& c) {
  if (c.grow_pred) {
    GPR_HIP(hipStreamSynchronize(p->stream));
    release_buf(p, p->predA);
    release_buf(p, p->predB);
    p->pred_rows = 0;
    p->predA = p->alloc<char>(c.chunk * p->mp * p->esz);
    p->predB = p->alloc<char>(c.chunk * p->mp * p->esz);
    p->pred_rows = c.chunk;
  }
  ensure_predict_scratch(p, c.chunk);
}

// Walks nt test points (x, row stride ld) in chunks: uploads a chunk into p->xt unless the points are on the device (then
// ld == D), projects it into p->pt where the model has a projection, calls body(lo, rows, rows_p, raw, pts) with the device
// pointers of the raw and the projected points, and synchronises the stream before the buffers are reused by the next chunk
// (device outputs are complete then).
template <typename F>
void walk_chunks(gprhip_problem* p, int64_t chunk, const double* x, int64_t ld, int64_t nt, int on_device, F&& body) {
  hipStream_t s = p->stream;
  const int D = p->D, d = p->d;
  for (int64_t lo = 0; lo < nt; lo += chunk) {
    const int rows = (int)std::min<int64_t>(chunk, nt - lo);
    const int rows_p = (int)round_up(rows, TILE);
    const double* raw = x + lo * ld;
    if (!on_device) {
      GPR_HIP(hipMemcpy2DAsync(p->xt, (size_t)D * sizeof(double), raw, (size_t)ld * sizeof(double), (size_t)D * sizeof(double),
                               (size_t)rows, hipMemcpyHostToDevice, s));
      raw = p->xt;
    }
    const double* pts = raw;
    if (p->has_proj()) {
      launch_project(raw, rows, D, d, p->tproj, p->pt, s);
      pts = p->pt;
    }
    body(lo, rows, rows_p, raw, pts);
    GPR_HIP(hipStreamSynchronize(s));
  }
}

// The model-state refusals of these calls, in one order: no model ("... to <verb>"), multiscales (where the call has no
// kernel for them), no factors (where variances are involved), a several-target state and untrustworthy fp32 coefficients
// (where means are involved; `after_targets` says where they come from instead).
void need_posterior_state(gprhip_problem* p, const char* fn, const char* verb, bool refuse_ms, bool want_var, bool want_mean,
                          const char* after_targets) {
  if (!p->have_model || p->stage != 0) {
    set_error(std::string(fn) + ": no completed evaluation to " + verb);
    throw HipFail{ST_STATE};
  }
  if (refuse_ms && p->has_ms()) {
    set_error(std::string(fn) + ": multiscales are not supported (the model state has log_multiscales_m05)");
    throw HipFail{ST_BAD_ARG};
  }
  if (want_var) need_factors(p, fn);
  if (want_mean && p->multi_state) {
    set_error(std::string(fn) + ": the last evaluation was gprhip_eval_targets (several target vectors): " + after_targets);
    throw HipFail{ST_STATE};
  }
  if (want_mean) need_trustworthy_coeffs(p, fn);
}

// Means.calc / Variances.calc (lib/fitc_gp.ml:418-425, :498-518) at nt test points, chunk by chunk,
// with the m x m state of the last evaluation: V_t = K_tm U^-1, Q_t = V_t R~^-1 (= K_tm R^-1).
template <typename TS>
void do_predict(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int predictive,
                double* means, double* variances) {
  need_posterior_state(p, "gprhip_predict", "predict from", false, variances, means,
                       "means come from gprhip_predict_targets, or from gprhip_predict after the next gprhip_eval");
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int mp = p->mp;
  const bool small = one_kernel_path(p);  // it needs the row buffers only, not the two chunk x mp matrices
  const ChunkPlan plan = chunk_plan(p, nt, !small);
  chunk_alloc(p, plan);
  const int64_t chunk = plan.chunk;
  TS* const bufA = static_cast<TS*>(chunk > p->chunk ? p->predA : p->bufA);
  TS* const bufB = static_cast<TS*>(chunk > p->chunk ? p->predB : p->bufB);
  double* rmean = p->prow;
  double* rk = p->prow + chunk;
  double* rb = p->prow + 2 * chunk;
  walk_chunks(p, chunk, test_inputs, ld, nt, 0, [&](int64_t lo, int rows, int rows_p, const double*, const double* pts) {
    if (small) {  // few inducing points: the whole chunk in one kernel (small.hip)
      SmallPredictArgs a;
      a.cp = p->cp; a.pts = pts; a.Z = p->Z; a.uinv = p->uinv; a.rinv = p->rinv; a.tvec = p->tvec;
      a.rows = rows; a.m = p->m; a.mp = mp; a.d = p->d; a.add = predictive ? p->h.sigma2 : 0.0;
      a.means = means ? rmean : nullptr; a.vars = variances ? rk : nullptr;
      launch_small_predict(a, s);
      if (means) GPR_HIP(hipMemcpyAsync(means + lo, rmean, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
      if (variances) GPR_HIP(hipMemcpyAsync(variances + lo, rk, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
      return;
    }
    launch_cov_cross<TS>(p->cp, pts, rows, rows_p, p->Z, p->m, mp, p->d, bufA, s);
    if (means) {
      launch_row_sumsq_dot<TS>(bufA, p->tvec, rows, mp, nullptr, rmean, s);
      GPR_HIP(hipMemcpyAsync(means + lo, rmean, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (variances) {
      GemmArgsT<TS> g;  // trsm ~side:`R chol_km
      g.A = bufA; g.lda = mp; g.B = inv_u<TS>(p); g.ldb = mp; g.C = bufB; g.ldc = mp;
      g.M = rows_p; g.N = mp; g.K = mp; g.tri = TRI_KHI_BN;
      launch_gemm(OP_NN, g, s);
      launch_row_sumsq_dot<TS>(bufB, nullptr, rows, mp, rk, nullptr, s);
      GemmArgsT<TS> q;  // trsm ~side:`R r_mat  (R = R~ U)
      q.A = bufB; q.lda = mp; q.B = inv_r<TS>(p); q.ldb = mp; q.C = bufA; q.ldc = mp;
      q.M = rows_p; q.N = mp; q.K = mp; q.tri = TRI_KHI_BN;
      launch_gemm(OP_NN, q, s);
      launch_row_sumsq_dot<TS>(bufA, nullptr, rows, mp, rb, nullptr, s);
      launch_variance_combine(rk, rb, rows, p->cp.sf2, predictive ? p->h.sigma2 : 0.0, rk, s);
      GPR_HIP(hipMemcpyAsync(variances + lo, rk, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
    }
  });
}

// gprhip_predict_input_grad: M = U^-1 (I - R~^-1 R~^-T) U^-T of the current model state (full symmetric), with the m x m
// machinery of the finish stage.  I - B~^-1 has its spectrum in [0, 1): in this whitened form M carries no cancellation of
// (K_m + jitter)^-1 against B^-1 beyond what the variance itself has.  binv, wtil and kj are scratch between evaluations.
void ensure_predict_m(gprhip_problem* p) {
  if (p->pg_m_valid) return;
  hipStream_t s = p->stream;
  const int mp = p->mp;
  tstart(p, "pg_m");
  triu_xxt(p, p->rinv, p->binv, s);  // B~^-1 = R~^-1 R~^-T (upper tiles; identity on the padding)
  launch_identity_minus_sym(p->binv, mp, p->wtil, s);
  const int ks = ((int64_t)(mp / TILE) * (mp / TILE) <= 256) ? mxm_slices(mp) : 1;
  GemmArgs y;  // Y = (I - B~^-1) U^-T
  y.A = p->wtil; y.lda = mp; y.B = p->uinv; y.ldb = mp; y.C = p->kj; y.ldc = mp;
  y.M = mp; y.N = mp; y.K = mp; y.tri = TRI_KLO_BN;
  gemm_splitk(p, OP_NT, y, ks);
  GemmArgs w;  // M = U^-1 Y
  w.A = p->uinv; w.lda = mp; w.B = p->kj; w.ldb = mp; w.C = p->pg_m; w.ldc = mp;
  w.M = mp; w.N = mp; w.K = mp; w.tri = TRI_KLO_BM;
  gemm_splitk(p, OP_NN, w, ks);
  tstop(p);
  p->pg_m_valid = true;
}

// The buffers of one call of gprhip_predict_input_grad / gprhip_acquire: the chunk plan, M, the chunk buffers and
// the gradient staging, allocated after a look at the device's free memory (a refusal leaves the problem as it was).
// want_var: K and G of a chunk are needed (matrices in memory unless the one-kernel path serves the shape);
// host_g: a gradient matrix is staged on the device ([rows][D]) in front of a transfer
struct PgPlan {
  int64_t chunk;
  bool small, mats;
  double *stage_g[2], *stage_p[2];  // gradient staging [rows][D] (host part) and [rows][d] (in front of the projection)
  double *bufA, *bufB;              // K and G of a chunk
  double *rmean, *rvar, *rval;      // three row vectors of xt_rows entries
};
// with_pg = false (gprhip_sample_paths): neither M nor the gradient staging is made -- K and K U^-1 of a chunk are all it needs
PgPlan pg_prepare(gprhip_problem* p, const char* fn, int64_t nt, bool want_var, bool host_g, bool with_pg = true,
                  int64_t extra_bytes = 0) {
  hipStream_t s = p->stream;
  const int mp = p->mp, D = p->D, d = p->d;
  const bool proj = p->has_proj();
  const bool small = one_kernel_path(p);
  const bool mats = !small && want_var;  // K and G of a chunk are matrices in memory
  const ChunkPlan cplan = chunk_plan(p, nt, mats);
  const int64_t chunk = cplan.chunk;
  const bool grow_pred = cplan.grow_pred, grow_xt = cplan.grow_xt;
  // everything this call allocates, after a look at the device's free memory: a refusal leaves the problem as it was
  const bool need_m = mats && with_pg && !p->pg_m;
  const bool grow_pg = with_pg && (host_g || proj) && (p->pg_rows < chunk || (host_g && !p->pg_host) || (proj && !p->pg_proj));
  const bool pg_host = host_g || p->pg_host, pg_proj = proj || p->pg_proj;
  const int64_t pg_len = 2 * chunk * ((pg_host ? D : 0) + (pg_proj ? d : 0));
  {
    int64_t need = extra_bytes;
    if (need_m) need += (int64_t)mp * mp * 8;
    if (grow_pred) need += 2 * chunk * mp * 8;
    if (grow_xt) need += chunk * (D + d + 3) * 8;
    if (grow_pg) need += pg_len * 8;
    if (need > 0) {
      size_t free_b = 0, total_b = 0;
      GPR_HIP(hipMemGetInfo(&free_b, &total_b));
      if ((size_t)need + (size_t(64) << 20) > free_b) {
        set_error(std::string(fn) + ": not enough device memory for M and the chunk buffers of the prediction gradient");
        throw HipFail{ST_OOM};
      }
    }
  }
  if (need_m) p->pg_m = p->alloc<double>((int64_t)mp * mp);
  chunk_alloc(p, cplan);
  if (grow_pg) {
    GPR_HIP(hipStreamSynchronize(s));
    release_buf(p, p->pg_buf);
    p->pg_rows = 0;
    p->pg_buf = p->alloc<double>(pg_len);
    p->pg_rows = chunk;
    p->pg_host = pg_host;
    p->pg_proj = pg_proj;
  }
  const int64_t pgr = p->pg_rows;
  PgPlan plan;
  plan.chunk = chunk; plan.small = small; plan.mats = mats;
  plan.stage_g[0] = p->pg_buf;                                               // [rows][D] (host part)
  plan.stage_g[1] = p->pg_buf ? p->pg_buf + pgr * D : nullptr;
  double* const stage_p0 = p->pg_buf ? p->pg_buf + (p->pg_host ? 2 * pgr * D : 0) : nullptr;
  plan.stage_p[0] = stage_p0;                                                // [rows][d] (projection)
  plan.stage_p[1] = stage_p0 ? stage_p0 + pgr * d : nullptr;
  plan.bufA = static_cast<double*>(chunk > p->chunk ? p->predA : p->bufA);
  plan.bufB = static_cast<double*>(chunk > p->chunk ? p->predB : p->bufB);
  plan.rmean = p->prow;
  plan.rvar = p->prow + p->xt_rows;
  plan.rval = p->prow + 2 * p->xt_rows;
  return plan;
}

// One chunk of the prediction gradient on the device: K and G = K M where the plan keeps them in memory, then the gradient
// kernel (predict_grad.hip; the one-kernel variant for few inducing points) and the back-projection of its d/dp where the
// model has a projection.  dst[q]: where the [rows][D] gradients end up (mean, variance; null: not wanted); acq: the criterion
// epilogue of gprhip_acquire, mv: that of gprhip_acquire_max_value (at most one of the two), whose one gradient goes to dst[0].
void pg_chunk(gprhip_problem* p, const PgPlan& plan, const double* pts, int rows, int rows_p, bool want_var, double add,
              double* mean_dev, double* var_dev, double* const dst[2], const AcqArgs* acq, const MvArgs* mv = nullptr) {
  hipStream_t s = p->stream;
  const int mp = p->mp, D = p->D, d = p->d;
  const bool proj = p->has_proj();
  // where the kernel writes: d/dp in front of a projection
  double* const kout[2] = {dst[0] ? (proj ? plan.stage_p[0] : dst[0]) : nullptr, dst[1] ? (proj ? plan.stage_p[1] : dst[1]) : nullptr};
  const int64_t kld = proj ? d : D;
  if (plan.small) {  // few inducing points: the whole chunk in one kernel
    tstart(p, "pg_grad");
    SmallPredictGradArgs a;
    a.cp = p->cp; a.pts = pts; a.Z = p->Z; a.shift = p->zshift; a.uinv = p->uinv; a.rinv = p->rinv; a.tvec = p->tvec;
    a.rows = rows; a.m = p->m; a.mp = mp; a.d = d; a.want_var = want_var ? 1 : 0; a.add = add;
    a.means = mean_dev; a.vars = var_dev; a.dmeans = kout[0]; a.dvars = kout[1]; a.ldg = kld;
    if (mv) launch_small_max_value_grad(a, *mv, s);
    else if (acq) launch_small_acquire_grad(a, *acq, s);
    else launch_small_predict_grad(a, s);
  } else {
    if (plan.mats) {
      tstart(p, "pg_cov");
      launch_cov_cross<double>(p->cp, pts, rows, rows_p, p->Z, p->m, mp, d, plan.bufA, s);
      tstop(p);
      tstart(p, "pg_gemm");
      GemmArgs g;  // G = K M
      g.A = plan.bufA; g.lda = mp; g.B = p->pg_m; g.ldb = mp; g.C = plan.bufB; g.ldc = mp;
      g.M = rows_p; g.N = mp; g.K = mp;
      launch_gemm(OP_NN, g, s);
      tstop(p);
    }
    tstart(p, "pg_grad");
    PredictGradArgs a;
    a.pts = pts; a.Z = p->Z; a.shift = p->zshift; a.tvec = p->tvec; a.G = plan.mats ? plan.bufB : nullptr;
    a.rows = rows; a.m = p->m; a.mp = mp; a.d = d;
    a.log_sf2 = p->cp.log_sf2; a.inv_ell2_05 = p->cp.inv_ell2_05; a.sf2 = p->cp.sf2; a.add = add;
    a.means = mean_dev; a.vars = var_dev; a.dmeans = kout[0]; a.dvars = kout[1]; a.ldg = kld;
    if (mv) launch_max_value_grad(a, *mv, s);
    else if (acq) launch_acquire_grad(a, *acq, s);
    else launch_predict_grad(a, s);
  }
  if (proj)
    for (int q = 0; q < 2; ++q)
      if (dst[q]) launch_input_grad_project(kout[q], rows, d, D, p->tproj, dst[q], D, s);
  tstop(p);
}

// the best k of a call, best first, into its three outputs (top_values / top_dvalues may be null)
void write_topk(const SpBest& best, int top_k, int D, int64_t* top_index, double* top_values, double* top_dvalues) {
  for (int j = 0; j < top_k; ++j) {
    if (j >= (int)best.idx.size()) {
      top_index[j] = -1;  // fewer than top_k candidates qualify: their values and gradients are left as they are
      continue;
    }
    top_index[j] = best.idx[j];
    if (top_values) top_values[j] = best.val[j];
    if (top_dvalues) std::copy(best.grad.begin() + (size_t)j * D, best.grad.begin() + (size_t)(j + 1) * D, top_dvalues + (int64_t)j * D);
  }
}

// Means / variances of do_predict and their gradients with respect to the test inputs (predict_grad.hip), chunk by chunk.
// The caller has checked the arguments and the limits.
void do_predict_input_grad(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int predictive, double* means,
                           double* variances, double* dmeans, double* dvariances, int64_t ldg, int on_device) {
  const bool want_mean = means || dmeans, want_var = variances || dvariances;
  need_posterior_state(p, "gprhip_predict_input_grad", "predict from", true, want_var, want_mean,
                       "means and their gradients are available after the next gprhip_eval");
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int D = p->D;
  const PgPlan plan = pg_prepare(p, "gprhip_predict_input_grad", nt, want_var, !on_device && (dmeans || dvariances));
  double *const rmean = plan.rmean, *const rvar = plan.rvar;
  if (plan.mats) ensure_predict_m(p);
  const double add = predictive ? p->h.sigma2 : 0.0;
  walk_chunks(p, plan.chunk, test_inputs, ld, nt, on_device, [&](int64_t lo, int rows, int rows_p, const double*, const double* pts) {
    // where the outputs of this chunk end up on the device
    double* const mean_dev = means ? (on_device ? means + lo : rmean) : nullptr;
    double* const var_dev = variances ? (on_device ? variances + lo : rvar) : nullptr;
    double* const dst[2] = {dmeans ? (on_device ? dmeans + lo * D : plan.stage_g[0]) : nullptr,
                            dvariances ? (on_device ? dvariances + lo * D : plan.stage_g[1]) : nullptr};
    pg_chunk(p, plan, pts, rows, rows_p, want_var, add, mean_dev, var_dev, dst, nullptr);
    if (!on_device) {
      if (means) GPR_HIP(hipMemcpyAsync(means + lo, rmean, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
      if (variances) GPR_HIP(hipMemcpyAsync(variances + lo, rvar, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
      double* const host[2] = {dmeans, dvariances};
      for (int q = 0; q < 2; ++q)
        if (host[q])
          GPR_HIP(hipMemcpy2DAsync(host[q] + lo * ldg, (size_t)ldg * sizeof(double), dst[q], (size_t)D * sizeof(double),
                                   (size_t)D * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost, s));
    }
  });
  if (p->timer.on) tcollect(p);
}

// the criterion needs the variance (the bound with kappa = 0 is the mean alone); the kernels' form of the criterion
bool acq_wants_var(const gprhip_acquisition* acq) { return !(acq->kind == GPRHIP_ACQ_BOUND && acq->kappa == 0.0); }
AcqArgs acq_args(const gprhip_acquisition* acq) {
  AcqArgs q;
  q.kind = acq->kind; q.s = acq->maximise ? 1.0 : -1.0; q.best = acq->best; q.xi = acq->xi; q.kappa = acq->kappa;
  q.var_floor = acq->var_floor; q.values = nullptr;
  return q;
}

// the extremes of a max-value call to the device (p->mv_extremes through the pinned mirror p->mv_host), once the call can no
// longer be refused
void mv_upload(gprhip_problem* p, MvArgs* mv, const double* host_extremes) {
  if (!p->mv_extremes) {
    p->mv_extremes = p->alloc<double>(GPRHIP_MAX_EXTREMES);
    GPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->mv_host), GPRHIP_MAX_EXTREMES * sizeof(double), hipHostMallocDefault));
  }
  // (every earlier call has synchronised the stream before it returned: the mirror is free)
  std::copy(host_extremes, host_extremes + mv->n, p->mv_host);
  GPR_HIP(hipMemcpyAsync(p->mv_extremes, p->mv_host, (size_t)mv->n * sizeof(double), hipMemcpyHostToDevice, p->stream));
  mv->extremes = p->mv_extremes;
}

// gprhip_acquire: the chunk loop of do_predict_input_grad with the criterion epilogue of the two kernels -- one value vector and
// one gradient matrix instead of two --, and the best top_k candidates selected on the device chunk by chunk (acquire.hip),
// the chunks' lists merged here with the same rule: value descending, the lower index first among equal values.
// The caller has checked the arguments and the limits.  The criterion is q (gprhip_acquire) or, where mv is not null, max-value
// entropy search over host_extremes (gprhip_acquire_max_value), which are uploaded once the call can no longer be refused.
void acquire_walk(gprhip_problem* p, const char* fn, bool want_var, double add, AcqArgs q, MvArgs* mv, const double* host_extremes,
                  const double* test_inputs, int64_t ld, int64_t nt, double* values, double* dvalues, int64_t ldg, double* means,
                  double* variances, int top_k, int64_t* top_index, double* top_values, double* top_dvalues, int on_device) {
  need_posterior_state(p, fn, "predict from", true, want_var, true,
                       "means and their gradients are available after the next gprhip_eval");
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int D = p->D;
  const bool want_grad = dvalues || (top_k > 0 && top_dvalues);
  const bool stage_grad = want_grad && !(on_device && dvalues);  // the gradient of a chunk stays in the library's staging
  const PgPlan plan = pg_prepare(p, fn, nt, want_var, stage_grad);
  if (mv) mv_upload(p, mv, host_extremes);
  if (top_k > 0 && !p->acq_scratch) {
    p->acq_scratch = p->alloc<char>(acq_select_scratch_bytes());
    p->acq_out = p->alloc<double>((int64_t)ACQ_MAX_TOP_K * (D + 2));
    GPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->acq_host), (size_t)ACQ_MAX_TOP_K * (D + 2) * sizeof(double),
                          hipHostMallocDefault));
  }
  if (plan.mats) ensure_predict_m(p);
  SpBest best;  // the best so far, over the chunks done
  walk_chunks(p, plan.chunk, test_inputs, ld, nt, on_device, [&](int64_t lo, int rows, int rows_p, const double*, const double* pts) {
    double* const mean_dev = means ? (on_device ? means + lo : plan.rmean) : nullptr;
    double* const var_dev = variances ? (on_device ? variances + lo : plan.rvar) : nullptr;
    double* const val_dev = (values && on_device) ? values + lo : ((values || top_k > 0) ? plan.rval : nullptr);
    double* const dst = want_grad ? (stage_grad ? plan.stage_g[0] : dvalues + lo * D) : nullptr;
    double* const dsts[2] = {dst, nullptr};
    q.values = val_dev;
    if (mv) mv->values = val_dev;
    pg_chunk(p, plan, pts, rows, rows_p, want_var, add, mean_dev, var_dev, dsts, mv ? nullptr : &q, mv);
    if (!on_device) {
      if (values) GPR_HIP(hipMemcpyAsync(values + lo, val_dev, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
      if (means) GPR_HIP(hipMemcpyAsync(means + lo, plan.rmean, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
      if (variances)
        GPR_HIP(hipMemcpyAsync(variances + lo, plan.rvar, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
      if (dvalues)
        GPR_HIP(hipMemcpy2DAsync(dvalues + lo * ldg, (size_t)ldg * sizeof(double), dst, (size_t)D * sizeof(double),
                                 (size_t)D * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost, s));
    }
    // the best top_k of the chunk, in pieces of at most 256 slabs, before its buffers are reused
    const int64_t piece_rows = (int64_t)ACQ_SELECT_MAX_SLABS * 2048;
    for (int64_t po = 0; top_k > 0 && po < rows; po += piece_rows) {
      const int pr = (int)std::min<int64_t>(piece_rows, rows - po);
      const bool gather_g = top_dvalues != nullptr;
      tstart(p, "acq_select");
      AcqSelectArgs sel;
      sel.values = val_dev + po; sel.rows = pr; sel.k = top_k; sel.grads = gather_g ? dst + po * D : nullptr; sel.D = D;
      sel.scratch = p->acq_scratch; sel.out = p->acq_out;
      launch_acq_select(sel, s);
      tstop(p);
      const int64_t blk = (int64_t)top_k * (gather_g ? D + 2 : 2);
      GPR_HIP(hipMemcpyAsync(p->acq_host, p->acq_out, (size_t)blk * sizeof(double), hipMemcpyDeviceToHost, s));
      GPR_HIP(hipStreamSynchronize(s));
      // (the device has sorted by the value itself: sign +1; an earlier entry stays in front of an equal later one)
      const double* const hi = p->acq_host;
      sp_merge_topk(best, top_k, 1.0, hi, hi + top_k, gather_g ? hi + 2 * top_k : nullptr, D, lo + po);
    }
  });
  write_topk(best, top_k, D, top_index, top_values, top_dvalues);
  if (p->timer.on) tcollect(p);
}

void do_acquire(gprhip_problem* p, const gprhip_acquisition* acq, const double* test_inputs, int64_t ld, int64_t nt,
                double* values, double* dvalues, int64_t ldg, double* means, double* variances, int top_k, int64_t* top_index,
                double* top_values, double* top_dvalues, int on_device) {
  acquire_walk(p, "gprhip_acquire", acq_wants_var(acq) || variances, acq->predictive ? p->h.sigma2 : 0.0, acq_args(acq), nullptr,
               nullptr, test_inputs, ld, nt, values, dvalues, ldg, means, variances, top_k, top_index, top_values, top_dvalues,
               on_device);
}

// gprhip_acquire_max_value: the walk of gprhip_acquire with the epilogue of mv_math.h; the latent variance, always needed
void do_acquire_max_value(gprhip_problem* p, const double* extremes, int n_extremes, int maximise, double var_floor,
                          const double* test_inputs, int64_t ld, int64_t nt, double* values, double* dvalues, int64_t ldg,
                          double* means, double* variances, int top_k, int64_t* top_index, double* top_values,
                          double* top_dvalues, int on_device) {
  MvArgs mv;
  mv.n = n_extremes; mv.s = maximise ? 1.0 : -1.0; mv.var_floor = var_floor; mv.extremes = nullptr; mv.values = nullptr;
  acquire_walk(p, "gprhip_acquire_max_value", true, 0.0, AcqArgs{}, &mv, extremes, test_inputs, ld, nt, values, dvalues, ldg,
               means, variances, top_k, top_index, top_values, top_dvalues, on_device);
}

// ---- what gprhip_acquire_refine and gprhip_sample_paths_refine share: one arena (rf_buf), one library-side loop
// The arena of a call with ns starts:  bnd (lower | upper | scale, [D] each) | Y X G GY ([ns][D] each) | A AY AL ([ns] each) |
// n_int_vectors integer vectors [ns] (evals | accepted | status, and draw_of for the sample paths) | the staging of a host trace
struct RefineWork {
  int64_t ns, len, trace_len;  // starts; doubles of the arena; of them the staging of a host trace, the arena's tail
  double *bnd, *Y, *X, *G, *GY, *A, *AY, *AL;
  int* ints;
  double* trace_dev;  // where the kernels write the trace: the caller's device buffer, the staging, or null
};
int64_t refine_work_len(int D, int64_t ns, int n_int_vectors, int64_t trace_len) {
  return 3 * D + 4 * ns * D + 3 * ns + (n_int_vectors * ns + 1) / 2 + trace_len;
}
// the sizes of a call's arena, before anything is allocated: w.len doubles are counted in front of pg_prepare where rf_buf is shorter
RefineWork refine_work_sizes(int D, int64_t ns, int n_int_vectors, int max_evals, const double* trace, int on_device) {
  RefineWork w{};
  w.ns = ns;
  w.trace_len = (trace && !on_device) ? ns * max_evals * (2 * D + 3) : 0;
  w.len = refine_work_len(D, ns, n_int_vectors, w.trace_len);
  return w;
}
// grows rf_buf to w.len doubles, makes the pinned count where the library-side loop will read it, carves the arena up and
// uploads the box, the scale and the caller's host trace
void refine_work(gprhip_problem* p, RefineWork& w, const double* lower, const double* upper, const double* scale, double* trace,
                 int on_device, bool host_loop) {
  hipStream_t s = p->stream;
  const int D = p->D;
  const int64_t ns = w.ns, nsD = ns * D;
  grow_buf(p, p->rf_buf, p->rf_len, w.len);
  if (host_loop && !p->rf_active) GPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->rf_active), sizeof(int), hipHostMallocDefault));
  w.bnd = p->rf_buf;
  w.Y = w.bnd + 3 * D; w.X = w.Y + nsD; w.G = w.X + nsD; w.GY = w.G + nsD;
  w.A = w.GY + nsD; w.AY = w.A + ns; w.AL = w.AY + ns;
  w.ints = reinterpret_cast<int*>(w.AL + ns);
  w.trace_dev = trace ? (on_device ? trace : w.bnd + (w.len - w.trace_len)) : nullptr;
  GPR_HIP(hipMemcpyAsync(w.bnd, lower, (size_t)D * 8, hipMemcpyHostToDevice, s));
  GPR_HIP(hipMemcpyAsync(w.bnd + D, upper, (size_t)D * 8, hipMemcpyHostToDevice, s));
  if (scale) GPR_HIP(hipMemcpyAsync(w.bnd + 2 * D, scale, (size_t)D * 8, hipMemcpyHostToDevice, s));
  if (w.trace_len > 0)  // records that no evaluation writes keep what the caller's buffer holds
    GPR_HIP(hipMemcpyAsync(w.trace_dev, trace, (size_t)w.trace_len * 8, hipMemcpyHostToDevice, s));
}
// hs clipped into the box, into Y
void refine_upload_clipped(gprhip_problem* p, const RefineWork& w, std::vector<double>& hs, const double* lower, const double* upper) {
  const int D = p->D;
  for (size_t i = 0; i < hs.size(); ++i) hs[i] = refine_clip(hs[i], lower[i % D], upper[i % D]);
  GPR_HIP(hipMemcpyAsync(w.Y, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, p->stream));
}
RefineOpts refine_opts(const gprhip_refine_options* opt) {
  RefineOpts o;
  o.max_evals = opt->max_evals; o.step0 = opt->step0; o.c1 = opt->c1; o.shrink = opt->shrink; o.grow = opt->grow;
  o.xtol = opt->xtol;
  return o;
}
// the state of the ns starts in the arena
RefineStepArgs refine_step_args(gprhip_problem* p, const RefineWork& w, bool scaled, const RefineOpts& o) {
  const int D = p->D;
  const int64_t ns = w.ns;
  RefineStepArgs st;
  st.ns = (int)ns; st.D = D; st.first = 1; st.lower = w.bnd; st.upper = w.bnd + D; st.scale = scaled ? w.bnd + 2 * D : nullptr;
  st.o = o;
  st.x = w.X; st.g = w.G; st.y = w.Y; st.gy = w.GY; st.ay = w.AY; st.a = w.A; st.alpha = w.AL;
  st.evals = w.ints; st.accepted = w.ints + ns; st.status = w.ints + 2 * ns; st.trace = w.trace_dev; st.active = p->rf_active;
  return st;
}
// a persistent kernel keeps the state in the caller's device buffers where there are some: nothing to copy afterwards
void refine_state_in_place(RefineStepArgs& st, double* x_out, double* values, double* dvalues, int* evals, int* accepted, int* status) {
  if (x_out) st.x = x_out;
  if (dvalues) st.g = dvalues;
  if (values) st.a = values;
  if (evals) st.evals = evals;
  if (accepted) st.accepted = accepted;
  if (status) st.status = status;
}
// The library-side loop: per evaluation the chunk walk over the trial points st.y (ns fits one chunk) -- eval(ev, pts, rows,
// rows_p) leaves the objective in st.ay and its gradient in st.gy --, then refine_step_kernel, which leaves the number of
// starts that go on in pinned memory: one integer per evaluation comes back.
template <typename F>
void refine_host_loop(gprhip_problem* p, const PgPlan& plan, RefineStepArgs& st, F&& eval) {
  for (int ev = 0; ev < st.o.max_evals; ++ev) {
    st.first = ev == 0;
    walk_chunks(p, plan.chunk, st.y, st.D, st.ns, 1, [&](int64_t, int rows, int rows_p, const double*, const double* pts) {
      eval(ev, pts, rows, rows_p);
      tstart(p, "rf_step");
      launch_refine_step(st, p->stream);
      tstop(p);
    });
    if (*static_cast<volatile int*>(p->rf_active) == 0) break;
  }
}
// from where the kernels left the state (st) to the caller's buffers, where those are others
void refine_copy_out(gprhip_problem* p, const RefineStepArgs& st, const RefineWork& w, double* x_out, int64_t ldx, double* values,
                     double* dvalues, int64_t ldg, int* evals, int* accepted, int* status, double* trace, int on_device) {
  hipStream_t s = p->stream;
  const size_t ns = (size_t)st.ns, row = (size_t)st.D * 8;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const double* const mats[2] = {st.x, st.g};
  double* const dst[2] = {x_out, dvalues};
  const int64_t lds[2] = {ldx, ldg};
  for (int j = 0; j < 2; ++j)
    if (dst[j] && dst[j] != mats[j]) GPR_HIP(hipMemcpy2DAsync(dst[j], (size_t)lds[j] * 8, mats[j], row, row, ns, kind, s));
  if (values && values != st.a) GPR_HIP(hipMemcpyAsync(values, st.a, ns * 8, kind, s));
  int* const idst[3] = {evals, accepted, status};
  const int* const isrc[3] = {st.evals, st.accepted, st.status};
  for (int j = 0; j < 3; ++j)
    if (idst[j] && idst[j] != isrc[j]) GPR_HIP(hipMemcpyAsync(idst[j], isrc[j], ns * sizeof(int), kind, s));
  if (w.trace_len > 0) GPR_HIP(hipMemcpyAsync(trace, w.trace_dev, (size_t)w.trace_len * 8, hipMemcpyDeviceToHost, s));
}

// gprhip_acquire_refine: projected gradient ascent with Armijo backtracking from ns starts (refine_step.h is the rule).
//   * at most 64 inducing points of at most 16 dimensions, no projection: one persistent kernel (refine.hip) -- the loop runs
//     on the device;
//   * every other shape: the loop runs here (refine_host_loop).  State and trial points stay in device buffers, an evaluation
//     is the chunk walk of gprhip_acquire on them.
// The criterion is acq or, where mv is not null (acq is then null), max-value entropy search over host_extremes
// (gprhip_acquire_max_value_refine): the latent variance, always needed; the extremes are uploaded as in acquire_walk.
// The caller has checked the arguments and the model state; hs: the starts on the host, [ns][D], finite.
void do_acquire_refine(gprhip_problem* p, const char* fn, const gprhip_acquisition* acq, MvArgs* mv, const double* host_extremes,
                       const gprhip_refine_options* opt, const double* lower, const double* upper, const double* scale,
                       const double* starts, std::vector<double>& hs, int64_t ns, double* x_out, int64_t ldx, double* values,
                       double* dvalues, int64_t ldg, int* evals, int* accepted, int* status, double* trace, int on_device) {
  const bool want_var = mv ? true : acq_wants_var(acq);
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int D = p->D;
  const bool small = one_kernel_path(p) && !p->has_proj();
  RefineWork w = refine_work_sizes(D, ns, 3, opt->max_evals, trace, on_device);
  const PgPlan plan = pg_prepare(p, fn, ns, want_var, false, true, p->rf_len < w.len ? w.len * 8 : 0);
  refine_work(p, w, lower, upper, scale, trace, on_device, true);
  RefineStepArgs st = refine_step_args(p, w, scale != nullptr, refine_opts(opt));
  AcqArgs q = mv ? AcqArgs{} : acq_args(acq);
  const double add = (!mv && acq->predictive) ? p->h.sigma2 : 0.0;
  if (mv) mv_upload(p, mv, host_extremes);
  if (small) {
    const bool direct = on_device != 0;  // the kernel reads and writes the caller's device buffers
    if (direct) refine_state_in_place(st, x_out, values, dvalues, evals, accepted, status);
    else GPR_HIP(hipMemcpyAsync(w.Y, hs.data(), (size_t)ns * D * 8, hipMemcpyHostToDevice, s));
    SmallPredictGradArgs a{};
    a.cp = p->cp; a.pts = direct ? starts : w.Y; a.Z = p->Z; a.shift = p->zshift; a.uinv = p->uinv; a.rinv = p->rinv;
    a.tvec = p->tvec; a.rows = (int)ns; a.m = p->m; a.mp = p->mp; a.d = p->d; a.want_var = want_var ? 1 : 0; a.add = add;
    SmallRefineArgs rf;  // (an output that is not wanted is not stored)
    rf.lower = st.lower; rf.upper = st.upper; rf.scale = st.scale; rf.o = st.o;
    rf.x_out = x_out ? st.x : nullptr; rf.values = values ? st.a : nullptr; rf.dvalues = dvalues ? st.g : nullptr;
    rf.evals = evals ? st.evals : nullptr; rf.accepted = accepted ? st.accepted : nullptr;
    rf.status = status ? st.status : nullptr; rf.trace = w.trace_dev;
    tstart(p, "rf_small");
    if (mv) launch_small_max_value_refine(a, *mv, rf, s);
    else launch_small_refine(a, q, rf, s);
    tstop(p);
  } else {
    refine_upload_clipped(p, w, hs, lower, upper);
    if (plan.mats) ensure_predict_m(p);
    q.values = w.AY;
    if (mv) mv->values = w.AY;
    refine_host_loop(p, plan, st, [&](int, const double* pts, int rows, int rows_p) {
      double* const dsts[2] = {w.GY, nullptr};
      pg_chunk(p, plan, pts, rows, rows_p, want_var, add, nullptr, nullptr, dsts, mv ? nullptr : &q, mv);
    });
  }
  refine_copy_out(p, st, w, x_out, ldx, values, dvalues, ldg, evals, accepted, status, trace, on_device);
  GPR_HIP(hipStreamSynchronize(s));
  if (p->timer.on) tcollect(p);
}

// The weights A = t 1^T + U^-1 (R~^-1 Z) of gprhip_sample_paths and gprhip_sample_paths_refine, formed once per call.
// path_weights_bytes: the device memory path_weights will allocate, for the count in front of pg_prepare.
int64_t path_weights_bytes(const gprhip_problem* p) { return p->sp_coef ? 0 : 2 * (int64_t)p->mp * SP_MAX_DRAWS * 8; }
// z: nd normal draws of m entries on the host (draw j at z + j ldz).  Returns A, [mp][SP_MAX_DRAWS] (the second half of sp_coef).
double* path_weights(gprhip_problem* p, const double* z, int64_t ldz, int nd) {
  const int m = p->m, mp = p->mp;
  // (the pinned buffer first: a failure leaves both pointers null.  The weight kernel reads it by its host address, as
  //  ship_kernel writes res_host: mapped, portable pinned memory has one address on host and device here)
  if (!p->sp_zhost)
    GPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->sp_zhost), (size_t)mp * SP_MAX_DRAWS * sizeof(double),
                          hipHostMallocPortable | hipHostMallocMapped));
  if (!p->sp_coef) p->sp_coef = p->alloc<double>(2 * (int64_t)mp * SP_MAX_DRAWS);
  // R~^-1 Z first, then U^-1 times it, plus t
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < nd; ++j) p->sp_zhost[(int64_t)i * SP_MAX_DRAWS + j] = z[(int64_t)j * ldz + i];
  double* const wA = p->sp_coef + (int64_t)mp * SP_MAX_DRAWS;
  tstart(p, "sp_coeff");
  p->sp_ns_last = 0;
  launch_sp_weights(p->rinv, p->uinv, p->sp_zhost, p->tvec, m, mp, nd, p->sp_coef, wA, p->stream);
  p->sp_ns_last = nd;
  tstop(p);
  return wA;
}

// gprhip_sample_paths: ns draws of the posterior as functions, evaluated at nt test points chunk by chunk
// (sample_paths.hip). The weights A = t 1^T + U^-1 (R~^-1 Z) are formed once per call; per chunk one kernel gives
// F = K A (draw-major; K never reaches memory), with eps the residual standard deviation sqrt(max(0, sf2 - |K_r U^-1|^2 (+
// sigma2))) eps is added in place, the best top_k of every draw are selected on the device (acquire.hip, one launch pair for
// all draws), the path gradient is evaluated at them, and the chunks' lists are merged here (sample_paths_host.h).
// The caller has checked the arguments.  The model state is read only: pg_m is neither needed nor touched.
void do_sample_paths(gprhip_problem* p, const double* z, int64_t ldz, int ns, const double* test_inputs, int64_t ld, int64_t nt,
                     const double* eps, int64_t lde, int predictive, double* samples, int64_t lds, int maximise, int top_k,
                     int64_t* top_index, double* top_values, double* top_dvalues, int on_device) {
  need_posterior_state(p, "gprhip_sample_paths", "draw from", true, true, true, "draws are available after the next gprhip_eval");
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int mp = p->mp, m = p->m, D = p->D, d = p->d;
  const bool resid = eps != nullptr;
  const bool stage_f = !(on_device && samples), stage_e = resid && !on_device;
  // this call's own buffers, as far as they must grow: counted from the plan's chunk before anything is allocated
  const int64_t rows_need =  // rows of a chunk of this call
      std::min<int64_t>(chunk_plan(p, nt, !one_kernel_path(p) && resid).chunk, round_up(nt, TILE));
  const int64_t piece_rows = (int64_t)ACQ_SELECT_MAX_SLABS * 2048;
  const int64_t out_stride = (int64_t)top_k * (D + 2);
  const int64_t scratch_need = top_k > 0 ? acq_select_many_scratch_bytes(std::min(rows_need, piece_rows), top_k, ns) : 0;
  int64_t extra = 0;
  extra += path_weights_bytes(p);
  if (stage_f && p->sp_f_rows < ns * rows_need) extra += ns * rows_need * 8;
  if (stage_e && p->sp_eps_rows < ns * rows_need) extra += ns * rows_need * 8;
  if (top_k > 0) {
    extra += std::max<int64_t>(0, scratch_need - p->sp_scratch_bytes);
    if (!p->sp_out) extra += (int64_t)SP_MAX_DRAWS * ACQ_MAX_TOP_K * (D + 2) * 8;
  }
  const PgPlan plan = pg_prepare(p, "gprhip_sample_paths", nt, resid, false, false, extra);
  double* const wA = path_weights(p, z, ldz, ns);
  if (stage_f) grow_buf(p, p->sp_f, p->sp_f_rows, ns * rows_need);
  if (stage_e) grow_buf(p, p->sp_eps, p->sp_eps_rows, ns * rows_need);
  if (top_k > 0) {
    grow_buf(p, p->sp_scratch, p->sp_scratch_bytes, scratch_need);
    if (!p->sp_out) {
      const int64_t len = (int64_t)SP_MAX_DRAWS * ACQ_MAX_TOP_K * (D + 2);
      p->sp_out = p->alloc<double>(len);
      GPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->sp_host), (size_t)len * sizeof(double), hipHostMallocDefault));
    }
  }
  const double add = predictive ? p->h.sigma2 : 0.0;
  const double sign = maximise ? 1.0 : -1.0;
  const bool want_g = top_k > 0 && top_dvalues;
  std::vector<SpBest> best(top_k > 0 ? ns : 0);
  walk_chunks(p, plan.chunk, test_inputs, ld, nt, on_device, [&](int64_t lo, int rows, int rows_p, const double*, const double* pts) {
    double* const Fd = stage_f ? p->sp_f : samples + lo;
    const int64_t ldf = stage_f ? rows_need : lds;
    tstart(p, "sp_path");
    SamplePathArgs a;
    a.pts = pts; a.Z = p->Z; a.shift = p->zshift; a.W = wA; a.ldw = SP_MAX_DRAWS; a.ns = ns;
    a.rows = rows; a.m = m; a.d = d; a.log_sf2 = p->cp.log_sf2; a.inv_ell2_05 = p->cp.inv_ell2_05;
    a.F = Fd; a.ldf = ldf; a.sumsq = nullptr;
    launch_sample_paths(a, s);
    tstop(p);
    if (resid) {
      const double* E = eps + lo;
      int64_t ldE = lde;
      if (!on_device) {
        GPR_HIP(hipMemcpy2DAsync(p->sp_eps, (size_t)rows_need * sizeof(double), eps + lo, (size_t)lde * sizeof(double),
                                 (size_t)rows * sizeof(double), (size_t)ns, hipMemcpyHostToDevice, s));
        E = p->sp_eps;
        ldE = rows_need;
      }
      tstart(p, "sp_resid");
      if (plan.small) {  // few inducing points: |K_r U^-1|^2 in one kernel, no chunk x mp matrix
        SamplePathArgs r = a;
        r.W = p->uinv; r.ldw = mp; r.ns = m; r.F = nullptr; r.sumsq = plan.rvar;
        launch_sp_row_sumsq(r, s);
      } else {
        launch_cov_cross<double>(p->cp, pts, rows, rows_p, p->Z, m, mp, d, plan.bufA, s);
        GemmArgs g;  // V = K U^-1
        g.A = plan.bufA; g.lda = mp; g.B = p->uinv; g.ldb = mp; g.C = plan.bufB; g.ldc = mp;
        g.M = rows_p; g.N = mp; g.K = mp; g.tri = TRI_KHI_BN;
        launch_gemm(OP_NN, g, s);
        launch_row_sumsq_dot<double>(plan.bufB, nullptr, rows, mp, plan.rvar, nullptr, s);
      }
      launch_sp_combine(Fd, ldf, E, ldE, plan.rvar, p->cp.sf2, add, rows, ns, s);
      tstop(p);
    }
    if (!on_device && samples)
      GPR_HIP(hipMemcpy2DAsync(samples + lo, (size_t)lds * sizeof(double), Fd, (size_t)ldf * sizeof(double),
                               (size_t)rows * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost, s));
    // the best top_k of every draw over the chunk, in pieces of at most 256 slabs, before its buffers are reused
    for (int64_t po = 0; top_k > 0 && po < rows; po += piece_rows) {
      const int pr = (int)std::min<int64_t>(piece_rows, rows - po);
      tstart(p, "sp_select");
      AcqSelectManyArgs sel;
      sel.values = Fd + po; sel.ldv = ldf; sel.rows = pr; sel.k = top_k; sel.ncols = ns; sel.sign = sign;
      sel.scratch = p->sp_scratch; sel.out = p->sp_out; sel.out_stride = out_stride;
      launch_acq_select_many(sel, s);
      if (want_g) {
        PathGradAtArgs g;
        g.pts = pts + po * d; g.Z = p->Z; g.shift = p->zshift; g.W = wA; g.tproj = p->has_proj() ? p->tproj : nullptr;
        g.rows = pr; g.m = m; g.d = d; g.D = D; g.k = top_k; g.ns = ns;
        g.log_sf2 = p->cp.log_sf2; g.inv_ell2_05 = p->cp.inv_ell2_05; g.out = p->sp_out; g.out_stride = out_stride;
        launch_path_grad_at(g, s);
      }
      tstop(p);
      GPR_HIP(hipMemcpyAsync(p->sp_host, p->sp_out, (size_t)(ns * out_stride) * sizeof(double), hipMemcpyDeviceToHost, s));
      GPR_HIP(hipStreamSynchronize(s));
      for (int j = 0; j < ns; ++j) {
        const double* const blk = p->sp_host + (int64_t)j * out_stride;
        sp_merge_topk(best[j], top_k, sign, blk, blk + top_k, want_g ? blk + 2 * top_k : nullptr, D, lo + po);
      }
    }
  });
  for (int j = 0; j < ns && top_k > 0; ++j) {
    const int64_t e = (int64_t)j * top_k;
    write_topk(best[j], top_k, D, top_index + e, top_values ? top_values + e : nullptr, top_dvalues ? top_dvalues + e * D : nullptr);
  }
  if (p->timer.on) tcollect(p);
}

// gprhip_sample_paths_refine: the rule of refine_step.h on drawn sample paths (path_refine.hip).  The weights A are formed
// once per call as gprhip_sample_paths forms them; start i climbs s f_{draw_of[i]}.
//   * no projection: one persistent kernel at every m -- an evaluation costs O(m d) per start, the loop runs on the device;
//   * with a projection: the loop runs here as route 2 of gprhip_acquire_refine does -- the trial points are projected, one
//     launch of the same evaluator, the back-projection of its gradient, refine_step_kernel, one integer back.
// The caller has checked the arguments and the model state; hs: the starts on the host, [ns][D], finite.  pg_m is neither
// needed nor formed.
void do_sample_paths_refine(gprhip_problem* p, const double* z, int64_t ldz, int nd, int maximise,
                            const gprhip_refine_options* opt, const double* lower, const double* upper, const double* scale,
                            std::vector<double>& hs, int64_t ns, const int* draw_of, double* x_out, int64_t ldx, double* values,
                            double* dvalues, int64_t ldg, int* evals, int* accepted, int* status, double* trace, int on_device) {
  const char* const fn = "gprhip_sample_paths_refine";
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int D = p->D, d = p->d;
  const bool proj = p->has_proj();
  RefineWork w = refine_work_sizes(D, ns, 4, opt->max_evals, trace, on_device);
  const PgPlan plan = pg_prepare(p, fn, ns, false, false, true, (p->rf_len < w.len ? w.len * 8 : 0) + path_weights_bytes(p));
  if (proj && plan.chunk < ns) {  // (a chunk holds every count of starts the call accepts)
    set_error(std::string(fn) + ": the starts do not fit one chunk of test points");
    throw HipFail{ST_BAD_ARG};
  }
  refine_work(p, w, lower, upper, scale, trace, on_device, proj);
  int* const draw_dev = w.ints + 3 * ns;
  GPR_HIP(hipMemcpyAsync(draw_dev, draw_of, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, s));
  refine_upload_clipped(p, w, hs, lower, upper);
  const double* const wA = path_weights(p, z, ldz, nd);
  RefineStepArgs st = refine_step_args(p, w, scale != nullptr, refine_opts(opt));
  if (!proj && on_device) refine_state_in_place(st, x_out, values, dvalues, evals, accepted, status);
  PathEvalArgs e;
  e.pts = w.Y; e.Z = p->Z; e.shift = p->zshift; e.W = wA; e.draw_of = draw_dev; e.status = st.status;
  e.rows = (int)ns; e.m = p->m; e.d = d; e.nd = nd; e.log_sf2 = p->cp.log_sf2; e.inv_ell2_05 = p->cp.inv_ell2_05;
  e.sign = maximise ? 1.0 : -1.0; e.val = w.AY; e.grad = w.GY; e.ldg = D;
  if (!proj) {
    tstart(p, "prf_kernel");
    launch_path_refine(e, st, s);
    tstop(p);
  } else {
    e.grad = plan.stage_p[0]; e.ldg = d;
    refine_host_loop(p, plan, st, [&](int ev, const double* pts, int rows, int) {
      tstart(p, "prf_eval");
      e.pts = pts; e.status = ev == 0 ? nullptr : st.status;
      launch_path_eval(e, s);
      launch_input_grad_project(e.grad, rows, d, D, p->tproj, w.GY, D, s);
      tstop(p);
    });
  }
  refine_copy_out(p, st, w, x_out, ldx, values, dvalues, ldg, evals, accepted, status, trace, on_device);
  GPR_HIP(hipStreamSynchronize(s));
  if (p->timer.on) tcollect(p);
}

// Temporary device memory of one posterior call (sizes depend on the number of test points).
struct DevBuf {
  std::vector<void*> ptrs;
  template <typename T>
  T* get(int64_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (size_t)std::max<int64_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      set_error("gprhip: device allocation failed (posterior buffers)");
      throw HipFail{ST_OOM};
    }
    ptrs.push_back(q);
    return static_cast<T*>(q);
  }
  ~DevBuf() {
    for (void* q : ptrs) (void)hipFree(q);
  }
};

// 2-norm condition estimate of A = K_m + jitter = U^T U of the current model state by power iteration on A (x <- U^T U x)
// and on A^-1 = U^-1 U^-T -- both factors are on the device, a step is two triangular matrix-vector products.  Power
// iteration approaches an extreme eigenvalue from inside the spectrum, so the estimate is a lower bound of the true
// condition number (within a small factor after 16 steps for the spectra a covariance matrix has).  Cached per evaluation.
// `enough`: a caller that only needs to know whether the estimate exceeds a threshold (the fp32-bulk guard) passes it -- the
// pivot cross-check below is itself a lower bound and comes from one small transfer, so an ill-conditioned factor is
// recognised without a single iteration step.
double condition_km(gprhip_problem* p, double enough = HUGE_VAL) {
  if (p->cond_km >= 0.0) return p->cond_km;
  if (!p->have_factors) {
    set_error("gprhip_condition: no factor of K_m on the device (evaluate, or load a predictor with co-variance coefficients)");
    throw HipFail{ST_STATE};
  }
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int mp = p->mp, m = p->m;
  DevBuf tmp;
  double* x0 = tmp.get<double>(3 * (int64_t)mp);
  double* const xv[2] = {x0, x0 + mp};
  double* y = x0 + 2 * (int64_t)mp;
  // Cross-check from the factor itself, first: every squared pivot U_ii^2 lies inside the spectrum of A (it is the
  // reciprocal of a diagonal entry of the inverse of a leading block, whose eigenvalues interlace A's), so
  // max U_ii^2 / min U_ii^2 is a lower bound of cond(A); the larger of the two estimates is reported.
  double pivot_ratio = 0.0;
  {
    hipLaunchKernelGGL(copy_diag_kernel, dim3((mp + 255) / 256), dim3(256), 0, s, p->umat, mp, y);
    std::vector<double> dg(mp);
    GPR_HIP(hipMemcpyAsync(dg.data(), y, (size_t)mp * sizeof(double), hipMemcpyDeviceToHost, s));
    GPR_HIP(hipStreamSynchronize(s));
    double dmax = 0.0, dmin = HUGE_VAL;
    for (int i = 0; i < m; ++i) {
      dmax = std::max(dmax, dg[i] * dg[i]);
      dmin = std::min(dmin, dg[i] * dg[i]);
    }
    if (dmin > 0.0) pivot_ratio = dmax / dmin;
    if (pivot_ratio >= enough) return pivot_ratio;  // (not cached: a later gprhip_condition wants the full estimate)
  }
  std::vector<double> h0(mp, 0.0);
  for (int i = 0; i < m; ++i) h0[i] = 1.0 + 0.5 * std::sin(1.0 + 0.37 * i);  // the padding (a decoupled identity block) stays 0
  // Rounds of 16 steps until both Rayleigh quotients have settled (relative change < 1e-2 over a round; at most 16 rounds:
  // lambda_max(A^-1) converges slowly when K_m + jitter has a cluster of small eigenvalues, and a fixed 16 steps could pass
  // exactly the coefficients the fp32 guard exists to refuse).  The two iterations advance side by side: one transfer and
  // one host synchronisation per round for both.
  double lam[2] = {0.0, 0.0}, prev[2] = {0.0, 0.0};
  bool settled[2] = {false, false};
  for (int which = 0; which < 2; ++which) {
    GPR_HIP(hipMemcpyAsync(xv[which], h0.data(), (size_t)mp * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(normalize_kernel, dim3(1), dim3(256), 0, s, xv[which], mp, p->scal + SC_LMAX + which);
  }
  for (int round = 0; round < 16 && !(settled[0] && settled[1]); ++round) {
    for (int which = 0; which < 2; ++which) {
      if (settled[which]) continue;
      const double* F = which == 0 ? p->umat : p->uinv;
      double* x = xv[which];
      for (int it = 0; it < 16; ++it) {
        if (which == 0) {  // x <- U^T (U x)
          launch_triu_matvec(F, mp, x, y, 0, s);
          launch_triu_matvec(F, mp, y, x, 1, s);
        } else {           // x <- U^-1 (U^-T x)
          launch_triu_matvec(F, mp, x, y, 1, s);
          launch_triu_matvec(F, mp, y, x, 0, s);
        }
        hipLaunchKernelGGL(normalize_kernel, dim3(1), dim3(256), 0, s, x, mp, p->scal + SC_LMAX + which);
      }
    }
    GPR_HIP(hipMemcpyAsync(lam, p->scal + SC_LMAX, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    GPR_HIP(hipStreamSynchronize(s));
    for (int which = 0; which < 2; ++which) {
      if (settled[which]) continue;
      if (round > 0 && std::fabs(lam[which] - prev[which]) <= 1e-2 * std::fabs(lam[which])) settled[which] = true;
      prev[which] = lam[which];
    }
  }
  p->cond_km = std::max(pivot_ratio, lam[0] * lam[1]);
  return p->cond_km;
}

// fp32-bulk problems: the mean coefficients t = U^-1 t~ inherit cond(K_m + jitter) times the fp32 unit roundoff of the
// n x m operands (measured: profiles/r03_f32_sweep.txt -- useless from cond ~ 1e6 on); their consumers refuse them then.
void need_trustworthy_coeffs(gprhip_problem* p, const char* who) {
  if (!p->f32 || p->f32_coeff_tol <= 0.0 || !p->have_factors) return;
  // (an estimate beyond twice the threshold settles the question: the pivot ratio alone may then answer, without iterating)
  const double cond = condition_km(p, 2.0 * p->f32_coeff_tol / 5.9604644775390625e-8);
  const double bound = cond * 5.9604644775390625e-8;
  if (bound > p->f32_coeff_tol) {
    char buf[320];
    snprintf(buf, sizeof buf,
             "%s: the mean coefficients of this fp32-bulk evaluation are not trustworthy: cond(K_m + jitter) ~ %.3g, "
             "error bound %.3g > %.3g (GPRHIP_F32_COEFF_TOL); evaluate with GPRHIP_F64 for coefficients / predictions "
             "(log evidence and gradient are unaffected)", who, cond, bound, p->f32_coeff_tol);
    set_error(buf);
    throw HipFail{GPRHIP_EPRECISION};
  }
}

void need_factors(gprhip_problem* p, const char* who) {
  if (!p->have_factors) {
    set_error(std::string(who) + ": the loaded predictor has no co-variance coefficients (chol_km, r_mat)");
    throw HipFail{ST_STATE};
  }
}

void need_model(gprhip_problem* p, const char* who) {
  if (!p->have_model || p->stage != 0) {
    set_error(std::string(who) + ": no completed evaluation to work from");
    throw HipFail{ST_STATE};
  }
}

// Trained.calc_means (lib/fitc_gp.ml:296-297) over the resident training inputs, and the residual sums
// Stats.calc needs (lib/fitc_gp.ml:353-373): sums = { sse, sum |y-mean|, max |y-mean|, sum y^2 }.
template <typename TS>
void do_train_stats(gprhip_problem* p, double* means, double* sums) {
  need_model(p, "gprhip_train_stats");
  if (p->multi_state) {
    set_error("gprhip_train_stats: the last evaluation was gprhip_eval_targets (several target vectors); the statistics are "
              "those of one target vector and need a gprhip_eval");
    throw HipFail{ST_STATE};
  }
  if (!p->have_targets || p->h.model_only) {
    set_error("gprhip_train_stats: the last evaluation had no targets");
    throw HipFail{ST_STATE};
  }
  need_trustworthy_coeffs(p, "gprhip_train_stats");
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  DevBuf tmp;
  double* rmean = tmp.get<double>(p->chunk);
  int64_t nblocks = 0;
  for (int c = 0; c < p->nchunks; ++c) nblocks += residual_stat_blocks((int)p->rows_of(c));
  double* part = tmp.get<double>(nblocks * 4);
  TS* const K = static_cast<TS*>(p->bufA);
  int64_t b0 = 0;
  for (int c = 0; c < p->nchunks; ++c) {
    const int rows = (int)p->rows_of(c);
    const int64_t lo = (int64_t)c * p->chunk;
    cov_chunk<TS>(p, c, K);
    launch_row_sumsq_dot<TS>(K, p->tvec, rows, p->mp, nullptr, rmean, s);
    launch_residual_stats(p->y + lo, rmean, rows, part + b0 * 4, s);
    b0 += residual_stat_blocks(rows);
    if (means)
      GPR_HIP(hipMemcpyAsync(means + lo, rmean, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  std::vector<double> hp((size_t)nblocks * 4);
  GPR_HIP(hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  GPR_HIP(hipStreamSynchronize(s));
  double sse = 0.0, sad = 0.0, mad = 0.0, sy2 = 0.0;
  for (int64_t b = 0; b < nblocks; ++b) {
    sse += hp[b * 4 + 0];
    sad += hp[b * 4 + 1];
    mad = std::max(mad, hp[b * 4 + 2]);
    sy2 += hp[b * 4 + 3];
  }
  sums[0] = sse; sums[1] = sad; sums[2] = mad; sums[3] = sy2;
}

// FITC_covariances.calc / FIC_covariances.calc (lib/fitc_gp.ml:585-599, :617-627) at nt test points, fp64:
//   V_t = K_tm U^-1, Q_t = K_tm R^-1 = V_t R~^-1
//   FITC: K_tt - V_t V_t^T + Q_t Q_t^T          FIC: Q_t Q_t^T + diag(k_tt - rowsum(K_tm.^2))
// (the FIC diagonal is what the reference computes at :620 -- from K_tm itself, not from V_t).
void do_covariances(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int kind,
                    int predictive, double* cov) {
  need_model(p, "gprhip_covariances");
  need_factors(p, "gprhip_covariances");
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int mp = p->mp;
  const int np = (int)round_up(nt, TILE);
  DevBuf tmp;
  double* xt = tmp.get<double>(nt * p->D);
  double* Kt = tmp.get<double>((int64_t)np * mp);
  double* Vt = tmp.get<double>((int64_t)np * mp);
  double* C = tmp.get<double>((int64_t)np * np);
  double* rv = tmp.get<double>(2 * (int64_t)np);
  GPR_HIP(hipMemcpy2DAsync(xt, (size_t)p->D * sizeof(double), test_inputs, (size_t)ld * sizeof(double),
                           (size_t)p->D * sizeof(double), (size_t)nt, hipMemcpyHostToDevice, s));
  const double* pts = xt;
  if (p->has_proj()) {
    double* pt = tmp.get<double>(nt * p->d);
    launch_project(xt, nt, p->D, p->d, p->tproj, pt, s);
    pts = pt;
  }
  launch_cov_cross<double>(p->cp, pts, (int)nt, np, p->Z, p->m, mp, p->d, Kt, s);
  GemmArgs g;  // trsm ~side:`R chol_km
  g.A = Kt; g.lda = mp; g.B = p->uinv; g.ldb = mp; g.C = Vt; g.ldc = mp;
  g.M = np; g.N = mp; g.K = mp; g.tri = TRI_KHI_BN;
  launch_gemm(OP_NN, g, s);
  if (kind == 0) {
    // Inputs.calc_upper: the plain kernel between the (projected) test points, no multiscales
    // (lib/cov_se_iso.ml:124, lib/cov_se_fat.ml:221 -> calc_upper_vanilla :85-100)
    CovParams plain = p->cp;
    plain.ms = nullptr;
    launch_cov_cross<double>(plain, pts, (int)nt, np, pts, (int)nt, np, p->d, C, s);
    GemmArgs a;  // syrk ~alpha:-1 tmp ~c:covariances
    a.A = Vt; a.lda = mp; a.B = Vt; a.ldb = mp; a.C = C; a.ldc = np;
    a.M = np; a.N = np; a.K = mp; a.alpha = -1.0; a.beta = 1.0;
    launch_gemm(OP_NT, a, s);
  } else {
    launch_row_sumsq_dot<double>(Kt, nullptr, (int)nt, mp, rv, nullptr, s);
    launch_const_minus(rv, (int)nt, p->cp.sf2, rv + np, s);
  }
  GemmArgs q;  // trsm ~side:`R r_mat  (R = R~ U)
  q.A = Vt; q.lda = mp; q.B = p->rinv; q.ldb = mp; q.C = Kt; q.ldc = mp;
  q.M = np; q.N = mp; q.K = mp; q.tri = TRI_KHI_BN;
  launch_gemm(OP_NN, q, s);
  GemmArgs b;  // syrk tmp ~c:covariances
  b.A = Kt; b.lda = mp; b.B = Kt; b.ldb = mp; b.C = C; b.ldc = np;
  b.M = np; b.N = np; b.K = mp; b.alpha = 1.0; b.beta = kind == 0 ? 1.0 : 0.0;
  launch_gemm(OP_NT, b, s);
  const double add = predictive ? p->h.sigma2 : 0.0;  // get ?predictive, :549-559
  if (kind != 0 || add != 0.0) launch_add_diag(C, np, (int)nt, kind != 0 ? rv + np : nullptr, add, s);
  // symmetric: row-major == column-major
  GPR_HIP(hipMemcpy2DAsync(cov, (size_t)nt * sizeof(double), C, (size_t)np * sizeof(double),
                           (size_t)nt * sizeof(double), (size_t)nt, hipMemcpyDeviceToHost, s));
  GPR_HIP(hipStreamSynchronize(s));
}

// Common_cov_sampler.calc + samples (lib/fitc_gp.ml:656-697): cov_chol = chol(cov + add_diag I + jitter I)
// (upper), samples[:, j] = means + cov_chol^T z[:, j].  z is supplied by the caller (the reference draws
// it from GSL's ziggurat generator).
void do_cov_samples(gprhip_problem* p, const double* cov, int64_t ld, int64_t nt, double add_diag,
                    double jitter, const double* means, const double* z, int64_t ns, double* samples) {
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int np = (int)round_up(nt, TILE);
  const int nsp = (int)round_up(ns, TILE);
  DevBuf tmp;
  double* raw = tmp.get<double>(nt * nt);
  double* A = tmp.get<double>((int64_t)np * np);
  double* dinv = tmp.get<double>((int64_t)np * TILE);
  double* Zd = tmp.get<double>((int64_t)nsp * np);
  double* S = tmp.get<double>((int64_t)nsp * np);
  double* mu = tmp.get<double>(nt);
  int* info = tmp.get<int>(1);
  GPR_HIP(hipMemcpy2DAsync(raw, (size_t)nt * sizeof(double), cov, (size_t)ld * sizeof(double),
                           (size_t)nt * sizeof(double), (size_t)nt, hipMemcpyHostToDevice, s));
  GPR_HIP(hipMemsetAsync(info, 0, sizeof(int), s));
  launch_sym_from_upper(raw, nt, (int)nt, A, np, add_diag + jitter, s);
  potrf_upper_n(s, A, np, dinv, info, p->engine_steps, (int)nt);
  int hinfo = 0;
  GPR_HIP(hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, s));
  // z: Fortran nt x ns == row-major [ns][nt]
  GPR_HIP(hipMemsetAsync(Zd, 0, (size_t)nsp * np * sizeof(double), s));
  GPR_HIP(hipMemcpy2DAsync(Zd, (size_t)np * sizeof(double), z, (size_t)nt * sizeof(double),
                           (size_t)nt * sizeof(double), (size_t)ns, hipMemcpyHostToDevice, s));
  GPR_HIP(hipMemcpyAsync(mu, means, (size_t)nt * sizeof(double), hipMemcpyHostToDevice, s));
  GemmArgs g;  // trmm ~transa:`T cov_chol samples  ==  (z^T U)^T
  g.A = Zd; g.lda = np; g.B = A; g.ldb = np; g.C = S; g.ldc = np;
  g.M = nsp; g.N = np; g.K = np; g.tri = TRI_KHI_BN;
  launch_gemm(OP_NN, g, s);
  launch_add_row_vector(S, np, (int)ns, (int)nt, mu, s);
  GPR_HIP(hipMemcpy2DAsync(samples, (size_t)nt * sizeof(double), S, (size_t)np * sizeof(double),
                           (size_t)nt * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost, s));
  GPR_HIP(hipStreamSynchronize(s));
  if (hinfo != 0) {
    set_error("Cov_sampler.calc: potrf: leading minor of order " + std::to_string(hinfo) +
              " is not positive definite");
    throw HipFail{ST_NOT_POSDEF};
  }
}

// Row-major padded upper factor -> Fortran m x m (upper triangle, zeros below) on the host.
void fetch_upper_fortran(gprhip_problem* p, const double* dev, double* out) {
  const int mp = p->mp, m = p->m;
  std::vector<double> h((size_t)mp * mp);
  GPR_HIP(hipMemcpyAsync(h.data(), dev, h.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  GPR_HIP(hipStreamSynchronize(p->stream));
  for (int c = 0; c < m; ++c)
    for (int r = 0; r < m; ++r) out[(size_t)c * m + r] = (r <= c) ? h[(size_t)r * mp + c] : 0.0;
}

// Fortran m x m upper factor on the host -> row-major padded mp x mp on the device (zeros below, identity padding).
void upload_upper_fortran(gprhip_problem* p, const double* in, double* dev) {
  const int mp = p->mp, m = p->m;
  std::vector<double> h((size_t)mp * mp, 0.0);
  for (int r = 0; r < mp; ++r)
    for (int c = r; c < mp; ++c)
      h[(size_t)r * mp + c] = (c < m) ? in[(size_t)c * m + r] : (r == c ? 1.0 : 0.0);
  GPR_HIP(hipMemcpyAsync(dev, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
  GPR_HIP(hipStreamSynchronize(p->stream));  // h goes out of scope
}

// Model.calc_co_variance_coeffs (lib/fitc_gp.ml:240): (chol_km, r_mat) = (U, R~ U) of the last evaluation.
void do_co_variance_coeffs(gprhip_problem* p, double* chol_km, double* r_mat) {
  need_model(p, "gprhip_co_variance_coeffs");
  need_factors(p, "gprhip_co_variance_coeffs");
  GPR_HIP(hipSetDevice(p->device));
  const int mp = p->mp;
  if (chol_km) fetch_upper_fortran(p, p->umat, chol_km);
  if (r_mat) {
    GemmArgs g;  // R = R~ U, both upper triangular
    g.A = p->bmat; g.lda = mp; g.B = p->umat; g.ldb = mp; g.C = p->wmat; g.ldc = mp;
    g.M = mp; g.N = mp; g.K = mp; g.tri = TRI_BAND; g.upper_only = 1;
    launch_gemm(OP_NN, g, p->stream);
    fetch_upper_fortran(p, p->wmat, r_mat);
  }
}

// inv of an upper factor that is already on the device: per-block inverses, then the recursive-doubling joins
void trtri_of_factor(gprhip_problem* p, double* U, double* X) {
  for (int j = 0; j < p->mp / TILE; ++j)
    launch_potrf_diag_flags(U, p->mp, j, p->dinv + (int64_t)j * TILE * TILE, p->info, 1, p->stream, p->m);
  trtri_upper(p, U, X, p->wmat);
}

// Mean_predictor.calc + Co_variance_predictor.calc (lib/fitc_gp.ml:386-391, :446-447): install the predictor
// state of a saved model -- kernel, inducing points, mean coefficients, (chol_km, r_mat) -- without an evaluation.
void do_load_predictor(gprhip_problem* p, const gprhip_hypers* h, const double* coeffs, const double* chol_km,
                       const double* r_mat) {
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int mp = p->mp, m = p->m;
  const int64_t mm = (int64_t)mp * mp;
  p->have_model = p->have_factors = p->have_v = p->have_k = false;
  p->multi_state = false;
  p->cond_km = -1.0;
  p->pg_m_valid = false;
  p->sp_ns_last = 0;
  forget_observations(p);
  upload_hypers(p, h);
  std::vector<double> t(mp, 0.0);
  if (coeffs) std::memcpy(t.data(), coeffs, (size_t)m * sizeof(double));
  GPR_HIP(hipMemcpyAsync(p->tvec, t.data(), (size_t)mp * sizeof(double), hipMemcpyHostToDevice, s));
  GPR_HIP(hipMemsetAsync(p->info, 0, 2 * sizeof(int), s));
  p->have_factors = chol_km != nullptr;
  if (chol_km) {
    upload_upper_fortran(p, chol_km, p->umat);
    trtri_of_factor(p, p->umat, p->uinv);
    upload_upper_fortran(p, r_mat, p->binv);       // R, scratch
    trtri_of_factor(p, p->binv, p->wtil);          // R^-1
    GemmArgs g;  // R~^-1 = U R^-1  (R = R~ U)
    g.A = p->umat; g.lda = mp; g.B = p->wtil; g.ldb = mp; g.C = p->rinv; g.ldc = mp;
    g.M = mp; g.N = mp; g.K = mp; g.tri = TRI_BAND; g.upper_only = 1;
    GPR_HIP(hipMemsetAsync(p->rinv, 0, (size_t)mm * sizeof(double), s));
    launch_gemm(OP_NN, g, s);
    GemmArgs b;  // R~ = R U^-1, kept for a later export
    b.A = p->binv; b.lda = mp; b.B = p->uinv; b.ldb = mp; b.C = p->bmat; b.ldc = mp;
    b.M = mp; b.N = mp; b.K = mp; b.tri = TRI_BAND; b.upper_only = 1;
    GPR_HIP(hipMemsetAsync(p->bmat, 0, (size_t)mm * sizeof(double), s));
    launch_gemm(OP_NN, b, s);
    if (p->f32) {
      launch_to_float(p->uinv, p->uinv_f, mm, s);
      launch_to_float(p->rinv, p->rinv_f, mm, s);
    }
  }
  GPR_HIP(hipStreamSynchronize(s));
  p->stage = 0;
  p->have_model = true;
  p->h.model_only = coeffs ? 0 : 1;
}

// ---- gprhip_observe / gprhip_posterior_save / gprhip_posterior_restore
// A training point enters the FITC posterior through its row v = K_xm U^-1 of V, s = sf2 - |v|^2 + sigma2 and y alone
// (lib/fitc_gp.ml:151-182): with w = v / sqrt(s), eta = y / sqrt(s), B~' = B~ + sum w w^T and c~' = c~ + sum w eta, so
// [R~' | b'] is the triangular factor of [R~ | b] stacked on [W | eta].
void need_observe_state(gprhip_problem* p, const char* fn) {
  need_posterior_state(p, fn, "work from", true, true, false, "");
  if (p->multi_state) {
    set_error(std::string(fn) + ": the last evaluation was gprhip_eval_targets (several target vectors); the single-target "
              "state it needs comes from gprhip_eval");
    throw HipFail{ST_STATE};
  }
}

// b = R~ (U t) of a predictor that was loaded (an evaluation leaves b itself, which is never re-made from t: the product
// cancels when K_m is ill-conditioned)
void ensure_b(gprhip_problem* p, double* tmp) {
  if (p->have_b || p->h.model_only) return;
  launch_triu_matvec(p->umat, p->mp, p->tvec, tmp, 0, p->stream);
  launch_triu_matvec(p->bmat, p->mp, tmp, p->bvec, 0, p->stream);
  p->have_b = true;
}

void do_observe(gprhip_problem* p, const double* inputs, int64_t ld, const double* targets, int k, double* dlog_evidence,
                int on_device) {
  const char* const fn = "gprhip_observe";
  const int D = p->D, m = p->m, mp = p->mp;
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  // finite inputs and targets (device buffers are read back once)
  {
    std::vector<double> hx, hy;
    const double* x = inputs;
    const double* y = targets;
    int64_t ldx = ld;
    if (on_device) {
      hx.resize((size_t)k * D);
      GPR_HIP(hipMemcpyAsync(hx.data(), inputs, hx.size() * 8, hipMemcpyDeviceToHost, s));
      if (targets) {
        hy.resize(k);
        GPR_HIP(hipMemcpyAsync(hy.data(), targets, (size_t)k * 8, hipMemcpyDeviceToHost, s));
        y = hy.data();
      }
      GPR_HIP(hipStreamSynchronize(s));
      x = hx.data();
      ldx = D;
    }
    bool finite = true;
    for (int i = 0; i < k; ++i) {
      for (int b = 0; b < D; ++b) finite = finite && std::isfinite(x[i * ldx + b]);
      if (y) finite = finite && std::isfinite(y[i]);
    }
    if (!finite) {
      set_error(std::string(fn) + ": a non-finite input or target");
      throw HipFail{ST_BAD_ARG};
    }
  }
  // buffers first: a refusal for memory leaves everything as it was
  const int64_t need = (int64_t)OBS_MAX_ROWS * mp + 4 * OBS_MAX_ROWS + (int64_t)TILE * 64 + 2 * TILE + 2 * (int64_t)mp + 2;
  if (p->obs_len < need) {
    GPR_HIP(hipStreamSynchronize(s));
    size_t free_b = 0, total_b = 0;
    GPR_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((uint64_t)need * 8 > (uint64_t)free_b) {
      set_error(std::string(fn) + ": not enough free device memory for the update's scratch");
      throw HipFail{ST_OOM};
    }
    grow_buf(p, p->obs_buf, p->obs_len, need);
  }
  double* const W = p->obs_buf;
  double* const eta = W + (int64_t)OBS_MAX_ROWS * mp;
  double* const rs = eta + OBS_MAX_ROWS;
  double* const ydev = rs + 2 * OBS_MAX_ROWS;
  double* const ubuf = ydev + OBS_MAX_ROWS;
  double* const vb = ubuf + (int64_t)TILE * 64;
  double* const ldr = vb + 2 * TILE;
  double* const tmpv = ldr + mp;
  double* const out = tmpv + mp;
  const ChunkPlan plan = chunk_plan(p, k, true);
  chunk_alloc(p, plan);
  double* const bufA = static_cast<double*>(plan.chunk > p->chunk ? p->predA : p->bufA);
  double* const bufB = static_cast<double*>(plan.chunk > p->chunk ? p->predB : p->bufB);
  // rows: the k points as one padded tile through the launches gprhip_predict uses for its variance, then W, eta, r and s
  walk_chunks(p, plan.chunk, inputs, ld, k, on_device, [&](int64_t, int rows, int rows_p, const double*, const double* pts) {
    tstart(p, "obs_rows");
    launch_cov_cross<double>(p->cp, pts, rows, rows_p, p->Z, m, mp, p->d, bufA, s);
    GemmArgs g;  // trsm ~side:`R chol_km
    g.A = bufA; g.lda = mp; g.B = p->uinv; g.ldb = mp; g.C = bufB; g.ldc = mp;
    g.M = rows_p; g.N = mp; g.K = mp; g.tri = TRI_KHI_BN;
    launch_gemm(OP_NN, g, s);
    launch_row_sumsq_dot<double>(bufB, nullptr, rows, mp, p->prow, nullptr, s);
    if (targets)
      GPR_HIP(hipMemcpyAsync(ydev, targets, (size_t)k * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    ObsRowsArgs a;
    a.V = bufB; a.sumsq = p->prow; a.y = targets ? ydev : nullptr; a.k = k; a.m = m; a.mp = mp;
    a.sf2 = p->cp.sf2; a.sigma2 = p->h.sigma2; a.W = W; a.eta = eta; a.rs = rs;
    launch_obs_rows(a, s);
    tstop(p);
  });
  // s comes back before anything of the state is written
  double hrs[2 * OBS_MAX_ROWS];
  GPR_HIP(hipMemcpyAsync(hrs, rs, sizeof hrs, hipMemcpyDeviceToHost, s));
  GPR_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < k; ++i)
    if (!(hrs[OBS_MAX_ROWS + i] > 0.0)) {
      char buf[200];
      snprintf(buf, sizeof buf, "%s: s = sf2 - |K_xm U^-1|^2 + sigma2 = %.3g of new point %d is not positive", fn,
               hrs[OBS_MAX_ROWS + i], i + 1);
      set_error(buf);
      throw HipFail{ST_NOT_POSDEF};
    }
  ensure_b(p, tmpv);
  tstart(p, "obs_update");
  ObsUpdateArgs u;
  u.R = p->bmat; u.m = m; u.mp = mp; u.k = k; u.W = W; u.b = targets ? p->bvec : nullptr; u.eta = eta;
  u.u = ubuf; u.vb = vb; u.ldr = ldr; u.out = out;
  launch_obs_update(u, s);
  tstop(p);
  tstart(p, "obs_inverse");
  trtri_of_factor(p, p->bmat, p->rinv);
  tstop(p);
  tstart(p, "obs_vectors");
  if (targets) {
    launch_triu_matvec(p->rinv, mp, p->bvec, p->ttil, 0, s);  // t~' = R~'^-1 b'
    launch_triu_matvec(p->uinv, mp, p->ttil, p->tvec, 0, s);  // t' = U^-1 t~'
  }
  tstop(p);
  double hout[2];
  GPR_HIP(hipMemcpyAsync(hout, out, sizeof hout, hipMemcpyDeviceToHost, s));
  GPR_HIP(hipStreamSynchronize(s));
  p->pg_m_valid = false;
  p->sp_ns_last = 0;
  p->n_observed += k;
  if (p->timer.on) tcollect(p);
  if (dlog_evidence) {
    double sum_log_s = 0.0, sum_isr = 0.0;
    for (int i = 0; i < k; ++i) {
      sum_log_s += std::log(hrs[OBS_MAX_ROWS + i]);
      sum_isr += hrs[i] / hrs[OBS_MAX_ROWS + i];
    }
    double dl = -0.5 * (2.0 * hout[0] + sum_log_s + (double)k * LOG_2PI);
    if (p->h.variational) dl += -0.5 * sum_isr;
    if (targets) dl += -0.5 * hout[1];
    *dlog_evidence = dl;
  }
}

void do_posterior_save(gprhip_problem* p) {
  need_observe_state(p, "gprhip_posterior_save");
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int64_t mp = p->mp, mm = mp * mp, len = 2 * mm + 3 * mp;
  if (!p->post_slot) {
    GPR_HIP(hipStreamSynchronize(s));
    size_t free_b = 0, total_b = 0;
    GPR_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((uint64_t)len * 8 > (uint64_t)free_b) {
      char buf[200];
      snprintf(buf, sizeof buf, "gprhip_posterior_save: the slot needs %.3f GB on device %d and %.3f GB are free", len * 8 / 1e9,
               p->device, free_b / 1e9);
      set_error(buf);
      throw HipFail{ST_OOM};
    }
    p->post_slot = p->alloc<double>(len);
  }
  double* q = p->post_slot;
  const double* const src[5] = {p->bmat, p->rinv, p->bvec, p->ttil, p->tvec};
  for (int i = 0; i < 5; ++i) {
    const int64_t cnt = i < 2 ? mm : mp;
    GPR_HIP(hipMemcpyAsync(q, src[i], (size_t)cnt * 8, hipMemcpyDeviceToDevice, s));
    q += cnt;
  }
  GPR_HIP(hipStreamSynchronize(s));
  p->slot_observed = p->n_observed;
  p->slot_have_b = p->have_b;
}

void do_posterior_restore(gprhip_problem* p) {
  need_observe_state(p, "gprhip_posterior_restore");
  if (!p->post_slot) {
    set_error("gprhip_posterior_restore: no posterior of this model state has been saved (gprhip_posterior_save; an evaluation "
              "and gprhip_load_predictor drop the slot)");
    throw HipFail{ST_STATE};
  }
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int64_t mp = p->mp, mm = mp * mp;
  const double* q = p->post_slot;
  double* const dst[5] = {p->bmat, p->rinv, p->bvec, p->ttil, p->tvec};
  for (int i = 0; i < 5; ++i) {
    const int64_t cnt = i < 2 ? mm : mp;
    GPR_HIP(hipMemcpyAsync(dst[i], q, (size_t)cnt * 8, hipMemcpyDeviceToDevice, s));
    q += cnt;
  }
  GPR_HIP(hipStreamSynchronize(s));
  p->n_observed = p->slot_observed;
  p->have_b = p->slot_have_b;
  p->pg_m_valid = false;
  p->sp_ns_last = 0;
}

// gprhip_set_targets_many: the n x k device buffers (and the m x k ones) are made here, not inside an evaluation
void do_set_targets_many(gprhip_problem* p, const double* targets, int64_t ld, int k) {
  GPR_HIP(hipSetDevice(p->device));
  const int mp = p->mp;
  const int64_t npad = p->npad();
  if (p->tg_k != k) {
    const int64_t n_small = 2 * TG_LD + 4 * (int64_t)mp * TG_LD;
    const int64_t n_part = (int64_t)std::max(targets_vty_blocks(p->n), targets_vty_blocks(mp)) * mp * TG_LD;
    const int64_t n_rowpart = ((npad + 255) / 256) * TG_LD;
    const int64_t need = (2 * (int64_t)k * npad + n_small + n_part + n_rowpart) * 8;
    GPR_HIP(hipStreamSynchronize(p->stream));
    size_t free_b = 0, total_b = 0;
    GPR_HIP(hipMemGetInfo(&free_b, &total_b));
    // (what an earlier target matrix holds comes back first; the V store of a problem not yet evaluated is still to come)
    const int64_t v_store = p->Vstore ? 0 : npad * mp * (int64_t)p->esz;
    if ((uint64_t)(need + v_store) > (uint64_t)free_b + (uint64_t)p->tg_bytes) {
      char buf[256];
      snprintf(buf, sizeof buf, "gprhip_set_targets_many: %d target vectors need %.3f GB on device %d (%.3f GB of it the V store "
               "the first evaluation adds) and %.3f GB are free", k, (need + v_store) / 1e9, p->device, v_store / 1e9,
               (free_b + p->tg_bytes) / 1e9);
      set_error(buf);
      throw HipFail{ST_OOM};
    }
    auto release = [p](double*& q) { release_buf(p, q); };
    release(p->tg_y); release(p->tg_w); release(p->tg_small); release(p->tg_part); release(p->tg_rowpart);
    // (the coefficient block went with tg_small.  multi_state stays: the single-target t / w are no more valid than before)
    p->tg_coeffs = false;
    p->alloc_bytes -= p->tg_bytes;
    p->tg_k = 0;
    p->tg_bytes = 0;
    const int64_t before = p->alloc_bytes;
    try {
      p->tg_y = p->alloc<double>((int64_t)k * npad);
      p->tg_w = p->alloc<double>((int64_t)k * npad);
      p->tg_small = p->alloc<double>(n_small);
      p->tg_part = p->alloc<double>(n_part);
      p->tg_rowpart = p->alloc<double>(n_rowpart);
    } catch (...) {
      // (the pre-check passed and an allocation failed all the same: nothing half-made stays -- the problem holds no target
      //  matrix, and its byte count is what it was without one)
      release(p->tg_y); release(p->tg_w); release(p->tg_small); release(p->tg_part); release(p->tg_rowpart);
      p->alloc_bytes = before;
      throw;
    }
    p->tg_bytes = p->alloc_bytes - before;
    GPR_HIP(hipMemsetAsync(p->tg_y, 0, (size_t)k * npad * sizeof(double), p->stream));
    GPR_HIP(hipMemsetAsync(p->tg_w, 0, (size_t)k * npad * sizeof(double), p->stream));
    GPR_HIP(hipMemsetAsync(p->tg_small, 0, (size_t)n_small * sizeof(double), p->stream));
  }
  GPR_HIP(hipMemcpy2DAsync(p->tg_y, (size_t)npad * sizeof(double), targets, (size_t)ld * sizeof(double),
                           (size_t)p->n * sizeof(double), (size_t)k, hipMemcpyHostToDevice, p->stream));
  GPR_HIP(hipStreamSynchronize(p->stream));
  p->tg_k = k;
}

// gprhip_eval_targets: the model parts of the evaluation run once as a model-only evaluation on the engine row path (v1, the
// model terms of W and X); the k-column steps of targets.hip put mean_k of the target terms in (v, W~, X are linear in them),
// and the assembled gradient of the mean is multiplied by k.
void do_eval_targets(gprhip_problem* p, const gprhip_hypers* h, int want_grad, gprhip_targets_result* res, double* l2,
                     double* grad_sum, double* coeffs) {
  const int k = p->tg_k;
  gprhip_hypers hm = *h;
  hm.model_only = 1;
  gprhip_result r{};
  p->multi = k;
  try {
    do_pass1<double>(p, &hm, want_grad, p->n, p->ar1);
    targets_pass1(p);
    do_pass2<double>(p, p->ar1, p->ar2);
    do_finish_enqueue(p, p->ar2);
    do_finish_collect(p, &r, grad_sum, nullptr);
  } catch (...) {
    p->multi = 0;
    throw;
  }
  p->multi = 0;
  p->multi_state = true;
  p->tg_coeffs = true;
  const int m = p->m;
  std::vector<double> hs(2 * TG_LD + (size_t)p->mp * TG_LD);
  GPR_HIP(hipMemcpy(hs.data(), p->tg_small, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
  res->l1 = r.l1;
  res->k = k;
  res->n_hypers = r.n_hypers;
  double l2sum = 0.0;
  for (int kk = 0; kk < k; ++kk) {
    l2[kk] = -0.5 * (hs[kk] - hs[TG_LD + kk]);  // -1/2 (|y~_k|^2 - |Q_n^T y~_k|^2), lib/fitc_gp.ml:290
    l2sum += l2[kk];
  }
  res->l_sum = k * r.l1 + l2sum;
  res->dl_dsigma2_sum = k * r.dl_dsigma2;
  if (want_grad)
    for (int64_t i = 0; i < r.n_hypers; ++i) grad_sum[i] *= k;
  if (coeffs) {
    const double* T = hs.data() + 2 * TG_LD;
    for (int kk = 0; kk < k; ++kk)
      for (int i = 0; i < m; ++i) coeffs[(size_t)kk * m + i] = T[(size_t)i * TG_LD + kk];
  }
}

// Means.calc (lib/fitc_gp.ml:418-425) per target column: means = K_tm T, test points in chunks of the training chunk
void do_predict_targets(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, double* means) {
  need_model(p, "gprhip_predict_targets");
  if (!p->multi_state || !p->tg_coeffs || !p->tg_k) {
    set_error(p->multi_state ? "gprhip_predict_targets: gprhip_set_targets_many changed the number of target vectors after the "
                               "last gprhip_eval_targets: its coefficients are gone"
                             : "gprhip_predict_targets: the last evaluation on this problem was not a gprhip_eval_targets");
    throw HipFail{ST_STATE};
  }
  GPR_HIP(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  const int mp = p->mp, k = p->tg_k;
  const int64_t chunk = p->chunk, npad = p->npad();
  ensure_predict_scratch(p, chunk);
  double* const K = static_cast<double*>(p->bufA);
  walk_chunks(p, chunk, test_inputs, ld, nt, 0, [&](int64_t lo, int rows, int rows_p, const double*, const double* pts) {
    launch_cov_cross<double>(p->cp, pts, rows, rows_p, p->Z, p->m, mp, p->d, K, s);
    launch_targets_rows(K, mp, rows, mp, 0, p->tg_T(), k, p->tg_w, 1, npad, s);  // (W_mat is scratch between evaluations)
    GPR_HIP(hipMemcpy2DAsync(means + lo, (size_t)nt * sizeof(double), p->tg_w, (size_t)npad * sizeof(double),
                             (size_t)rows * sizeof(double), (size_t)k, hipMemcpyDeviceToHost, s));
  });
  p->x_last = nullptr;  // (the chunk buffer that may have held X has been overwritten)
}

void tdrop(gprhip_problem* p) {  // a failed evaluation leaves its stage timers behind
  if (!p) return;
  for (auto& e : p->timer.ev) {
    hipEventDestroy(e.second.first);
    hipEventDestroy(e.second.second);
  }
  p->timer.ev.clear();
}

template <typename F>
int guarded(F&& f, gprhip_problem* p = nullptr) {
  try {
    f();
    return GPRHIP_OK;
  } catch (const HipFail& e) {
    tdrop(p);
    return e.status;
  } catch (const std::bad_alloc&) {
    set_error("gprhip: host allocation failed");
    return GPRHIP_EOOM;
  } catch (...) {
    set_error("gprhip: unexpected C++ exception");
    return GPRHIP_EHIP;
  }
}

}  // namespace

namespace gprhip {
double* problem_ar1(gprhip_problem* p) { return p->ar1; }
double* problem_ar2(gprhip_problem* p) { return p->ar2; }
hipStream_t problem_hip_stream(gprhip_problem* p) { return p->stream; }
int problem_device(const gprhip_problem* p) { return p->device; }
int64_t problem_rows(const gprhip_problem* p) { return p->n; }
int problem_finish_enqueue(gprhip_problem* p, const double* d_ar2, int light) {
  return guarded([&] { do_finish_enqueue(p, d_ar2, light != 0); }, p);
}
int problem_finish_collect(gprhip_problem* p, gprhip_result* res, double* grad, double* coeffs, int light) {
  return guarded([&] { do_finish_collect(p, res, grad, coeffs, light != 0); }, p);
}
}  // namespace gprhip

extern "C" {

const char* gprhip_last_error(void) { return last_error().c_str(); }
const char* gprhip_version(void) { return "gprhip 0.4 (gfx950)"; }

int gprhip_device_count(int* count) {
  return guarded([&] {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) c = 0;
    *count = c;
  });
}

int gprhip_problem_create(int device, int cov_kind, int64_t n, int D, int d, int m, int64_t chunk_rows,
                          gprhip_problem** out) {
  return gprhip_problem_create_ex(device, cov_kind, GPRHIP_F64, n, D, d, m, chunk_rows, out);
}

// share (lanes of a batch): the problem whose inputs, targets and stream the new one borrows, and its slice of the batch's
// parameter blocks; the batch has compared the memory of all its lanes with the device's before the first one is made
struct LaneShare {
  gprhip_problem* parent;
  double *hy_dev, *hy_host;
};
static int64_t hy_block_len(int cov_kind, int mp, int D, int d) {
  const bool fat = cov_kind == GPRHIP_COV_SE_FAT;
  return (int64_t)mp * d + 64 + (fat ? round_up((int64_t)D * d, 2) + mp + (int64_t)mp * d : 0);
}
static int problem_create_impl(int device, int cov_kind, int precision, int64_t n, int D, int d, int m, int64_t chunk_rows,
                               gprhip_problem** out, const LaneShare* share);

int gprhip_problem_create_ex(int device, int cov_kind, int precision, int64_t n, int D, int d, int m,
                             int64_t chunk_rows, gprhip_problem** out) {
  return problem_create_impl(device, cov_kind, precision, n, D, d, m, chunk_rows, out, nullptr);
}

static int problem_create_impl(int device, int cov_kind, int precision, int64_t n, int D, int d, int m, int64_t chunk_rows,
                               gprhip_problem** out, const LaneShare* share) {
  return guarded([&] {
    if (precision != GPRHIP_F64 && precision != GPRHIP_F32_BULK) {
      set_error("gprhip_problem_create_ex: unknown precision");
      throw HipFail{ST_BAD_ARG};
    }
    if (!out || n < 1 || D < 1 || d < 1 || m < 1 ||
        (cov_kind != GPRHIP_COV_SE_ISO && cov_kind != GPRHIP_COV_SE_FAT) ||
        (cov_kind == GPRHIP_COV_SE_ISO && d != D)) {
      set_error("gprhip_problem_create: invalid arguments (need n,D,d,m >= 1, d == D for Cov_se_iso)");
      throw HipFail{ST_BAD_ARG};
    }
    check_single_hip_runtime("gprhip_problem_create");
    GPR_HIP(hipSetDevice(device));
    gemm_init();
    auto* p = new gprhip_problem();
    *out = p;
    p->device = device; p->kind = cov_kind; p->n = n; p->D = D; p->d = d; p->m = m;
    p->f32 = (precision == GPRHIP_F32_BULK);
    p->esz = p->f32 ? 4 : 8;
    p->mp = (int)round_up(m, TILE);
    const Sizing z = problem_sizing(n, p->mp, chunk_rows, !p->f32);
    const int64_t chunk = z.chunk;
    p->chunk = chunk;
    p->nchunks = z.nchunks;
    p->slice_rows = z.slice_rows;
    p->kslices = z.kslices;
    if (share) {
      p->is_lane = true;
      p->lane_of = share->parent;
    }
    if (!share) {  // the whole resident set of the problem against what the device has free, BEFORE anything is allocated: a shard that
       // cannot hold its V store fails here, by name and with the figures, not in the first evaluation's hipMalloc
      gprhip_memory_plan_t plan;
      memory_plan(cov_kind, precision, n, D, d, m, chunk_rows, &plan);
      size_t free_b = 0, total_b = 0;
      GPR_HIP(hipMemGetInfo(&free_b, &total_b));
      const bool verbose = getenv("GPRHIP_VERBOSE") && atoi(getenv("GPRHIP_VERBOSE")) != 0;
      if (verbose)
        fprintf(stderr, "gprhip: device %d: problem n=%lld m=%d d=%d (%s): resident %.3f GB = V %.3f + chunk buffers %.3f + "
                        "split-K slices %.3f + inputs %.3f + rows %.3f + m x m %.3f + rest %.3f  (optional K_nm copy %.3f); "
                        "free %.3f of %.3f GB\n", device, (long long)n, m, d, p->f32 ? "fp32-bulk" : "fp64",
                plan.total / 1e9, plan.v_store / 1e9, plan.chunk_buffers / 1e9, plan.slices / 1e9, plan.inputs / 1e9,
                plan.row_vectors / 1e9, plan.mxm / 1e9, plan.rest / 1e9, plan.k_store_optional / 1e9, free_b / 1e9, total_b / 1e9);
      if ((uint64_t)plan.total > (uint64_t)free_b) {
        char buf[320];
        snprintf(buf, sizeof buf, "gprhip_problem_create: the problem needs %.1f GB on device %d (V = K_nm U^-1 of %lld rows x %d: "
                 "%.1f GB, split-K slices %.1f GB, chunk buffers %.1f GB) and %.1f GB are free of %.1f GB: shard the rows over more "
                 "devices (gprhip_ctx_create) or use the fp32-bulk mode", plan.total / 1e9, device, (long long)n, p->mp,
                 plan.v_store / 1e9, plan.slices / 1e9, plan.chunk_buffers / 1e9, free_b / 1e9, total_b / 1e9);
        set_error(buf);
        delete p;
        *out = nullptr;
        throw HipFail{ST_OOM};
      }
    }
    if (const char* e = getenv("GPRHIP_TIMING")) {
      p->timer.on = atoi(e) >= 2;
      p->timer.kernel = atoi(e) >= 1;
    }
    if (const char* e = getenv("GPRHIP_TILE_ORDER")) p->tile_order = atoi(e);
    if (const char* e = getenv("GPRHIP_GRAD_SCALAR")) p->grad_scalar = atoi(e);
    if (const char* e = getenv("GPRHIP_K_RESIDENT")) p->k_resident = atoi(e);
    if (const char* e = getenv("GPRHIP_W_AS_WS")) p->w_as_ws = atoi(e);
    if (const char* e = getenv("GPRHIP_SMALL_PATH")) p->small_path = atoi(e);
    if (const char* e = getenv("GPRHIP_MID_PATH")) p->mid_path = atoi(e);
    if (const char* e = getenv("GPRHIP_MID_GRAM")) p->mid_gram = atoi(e);
    if (const char* e = getenv("GPRHIP_F32_COEFF_TOL")) p->f32_coeff_tol = atof(e);
    if (const char* e = getenv("GPRHIP_MERGED_X")) p->merged_x_mode = atoi(e);
    if (const char* e = getenv("GPRHIP_POTRF_ENGINE")) p->engine_steps = atoi(e) != 0;
#ifdef GPRHIP_LAB  // the measured-slower variants (DESIGN sections 4, 14): switches of the lab build only
    if (const char* e = getenv("GPRHIP_POTRF_CHAIN")) p->potrf_chain_mode = atoi(e);
    if (const char* e = getenv("GPRHIP_COV_OVERLAP")) p->cov_overlap = atoi(e);
#endif
    if (share) p->stream = share->parent->stream;
    else GPR_HIP(hipStreamCreate(&p->stream));
    GPR_HIP(hipStreamCreate(&p->stream2));
    for (int k = 0; k < 2; ++k) {
      GPR_HIP(hipEventCreateWithFlags(&p->ev_cov[k], hipEventDisableTiming));
      GPR_HIP(hipEventCreateWithFlags(&p->ev_vdone[k], hipEventDisableTiming));
    }
#ifdef GPRHIP_LAB
    if (p->mp >= 3 * TILE && getenv("GPRHIP_POTRF_LOOKAHEAD") && atoi(getenv("GPRHIP_POTRF_LOOKAHEAD")) > 0) {  // (A/B runs only)
      p->potrf_aux.min_rest = atoi(getenv("GPRHIP_POTRF_LOOKAHEAD"));
      GPR_HIP(hipStreamCreate(&p->potrf_aux.side));
      for (int k = 0; k < 2; ++k) {
        GPR_HIP(hipEventCreateWithFlags(&p->potrf_aux.ev_panel[k], hipEventDisableTiming));
        GPR_HIP(hipEventCreateWithFlags(&p->potrf_aux.ev_rest[k], hipEventDisableTiming));
      }
    }
#endif
    GPR_HIP(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    GPR_HIP(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
    GPR_HIP(hipEventCreateWithFlags(&p->ev_rf, hipEventDisableTiming));
    GPR_HIP(hipEventCreateWithFlags(&p->ev_binv, hipEventDisableTiming));
    const int mp = p->mp;
    const int64_t mm = (int64_t)mp * mp;
    const int64_t npad = (int64_t)p->nchunks * chunk;
    if (share) {
      p->X = share->parent->X;
      p->y = share->parent->y;
    } else {
      p->X = p->alloc<double>(n * D);
      p->y = p->alloc<double>(npad);
    }
    if (cov_kind == GPRHIP_COV_SE_FAT) p->P = p->alloc<double>(n * d);
    {  // the per-evaluation parameter block and its pinned host mirror (upload_hypers)
      const bool fat = cov_kind == GPRHIP_COV_SE_FAT;
      const int64_t o_shift = (int64_t)mp * d, o_tproj = o_shift + 64, o_het = o_tproj + (fat ? round_up((int64_t)D * d, 2) : 0),
                    o_ms = o_het + (fat ? mp : 0);
      p->hy_len = o_ms + (fat ? (int64_t)mp * d : 0);
      if (share) {
        p->hy_dev = share->hy_dev;
        p->hy_host = share->hy_host;
      } else {
        p->hy_dev = p->alloc<double>(p->hy_len);
        GPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->hy_host), (size_t)p->hy_len * sizeof(double), hipHostMallocDefault));
      }
      GPR_HIP(hipEventCreateWithFlags(&p->ev_hy, hipEventDisableTiming));
      p->Z = p->hy_dev; p->hZ = p->hy_host;
      p->zshift = p->hy_dev + o_shift; p->hShift = p->hy_host + o_shift;
      if (fat) {
        p->tproj = p->hy_dev + o_tproj; p->hTproj = p->hy_host + o_tproj;
        p->het = p->hy_dev + o_het; p->hHet = p->hy_host + o_het;
        p->ms = p->hy_dev + o_ms; p->hMs = p->hy_host + o_ms;
      }
    }
    p->km = p->alloc<double>(mm); p->kj = p->alloc<double>(mm); p->umat = p->alloc<double>(mm);
    p->uinv = p->alloc<double>(mm); p->bmat = p->alloc<double>(mm);
    p->rinv = p->alloc<double>(mm); p->binv = p->alloc<double>(mm); p->wtil = p->alloc<double>(mm);
    p->rfinv = p->alloc<double>(mm);
    p->wmat = p->alloc<double>(mm);
    p->tmp = p->alloc<double>((int64_t)mp * TILE);
    p->dinv = p->alloc<double>((int64_t)(mp / TILE) * TILE * TILE);
    p->bvec = p->alloc<double>(mp); p->ttil = p->alloc<double>(mp);
    {  // the result block and its pinned mirror; the tails of the exchange buffers land in ex_host (do_finish_enqueue)
      p->res_len = NSCAL + 2 + mp + p->km_rows() * mp + mp;
      p->ex_len = A1_TAIL + p->col_rows() * mp + (int64_t)p->dbig() * d + A2_TAIL;
      p->res_dev = p->alloc<double>(p->res_len + p->ex_len);
      p->ex_dev = p->res_dev + p->res_len;
      p->scal = p->res_dev;
      p->info = reinterpret_cast<int*>(p->res_dev + NSCAL);
      p->tvec = p->res_dev + NSCAL + 2;
      p->kmred = p->tvec + mp;
      p->wdiag = p->kmred + p->km_rows() * mp;
      GPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->res_host), (size_t)(p->res_len + p->ex_len) * sizeof(double),
                            hipHostMallocPortable | hipHostMallocMapped));  // (kernels of this device write into it)
      p->ex_host = p->res_host + p->res_len;
    }
    p->r = p->alloc<double>(npad); p->is = p->alloc<double>(npad); p->yis = p->alloc<double>(npad);
    p->w = p->alloc<double>(npad); p->v = p->alloc<double>(npad);
    if (cov_kind == GPRHIP_COV_SE_FAT) {
      p->es = p->alloc<double>(npad);
      p->projpart = p->alloc<double>(((chunk + 255) / 256) * (int64_t)D * d);
    }
    p->rp1 = p->alloc<double>(chunk * 4 * (mp / TILE)); p->rp2 = p->alloc<double>(chunk * 4 * (mp / TILE));
    p->bufA = p->alloc<char>(chunk * mp * p->esz); p->bufB = p->alloc<char>(chunk * mp * p->esz);
    if (p->f32) {
      p->uinv_f = p->alloc<float>(mm);
      p->rinv_f = p->alloc<float>(mm);
      p->rfinv_f = p->alloc<float>(mm);
      p->is_f = p->alloc<float>(npad); p->yis_f = p->alloc<float>(npad); p->v_f = p->alloc<float>(npad);
    }
    p->slices_bytes = (int64_t)p->kslices * mm * p->esz;
    p->slices = p->alloc<char>(p->slices_bytes);
    p->rowpart = p->alloc<double>((int64_t)pass1_row_blocks((int)chunk) * 4);
    p->gemvpart = p->alloc<double>((int64_t)p->kslices * mp);  // c~ partials, one row per k-slice
    p->grad_slab = pick_grad_slab((int)p->col_rows(), n, chunk, mp);
    const int64_t gslab = p->grad_slab;
    const int64_t nslab = (chunk + gslab - 1) / gslab;
    p->colpart = p->alloc<double>(nslab * p->col_rows() * mp);
    p->scalpart = p->alloc<double>(nslab * (mp / TILE) * 2);
    p->kmpart = p->alloc<double>((int64_t)((m + km_slab_rows(m) - 1) / km_slab_rows(m)) * p->km_rows() * mp);
    p->ar1 = p->alloc<double>(gprhip_ar1_len(p));
    p->ar2 = p->alloc<double>(gprhip_ar2_len(p));
    {
      gprhip_memory_plan_t plan;
      memory_plan(cov_kind, precision, n, D, d, m, chunk_rows, &plan);
      p->planned_bytes = plan.total;
      if (getenv("GPRHIP_VERBOSE") && atoi(getenv("GPRHIP_VERBOSE")) != 0)
        fprintf(stderr, "gprhip: device %d: allocated %.3f GB at creation, %.3f GB planned without the V store\n", device,
                p->alloc_bytes / 1e9, (plan.total - plan.v_store) / 1e9);
    }
    if (!share) GPR_HIP(hipMemsetAsync(p->y, 0, (size_t)npad * sizeof(double), p->stream));
    // R^-1 is written on its upper tiles only; the fp32 conversion reads the whole square
    GPR_HIP(hipMemsetAsync(p->rfinv, 0, (size_t)mm * sizeof(double), p->stream));
    GPR_HIP(hipStreamSynchronize(p->stream));
  });
}

void gprhip_problem_destroy(gprhip_problem* p) {
  if (!p) return;
  hipSetDevice(p->device);
  if (p->stream) {
    hipStreamSynchronize(p->stream);
    if (!p->is_lane) hipStreamDestroy(p->stream);
  }
  batch_orphan_all(p);  // batches that borrow this problem lose their inputs, targets and stream: they can only be destroyed
  if (p->stream2) {
    hipStreamSynchronize(p->stream2);
    hipStreamDestroy(p->stream2);
  }
  if (p->ev_hy) hipEventDestroy(p->ev_hy);
  if (p->hy_host && !p->is_lane) hipHostFree(p->hy_host);
  if (p->res_host) hipHostFree(p->res_host);
  if (p->acq_host) hipHostFree(p->acq_host);
  if (p->mv_host) hipHostFree(p->mv_host);
  if (p->rf_active) hipHostFree(p->rf_active);
  if (p->sp_zhost) hipHostFree(p->sp_zhost);
  if (p->sp_host) hipHostFree(p->sp_host);
  if (p->ev_fork) hipEventDestroy(p->ev_fork);
  if (p->ev_join) hipEventDestroy(p->ev_join);
  if (p->ev_rf) hipEventDestroy(p->ev_rf);
  if (p->ev_binv) hipEventDestroy(p->ev_binv);
  for (int k = 0; k < 2; ++k) {
    if (p->ev_cov[k]) hipEventDestroy(p->ev_cov[k]);
    if (p->ev_vdone[k]) hipEventDestroy(p->ev_vdone[k]);
  }
  if (p->potrf_aux.side) {
    hipStreamSynchronize(p->potrf_aux.side);
    hipStreamDestroy(p->potrf_aux.side);
    for (int k = 0; k < 2; ++k) {
      hipEventDestroy(p->potrf_aux.ev_panel[k]);
      hipEventDestroy(p->potrf_aux.ev_rest[k]);
    }
  }
  if (p->timer.k0) {
    hipEventDestroy(p->timer.k0);
    hipEventDestroy(p->timer.k1);
  }
  for (void* a : p->allocs) hipFree(a);
#ifdef GPRHIP_LAB
  potrf_chain_destroy(p->chain);
#endif
  delete p;
}

int gprhip_set_inputs(gprhip_problem* p, const double* inputs, int64_t ld) {
  return guarded([&] {
    if (!p || !inputs || ld < p->D) {
      set_error("gprhip_set_inputs: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    GPR_HIP(hipSetDevice(p->device));
    GPR_HIP(hipMemcpy2DAsync(p->X, (size_t)p->D * sizeof(double), inputs, (size_t)ld * sizeof(double),
                             (size_t)p->D * sizeof(double), (size_t)p->n, hipMemcpyHostToDevice,
                             p->stream));
    GPR_HIP(hipStreamSynchronize(p->stream));
    p->have_inputs = true;
  });
}

int gprhip_set_targets(gprhip_problem* p, const double* targets) {
  return guarded([&] {
    if (!p || !targets) {
      set_error("gprhip_set_targets: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    GPR_HIP(hipSetDevice(p->device));
    GPR_HIP(hipMemcpyAsync(p->y, targets, (size_t)p->n * sizeof(double), hipMemcpyHostToDevice, p->stream));
    GPR_HIP(hipStreamSynchronize(p->stream));
    p->have_targets = true;
  });
}

int gprhip_set_inputs_device(gprhip_problem* p, const double* d_inputs) {
  return guarded([&] {
    if (!p || !d_inputs) {
      set_error("gprhip_set_inputs_device: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    GPR_HIP(hipSetDevice(p->device));
    GPR_HIP(hipMemcpyAsync(p->X, d_inputs, (size_t)p->n * p->D * sizeof(double), hipMemcpyDeviceToDevice,
                           p->stream));
    GPR_HIP(hipStreamSynchronize(p->stream));
    p->have_inputs = true;
  });
}

int gprhip_set_targets_device(gprhip_problem* p, const double* d_targets) {
  return guarded([&] {
    if (!p || !d_targets) {
      set_error("gprhip_set_targets_device: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    GPR_HIP(hipSetDevice(p->device));
    GPR_HIP(hipMemcpyAsync(p->y, d_targets, (size_t)p->n * sizeof(double), hipMemcpyDeviceToDevice,
                           p->stream));
    GPR_HIP(hipStreamSynchronize(p->stream));
    p->have_targets = true;
  });
}

int gprhip_batch_create(gprhip_problem* p, int lanes, gprhip_batch** out) {
  return guarded([&] {
    if (out) *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
      (void)hipGetLastError();
      set_error("gprhip_batch_create: no HIP device is visible");
      throw HipFail{ST_HIP_ERROR};
    }
    if (!p || !out || p->is_lane || lanes < 1 || lanes > GPRHIP_MAX_BATCH) {
      set_error("gprhip_batch_create: invalid arguments (need a problem and 1 <= lanes <= GPRHIP_MAX_BATCH)");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32 || !p->small_path || p->engine_steps || !small_path_fits(p->m, p->mp, p->d, 0, p->n, false)) {
      set_error("gprhip_batch_create: batches run the small path only (fp64, at most 64 inducing points of at most 16 "
                "dimensions, GPRHIP_SMALL_PATH not 0): evaluate this problem with gprhip_eval");
      throw HipFail{ST_BAD_ARG};
    }
    GPR_HIP(hipSetDevice(p->device));
    auto* b = new gprhip_batch();
    try {
      // a lane's slice of the upload block: its parameter block, then one struct per launch, each on a 16-byte boundary
      int64_t off = round_up(hy_block_len(p->kind, p->mp, p->D, p->d) * (int64_t)sizeof(double), 16);
      auto place = [&](int64_t& o, size_t bytes) {
        o = off;
        off += round_up((int64_t)bytes, 16);
      };
      place(b->o_km, sizeof(PotrfKmLane)); place(b->o_p1, sizeof(SmallPass1Args)); place(b->o_r1, sizeof(SmallReduce1Args));
      place(b->o_fuse, sizeof(PotrfFuseLane)); place(b->o_p2, sizeof(SmallPass2Args)); place(b->o_r2, sizeof(SmallReduce2Args));
      place(b->o_fin, sizeof(SmallFinishArgs)); place(b->o_ship, sizeof(ShipArgs));
      b->stride = round_up(off, 64);
      {  // all lanes against what the device has free, before the first allocation
        const int64_t need = lanes * (batch_lane_bytes(p) + b->stride);
        size_t free_b = 0, total_b = 0;
        GPR_HIP(hipMemGetInfo(&free_b, &total_b));
        if ((uint64_t)need > (uint64_t)free_b) {
          char buf[256];
          snprintf(buf, sizeof buf, "gprhip_batch_create: %d lanes need %.2f GB on device %d (%.1f MB each) and %.2f GB are free "
                   "of %.2f GB", lanes, need / 1e9, p->device, need / 1e6 / lanes, free_b / 1e9, total_b / 1e9);
          set_error(buf);
          throw HipFail{ST_OOM};
        }
      }
      GPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->up_host), (size_t)(b->stride * lanes), hipHostMallocDefault));
      std::memset(b->up_host, 0, (size_t)(b->stride * lanes));
      GPR_HIP(hipMalloc(reinterpret_cast<void**>(&b->up_dev), (size_t)(b->stride * lanes)));
      for (int j = 0; j < lanes; ++j) {
        LaneShare sh{p, reinterpret_cast<double*>(b->up_dev + j * b->stride), reinterpret_cast<double*>(b->up_host + j * b->stride)};
        gprhip_problem* l = nullptr;
        const int st = problem_create_impl(p->device, p->kind, GPRHIP_F64, p->n, p->D, p->d, p->m, p->chunk, &l, &sh);
        if (l) b->lanes.push_back(l);
        if (st != GPRHIP_OK) throw HipFail{st};
        // what an evaluation would otherwise allocate when it first runs (ensure_eval_scratch): nothing is left for later
        l->Vstore = l->alloc<double>((int64_t)l->nchunks * l->chunk * l->mp);
        l->small_part = l->alloc<double>(small_part_len(l->d, l->D));
        if (l->d <= 8) l->small_k = l->alloc<double>(round_up(l->n, TILE) * 64);
      }
      GPR_HIP(hipStreamSynchronize(p->stream));
    } catch (...) {
      (void)hipGetLastError();
      const std::string msg = last_error();
      b->parent = nullptr;
      gprhip_batch_destroy(b);
      set_error(msg);
      throw;
    }
    b->parent = p;
    p->batches.push_back(b);
    *out = b;
  });
}

void gprhip_batch_destroy(gprhip_batch* b) {
  if (!b) return;
  if (b->parent) {
    hipSetDevice(b->parent->device);
    hipStreamSynchronize(b->parent->stream);
    auto& v = b->parent->batches;
    v.erase(std::remove(v.begin(), v.end(), b), v.end());
  }
  for (gprhip_problem* l : b->lanes) {
    if (!b->parent) l->stream = nullptr;
    gprhip_problem_destroy(l);
  }
  if (b->up_host) hipHostFree(b->up_host);
  if (b->up_dev) hipFree(b->up_dev);
  delete b;
}

int gprhip_batch_lanes(const gprhip_batch* b) { return b ? (int)b->lanes.size() : 0; }

gprhip_problem* gprhip_batch_lane(gprhip_batch* b, int j) {
  return (b && j >= 0 && j < (int)b->lanes.size()) ? b->lanes[j] : nullptr;
}

int gprhip_batch_eval(gprhip_batch* b, int count, const gprhip_hypers* h, int want_grad, gprhip_result* res, double* grad,
                      int64_t ldg, double* coeffs, int* status) {
  gprhip_problem* l0 = (b && !b->lanes.empty()) ? b->lanes[0] : nullptr;
  return guarded([&] { batch_eval(b, count, h, want_grad, res, grad, ldg, coeffs, status); }, l0);
}

int64_t gprhip_n_hypers(const gprhip_problem* p, int flags) {
  if (!p) return 0;
  if (p->kind == GPRHIP_COV_SE_ISO) return 2 + (int64_t)p->d * p->m;
  return 1 + (int64_t)p->d * p->m + ((flags & 1) ? (int64_t)p->D * p->d : 0) + ((flags & 2) ? p->m : 0) +
         ((flags & 4) ? (int64_t)p->d * p->m : 0);
}

int gprhip_memory_plan(int cov_kind, int precision, int64_t n, int D, int d, int m, int64_t chunk_rows,
                       gprhip_memory_plan_t* plan) {
  return guarded([&] {
    if (!plan || n < 1 || D < 1 || d < 1 || m < 1 || (cov_kind != GPRHIP_COV_SE_ISO && cov_kind != GPRHIP_COV_SE_FAT) ||
        (precision != GPRHIP_F64 && precision != GPRHIP_F32_BULK)) {
      set_error("gprhip_memory_plan: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    memory_plan(cov_kind, precision, n, D, d, m, chunk_rows, plan);
  });
}

int64_t gprhip_exchange_len(int cov_kind, int D, int d, int m, int which) {
  if (m < 1 || d < 1 || D < 1 || (which != 1 && which != 2) || (cov_kind != GPRHIP_COV_SE_ISO && cov_kind != GPRHIP_COV_SE_FAT))
    return 0;
  const int mp = (int)round_up(m, TILE);
  if (which == 1) return packed_upper_len(mp) + mp + A1_TAIL;
  const bool fat = cov_kind == GPRHIP_COV_SE_FAT;
  const int64_t dbig = fat ? D : 0, col_rows = d + 1 + dbig + (fat ? d : 0);  // gprhip_problem::col_rows / dbig
  return packed_upper_len(mp) + col_rows * mp + dbig * d + A2_TAIL;
}
int64_t gprhip_exchange_offset(int m, int r, int c) {
  const int mp = (int)round_up(m, TILE);
  if (m < 1 || r < 0 || c < 0 || r >= mp || c >= mp || r / TILE > c / TILE) return -1;
  return packed_upper_off(r, c);
}
int64_t gprhip_ar1_len(const gprhip_problem* p) { return p ? gprhip_exchange_len(p->kind, p->D, p->d, p->m, 1) : 0; }
int64_t gprhip_ar2_len(const gprhip_problem* p) { return p ? gprhip_exchange_len(p->kind, p->D, p->d, p->m, 2) : 0; }

int gprhip_eval_pass1(gprhip_problem* p, const gprhip_hypers* h, int want_grad, int64_t n_total,
                      double* d_ar1) {
  return guarded([&] {
    if (!p || !d_ar1) {
      set_error("gprhip_eval_pass1: NULL argument");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) do_pass1<float>(p, h, want_grad, n_total, d_ar1);
    else do_pass1<double>(p, h, want_grad, n_total, d_ar1);
  }, p);
}

int gprhip_eval_pass2(gprhip_problem* p, const double* d_ar1, double* d_ar2) {
  return guarded([&] {
    if (!p || !d_ar1 || !d_ar2) {
      set_error("gprhip_eval_pass2: NULL argument");
      throw HipFail{ST_BAD_ARG};
    }
    // keep the reduced exchange-1 buffer where finish() reads its scalar tail
    if (d_ar1 != p->ar1)
      GPR_HIP(hipMemcpyAsync(p->ar1, d_ar1, (size_t)gprhip_ar1_len(p) * sizeof(double),
                             hipMemcpyDeviceToDevice, p->stream));
    if (p->f32) do_pass2<float>(p, p->ar1, d_ar2);
    else do_pass2<double>(p, p->ar1, d_ar2);
  }, p);
}

int gprhip_eval_finish(gprhip_problem* p, const double* d_ar2, gprhip_result* res, double* grad,
                       double* coeffs) {
  return guarded([&] {
    if (!p || !d_ar2 || !res || (p->want_grad && !grad)) {
      set_error("gprhip_eval_finish: NULL argument");
      throw HipFail{ST_BAD_ARG};
    }
    do_finish_enqueue(p, d_ar2);
    do_finish_collect(p, res, grad, coeffs);
  }, p);
}

int gprhip_eval(gprhip_problem* p, const gprhip_hypers* h, int want_grad, gprhip_result* res,
                double* grad, double* coeffs) {
  return guarded([&] {
    if (!p || !res || (want_grad && !grad)) {
      set_error("gprhip_eval: NULL argument");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) {
      do_pass1<float>(p, h, want_grad, p->n, p->ar1);
      do_pass2<float>(p, p->ar1, p->ar2);
    } else {
      do_pass1<double>(p, h, want_grad, p->n, p->ar1);
      do_pass2<double>(p, p->ar1, p->ar2);
    }
    do_finish_enqueue(p, p->ar2);
    do_finish_collect(p, res, grad, coeffs);
  }, p);
}

int gprhip_eval_input_grad(gprhip_problem* p, const gprhip_hypers* h, gprhip_result* res, double* grad, double* coeffs,
                           double* dl_dinputs, int64_t ld, int on_device) {
  return guarded([&] {
    if (!p || !h || !h->inducing || !res || !grad) {
      set_error("gprhip_eval_input_grad: NULL argument");
      throw HipFail{ST_BAD_ARG};
    }
    if (!dl_dinputs) {
      set_error("gprhip_eval_input_grad: dl_dinputs is NULL");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) {
      set_error("gprhip_eval_input_grad: the input gradient is evaluated in fp64 only (GPRHIP_F32_BULK problem)");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->is_lane) {
      set_error("gprhip_eval_input_grad: not available on a lane of a batch");
      throw HipFail{ST_BAD_ARG};
    }
    if (h->log_multiscales_m05) {
      set_error("gprhip_eval_input_grad: multiscales are not supported (log_multiscales_m05 != NULL)");
      throw HipFail{ST_BAD_ARG};
    }
    if (on_device ? ld != p->D : ld < p->D) {
      set_error("gprhip_eval_input_grad: bad ld (need ld == D for a device buffer, ld >= D for a host buffer)");
      throw HipFail{ST_BAD_ARG};
    }
    check_hypers(p, h);
    if (!p->have_inputs || (!p->have_targets && !h->model_only)) {
      set_error("gprhip: inputs/targets not set");
      throw HipFail{ST_STATE};
    }
    if (h->reuse_v && !p->have_v) {
      set_error("gprhip: reuse_v set but this problem holds no V of a previous evaluation");
      throw HipFail{ST_STATE};
    }
    GPR_HIP(hipSetDevice(p->device));
    // the library's own buffers of this call, after a look at the device's free memory: a refusal leaves the problem as it was
    const bool proj = p->kind == GPRHIP_COV_SE_FAT && h->tproj != nullptr;
    const int64_t need_buf = (!on_device && !p->xg_buf) ? p->n * p->D : 0;
    const int64_t need_g = (proj && !p->xg_g) ? p->chunk * p->d : 0;
    if (need_buf + need_g > 0) {
      size_t free_b = 0, total_b = 0;
      GPR_HIP(hipMemGetInfo(&free_b, &total_b));
      if ((size_t)(need_buf + need_g) * sizeof(double) + (size_t(64) << 20) > free_b) {
        set_error("gprhip_eval_input_grad: not enough device memory for the input-gradient buffers");
        throw HipFail{ST_OOM};
      }
      if (need_buf) p->xg_buf = p->alloc<double>(need_buf);
      if (need_g) p->xg_g = p->alloc<double>(need_g);
    }
    p->xgrad = true;
    p->xg_engine = p->nchunks > 1;
    p->xg_dst = on_device ? dl_dinputs : p->xg_buf;
    try {
      do_pass1<double>(p, h, 1, p->n, p->ar1);
      do_pass2<double>(p, p->ar1, p->ar2);
      do_finish_enqueue(p, p->ar2);
      do_finish_collect(p, res, grad, coeffs);
      GPR_HIP(hipStreamSynchronize(p->stream));
      if (!on_device)
        GPR_HIP(hipMemcpy2D(dl_dinputs, (size_t)ld * sizeof(double), p->xg_buf, (size_t)p->D * sizeof(double),
                            (size_t)p->D * sizeof(double), (size_t)p->n, hipMemcpyDeviceToHost));
    } catch (...) {
      p->xgrad = p->xg_engine = false;
      p->xg_dst = nullptr;
      throw;
    }
    p->xgrad = p->xg_engine = false;
    p->xg_dst = nullptr;
  }, p);
}

int gprhip_set_targets_many(gprhip_problem* p, const double* targets, int64_t ld, int k) {
  return guarded([&] {
    if (!p || !targets || k < 1 || k > GPRHIP_MAX_TARGETS || ld < p->n) {
      set_error("gprhip_set_targets_many: invalid arguments (need 1 <= k <= GPRHIP_MAX_TARGETS, ld >= n)");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) {
      set_error("gprhip_set_targets_many: several target vectors are evaluated in fp64 only (GPRHIP_F32_BULK problem)");
      throw HipFail{ST_BAD_ARG};
    }
    do_set_targets_many(p, targets, ld, k);
  }, p);
}

int gprhip_eval_targets(gprhip_problem* p, const gprhip_hypers* h, int want_grad, gprhip_targets_result* res, double* l2,
                        double* grad_sum, double* coeffs) {
  return guarded([&] {
    if (!p || !h || !res || !l2 || (want_grad && !grad_sum)) {
      set_error("gprhip_eval_targets: NULL argument");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) {
      set_error("gprhip_eval_targets: several target vectors are evaluated in fp64 only (GPRHIP_F32_BULK problem)");
      throw HipFail{ST_BAD_ARG};
    }
    if (h->model_only) {
      set_error("gprhip_eval_targets: model_only = 1 (an evaluation without targets is gprhip_eval)");
      throw HipFail{ST_BAD_ARG};
    }
    if (!p->tg_k) {
      set_error("gprhip_eval_targets: no target matrix set (gprhip_set_targets_many)");
      throw HipFail{ST_STATE};
    }
    do_eval_targets(p, h, want_grad, res, l2, grad_sum, coeffs);
  }, p);
}

int gprhip_predict_targets(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, double* means) {
  return guarded([&] {
    if (!p || !test_inputs || !means || nt < 1 || ld < p->D) {
      set_error("gprhip_predict_targets: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    do_predict_targets(p, test_inputs, ld, nt, means);
  });
}

int gprhip_predict(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int predictive,
                   double* means, double* variances) {
  return guarded([&] {
    if (!p || !test_inputs || nt < 1 || ld < p->D) {
      set_error("gprhip_predict: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) do_predict<float>(p, test_inputs, ld, nt, predictive, means, variances);
    else do_predict<double>(p, test_inputs, ld, nt, predictive, means, variances);
  });
}

int gprhip_predict_input_grad(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int predictive,
                              double* means, double* variances, double* dmeans, double* dvariances, int64_t ldg,
                              int on_device) {
  return guarded([&] {
    if (!p || !test_inputs || nt < 1) {
      set_error("gprhip_predict_input_grad: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    if (!means && !variances && !dmeans && !dvariances) {
      set_error("gprhip_predict_input_grad: all four outputs are NULL");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) {
      set_error("gprhip_predict_input_grad: the prediction gradient is evaluated in fp64 only (GPRHIP_F32_BULK problem)");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->d > 64) {
      set_error("gprhip_predict_input_grad: at most 64 point dimensions on the kernel side (d)");
      throw HipFail{ST_BAD_ARG};
    }
    if (on_device ? ld != p->D : ld < p->D) {
      set_error("gprhip_predict_input_grad: bad ld (need ld == D for device buffers, ld >= D for host buffers)");
      throw HipFail{ST_BAD_ARG};
    }
    if ((dmeans || dvariances) && (on_device ? ldg != p->D : ldg < p->D)) {
      set_error("gprhip_predict_input_grad: bad ldg (need ldg == D for device buffers, ldg >= D for host buffers)");
      throw HipFail{ST_BAD_ARG};
    }
    do_predict_input_grad(p, test_inputs, ld, nt, predictive, means, variances, dmeans, dvariances, ldg, on_device);
  }, p);
}

// what gprhip_acquire and gprhip_acquire_refine refuse of a criterion
void check_acquisition(const char* fn, const gprhip_acquisition* acq) {
  const char* why = nullptr;
  if (!acq) why = "invalid arguments (acq is NULL)";
  else if (acq->kind < GPRHIP_ACQ_EI || acq->kind > GPRHIP_ACQ_BOUND) why = "unknown kind (one of GPRHIP_ACQ_EI, _LOG_EI, _PI, _BOUND)";
  else if (!(acq->xi >= 0.0) || !(acq->kappa >= 0.0)) why = "xi and kappa must not be negative";
  else if (!(acq->var_floor > 0.0) || !std::isfinite(acq->var_floor)) why = "var_floor must be positive and finite";
  else if (!std::isfinite(acq->best)) why = "best must be finite";
  if (!why) return;
  set_error(std::string(fn) + ": " + why);
  throw HipFail{ST_BAD_ARG};
}

int gprhip_acquire(gprhip_problem* p, const gprhip_acquisition* acq, const double* test_inputs, int64_t ld, int64_t nt,
                   double* values, double* dvalues, int64_t ldg, double* means, double* variances, int top_k,
                   int64_t* top_index, double* top_values, double* top_dvalues, int on_device) {
  return guarded([&] {
    check_acquisition("gprhip_acquire", acq);
    if (top_k < 0 || top_k > GPRHIP_MAX_TOP_K) {
      set_error("gprhip_acquire: top_k must lie in 0 .. GPRHIP_MAX_TOP_K (64)");
      throw HipFail{ST_BAD_ARG};
    }
    if (top_k > 0 && !top_index) {
      set_error("gprhip_acquire: top_k > 0 needs top_index");
      throw HipFail{ST_BAD_ARG};
    }
    if (!values && !dvalues && !means && !variances && top_k == 0) {
      set_error("gprhip_acquire: nothing is requested (the four outputs are NULL and top_k is 0)");
      throw HipFail{ST_BAD_ARG};
    }
    if (!p || !test_inputs || nt < 1) {
      set_error("gprhip_acquire: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) {
      set_error("gprhip_acquire: the prediction gradient is evaluated in fp64 only (GPRHIP_F32_BULK problem)");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->d > 64) {
      set_error("gprhip_acquire: at most 64 point dimensions on the kernel side (d)");
      throw HipFail{ST_BAD_ARG};
    }
    if (on_device ? ld != p->D : ld < p->D) {
      set_error("gprhip_acquire: bad ld (need ld == D for device buffers, ld >= D for host buffers)");
      throw HipFail{ST_BAD_ARG};
    }
    if (dvalues && (on_device ? ldg != p->D : ldg < p->D)) {
      set_error("gprhip_acquire: bad ldg (need ldg == D for device buffers, ldg >= D for host buffers)");
      throw HipFail{ST_BAD_ARG};
    }
    do_acquire(p, acq, test_inputs, ld, nt, values, dvalues, ldg, means, variances, top_k, top_index, top_values, top_dvalues,
               on_device);
  }, p);
}

int gprhip_acquire_max_value(gprhip_problem* p, const double* extremes, int n_extremes, int maximise, double var_floor,
                             const double* test_inputs, int64_t ld, int64_t nt, double* values, double* dvalues, int64_t ldg,
                             double* means, double* variances, int top_k, int64_t* top_index, double* top_values,
                             double* top_dvalues, int on_device) {
  return guarded([&] {
    auto refuse = [](const char* why) {
      set_error(std::string("gprhip_acquire_max_value: ") + why);
      throw HipFail{ST_BAD_ARG};
    };
    if (n_extremes < 1 || n_extremes > GPRHIP_MAX_EXTREMES) refuse("n_extremes must lie in 1 .. GPRHIP_MAX_EXTREMES (64)");
    if (!extremes) refuse("invalid arguments (extremes is NULL)");
    for (int j = 0; j < n_extremes; ++j)
      if (!std::isfinite(extremes[j])) refuse("the extremes must be finite");
    if (!(var_floor > 0.0) || !std::isfinite(var_floor)) refuse("var_floor must be positive and finite");
    if (top_k < 0 || top_k > GPRHIP_MAX_TOP_K) refuse("top_k must lie in 0 .. GPRHIP_MAX_TOP_K (64)");
    if (top_k > 0 && !top_index) refuse("top_k > 0 needs top_index");
    if (!values && !dvalues && !means && !variances && top_k == 0)
      refuse("nothing is requested (the four outputs are NULL and top_k is 0)");
    if (!p || !test_inputs || nt < 1) refuse("invalid arguments");
    if (p->f32) refuse("the prediction gradient is evaluated in fp64 only (GPRHIP_F32_BULK problem)");
    if (p->d > 64) refuse("at most 64 point dimensions on the kernel side (d)");
    if (on_device ? ld != p->D : ld < p->D) refuse("bad ld (need ld == D for device buffers, ld >= D for host buffers)");
    if (dvalues && (on_device ? ldg != p->D : ldg < p->D))
      refuse("bad ldg (need ldg == D for device buffers, ldg >= D for host buffers)");
    do_acquire_max_value(p, extremes, n_extremes, maximise, var_floor, test_inputs, ld, nt, values, dvalues, ldg, means, variances,
                         top_k, top_index, top_values, top_dvalues, on_device);
  }, p);
}

// what gprhip_acquire_refine and gprhip_sample_paths_refine refuse of the options, the number of starts and the outputs ...
void check_refine_options(const char* fn, const gprhip_refine_options* opt, int64_t ns, bool any_output) {
  auto refuse = [&](const std::string& why) {
    set_error(std::string(fn) + ": " + why);
    throw HipFail{ST_BAD_ARG};
  };
  if (!opt) refuse("invalid arguments (opt is NULL)");
  if (opt->max_evals < 1 || opt->max_evals > GPRHIP_REFINE_MAX_EVALS) refuse("max_evals must lie in 1 .. GPRHIP_REFINE_MAX_EVALS (1000)");
  if (!(opt->step0 > 0.0 && opt->step0 <= 1.0)) refuse("step0 must lie in (0, 1]");
  if (!(opt->c1 >= 0.0 && opt->c1 < 1.0)) refuse("c1 must lie in [0, 1)");
  if (!(opt->shrink > 0.0 && opt->shrink < 1.0)) refuse("shrink must lie in (0, 1)");
  if (!(opt->grow >= 1.0) || !std::isfinite(opt->grow)) refuse("grow must be finite and at least 1");
  if (!(opt->xtol >= 0.0) || !std::isfinite(opt->xtol)) refuse("xtol must be finite and not negative");
  if (ns < 1 || ns > GPRHIP_REFINE_MAX_STARTS) refuse("ns must lie in 1 .. GPRHIP_REFINE_MAX_STARTS (4096)");
  if (!any_output) refuse("nothing is requested (all outputs are NULL)");
}

// ... and of the leading dimensions, the box and the scale (p, lower and upper are not NULL)
void check_refine_box(const char* fn, const gprhip_problem* p, const double* lower, const double* upper, const double* scale,
                      int64_t ld, const double* x_out, int64_t ldx, const double* dvalues, int64_t ldg, int on_device) {
  auto refuse = [&](const std::string& why) {
    set_error(std::string(fn) + ": " + why);
    throw HipFail{ST_BAD_ARG};
  };
  const int D = p->D;
  if (on_device ? ld != D : ld < D) refuse("bad ld (need ld == D for device buffers, ld >= D for host buffers)");
  if (x_out && (on_device ? ldx != D : ldx < D)) refuse("bad ldx (need ldx == D for device buffers, ldx >= D for host buffers)");
  if (dvalues && (on_device ? ldg != D : ldg < D)) refuse("bad ldg (need ldg == D for device buffers, ldg >= D for host buffers)");
  for (int k = 0; k < D; ++k) {
    if (!std::isfinite(lower[k]) || !std::isfinite(upper[k]) || !(lower[k] < upper[k])) refuse("lower and upper must be finite with lower < upper");
    if (scale && (!(scale[k] > 0.0) || !std::isfinite(scale[k]))) refuse("scale must be positive and finite");
  }
}

// the starts on the host, [ns][D]; a non-finite one is refused.  Called after the model-state checks: the starts of a device
// call are read back here, and a refused call enqueues nothing
std::vector<double> refine_starts(const char* fn, gprhip_problem* p, const double* starts, int64_t ld, int64_t ns, int on_device) {
  const int D = p->D;
  std::vector<double> hs((size_t)ns * D);
  if (on_device) {
    GPR_HIP(hipSetDevice(p->device));
    GPR_HIP(hipMemcpy(hs.data(), starts, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
  } else {
    for (int64_t i = 0; i < ns; ++i) std::copy(starts + i * ld, starts + i * ld + D, hs.begin() + i * D);
  }
  for (double v : hs)
    if (!std::isfinite(v)) {
      set_error(std::string(fn) + ": the starts must be finite");
      throw HipFail{ST_BAD_ARG};
    }
  return hs;
}

int gprhip_acquire_refine(gprhip_problem* p, const gprhip_acquisition* acq, const gprhip_refine_options* opt, const double* lower,
                          const double* upper, const double* scale, const double* starts, int64_t ld, int64_t ns, double* x_out,
                          int64_t ldx, double* values, double* dvalues, int64_t ldg, int* evals, int* accepted, int* status,
                          double* trace, int on_device) {
  return guarded([&] {
    const char* const fn = "gprhip_acquire_refine";
    auto refuse = [&](const std::string& why) {
      set_error(std::string(fn) + ": " + why);
      throw HipFail{ST_BAD_ARG};
    };
    check_acquisition(fn, acq);
    check_refine_options(fn, opt, ns, x_out || values || dvalues || evals || accepted || status || trace);
    if (!p || !starts || !lower || !upper) refuse("invalid arguments");
    if (p->f32) refuse("the prediction gradient is evaluated in fp64 only (GPRHIP_F32_BULK problem)");
    if (p->d > 64) refuse("at most 64 point dimensions on the kernel side (d)");
    check_refine_box(fn, p, lower, upper, scale, ld, x_out, ldx, dvalues, ldg, on_device);
    // the model state before the starts are read back from the device: a refused call enqueues nothing
    need_posterior_state(p, fn, "predict from", true, acq_wants_var(acq), true,
                         "means and their gradients are available after the next gprhip_eval");
    std::vector<double> hs = refine_starts(fn, p, starts, ld, ns, on_device);
    do_acquire_refine(p, fn, acq, nullptr, nullptr, opt, lower, upper, scale, starts, hs, ns, x_out, ldx, values, dvalues, ldg, evals,
                      accepted, status, trace, on_device);
  }, p);
}

int gprhip_acquire_max_value_refine(gprhip_problem* p, const double* extremes, int n_extremes, int maximise, double var_floor,
                                    const gprhip_refine_options* opt, const double* lower, const double* upper,
                                    const double* scale, const double* starts, int64_t ld, int64_t ns, double* x_out,
                                    int64_t ldx, double* values, double* dvalues, int64_t ldg, int* evals, int* accepted,
                                    int* status, double* trace, int on_device) {
  return guarded([&] {
    const char* const fn = "gprhip_acquire_max_value_refine";
    auto refuse = [&](const std::string& why) {
      set_error(std::string(fn) + ": " + why);
      throw HipFail{ST_BAD_ARG};
    };
    if (n_extremes < 1 || n_extremes > GPRHIP_MAX_EXTREMES) refuse("n_extremes must lie in 1 .. GPRHIP_MAX_EXTREMES (64)");
    if (!extremes) refuse("invalid arguments (extremes is NULL)");
    for (int j = 0; j < n_extremes; ++j)
      if (!std::isfinite(extremes[j])) refuse("the extremes must be finite");
    if (!(var_floor > 0.0) || !std::isfinite(var_floor)) refuse("var_floor must be positive and finite");
    check_refine_options(fn, opt, ns, x_out || values || dvalues || evals || accepted || status || trace);
    if (!p || !starts || !lower || !upper) refuse("invalid arguments");
    if (p->f32) refuse("the prediction gradient is evaluated in fp64 only (GPRHIP_F32_BULK problem)");
    if (p->d > 64) refuse("at most 64 point dimensions on the kernel side (d)");
    check_refine_box(fn, p, lower, upper, scale, ld, x_out, ldx, dvalues, ldg, on_device);
    // the model state before the starts are read back from the device: a refused call enqueues nothing
    need_posterior_state(p, fn, "predict from", true, true, true,
                         "means and their gradients are available after the next gprhip_eval");
    std::vector<double> hs = refine_starts(fn, p, starts, ld, ns, on_device);
    MvArgs mv;
    mv.n = n_extremes; mv.s = maximise ? 1.0 : -1.0; mv.var_floor = var_floor; mv.extremes = nullptr; mv.values = nullptr;
    do_acquire_refine(p, fn, nullptr, &mv, extremes, opt, lower, upper, scale, starts, hs, ns, x_out, ldx, values, dvalues, ldg,
                      evals, accepted, status, trace, on_device);
  }, p);
}

int gprhip_sample_paths_refine(gprhip_problem* p, const double* z, int64_t ldz, int nd, int maximise,
                               const gprhip_refine_options* opt, const double* lower, const double* upper, const double* scale,
                               const double* starts, int64_t ld, int64_t ns, const int* draw_of, double* x_out, int64_t ldx,
                               double* values, double* dvalues, int64_t ldg, int* evals, int* accepted, int* status,
                               double* trace, int on_device) {
  return guarded([&] {
    const char* const fn = "gprhip_sample_paths_refine";
    auto refuse = [&](const std::string& why) {
      set_error(std::string(fn) + ": " + why);
      throw HipFail{ST_BAD_ARG};
    };
    if (nd < 1 || nd > GPRHIP_MAX_DRAWS) refuse("nd must lie in 1 .. GPRHIP_MAX_DRAWS (64)");
    check_refine_options(fn, opt, ns, x_out || values || dvalues || evals || accepted || status || trace);
    if (!p || !z || !starts || !draw_of || !lower || !upper) refuse("invalid arguments");
    if (p->f32) refuse("sample paths are evaluated in fp64 only (GPRHIP_F32_BULK problem)");
    if (p->d > 64) refuse("at most 64 point dimensions on the kernel side (d)");
    if (ldz < p->m) refuse("bad ldz (need ldz >= m)");
    check_refine_box(fn, p, lower, upper, scale, ld, x_out, ldx, dvalues, ldg, on_device);
    for (int64_t i = 0; i < ns; ++i)
      if (draw_of[i] < 0 || draw_of[i] >= nd) refuse("draw_of must lie in 0 .. nd - 1");
    need_posterior_state(p, fn, "draw from", true, true, true, "draws are available after the next gprhip_eval");
    std::vector<double> hs = refine_starts(fn, p, starts, ld, ns, on_device);
    do_sample_paths_refine(p, z, ldz, nd, maximise, opt, lower, upper, scale, hs, ns, draw_of, x_out, ldx, values, dvalues, ldg,
                           evals, accepted, status, trace, on_device);
  }, p);
}

int gprhip_sample_paths(gprhip_problem* p, const double* z, int64_t ldz, int ns, const double* test_inputs, int64_t ld, int64_t nt,
                        const double* eps, int64_t lde, int predictive, double* samples, int64_t lds, int maximise, int top_k,
                        int64_t* top_index, double* top_values, double* top_dvalues, int on_device) {
  return guarded([&] {
    SpCall c;
    c.have_p = p != nullptr;
    if (p) {
      c.D = p->D; c.d = p->d; c.m = p->m; c.f32 = p->f32;
    }
    c.z = z; c.ldz = ldz; c.ns = ns; c.test_inputs = test_inputs; c.ld = ld; c.nt = nt; c.eps = eps; c.lde = lde;
    c.samples = samples; c.lds = lds; c.top_k = top_k; c.top_index = top_index; c.on_device = on_device;
    if (const char* why = sp_check_args(c)) {
      set_error(std::string("gprhip_sample_paths: ") + why);
      throw HipFail{ST_BAD_ARG};
    }
    do_sample_paths(p, z, ldz, ns, test_inputs, ld, nt, eps, lde, predictive, samples, lds, maximise, top_k, top_index,
                    top_values, top_dvalues, on_device);
  }, p);
}

int gprhip_train_stats(gprhip_problem* p, double* means, double* sums) {
  return guarded([&] {
    if (!p || !sums) {
      set_error("gprhip_train_stats: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    if (p->f32) do_train_stats<float>(p, means, sums);
    else do_train_stats<double>(p, means, sums);
  });
}

int gprhip_covariances(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int kind,
                       int predictive, double* cov) {
  return guarded([&] {
    if (!p || !test_inputs || !cov || nt < 1 || ld < p->D || (kind != 0 && kind != 1) || nt > (1 << 20)) {
      set_error("gprhip_covariances: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    do_covariances(p, test_inputs, ld, nt, kind, predictive, cov);
  });
}

int gprhip_cov_samples(gprhip_problem* p, const double* cov, int64_t ld, int64_t nt, double add_diag,
                       double jitter, const double* means, const double* z, int64_t ns, double* samples) {
  return guarded([&] {
    if (!p || !cov || !means || !z || !samples || nt < 1 || ns < 1 || ld < nt || nt > (1 << 20)) {
      set_error("gprhip_cov_samples: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    do_cov_samples(p, cov, ld, nt, add_diag, jitter, means, z, ns, samples);
  });
}

int gprhip_co_variance_coeffs(gprhip_problem* p, double* chol_km, double* r_mat) {
  return guarded([&] {
    if (!p) {
      set_error("gprhip_co_variance_coeffs: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    do_co_variance_coeffs(p, chol_km, r_mat);
  });
}

int gprhip_load_predictor(gprhip_problem* p, const gprhip_hypers* h, const double* coeffs, const double* chol_km,
                          const double* r_mat) {
  return guarded([&] {
    if (!p || !h || (chol_km == nullptr) != (r_mat == nullptr) || (!coeffs && !chol_km)) {
      set_error("gprhip_load_predictor: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    do_load_predictor(p, h, coeffs, chol_km, r_mat);
  });
}

int gprhip_observe(gprhip_problem* p, const double* inputs, int64_t ld, const double* targets, int k, double* dlog_evidence,
                   int on_device) {
  return guarded([&] {
    const char* why = nullptr;
    if (!p || !inputs) why = "invalid arguments (problem or inputs NULL)";
    else if (k < 1 || k > GPRHIP_MAX_OBSERVE) why = "k must lie in 1 .. GPRHIP_MAX_OBSERVE (64)";
    else if (on_device ? ld != p->D : ld < p->D) why = "bad ld (need ld == D for device buffers, ld >= D for host buffers)";
    else if (p->f32) why = "the update runs in fp64 only (GPRHIP_F32_BULK problem)";
    else if (p->d > 64) why = "at most 64 point dimensions on the kernel side (d)";
    if (why) {
      set_error(std::string("gprhip_observe: ") + why);
      throw HipFail{ST_BAD_ARG};
    }
    need_observe_state(p, "gprhip_observe");
    if ((targets == nullptr) != (p->h.model_only != 0)) {
      set_error(p->h.model_only ? "gprhip_observe: the model state has no targets (model_only, or a predictor loaded without "
                                  "coefficients): targets must be NULL"
                                : "gprhip_observe: the model state has targets: targets must not be NULL");
      throw HipFail{ST_BAD_ARG};
    }
    do_observe(p, inputs, ld, targets, k, dlog_evidence, on_device);
  }, p);
}

int gprhip_posterior_save(gprhip_problem* p) {
  return guarded([&] {
    if (!p) {
      set_error("gprhip_posterior_save: NULL problem");
      throw HipFail{ST_BAD_ARG};
    }
    do_posterior_save(p);
  });
}

int gprhip_posterior_restore(gprhip_problem* p) {
  return guarded([&] {
    if (!p) {
      set_error("gprhip_posterior_restore: NULL problem");
      throw HipFail{ST_BAD_ARG};
    }
    do_posterior_restore(p);
  });
}

int64_t gprhip_observed_count(const gprhip_problem* p) { return p ? p->n_observed : 0; }

int gprhip_condition(gprhip_problem* p, double* cond_km, double* coeff_error_bound) {
  return guarded([&] {
    if (!p) {
      set_error("gprhip_condition: NULL problem");
      throw HipFail{ST_BAD_ARG};
    }
    need_model(p, "gprhip_condition");
    const double c = condition_km(p);
    if (cond_km) *cond_km = c;
    if (coeff_error_bound) *coeff_error_bound = c * (p->f32 ? 5.9604644775390625e-8 : 1.1102230246251565e-16);
  });
}

int gprhip_sync(gprhip_problem* p) {
  return guarded([&] {
    if (!p) {
      set_error("gprhip_sync: NULL problem");
      throw HipFail{ST_BAD_ARG};
    }
    GPR_HIP(hipSetDevice(p->device));
    GPR_HIP(hipStreamSynchronize(p->stream));
  });
}

void* gprhip_stream(gprhip_problem* p) { return p ? (void*)p->stream : nullptr; }

int gprhip_set_timing(gprhip_problem* p, int level) {
  return guarded([&] {
    if (!p || level < 0 || level > 2) {
      set_error("gprhip_set_timing: invalid arguments");
      throw HipFail{ST_BAD_ARG};
    }
    p->timer.kernel = level >= 1;
    p->timer.on = level >= 2;
  });
}

int gprhip_debug_fetch(gprhip_problem* p, const char* name, double* out, int64_t len) {
  return guarded([&] {
    if (!p || !out) {
      set_error("gprhip_debug_fetch: NULL argument");
      throw HipFail{ST_BAD_ARG};
    }
    const double* src = nullptr;
    int64_t avail = 0;
    std::string nm = name ? name : "";
    // per-row vectors are stored chunk by chunk with padding; only nchunks == 1 keeps them contiguous
    if (nm == "r") { src = p->r; avail = p->n; }
    else if (nm == "is") { src = p->is; avail = p->n; }
    else if (nm == "v") { src = p->v; avail = p->n; }
    else if (nm == "w") { src = p->w; avail = p->n; }
    else if (nm == "t") { src = p->tvec; avail = p->m; }
    else if (nm == "w_mat" || nm == "x_rows") {
      // the gradient factors of Trained.prepare_hyper (lib/fitc_gp.ml:1192-1207) as the last gradient evaluation left
      // them: W (m x m, symmetric, Fortran) and the first rows of X (Fortran rows x m) -- with "km", "knm_rows" and "v"
      // they let a test contract finite differences of the covariance matrices exactly as Shared.calc_log_evidence does
      // (lib/fitc_gp.ml:1005-1021)
      need_model(p, "gprhip_debug_fetch");
      if (!p->want_grad) {
        set_error("gprhip_debug_fetch: the last evaluation was evidence-only");
        throw HipFail{ST_STATE};
      }
      GPR_HIP(hipSetDevice(p->device));
      const int m = p->m, mp = p->mp;
      if (nm == "w_mat") {
        if (len < (int64_t)m * m) {
          set_error("gprhip_debug_fetch: \"w_mat\" needs m*m doubles");
          throw HipFail{ST_BAD_ARG};
        }
        std::vector<double> h((size_t)mp * mp);
        GPR_HIP(hipMemcpyAsync(h.data(), p->wmat, h.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        GPR_HIP(hipStreamSynchronize(p->stream));
        for (int c = 0; c < m; ++c)
          for (int r = 0; r < m; ++r) out[(size_t)c * m + r] = h[(size_t)r * mp + c];
        return;
      }
      const int64_t rows = len / m;
      if (!p->x_last || p->f32 || rows < 1 || rows > p->rows_of(0)) {
        set_error("gprhip_debug_fetch: \"x_rows\" needs an fp64 problem whose rows fit one chunk, and len = rows*m");
        throw HipFail{ST_BAD_ARG};
      }
      std::vector<double> h((size_t)rows * mp);
      GPR_HIP(hipMemcpyAsync(h.data(), p->x_last, h.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
      GPR_HIP(hipStreamSynchronize(p->stream));
      for (int c = 0; c < m; ++c)
        for (int64_t r = 0; r < rows; ++r) out[(size_t)c * rows + r] = h[(size_t)r * mp + c];
      return;
    }
    else if (nm == "km" || nm == "knm_rows") {
      // element-wise pins of the covariance kernels (the counterpart of Test.check_deriv_hyper's matrix checks,
      // lib/fitc_gp.ml:1223-1396): K_m as stored, and the first rows of K_nm rebuilt by the chunk builder
      need_model(p, "gprhip_debug_fetch");
      GPR_HIP(hipSetDevice(p->device));
      const int m = p->m, mp = p->mp;
      if (nm == "km") {
        if (len < (int64_t)m * m) {
          set_error("gprhip_debug_fetch: \"km\" needs m*m doubles");
          throw HipFail{ST_BAD_ARG};
        }
        std::vector<double> h((size_t)mp * mp);
        GPR_HIP(hipMemcpyAsync(h.data(), p->km, h.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        GPR_HIP(hipStreamSynchronize(p->stream));
        for (int c = 0; c < m; ++c)
          for (int r = 0; r < m; ++r) out[(size_t)c * m + r] = (r <= c) ? h[(size_t)r * mp + c] : 0.0;
        return;
      }
      const int64_t rows = len / m;
      if (rows < 1 || rows > p->rows_of(0) || !p->have_inputs) {
        set_error("gprhip_debug_fetch: \"knm_rows\" needs len = rows*m with 1 <= rows <= the first row chunk");
        throw HipFail{ST_BAD_ARG};
      }
      void* const kbuf = (p->x_last == p->bufA) ? p->bufB : p->bufA;  // the chunk buffer that does not hold X
      std::vector<double> h((size_t)rows * mp);
      if (p->f32) {
        cov_chunk<float>(p, 0, static_cast<float*>(kbuf));
        std::vector<float> hf((size_t)rows * mp);
        GPR_HIP(hipMemcpyAsync(hf.data(), kbuf, hf.size() * sizeof(float), hipMemcpyDeviceToHost, p->stream));
        GPR_HIP(hipStreamSynchronize(p->stream));
        for (size_t i = 0; i < hf.size(); ++i) h[i] = hf[i];
      } else {
        cov_chunk<double>(p, 0, static_cast<double*>(kbuf));
        GPR_HIP(hipMemcpyAsync(h.data(), kbuf, h.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        GPR_HIP(hipStreamSynchronize(p->stream));
      }
      for (int c = 0; c < m; ++c)
        for (int64_t r = 0; r < rows; ++r) out[(size_t)c * rows + r] = h[(size_t)r * mp + c];
      return;
    }
    else if (nm == "uinv" || nm == "rinv") {
      // U^-1 and R~^-1 as the posterior calls read them (after an evaluation of one or several target vectors, or a loaded
      // predictor with co-variance coefficients): with "t" every posterior output is a short contraction of operands a test
      // holds exactly.  A copy only; nothing of the model state changes.
      need_model(p, "gprhip_debug_fetch");
      if (!p->have_factors) {
        set_error("gprhip_debug_fetch: \"" + nm + "\" needs the factors of an evaluation, or of a predictor loaded with "
                  "co-variance coefficients (chol_km, r_mat)");
        throw HipFail{ST_STATE};
      }
      if (len < (int64_t)p->m * p->m) {
        set_error("gprhip_debug_fetch: \"" + nm + "\" needs m*m doubles");
        throw HipFail{ST_BAD_ARG};
      }
      GPR_HIP(hipSetDevice(p->device));
      fetch_upper_fortran(p, nm == "uinv" ? p->uinv : p->rinv, out);
      return;
    }
    else if (nm == "rtil" || nm == "bvec") {
      // R~ and b = R~^-T c~ as gprhip_observe reads and updates them, under the state conditions of "rinv" ("bvec": a state with
      // targets; a loaded predictor forms b = R~ (U t) here as the first gprhip_observe would).  With "uinv" they are the whole
      // pre-state of an update.
      need_model(p, "gprhip_debug_fetch");
      if (!p->have_factors || (nm == "bvec" && (p->h.model_only || p->multi_state))) {
        set_error("gprhip_debug_fetch: \"" + nm + "\" needs the factors of an evaluation, or of a predictor loaded with "
                  "co-variance coefficients (chol_km, r_mat)" + (nm == "bvec" ? ", and a single target vector" : ""));
        throw HipFail{ST_STATE};
      }
      if (len < (nm == "rtil" ? (int64_t)p->m * p->m : (int64_t)p->m)) {
        set_error("gprhip_debug_fetch: \"" + nm + "\" needs " + (nm == "rtil" ? "m*m" : "m") + " doubles");
        throw HipFail{ST_BAD_ARG};
      }
      GPR_HIP(hipSetDevice(p->device));
      if (nm == "rtil") {
        fetch_upper_fortran(p, p->bmat, out);
        return;
      }
      if (!p->have_b) {
        DevBuf tmp;
        ensure_b(p, tmp.get<double>(p->mp));
        GPR_HIP(hipStreamSynchronize(p->stream));
      }
      GPR_HIP(hipMemcpyAsync(out, p->bvec, (size_t)p->m * sizeof(double), hipMemcpyDeviceToHost, p->stream));
      GPR_HIP(hipStreamSynchronize(p->stream));
      return;
    }
    else if (nm == "pg_m") {
      // M = U^-1 (I - R~^-1 R~^-T) U^-T as pg_chunk's product G = K M reads it (ensure_predict_m), full.  With "t", "uinv" and
      // "rinv" it makes every output of gprhip_predict_input_grad a short contraction of operands a test holds exactly.
      // A copy only; nothing of the model state changes.
      need_model(p, "gprhip_debug_fetch");
      if (!p->pg_m || !p->pg_m_valid) {
        set_error("gprhip_debug_fetch: \"pg_m\" needs M of the current model state: it is formed by the first "
                  "gprhip_predict_input_grad or gprhip_acquire call that asks for a variance part with K and G in memory");
        throw HipFail{ST_STATE};
      }
      const int64_t m = p->m, mp = p->mp;
      if (len < m * m) {
        set_error("gprhip_debug_fetch: \"pg_m\" needs m*m doubles");
        throw HipFail{ST_BAD_ARG};
      }
      const int64_t w = len >= mp * mp ? mp : m;  // mp*mp doubles: the padded matrix as it is stored
      GPR_HIP(hipSetDevice(p->device));
      std::vector<double> h((size_t)mp * mp);
      GPR_HIP(hipMemcpyAsync(h.data(), p->pg_m, h.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
      GPR_HIP(hipStreamSynchronize(p->stream));
      for (int64_t c = 0; c < w; ++c)
        for (int64_t r = 0; r < w; ++r) out[(size_t)(c * w + r)] = h[(size_t)(r * mp + c)];
      return;
    }
    else if (nm == "sp_a") {
      // the weights A = t 1^T + U^-1 (R~^-1 Z) of the last gprhip_sample_paths / gprhip_sample_paths_refine call, as
      // sample_paths_kernel, path_grad_at_kernel and path_eval read them: the second half of sp_coef, [mp][64].  With "t",
      // "uinv" and "rinv" the weights are a short contraction of operands a test holds exactly, and every output of the two
      // calls one of the weights.  A copy only; nothing of the model state changes.
      need_model(p, "gprhip_debug_fetch");
      if (!p->sp_coef || p->sp_ns_last < 1) {
        set_error("gprhip_debug_fetch: \"sp_a\" needs the weights of a gprhip_sample_paths or gprhip_sample_paths_refine "
                  "call on the current model state");
        throw HipFail{ST_STATE};
      }
      const int64_t m = p->m, mp = p->mp, ns = p->sp_ns_last;
      if (len < m * ns) {
        set_error("gprhip_debug_fetch: \"sp_a\" needs m doubles for each draw of that call");
        throw HipFail{ST_BAD_ARG};
      }
      const bool padded = len >= mp * SP_MAX_DRAWS;  // mp*64 doubles: the padded block as it is stored
      const int64_t rows = padded ? mp : m, cols = padded ? SP_MAX_DRAWS : ns;
      GPR_HIP(hipSetDevice(p->device));
      std::vector<double> h((size_t)mp * SP_MAX_DRAWS);
      GPR_HIP(hipMemcpyAsync(h.data(), p->sp_coef + mp * SP_MAX_DRAWS, h.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
      GPR_HIP(hipStreamSynchronize(p->stream));
      for (int64_t c = 0; c < cols; ++c)
        for (int64_t r = 0; r < rows; ++r) out[(size_t)(c * rows + r)] = h[(size_t)(r * SP_MAX_DRAWS + c)];
      return;
    }
    else {
      set_error("gprhip_debug_fetch: unknown name");
      throw HipFail{ST_BAD_ARG};
    }
    if (len > avail) len = avail;
    GPR_HIP(hipSetDevice(p->device));
    GPR_HIP(hipStreamSynchronize(p->stream));
    if (avail == p->m || p->nchunks == 1) {
      GPR_HIP(hipMemcpy(out, src, (size_t)len * sizeof(double), hipMemcpyDeviceToHost));
    } else {
      for (int c = 0; c < p->nchunks; ++c) {
        int64_t lo = (int64_t)c * p->chunk;
        if (lo >= len) break;
        int64_t cnt = std::min<int64_t>(p->rows_of(c), len - lo);
        GPR_HIP(hipMemcpy(out + lo, src + lo, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost));
      }
    }
  });
}

int gprhip_last_timings(gprhip_problem* p, const char** names, float* ms, int cap) {
  if (!p || !names || !ms) return 0;
  int n = (int)std::min<size_t>(p->tnames.size(), (size_t)cap);
  for (int i = 0; i < n; ++i) {
    names[i] = p->tnames[i].c_str();
    ms[i] = p->tms[i];
  }
  return n;
}

}  // extern "C"
