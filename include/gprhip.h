/* gprhip -- C ABI of the MI355X-native FITC/SPGP core (libgprhip.so).
 *
 * Drop-in boundary for one path of mmottl/gpr: one evaluation of the FITC log evidence and its
 * full hyper-parameter gradient, i.e. what Gpr.Fitc_gp.Make_deriv(Cov_se_iso.Deriv).FITC /
 * (Cov_se_fat.Deriv) compute in
 *     Deriv.Inducing.calc -> Deriv.Inputs.calc -> Deriv.Model.calc -> Deriv.Trained.calc ->
 *     Trained.calc_log_evidence_sigma2 -> Trained.prepare_hyper -> Trained.calc_log_evidence (per hyper)
 * (reference lib/fitc_gp.ml:881-888, :902-911, :1051-1078, :1158-1207, :1005-1021; driven by
 * multim_dcommon lib/fitc_gp.ml:1612-1636).  The reference has no native stubs of its own for this
 * path (it reaches C only through Lacaml); these entry points are what an OCaml stub layer, or the
 * ctypes host layer in gpr_amd/, binds.  See INTEGRATION.md for the OCaml `external` side.
 *
 * Conventions
 *   - All matrices cross the boundary as raw double pointers in the reference's own layout:
 *     Fortran (column-major) Bigarrays -- inputs D x n (one point per column), inducing d x m,
 *     tproj D x d (lib/interfaces.ml:190-195, bin/ocaml_gpr.ml:196-202).
 *   - Host pointers are borrowed for the duration of the call only.
 *   - Every function returns 0 on success or a GPRHIP_E* code; gprhip_last_error() gives the
 *     message (thread-local).  No C++ exception crosses the boundary.
 *   - A context/problem must not be used from two host threads at once.  The one exception is lifetime: the destroy
 *     calls of a context and of its sharded problems may come from different threads in any order (finalisers of a
 *     garbage-collected host on another domain); that bookkeeping is guarded inside the library.
 */
#ifndef GPRHIP_H
#define GPRHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  GPRHIP_OK = 0,
  GPRHIP_EBADARG = 1,    /* reference: Failure / Invalid_argument on argument checks            */
  GPRHIP_ENOTPOSDEF = 2, /* reference: Lacaml Failure on potrf info > 0                          */
  GPRHIP_EHIP = 3,       /* HIP runtime error                                                    */
  GPRHIP_EOOM = 4,       /* device out of memory                                                 */
  GPRHIP_ESTATE = 5,     /* call sequence violated (e.g. pass2 before pass1)                     */
  GPRHIP_ECOMM = 6,      /* RCCL could not be loaded / initialised, or a collective failed       */
  GPRHIP_EPRECISION = 7  /* fp32-bulk mean coefficients refused: K_m too ill-conditioned for them */
};

enum { GPRHIP_COV_SE_ISO = 0, GPRHIP_COV_SE_FAT = 1 }; /* lib/cov_se_iso.ml, lib/cov_se_fat.ml */

/* Arithmetic of the n x m contractions.  The reference is fp64 only (Lacaml.D, lib/fitc_gp.ml:23).
 *   GPRHIP_F64      : everything fp64 (reference parity).
 *   GPRHIP_F32_BULK : K_nm and every n x m intermediate stored in fp32, n x m x m contractions on the
 *                     fp32 MFMA with split-K partial sums combined in fp64; covariance evaluation,
 *                     row reductions, and all m x m factorisations/solves stay fp64 (BASELINE.json
 *                     config 3).  Agreement with the fp64 reference is ~1e-5 relative. */
enum { GPRHIP_F64 = 0, GPRHIP_F32_BULK = 1 };

typedef struct gprhip_problem gprhip_problem;

/* Number of visible HIP devices (does not initialise a device). */
int gprhip_device_count(int* count);

/* Device memory one shard of a problem holds, in bytes (pure arithmetic, no device): what gprhip_problem_create allocates
 * plus the resident V = K_nm U^-1 store the first evaluation adds.  gprhip_problem_create compares `total` with the free
 * memory of its device BEFORE allocating anything and returns GPRHIP_EOOM with these figures in the message when the shard
 * cannot fit (nothing is spilled to the host); GPRHIP_VERBOSE=1 prints the plan of every problem created.
 * Replaces: nothing -- the reference allocates Bigarrays as it goes (lib/fitc_gp.ml:105-229) and dies in caml_ba_alloc. */
typedef struct {
  int64_t total;            /* sum of the fields below except k_store_optional */
  int64_t v_store;          /* V = K_nm U^-1 of all rows of the shard (n rounded up to chunks x m rounded up to 128) */
  int64_t chunk_buffers;    /* two row-chunk temporaries (K / Q' / X~ / X) and the GEMM epilogues' per-row partials */
  int64_t slices;           /* split-K partial sums of the SYRK-shaped launches */
  int64_t inputs;           /* training inputs, targets, projected inputs (Cov_se_fat) */
  int64_t row_vectors;      /* r, 1/s, y/s, w, v (, E row sums) */
  int64_t mxm;              /* the m x m matrices: K_m, U, U^-1, B~, R~^-1, B~^-1, W~, W, R^-1, scratch */
  int64_t rest;             /* exchange buffers, gradient / trace partials, result block */
  int64_t k_store_optional; /* Cov_se_fat: a second n x m matrix (K_nm kept for the gradient pass), taken only while it
                               leaves 4 GB free and stays below 40 % of the device; not in `total` */
  int64_t chunk_rows;       /* rows per chunk the problem will use */
  int64_t kslices;          /* split-K slices reserved */
} gprhip_memory_plan_t;
int gprhip_memory_plan(int cov_kind, int precision, int64_t n, int D, int d, int m, int64_t chunk_rows,
                       gprhip_memory_plan_t* plan);

/* Create the device-resident state for one shard of a FITC problem on HIP device `device`:
 *   n  training points held by this shard, D input dimension, d kernel-space dimension
 *   (d == D for Cov_se_iso; Cov_se_fat: d = Params.d, the tproj target dimension), m inducing points.
 *   chunk_rows: rows of K_nm processed per streaming step (0 = library default).
 * Replaces: the Bigarray allocations spread over Eval_inputs / Eval_model (lib/fitc_gp.ml:105-229). */
int gprhip_problem_create(int device, int cov_kind, int64_t n, int D, int d, int m, int64_t chunk_rows,
                          gprhip_problem** out);
int gprhip_problem_create_ex(int device, int cov_kind, int precision, int64_t n, int D, int d, int m,
                             int64_t chunk_rows, gprhip_problem** out);
void gprhip_problem_destroy(gprhip_problem* p);

/* Training inputs (Fortran D x n, leading dimension ld >= D) and targets (n): copied to the device.
 * Replaces: Spec.Inputs.t / targets arguments of Deriv.Inputs.calc and Deriv.Trained.calc. */
int gprhip_set_inputs(gprhip_problem* p, const double* inputs, int64_t ld);
int gprhip_set_targets(gprhip_problem* p, const double* targets);
/* Same, from device pointers (inputs already resident in HBM; point-major [n][D], contiguous). */
int gprhip_set_inputs_device(gprhip_problem* p, const double* d_inputs);
int gprhip_set_targets_device(gprhip_problem* p, const double* d_targets);

/* ---- Several target vectors on one model ---------------------------------------------------------------------------
 * The reference separates Model (kernel, inducing points, inputs, sigma2) from Trained (a model plus ONE target vector) so
 * that one model serves many target vectors: everything expensive depends on the model only, a target vector adds
 * O(n m) work (lib/fitc_gp.ml:279-292, :1158-1207).  These three calls evaluate up to GPRHIP_MAX_TARGETS target vectors
 * against one model in ONE evaluation -- multi-output regression with shared hyper-parameters: one GP per column, the
 * log evidence summed.  The gradient entries are linear in (v, W, X) (lib/fitc_gp.ml:1005-1021), so the model parts run
 * once and the two rank-1 target terms become rank-k terms.
 *
 *   gprhip_set_targets_many   Fortran n x k host matrix (ld >= n), 1 <= k <= GPRHIP_MAX_TARGETS; replaces any earlier target
 *                             MATRIX (the target vector of gprhip_set_targets is a different buffer and is kept).  Allocates
 *                             its n x k device buffers here, after comparing them with the free memory of the device:
 *                             GPRHIP_EOOM from that comparison leaves the problem as it was
 *                             (an allocation that fails all the same leaves it without a target matrix).
 *   gprhip_eval_targets       l2[k]; grad_sum[n_hypers] (want_grad != 0) = gradient of the SUMMED log evidence in the order of
 *                             gprhip_eval; coeffs (may be NULL) Fortran m x k, column j = Trained.calc_mean_coeffs of target
 *                             j.  l_j = l1 + l2[j]; l_sum = k l1 + sum l2; dl_dsigma2_sum likewise.  h->reuse_v is honoured.
 *   gprhip_predict_targets    means: Fortran nt x k = K_tm coeffs of the last gprhip_eval_targets (Means.calc per column).
 *
 * Contract
 *   - fp64, one device: a GPRHIP_F32_BULK problem, k out of range or h->model_only = 1 -> GPRHIP_EBADARG;
 *     gprhip_eval_targets before gprhip_set_targets_many, or gprhip_predict_targets without a completed
 *     gprhip_eval_targets before it -> GPRHIP_ESTATE.  Nothing is evaluated in either case.
 *   - gprhip_set_targets_many with the k of the last gprhip_eval_targets keeps that evaluation's coefficients for
 *     gprhip_predict_targets; with another k it discards them, and gprhip_predict_targets returns GPRHIP_ESTATE until the
 *     next gprhip_eval_targets (gprhip_predict means and gprhip_train_stats go on refusing as below).
 *   - After gprhip_eval_targets the MODEL state (U, R) is valid: gprhip_predict variances, gprhip_covariances,
 *     gprhip_co_variance_coeffs, gprhip_condition work.  The single-target state is not: gprhip_predict MEANS and
 *     gprhip_train_stats return GPRHIP_ESTATE until the next gprhip_eval -- never an answer for "some" column.
 *   - gprhip_set_targets / gprhip_eval are untouched and may be interleaved with these calls on one problem.
 *   - Every k (1 included) takes the engine row path whatever m is; results repeat bit for bit from run to run.
 *   - The staged / sharded calls do not take several targets (their exchange-1 buffer carries one c~; its length is ABI). */
#define GPRHIP_MAX_TARGETS 16
int gprhip_set_targets_many(gprhip_problem* p, const double* targets, int64_t ld, int k);
typedef struct {
  double l1;             /* Model.calc_log_evidence (the same for every target)      */
  double l_sum;          /* sum_j Trained.calc_log_evidence of target j              */
  double dl_dsigma2_sum; /* sum_j calc_log_evidence_sigma2 (0 unless want_grad != 0) */
  int64_t n_hypers;
  int k;
} gprhip_targets_result;

/* Hyper-parameters of one evaluation.
 *   log_ell    : Cov_se_iso.Params.log_ell (ignored for Cov_se_fat)          lib/cov_se_iso.ml:23-25
 *   log_sf2    : Params.log_sf2
 *   sigma2     : noise variance (>= 0, else GPRHIP_EBADARG: lib/fitc_gp.ml:148-149)
 *   inducing   : Fortran d x m inducing points (Spec.Inducing.t)
 *   tproj      : Fortran D x d projection (Cov_se_fat.Params.tproj) or NULL
 *   variational: 0 = Make_FITC_deriv (Standard), 1 = Make_variational_FITC_deriv  lib/fitc_gp.ml:262-263
 *   model_only : 1 = evidence/gradient of the model without targets (Deriv.Model.*), 0 = Trained.*
 *   jitter     : Utils.cholesky_jitter (lib/utils.ml:35); pass 1e-6 for the reference behaviour
 *   log_hetero_skedasticity : Cov_se_fat.Params.log_hetero_skedasticity (m entries) or NULL:
 *                exp() of it is added to diag(K_m)                             lib/cov_se_fat.ml:136-142
 *   log_multiscales_m05 : Cov_se_fat.Params.log_multiscales_m05 (Fortran d x m) or NULL: per inducing point
 *                and dimension a length scale exp(.)+0.5                        lib/cov_se_fat.ml:66-69, :115-134
 *   reuse_v    : 1 = only sigma2 (and targets) changed since the previous evaluation on this problem:
 *                K_nm, V = K_nm U^-1 and r are reused instead of recomputed -- Model.update_sigma2,
 *                lib/fitc_gp.ml:234-236, :1083-1090.  The caller guarantees kernel parameters and inducing
 *                points are unchanged (they are still passed and uploaded). */
typedef struct {
  double log_ell;
  double log_sf2;
  double sigma2;
  const double* inducing;
  const double* tproj;
  int variational;
  int model_only;
  double jitter;
  const double* log_hetero_skedasticity;
  const double* log_multiscales_m05;
  int reuse_v;
} gprhip_hypers;

/* Results.  Gradient order is the reference's Hyper.get_all order:
 *   Cov_se_iso: [Log_ell; Log_sf2; Inducing_hyper{ind=1,dim=1..d}; {ind=2,..}; ...]   lib/cov_se_iso.ml:188-202
 *   Cov_se_fat: [Log_sf2; Inducing_hyper (ind-major); Proj{big_dim,small_dim} (big-major);
 *                Log_hetero_skedasticity 1..m; Log_multiscale_m05 (ind-major)]  lib/cov_se_fat.ml:290-342
 * l1 = Model.calc_log_evidence, l = Trained.calc_log_evidence, dl_dsigma2 = calc_log_evidence_sigma2. */
typedef struct {
  double l1;
  double l2;
  double l;
  double dl_dsigma2;
  int64_t n_hypers;
} gprhip_result;

/* flags: bit 0 = tproj given, bit 1 = log_hetero_skedasticity given, bit 2 = log_multiscales_m05 given */
int64_t gprhip_n_hypers(const gprhip_problem* p, int flags);

/* One complete evaluation on one device (shard == whole problem).
 *   want_grad = 0: log evidence only (multim_f, lib/fitc_gp.ml:1601-1610)
 *   want_grad = 1: + dl_dsigma2 and grad[n_hypers] (multim_dcommon, lib/fitc_gp.ml:1612-1636)
 *   coeffs (m, may be NULL): Trained.calc_mean_coeffs (lib/fitc_gp.ml:294). */
int gprhip_eval(gprhip_problem* p, const gprhip_hypers* h, int want_grad, gprhip_result* res,
                double* grad, double* coeffs);
/* Several target vectors (see gprhip_set_targets_many above). */
int gprhip_eval_targets(gprhip_problem* p, const gprhip_hypers* h, int want_grad, gprhip_targets_result* res, double* l2,
                        double* grad_sum, double* coeffs);

/* ---- Gradient with respect to the training inputs -------------------------------------------------------------------
 * A gradient evaluation (want_grad = 1 semantics: res, grad, coeffs exactly as gprhip_eval returns them) that also returns
 * dl/dx for every training input -- what a caller needs when the inputs are themselves the output of something trainable
 * (a feature extractor in front of the GP, a learned input warping, latent inputs).  For the squared-exponential kernels
 * diag K_n and K_m do not depend on the training inputs: with E = X .* K_nm and p_r the point the kernel sees,
 *   dl/dp_rk = inv_ell2 sum_c E_rc (p_rk - z_ck),   dl/dx_r = tproj dl/dp_r   (Cov_se_fat with a projection)
 * evaluated per row chunk in pass 2 (stage timer "p2_xgrad").  For a model-only evaluation it is dl1/dx.
 *   on_device = 0: dl_dinputs is a host buffer, Fortran D x n, ld >= D (the layout of gprhip_set_inputs; rows D..ld-1 of
 *                  every column are left untouched).  The library keeps an n x D device buffer for it, allocated at the
 *                  first such call after a comparison with the device's free memory: GPRHIP_EOOM leaves the problem as
 *                  it was.
 *   on_device = 1: dl_dinputs is a device pointer, point-major [n][D], ld == D (the layout of gprhip_set_inputs_device),
 *                  written directly; complete when the call returns.
 * Limits: fp64 and one device only.  GPRHIP_EBADARG for a GPRHIP_F32_BULK problem, for log_multiscales_m05 != NULL (the
 * multiscale exponent needs per-column weights), for dl_dinputs == NULL and for a bad ld.  reuse_v, variational,
 * model_only, tproj and log_hetero_skedasticity are honoured; GPRHIP_ESTATE applies as for the plain evaluation.  A refused
 * call enqueues nothing and leaves the problem's state valid; after a completed one the problem serves predictions etc.
 * exactly as after the plain evaluation.
 * Row path: a single-chunk problem keeps its path, and res, grad and coeffs then equal the plain evaluation's bit for bit.
 * A shape of the one-kernel row passes (at most 256 inducing points) held in SEVERAL chunks takes the engine row path for
 * this call -- those passes keep X only for single-chunk problems -- so there res, grad and coeffs agree with the plain
 * evaluation to rounding only.
 * The plain, the several-target, the batched, the staged and the sharded evaluations are untouched and do not take this
 * output. */
int gprhip_eval_input_grad(gprhip_problem* p, const gprhip_hypers* h, gprhip_result* res, double* grad, double* coeffs,
                           double* dl_dinputs, int64_t ld, int on_device);

/* Staged form for row-sharded evaluation across devices (one process per device).  Between the
 * stages the caller sums the exchange buffers over all shards (RCCL all-reduce on the same HIP
 * stream or after a stream sync -- the buffers are plain device memory owned by the caller):
 *     gprhip_eval_pass1(p, h, want_grad, ar1)      ar1: gprhip_ar1_len(p) doubles
 *     all-reduce(sum, ar1)
 *     gprhip_eval_pass2(p, ar1, ar2)               ar2: gprhip_ar2_len(p) doubles
 *     all-reduce(sum, ar2)
 *     gprhip_eval_finish(p, ar2, res, grad, coeffs)
 * n used in the n*log(2*pi) term is n_total given here (sum over shards). */
int64_t gprhip_ar1_len(const gprhip_problem* p);
int64_t gprhip_ar2_len(const gprhip_problem* p);
/* The same lengths from the problem's dimensions alone (no device, no handle; which = 1 | 2), and the position of entry
 * (r, c) of the symmetric m x m part that heads both buffers -- stored as its upper 128 x 128 tiles only, tile (bm <= bn)
 * at ((bn (bn + 1) / 2 + bm) * 128 * 128, row-major inside (r, c < m rounded up to 128; the tile of (r, c) must be on or
 * above the diagonal, else -1).  A host that owns the collective sizes and fills its buffers with these. */
/* What the two buffers hold, mp = m rounded up to 128, E = X .* K_nm, all sums over the shard's rows:
 *   exchange 1  [packed tiles of B~_part = V^T diag(1/s) V | c~ = V^T (y ./ s) (mp) | tail (4)]
 *               tail: 0 sum log s, 1 sum y^2 / s, 2 sum r / s, 3 unused
 *   exchange 2  [packed tiles of G~_part = V^T diag(v) V | column block (col_rows x mp) | `Proj second term (dbig x d) | tail (8)]
 *               col_rows = d + 1 and dbig = 0 for Cov_se_iso; d + 1 + D + d and dbig = D for Cov_se_fat
 *               column block rows: sum_r E_rc; sum_r p_kr E_rc (d rows); with a projection sum_r x_br E_rc (D rows); with
 *               multiscales sum_r p_kr^2 E_rc (d rows) directly behind the rows before them; every further row zero
 *               `Proj second term, big-major: sum_r x_br p_kr sum_c E_rc [/ ms_kc]; zero without a projection
 *               tail: 0 sum v, 1 sum 1/s, 2 sum w res, 3 sum v1, 4 sum E, 5 sum E |p_r - z_c|^2 (read for Cov_se_iso only),
 *               6, 7 unused
 * A gradient evaluation writes every entry of both buffers, whatever they held; an evidence-only one writes all of exchange
 * 1 and zeroes the tail of exchange 2 alone.  Entries of a tile with row or column >= m, entries of c~ and of the column block
 * with column >= m, unused rows of the column block and unused tail slots are +0.0: they are summed with every other
 * shard's.  Entries below the diagonal (r > c) of a diagonal tile are finite but otherwise unspecified (the mirror image, or
 * zero, by kernel family), and pass 2 and the finish stage never read them. */
int64_t gprhip_exchange_len(int cov_kind, int D, int d, int m, int which);
int64_t gprhip_exchange_offset(int m, int r, int c);
int gprhip_eval_pass1(gprhip_problem* p, const gprhip_hypers* h, int want_grad, int64_t n_total,
                      double* d_ar1);
int gprhip_eval_pass2(gprhip_problem* p, const double* d_ar1, double* d_ar2);
int gprhip_eval_finish(gprhip_problem* p, const double* d_ar2, gprhip_result* res, double* grad,
                       double* coeffs);
/* Block the host until all work queued by the stage calls has finished. */
int gprhip_sync(gprhip_problem* p);
/* The HIP stream (hipStream_t) the problem enqueues on, for callers that order other work after it. */
void* gprhip_stream(gprhip_problem* p);

/* ---- Single-process, multi-device evaluation ---------------------------------------------------------------------
 * The reference's host is ONE process (bin/ocaml_gpr.ml:176-177, :340-342: one functor application, one optimiser
 * loop), so the way it reaches the GPUs of a node is a context that owns one shard per device and does the exchange
 * steps itself -- the calls above with "the caller does the all-reduce" serve one-process-per-GPU hosts
 * (gpr_amd/dist.py under torch.distributed).
 *
 *   gprhip_ctx_create(devices, ndev)        the devices of the node to use; loads RCCL (dlopen, so that single-device
 *                                           use of the library has no RCCL dependency) and creates one communicator
 *                                           per device (ncclCommInitAll) when ndev > 1
 *   gprhip_sharded_create(ctx, ...)         one gprhip_problem per device; shard i owns the contiguous training rows
 *                                           [lo_i, hi_i) (sizes differ by at most one, as gpr_amd.dist.shard_rows)
 *   gprhip_sharded_set_inputs / _targets    the whole D x n / n host arrays; every shard copies its own rows
 *   gprhip_sharded_eval                     pass 1 on every device (one host thread per device enqueues on that
 *                                           device's stream), grouped ncclAllReduce(sum, fp64) of the packed exchange
 *                                           buffers on those same streams -- no host synchronisation, no event hop --
 *                                           pass 2, second all-reduce (gradient evaluations only), finish on the first
 *                                           device.  Results are those of gprhip_eval on the unsharded problem up to the
 *                                           summation order of the exchange buffers; with ndev == 1 they are bit-identical.
 * Validation mode: if `devices` names ONE device ndev > 1 times, the shards share that device and the exchange step is
 * a fixed-order device-local sum instead of RCCL (which refuses duplicate devices) -- the ndev-way partition and all of
 * its bookkeeping can then be exercised on a one-GPU box.  Mixed lists (some devices repeated) are refused.
 * GPRHIP_CTX_RCCL=1 in the environment at creation makes a one-device context go through RCCL as well (a one-rank
 * communicator): exercises the dlopen / ncclCommInitAll / ncclAllReduce path on a one-GPU box.
 * GPRHIP_RCCL_LIB names the shared object to load (default: librccl.so.1, then librccl.so, then /opt/rocm/lib). */
typedef struct gprhip_ctx gprhip_ctx;
typedef struct gprhip_sharded gprhip_sharded;

enum { GPRHIP_COMM_NONE = 0, GPRHIP_COMM_RCCL = 1, GPRHIP_COMM_SAME_DEVICE = 2 };

/* The row partition itself (pure arithmetic, no device): shard idx of ndev owns rows [*row_lo, *row_hi) of n. */
int gprhip_shard_rows(int64_t n, int ndev, int idx, int64_t* row_lo, int64_t* row_hi);

int gprhip_ctx_create(const int* devices, int ndev, gprhip_ctx** out);
/* May be called while sharded problems of the context are still alive (a garbage-collected host finalises handles in
 * any order): the context is then released together with the last of them. */
void gprhip_ctx_destroy(gprhip_ctx* ctx);
int gprhip_ctx_ndev(const gprhip_ctx* ctx);
int gprhip_ctx_comm_mode(const gprhip_ctx* ctx); /* GPRHIP_COMM_* */

/* Arguments as gprhip_problem_create_ex, n = training points of the WHOLE problem (>= ndev). */
int gprhip_sharded_create(gprhip_ctx* ctx, int cov_kind, int precision, int64_t n, int D, int d, int m,
                          int64_t chunk_rows, gprhip_sharded** out);
void gprhip_sharded_destroy(gprhip_sharded* sp);
/* Shard idx (0 <= idx < ndev): its device, its row range [*row_lo, *row_hi) of the whole problem (any pointer may be
 * NULL), and its device problem -- the m x m model state is replicated, so gprhip_predict, gprhip_covariances,
 * gprhip_co_variance_coeffs, ... work on any shard's problem after an evaluation; gprhip_train_stats and the per-row
 * names of gprhip_debug_fetch cover that shard's rows. */
int gprhip_sharded_shard(const gprhip_sharded* sp, int idx, int* device, int64_t* row_lo, int64_t* row_hi);
gprhip_problem* gprhip_sharded_problem(gprhip_sharded* sp, int idx);
int gprhip_sharded_set_inputs(gprhip_sharded* sp, const double* inputs, int64_t ld); /* Fortran D x n, host */
int gprhip_sharded_set_targets(gprhip_sharded* sp, const double* targets);           /* n, host          */
/* As gprhip_eval. */
int gprhip_sharded_eval(gprhip_sharded* sp, const gprhip_hypers* h, int want_grad, gprhip_result* res, double* grad,
                        double* coeffs);
/* Posterior prediction with all devices (gprhip_predict on every shard's problem for its share of the test points --
 * the model state is replicated, the test points are split like the training rows): means / variances as there. */
int gprhip_sharded_predict(gprhip_sharded* sp, const double* test_inputs, int64_t ld, int64_t nt, int predictive,
                           double* means, double* variances);
/* Training-set statistics over all shards (gprhip_train_stats per shard, combined sum / sum / max / sum): means (n,
 * whole problem, may be NULL) and sums[4]. */
int gprhip_sharded_train_stats(gprhip_sharded* sp, double* means, double* sums);
/* Exchange steps of the last evaluation: their count (1 evidence-only, 2 gradient; 0 with one device and no forced
 * RCCL), bytes per device of each, and -- after gprhip_sharded_set_timing(sp, 1) -- their milliseconds on the first
 * shard's stream (HIP events; includes waiting for the slowest shard). */
int gprhip_sharded_comm_stats(const gprhip_sharded* sp, int* collectives, int64_t bytes[2], float ms[2]);
int gprhip_sharded_set_timing(gprhip_sharded* sp, int level);

/* Posterior prediction at test points with the model state left by the last evaluation on `p`
 * (kernel, inducing points, U = chol_km, R = r_mat, mean coefficients):
 *   means[i]     = K_tm[i,:] . coeffs                          Means.calc     lib/fitc_gp.ml:418-425
 *   variances[i] = k_ii - |K_tm U^-1|_i^2 + |K_tm R^-1|_i^2    Variances.calc lib/fitc_gp.ml:498-518
 *                  (+ sigma2 when predictive != 0: Variances.get ?predictive, :520-529)
 * test_inputs: Fortran D x nt (ld >= D), host.  means / variances: nt doubles, host; either may be NULL.
 * The last evaluation must have had targets (model_only = 0) for the means to be meaningful. */
int gprhip_predict(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int predictive,
                   double* means, double* variances);
int gprhip_predict_targets(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, double* means);

/* Means and variances as gprhip_predict, together with their gradients with respect to the test inputs -- what maximising
 * an acquisition function over candidate points, propagating an input uncertainty, a sensitivity analysis or a feature
 * extractor in front of the GP at prediction time needs (an extension beyond the reference's implemented surface).  With
 * p_r the point the kernel sees (x*_r, or tproj^T x*_r), K_rc = k(p_r, z_c), t the mean coefficients and
 *   M = U^-1 (I - R~^-1 R~^-T) U^-T  (= (K_m + jitter)^-1 - B^-1),   G = K M:
 *   means[r]     = sum_c K_rc t_c                            dmeans[:, r]     = tproj (-inv_ell2 sum_c K_rc t_c  (p_r - z_c))
 *   variances[r] = sf2 - sum_c K_rc G_rc (+ sigma2)          dvariances[:, r] = tproj (2 inv_ell2 sum_c K_rc G_rc (p_r - z_c))
 * (inv_ell2 = exp(-2 log_ell) for Cov_se_iso, 1 for Cov_se_fat; the tproj factor only with a projection).  `predictive`
 * adds sigma2 to the variances only; the gradients do not depend on it.
 *   on_device = 0: test_inputs is a host buffer, Fortran D x nt, ld >= D; means / variances are nt doubles on the host;
 *                  dmeans / dvariances are host buffers, Fortran D x nt, ldg >= D (rows D..ldg-1 of every column are left
 *                  untouched).
 *   on_device = 1: all five are device pointers on the problem's device, the inputs and gradients point-major [nt][D] with
 *                  ld == ldg == D; the outputs are written in place and are complete when the call returns.
 * Each of the four outputs may be NULL; all four NULL is GPRHIP_EBADARG.  A request without variances and dvariances forms
 * neither M nor G.
 * State: as gprhip_predict -- GPRHIP_ESTATE without a completed evaluation or a loaded predictor, for variances /
 * dvariances on a loaded predictor without factors, and for means / dmeans after gprhip_eval_targets; the fp32-bulk
 * coefficient guard applies to means / dmeans.
 * Limits: fp64 problems, one device, no multiscales in the model state, at most 64 point dimensions on the kernel side (d;
 * D in front of a projection may be anything).  Anything outside them is GPRHIP_EBADARG.  A refused call enqueues nothing
 * and leaves the state valid; the call never changes the predictor state.
 * Memory: M (m x m, padded) is formed once per model state and kept until the next evaluation or gprhip_load_predictor;
 * its allocation and the gradient staging buffers are compared with the device's free memory first: GPRHIP_EOOM leaves
 * everything as it was.  Test points go through in the chunks of gprhip_predict.
 * Stage timers: "pg_m" (M), and per chunk "pg_cov" (K), "pg_gemm" (G = K M), "pg_grad" (the gradient kernel; for at most 64
 * inducing points of at most 16 dimensions the whole chunk is this one kernel). */
int gprhip_predict_input_grad(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int predictive,
                              double* means, double* variances, double* dmeans, double* dvariances, int64_t ldg,
                              int on_device);

/* An acquisition criterion over candidate points, with its gradient with respect to them and the best top_k candidates --
 * the scoring phase of Bayesian optimisation or active learning, built on the posterior and its input gradients above (an
 * extension beyond the reference's implemented surface).  Every criterion is "larger is better".  With mu_r / sigma2_r the mean
 * and variance of gprhip_predict_input_grad at candidate r (sigma2 added when `predictive`),
 *   s = +1 if maximise else -1,  v = max(sigma2_r, var_floor),  sigma = sqrt(v),  delta = s (mu_r - best) - xi,  u = delta / sigma,
 *   Phi / phi the standard normal cdf / pdf,  h(u) = phi(u) + u Phi(u):
 *   kind      value a                              c_mu = da/dmu                   c_v = da/dsigma2
 *   EI        delta Phi(u) + sigma phi(u)          s Phi(u)                        phi(u) / (2 sigma)
 *   LOG_EI    log sigma + log h(u)                 s Phi(u) / (sigma h(u))         phi(u) / (2 v h(u))
 *   PI        Phi(u)                               s phi(u) / sigma                -u phi(u) / (2 v)
 *   BOUND     s mu + kappa sigma                   s                               kappa / (2 sigma)
 * values[r] = a, dvalues[:, r] = c_mu dmeans[:, r] + c_v dvariances[:, r] with the two gradients of
 * gprhip_predict_input_grad; c_v = 0 where the variance was clamped (sigma2_r < var_floor).  Phi keeps its relative accuracy
 * in the lower tail, and LOG_EI stays finite and accurate where EI underflows (u < -38).  means / variances are those of
 * gprhip_predict_input_grad (the variance before the clamp).  BOUND with kappa == 0 and variances == NULL runs the mean part
 * alone: neither M nor G is formed.
 *   on_device = 0: test_inputs (Fortran D x nt, ld >= D), values / means / variances (nt) and dvalues (Fortran D x nt,
 *                  ldg >= D, rows D..ldg-1 left untouched) are host buffers.
 *   on_device = 1: they are device pointers on the problem's device, inputs and gradient point-major [nt][D], ld == ldg == D.
 * Each of the four may be NULL.
 * top_k > 0: top_index[0 .. top_k) (HOST, always) receives the indices of the top_k largest values over all nt candidates,
 * value descending, the lower index first among equal values; NaN values are never selected.  top_values (top_k, may be
 * NULL) and top_dvalues (D x top_k, leading dimension D, may be NULL) receive the value and the gradient at each.  Where
 * fewer than top_k candidates qualify the remaining top_index entries are -1 and their top_values / top_dvalues are left
 * untouched.  The selection runs on the device without atomics (two runs give the same bits); with values, dvalues, means
 * and variances all NULL nothing of size nt leaves the device.
 * GPRHIP_EBADARG: an unknown kind, xi < 0, kappa < 0, var_floor not positive and finite, a non-finite best, top_k outside
 * 0 .. GPRHIP_MAX_TOP_K, top_k > 0 without top_index, nothing requested (the four outputs NULL and top_k == 0), bad ld / ldg.
 * State and limits: as gprhip_predict_input_grad -- GPRHIP_ESTATE without a completed evaluation or a loaded predictor, on a
 * loaded predictor without factors (unless the mean part alone runs), and after gprhip_eval_targets; the fp32-bulk
 * coefficient guard applies; fp64 problems, one device, no multiscales, at most 64 point dimensions on the kernel side.  A
 * refused call enqueues nothing and leaves the state valid; the call never changes the predictor state.
 * Stage timers: those of gprhip_predict_input_grad, and per chunk "acq_select" (the selection). */
enum { GPRHIP_ACQ_EI = 0, GPRHIP_ACQ_LOG_EI = 1, GPRHIP_ACQ_PI = 2, GPRHIP_ACQ_BOUND = 3 };
#define GPRHIP_MAX_TOP_K 64
typedef struct {
  int kind;          /* one of GPRHIP_ACQ_* */
  int maximise;      /* 1: larger targets are better; 0: smaller */
  int predictive;    /* as gprhip_predict: add sigma2 to the variance the criterion sees */
  double best;       /* incumbent f* (EI, LOG_EI, PI) */
  double xi;         /* margin >= 0 (EI, LOG_EI, PI) */
  double kappa;      /* >= 0 (BOUND) */
  double var_floor;  /* > 0, finite: the criterion sees v = max(variance, var_floor) */
} gprhip_acquisition;
int gprhip_acquire(gprhip_problem* p, const gprhip_acquisition* acq, const double* test_inputs, int64_t ld, int64_t nt,
                   double* values, double* dvalues, int64_t ldg, double* means, double* variances, int top_k,
                   int64_t* top_index, double* top_values, double* top_dvalues, int on_device);

/* Max-value entropy search over candidate points (MES, Wang & Jegelka 2017), with its gradient and the best top_k candidates:
 * how much observing a candidate tells about the VALUE of the optimum, from the extreme values of drawn sample paths -- the
 * second consumer, after Thompson sampling, of what gprhip_sample_paths_refine produces (an extension beyond the reference's
 * implemented surface).  "Larger is better", as every criterion of gprhip_acquire.  With mu_r / sigma2_r the mean and the LATENT
 * variance of gprhip_predict_input_grad at candidate r (predictive = 0: sigma2 is not added),
 *   s = +1 if maximise else -1,  v = max(sigma2_r, var_floor),  sigma = sqrt(v),
 *   e_j, j < n_extremes: the extreme value of f on drawn path j -- its maximum when maximising, else its minimum,
 *   gamma_j = s (e_j - mu_r) / sigma,  lambda = phi / Phi,
 *   psi(gamma)  = gamma lambda(gamma) / 2 - log Phi(gamma)       (> 0, decreasing)
 *   psi'(gamma) = -(lambda / 2) (1 + gamma (gamma + lambda))
 *   a    = (1 / S) sum_j psi(gamma_j)
 *   c_mu = da/dmu     = (1 / S) sum_j psi'(gamma_j) (-s / sigma)
 *   c_v  = da/dsigma2 = (1 / S) sum_j psi'(gamma_j) (-gamma_j / (2 v)),  0 where the variance was clamped
 * values[r] = a, dvalues[:, r] = c_mu dmeans[:, r] + c_v dvariances[:, r].  gamma_j < 0 (a drawn extreme on the wrong side of
 * the mean at the candidate) is legal and accurate: nothing cancels (gpr_amd/csrc/mv_math.h), and the results keep their
 * relative accuracy down to the subnormal range; |gamma| beyond 1e130 overflows.  The sums over j run in a fixed order, without
 * atomics: two runs give the same bits.  gprhip_sample_paths_refine reports the objective s f: e_j = s times its best value
 * of draw j.
 * extremes: HOST, always (n_extremes doubles).  Every other buffer, on_device, ld / ldg, means / variances and the top_k outputs
 * are those of gprhip_acquire, word for word.
 * GPRHIP_EBADARG: n_extremes outside 1 .. GPRHIP_MAX_EXTREMES, extremes NULL, a non-finite extreme, var_floor not positive and
 * finite, top_k outside 0 .. GPRHIP_MAX_TOP_K, top_k > 0 without top_index, nothing requested, bad ld / ldg.
 * State and limits: as gprhip_acquire with a criterion that needs the variance -- GPRHIP_ESTATE without a completed evaluation
 * or a loaded predictor, on a loaded predictor without factors, and after gprhip_eval_targets; fp64 problems, one device, no
 * multiscales, at most 64 point dimensions on the kernel side.  A refused call enqueues nothing and leaves the state valid; the
 * call never changes the predictor state.  gprhip_acquire_max_value_refine refines candidates of this criterion.
 * Stage timers: those of gprhip_predict_input_grad, and per chunk "acq_select". */
#define GPRHIP_MAX_EXTREMES 64
int gprhip_acquire_max_value(gprhip_problem* p, const double* extremes /* HOST always */, int n_extremes, int maximise,
                             double var_floor, const double* test_inputs, int64_t ld, int64_t nt, double* values,
                             double* dvalues, int64_t ldg, double* means, double* variances, int top_k, int64_t* top_index,
                             double* top_values, double* top_dvalues, int on_device);

/* Refines candidates of an acquisition criterion on the device: projected gradient ascent with Armijo backtracking from ns
 * starting points inside a box, every start on its own -- what follows gprhip_acquire's top_k when the maximiser is wanted and
 * not the best grid point (an extension beyond the reference's implemented surface).  The criterion is any gprhip_acquisition,
 * its value a and gradient g those of gprhip_acquire.  With w_k = upper_k - lower_k, per start:
 *   1. x = clip(start); (a, g) at x; evals = 1.  a NaN: status GPRHIP_REFINE_ST_NAN.
 *   2. dir_k = scale_k g_k, set to 0 where the bound is active and dir_k points out of the box (and where g_k is NaN).  All
 *      dir_k == 0: GPRHIP_REFINE_ST_CONVERGED.  Otherwise alpha = (step0 min_k w_k) / max_k |dir_k|.
 *   3. While evals < max_evals:  y = clip(x + alpha dir) (y_k = x_k where dir_k == 0), delta = y - x.  If
 *      max_k |delta_k| / w_k <= xtol: CONVERGED.  Otherwise (a_y, g_y) at y, ++evals.  If a_y >= a + c1 sum_k g_k delta_k (false
 *      for NaN): accept -- x, a, g = y, a_y, g_y, ++accepted, dir again (all zero: CONVERGED), alpha *= grow.  Else
 *      alpha *= shrink.
 *   4. GPRHIP_REFINE_ST_MAX_EVALS when the evaluations run out.
 * lower / upper / scale: HOST always, D doubles each; scale == NULL means all ones.
 * Outputs per start, each may be NULL: x_out (D), values and dvalues (D) -- the value and gradient at x_out from the evaluation
 * that produced it, there is no extra evaluation --, evals, accepted, status (int), and trace, [ns][max_evals][2 D + 3] doubles
 * in either mode: evaluation j of a start writes record j = (y, g_y, a_y, alpha, accepted as 0 / 1); record 0 is the clipped
 * start with alpha = 0 and accepted = 1; records after the last evaluation are left untouched.
 *   on_device = 0: starts (Fortran D x ns, ld >= D), x_out (D x ns, ldx >= D), dvalues (D x ns, ldg >= D; rows beyond D left
 *                  untouched), values / evals / accepted / status (ns) and trace are host buffers.
 *   on_device = 1: they are device pointers on the problem's device, starts / x_out / dvalues point-major [ns][D],
 *                  ld == ldx == ldg == D; the starts are read back once to be checked.
 * Two routes, one rule.  At most 64 inducing points of at most 16 dimensions without a projection: ONE persistent kernel, 64
 * starts per workgroup, the model in LDS and the loop on the device.  Every other shape gprhip_acquire accepts: the loop runs in
 * the library on device buffers -- an evaluation is gprhip_acquire's chunk walk, a step kernel follows, and one integer (the
 * number of starts that go on) comes back per evaluation.  A start's result does not depend on the other starts; two runs give
 * the same bits.
 * GPRHIP_EBADARG: everything gprhip_acquire refuses of the criterion; max_evals outside 1 .. GPRHIP_REFINE_MAX_EVALS, step0
 * outside (0, 1], c1 outside [0, 1), shrink outside (0, 1), grow < 1, xtol < 0 (or any of them not finite); scale not positive and
 * finite; lower >= upper or non-finite bounds; a non-finite start; ns outside 1 .. GPRHIP_REFINE_MAX_STARTS; all outputs NULL;
 * bad ld / ldx / ldg.  State and limits: as gprhip_acquire (GPRHIP_ESTATE under the same conditions; BOUND with kappa == 0 runs
 * the mean part alone and needs no factors).  New buffers are checked against the free device memory first (GPRHIP_EOOM).  A
 * refused call enqueues nothing; the call never changes the predictor state.
 * Limits: no optimiser other than this one (no L-BFGS, no q-batch criteria: greedy batches go through gprhip_observe);
 * drawn sample paths are refined by gprhip_sample_paths_refine, not here; fp64 problems, one device, no multiscales.
 * Stage timers: "rf_small" (the persistent kernel); on the other route those of gprhip_acquire per evaluation and "rf_step". */
enum { GPRHIP_REFINE_ST_CONVERGED = 0, GPRHIP_REFINE_ST_MAX_EVALS = 1, GPRHIP_REFINE_ST_NAN = 2 };
#define GPRHIP_REFINE_MAX_EVALS 1000
#define GPRHIP_REFINE_MAX_STARTS 4096
typedef struct {
  int max_evals;  /* 1 .. GPRHIP_REFINE_MAX_EVALS: evaluations per start, the one at the start included */
  double step0;   /* (0, 1]: the first step moves the fastest component by step0 times the narrowest width */
  double c1;      /* [0, 1): Armijo's sufficient-increase constant */
  double shrink;  /* (0, 1): step factor after a rejected trial */
  double grow;    /* >= 1: step factor after an accepted trial */
  double xtol;    /* >= 0: a trial step below xtol of the box widths ends the start */
} gprhip_refine_options;
int gprhip_acquire_refine(gprhip_problem* p, const gprhip_acquisition* acq, const gprhip_refine_options* opt, const double* lower,
                          const double* upper, const double* scale, const double* starts, int64_t ld, int64_t ns, double* x_out,
                          int64_t ldx, double* values, double* dvalues, int64_t ldg, int* evals, int* accepted, int* status,
                          double* trace, int on_device);

/* Refines candidates of max-value entropy search on the device: the maximiser of the information criterion, what follows
 * gprhip_acquire_max_value's top_k when it is wanted and not the best grid point (an extension beyond the reference's
 * implemented surface).  The criterion, its value a and gradient g, the LATENT variance, var_floor and the extremes (HOST
 * always, n_extremes doubles, 1 .. GPRHIP_MAX_EXTREMES, finite) are those of gprhip_acquire_max_value, word for word;
 * gprhip_acquisition has no kind for it, the extremes do not fit its layout.
 * The rule (steps 1 - 4), gprhip_refine_options, the status codes, lower / upper / scale (HOST always, D doubles each; scale
 * == NULL means all ones), every output and its layout in either mode, on_device, GPRHIP_REFINE_MAX_STARTS and
 * GPRHIP_REFINE_MAX_EVALS are those of gprhip_acquire_refine, word for word -- the trace is [ns][max_evals][2 D + 3] doubles,
 * evaluation j of a start writes record j = (y, g_y, a_y, alpha, accepted as 0 / 1), record 0 is the clipped start with
 * alpha = 0 and accepted = 1, and records after the last evaluation are left untouched.
 * Two routes, one rule, as gprhip_acquire_refine.  At most 64 inducing points of at most 16 dimensions without a projection:
 * ONE persistent kernel, the evaluator of gprhip_acquire_max_value's one-kernel path inside the loop; the four lanes of a
 * start take every fourth extreme and join their sums in the order of that kernel.  Every other shape: the loop runs in the
 * library on device buffers, an evaluation is gprhip_acquire_max_value's chunk walk -- the very kernels, the same bits at the
 * same point --, a step kernel follows, and one integer comes back per evaluation.  A start's result does not depend on the
 * other starts; no atomics: two runs give the same bits.
 * GPRHIP_EBADARG: what gprhip_acquire_max_value refuses of n_extremes, extremes and var_floor; what gprhip_acquire_refine
 * refuses of the options, the box, scale, the starts, ns, the outputs and ld / ldx / ldg.  State and limits: as
 * gprhip_acquire_max_value (GPRHIP_ESTATE under the same conditions; the variance part is always needed).  New buffers are
 * checked against the free device memory first (GPRHIP_EOOM).  A refused call enqueues nothing; the call never changes the
 * predictor state.
 * Limits: those of gprhip_acquire_refine; the latent-variance form of the criterion only.
 * Stage timers: "rf_small" (the persistent kernel); on the other route those of gprhip_acquire_max_value per evaluation and
 * "rf_step". */
int gprhip_acquire_max_value_refine(gprhip_problem* p, const double* extremes /* HOST always */, int n_extremes, int maximise,
                                    double var_floor, const gprhip_refine_options* opt, const double* lower, const double* upper,
                                    const double* scale, const double* starts, int64_t ld, int64_t ns, double* x_out,
                                    int64_t ldx, double* values, double* dvalues, int64_t ldg, int* evals, int* accepted,
                                    int* status, double* trace, int on_device);

/* Posterior sample paths over test points, with the best top_k points of every draw -- Thompson sampling, batch selection by
 * independent draws, posterior pictures over a grid (an extension beyond the reference's implemented surface; its Cov_sampler
 * forms and factors an nt x nt covariance).  The FITC posterior is a Gaussian over m weights, so a draw is a FUNCTION of x,
 * fixed by z and evaluable at any set of points for O(nt m):
 *   a_j = t + U^-1 (R~^-1 z_j),  z_j ~ N(0, I_m)          (R = R~ U = r_mat: Cov a = R^-1 R^-T = B^-1, mean a = t = the mean coefficients)
 *   f_j(x) = sum_c k(x, z_c) a_cj                          -- the path part
 *   samples[r, j] = f_j(x_r) + sqrt(max(0, sf2 - |K_r U^-1|^2 (+ sigma2 if predictive))) eps[r, j],  eps ~ N(0, 1) independent
 * Over z and eps the mean is gprhip_predict's mean, the variance exactly gprhip_predict's variance, and the covariance of
 * two different points Q Q^T with Q = K_tm R^-1 -- the off-diagonal of gprhip_covariances kind 1: the posterior under the
 * conditional independence FITC itself assumes.  The normal draws are the caller's (as with gprhip_cov_samples): the library
 * stays deterministic.
 *   z: HOST always, Fortran m x ns (ldz >= m), 1 <= ns <= GPRHIP_MAX_DRAWS.
 *   eps: nt x ns (lde >= nt), or NULL: the path part only (`predictive` is then ignored).
 *   samples: nt x ns (lds >= nt); may be NULL (with top_k > 0: nothing of size nt leaves the device).
 *   on_device = 0: test_inputs (Fortran D x nt, ld >= D), eps and samples (Fortran nt x ns) are host buffers.
 *   on_device = 1: device pointers on the problem's device: test_inputs point-major [nt][D] (ld == D), eps / samples
 *                  draw-major [ns][lde] / [ns][lds] -- the same memory layout.
 * top_k > 0: per draw j, top_index[j * top_k + (0 .. top_k)) (HOST, always) receives the indices of the top_k largest
 * (maximise = 0: smallest) entries of samples[:, j], best first, the lower index first among equal values; NaN is never
 * selected; where fewer qualify the remaining indices are -1 and their values / gradients are left untouched.  top_values
 * (HOST, top_k x ns, may be NULL) receives the entries themselves, top_dvalues (HOST, D x top_k x ns, may be NULL) the
 * gradient of the PATH part f_j with respect to the test input at each winner.  The selection runs on the device without
 * atomics: two runs give the same bits.
 * GPRHIP_EBADARG: ns outside 1 .. GPRHIP_MAX_DRAWS, top_k outside 0 .. GPRHIP_MAX_TOP_K, top_k > 0 without top_index, nothing
 * requested (samples NULL and top_k == 0), bad ldz / ld / lde / lds, an fp32-bulk problem, a model state with multiscales,
 * more than 64 point dimensions on the kernel side.  GPRHIP_ESTATE: no completed evaluation or loaded predictor, a predictor
 * loaded without factors, after gprhip_eval_targets.  The fp32-bulk coefficient guard applies.  New buffers are checked against
 * the free device memory first (GPRHIP_EOOM).  A refused call enqueues nothing; the call never changes the predictor state.
 * Stage timers: "sp_coeff" (the weights, once per call), and per chunk "sp_path" (F = K A, K recomputed on the fly),
 * "sp_resid" (with eps: the residual standard deviation and its addition), "sp_select" (selection and the winners' gradients). */
#define GPRHIP_MAX_DRAWS 64
int gprhip_sample_paths(gprhip_problem* p, const double* z, int64_t ldz, int ns, const double* test_inputs, int64_t ld,
                        int64_t nt, const double* eps, int64_t lde, int predictive, double* samples, int64_t lds, int maximise,
                        int top_k, int64_t* top_index, double* top_values, double* top_dvalues, int on_device);

/* Refines drawn sample paths on the device: the maximiser (maximise = 0: minimiser) of each draw f_j, what Thompson sampling
 * wants after gprhip_sample_paths has named the best grid points of every draw (an extension beyond the reference's
 * implemented surface).
 *   z: HOST always, Fortran m x nd (ldz >= m), 1 <= nd <= GPRHIP_MAX_DRAWS.  Column j fixes draw j exactly as in
 *      gprhip_sample_paths: a_j = t + U^-1 (R~^-1 z_j), f_j(x) = sum_c k(x, z_c) a_cj.  The same z gives the same function.
 *   draw_of: HOST always, ns ints in 0 .. nd - 1: the draw that each start climbs.  Any assignment is allowed; the usual one
 *      is the top_k winners of draw j as the starts of draw j.
 * The objective of start i is o(x) = s f_{draw_of[i]}(x) with s = +1 if maximise, else -1, its gradient s grad f: "larger is
 * better", as with the criteria.  values, dvalues and the trace hold the OBJECTIVE and its gradient -- the numbers the rule
 * sees --, not the unsigned path: with maximise = 0 they are -f and -grad f.
 * The rule (steps 1 - 4), gprhip_refine_options, the status codes, lower / upper / scale (HOST always, D doubles each; scale
 * == NULL means all ones), every output and its layout in either mode, on_device, GPRHIP_REFINE_MAX_STARTS and
 * GPRHIP_REFINE_MAX_EVALS are those of gprhip_acquire_refine, word for word -- the trace is [ns][max_evals][2 D + 3] doubles,
 * evaluation j of a start writes record j = (y, g_y, a_y, alpha, accepted as 0 / 1), record 0 is the clipped start with
 * alpha = 0 and accepted = 1, and records after the last evaluation are left untouched.
 * Two routes, one rule, one evaluator.  A draw has m weights, so an evaluation with its gradient costs O(m d) per start: without
 * a projection ONE persistent kernel runs the loop on the device at every m (64 starts per workgroup; the panels of Z - s and
 * of the weights are staged again for every evaluation).  With a projection the loop runs in the library on device buffers:
 * the trial points are projected, one launch of the same evaluator, the back-projection of its gradient, a step kernel, and
 * one integer (the number of starts that go on) comes back per evaluation.  A start's result does not depend on the other
 * starts, nor on their draws; it depends on nd only through the weights (gprhip_sample_paths' weight kernel splits its sums
 * by the number of draws).  No atomics: two runs give the same bits.
 * GPRHIP_EBADARG: what gprhip_acquire_refine refuses of the options, the box, scale, the starts, ns, the outputs and ld / ldx /
 * ldg; nd outside 1 .. GPRHIP_MAX_DRAWS; a draw_of entry outside 0 .. nd - 1; bad ldz; an fp32-bulk problem, a model state with
 * multiscales, more than 64 point dimensions on the kernel side.  GPRHIP_ESTATE: as gprhip_sample_paths.  New buffers are
 * checked against the free device memory first (GPRHIP_EOOM).  A refused call enqueues nothing; the call never changes the
 * predictor state; the matrix M of gprhip_predict_input_grad is neither needed nor formed.  A non-finite z is not refused: a
 * NaN objective ends the start with GPRHIP_REFINE_ST_NAN, the starts of other draws are not touched by it.
 * Limits: plain projected ascent (no L-BFGS); the path part only (no eps); fp64 problems, one device, no multiscales, d <= 64,
 * nd <= 64, ns <= 4096.
 * Stage timers: "sp_coeff" (the weights, once per call), "prf_kernel" (the persistent kernel); with a projection "prf_eval"
 * (projection, evaluator and back-projection) and "rf_step" per evaluation. */
int gprhip_sample_paths_refine(gprhip_problem* p, const double* z, int64_t ldz, int nd, int maximise,
                               const gprhip_refine_options* opt, const double* lower, const double* upper, const double* scale,
                               const double* starts, int64_t ld, int64_t ns, const int* draw_of, double* x_out, int64_t ldx,
                               double* values, double* dvalues, int64_t ldg, int* evals, int* accepted, int* status,
                               double* trace, int on_device);

/* Training-set residual statistics with the model state left by the last evaluation (which must have had
 * targets): means[i] = K_nm[i,:] . coeffs over the resident training inputs (Trained.calc_means,
 * lib/fitc_gp.ml:296-297; host, n doubles, may be NULL) and
 *   sums[0] = sum (y-mean)^2   sums[1] = sum |y-mean|   sums[2] = max |y-mean|   sums[3] = sum y^2
 * from which Stats.calc (lib/fitc_gp.ml:353-373) derives sse/mse/rmse/smse/msll/mad/maxad.  For a row shard
 * the sums are this shard's; combine with sum/sum/max/sum. */
int gprhip_train_stats(gprhip_problem* p, double* means, double* sums);

/* Posterior covariance matrix between nt test points (fp64 in both precision modes):
 *   kind 0: FITC_covariances.calc  K_tt - V_t V_t^T + Q_t Q_t^T                    lib/fitc_gp.ml:585-599
 *   kind 1: FIC_covariances.calc   Q_t Q_t^T + diag(k_tt - rowsum(K_tm .^ 2))      lib/fitc_gp.ml:617-627
 * with V_t = K_tm U^-1, Q_t = K_tm R^-1.  predictive != 0 adds sigma2 to the diagonal (Common_covariances.get,
 * :549-559).  test_inputs: Fortran D x nt (ld >= D), host.  cov: nt x nt, ld = nt, host; the full symmetric
 * matrix is written (the reference defines the upper triangle only). */
int gprhip_covariances(gprhip_problem* p, const double* test_inputs, int64_t ld, int64_t nt, int kind,
                       int predictive, double* cov);

/* Common_cov_sampler.calc + samples (lib/fitc_gp.ml:656-697): factor chol(cov + (add_diag + jitter) I) (upper
 * triangle of the Fortran nt x nt `cov`, ld >= nt, is read) and return samples[:, j] = means + chol^T z[:, j]
 * for the ns columns of z (Fortran nt x ns standard normal draws supplied by the caller; samples likewise).
 * add_diag = sigma2 for ?predictive = true, else 0; jitter = Utils.cholesky_jitter.  Uses only the device
 * and stream of `p`.  GPRHIP_ENOTPOSDEF if the factorisation fails. */
int gprhip_cov_samples(gprhip_problem* p, const double* cov, int64_t ld, int64_t nt, double add_diag,
                       double jitter, const double* means, const double* z, int64_t ns, double* samples);

/* Model.calc_co_variance_coeffs (lib/fitc_gp.ml:240): the pair (chol_km, r_mat) of the last evaluation, each a
 * Fortran m x m upper-triangular factor (zeros below the diagonal), host; either may be NULL.  Together with the
 * kernel parameters, the inducing points and the mean coefficients this is what bin/ocaml_gpr.ml:207-232 stores
 * in its model file. */
int gprhip_co_variance_coeffs(gprhip_problem* p, double* chol_km, double* r_mat);

/* Install the predictor state of a saved model without evaluating anything -- Mean_predictor.calc
 * (lib/fitc_gp.ml:386-391) + Inducing.calc + Co_variance_predictor.calc (:446-447), the `test` flow of
 * bin/ocaml_gpr.ml:373-413.  h: kernel parameters, inducing points, sigma2 (as for gprhip_eval); coeffs: m mean
 * coefficients (NULL: variances/covariances only); chol_km, r_mat: as returned by gprhip_co_variance_coeffs
 * (both NULL: means only -- variance/covariance calls then return GPRHIP_ESTATE).
 * Afterwards gprhip_predict / gprhip_covariances work on `p`; training inputs need not have been set
 * (create the problem with n = the largest test batch you intend to pass). */
int gprhip_load_predictor(gprhip_problem* p, const gprhip_hypers* h, const double* coeffs, const double* chol_km,
                          const double* r_mat);

/* Folds k new observations (1 <= k <= GPRHIP_MAX_OBSERVE) into the predictor state left by the last evaluation or
 * gprhip_load_predictor, without a refit -- what closes the loop acquire -> refine -> observe, and what greedy batch selection
 * (kriging believer, constant liar) needs: a posterior conditioned on a fantasised observation and a cheap way back (an
 * extension beyond the reference's implemented surface).  At fixed hyper-parameters and inducing points a training point
 * enters the FITC posterior only through its row v = K_xm U^-1, s = sf2 - |v|^2 + sigma2 and y (lib/fitc_gp.ml:151-182; the
 * variational model has the same posterior, only l1 differs, :262-263).  With w_i = v_i / sqrt(s_i), eta_i = y_i / sqrt(s_i):
 *   B~' = B~ + sum w_i w_i^T,  c~' = c~ + sum w_i eta_i,  so [R~' | b'] is the triangular factor of [R~ | b] stacked on [W | eta]
 * -- a triangular-pentagonal QR update, O(k m^2), orthogonal, in the whitened coordinates; then
 * R~'^-1, t~' = R~'^-1 b' and t' = U^-1 t~'.
 *   inputs: on_device = 0: HOST, Fortran D x k (ld >= D); on_device = 1: device, point-major [k][D] (ld == D).
 *   targets: k doubles in the same memory space.  A state without targets (model_only = 1, or a predictor loaded without
 *            coefficients) takes targets == NULL and updates the factors only; a state with targets refuses NULL.
 *   dlog_evidence (HOST, may be NULL): the joint log density of the new targets given everything before them, i.e. the
 *            evidence of the enlarged data set minus the evidence before, at fixed hyper-parameters:
 *              dl1 = -1/2 (2 sum_j log(R~'_jj / R~_jj) + sum_i log s_i + k log 2 pi)   (-1/2 sum_i r_i / s_i more when the
 *                    state's evaluation was variational; r_i = sf2 - |v_i|^2)
 *              dl2 = -1/2 |rho|^2,  rho = what the QR leaves of eta  (|eta|^2 + |b|^2 = |b'|^2 + |rho|^2)
 *            Without targets it holds dl1 alone.
 * Afterwards every posterior call reads the conditioned model: gprhip_predict, gprhip_predict_input_grad, gprhip_acquire,
 * gprhip_acquire_refine, gprhip_acquire_max_value_refine, gprhip_sample_paths, gprhip_sample_paths_refine,
 * gprhip_covariances, gprhip_train_stats, gprhip_co_variance_coeffs -- a model file saved afterwards holds the conditioned predictor.  The matrix M of
 * gprhip_predict_input_grad and the weights of gprhip_sample_paths are formed again at their next use (debug names "pg_m" and
 * "sp_a" are GPRHIP_ESTATE until then; "w_mat" is scratch of the update).  The condition estimate stays: K_m is unchanged.
 * WHAT DOES NOT CHANGE: the resident training set (inputs, targets, V and the validity of reuse_v).  The next gprhip_eval
 * recomputes from the n original rows and FORGETS the observations; gprhip_train_stats goes over the n resident rows only.
 * GPRHIP_EBADARG: k out of range, bad ld, a non-finite input or target (device buffers are read back once to be checked), a
 *   GPRHIP_F32_BULK problem, multiscales in the model state, more than 64 point dimensions on the kernel side, targets given
 *   to a state without targets or withheld from one with them.
 * GPRHIP_ESTATE: no model, a predictor loaded without factors, after gprhip_eval_targets, an evaluation in flight.
 * GPRHIP_ENOTPOSDEF: some s_i <= 0 (possible at sigma2 = 0 on an inducing point).  The k values of s come back to the host
 *   BEFORE anything of the state is written: a refused call leaves every bit of the state as it was.
 * GPRHIP_EOOM: the scratch of the first call ((64 + 2) mp + 8.7 K doubles) against the free device memory.
 * No atomics: two runs give the same bits.  Stage timers: "obs_rows" (K, V = K U^-1 by gprhip_predict's launches, then W and
 * eta), "obs_update" (the QR update: per 128-column block row one diagonal launch and one trailing launch), "obs_inverse"
 * (R~'^-1 by the inverse pass of gprhip_load_predictor, O(m^3)), "obs_vectors" (t~', t').
 *
 * gprhip_posterior_save copies R~, R~^-1, b, t~, t (2 mp^2 + 3 mp doubles, mp = m rounded up to 128, device to device) and the
 * observed count into ONE slot, allocated at the first save after a comparison with the free device memory (GPRHIP_EOOM);
 * gprhip_posterior_restore copies them back and keeps the slot, so it may be used again.  An evaluation,
 * gprhip_load_predictor and gprhip_problem_destroy drop the slot: gprhip_posterior_restore without a saved slot of this model
 * state is GPRHIP_ESTATE.  Both need the state gprhip_observe needs.  The batch loop:
 *   save -> observe(fantasy) -> acquire -> observe(fantasy) -> ... -> restore.
 * gprhip_observed_count: observations folded in since the last evaluation or gprhip_load_predictor. */
#define GPRHIP_MAX_OBSERVE 64
int gprhip_observe(gprhip_problem* p, const double* inputs, int64_t ld, const double* targets, int k,
                   double* dlog_evidence, int on_device);
int gprhip_posterior_save(gprhip_problem* p);      /* one slot: R~, R~^-1, b, t~, t and the observed count */
int gprhip_posterior_restore(gprhip_problem* p);   /* GPRHIP_ESTATE without a saved slot of this model state */
int64_t gprhip_observed_count(const gprhip_problem* p);

/* Conditioning of the inducing covariance of the current model state: *cond_km = an estimate (power iteration on
 * U^T U and U^-1 U^-T, a lower bound within a small factor) of the 2-norm condition number of K_m + jitter, and
 * *coeff_error_bound = cond_km * unit roundoff of the n x m operands (2^-24 for GPRHIP_F32_BULK, 2^-53 for GPRHIP_F64):
 * the relative accuracy the mean coefficients (Trained.calc_mean_coeffs, lib/fitc_gp.ml:294, :288-292) can be trusted
 * to.  Log evidence and gradient do not carry that factor.  Either pointer may be NULL.
 * GPRHIP_F32_BULK problems enforce it: when the bound exceeds GPRHIP_F32_COEFF_TOL (environment, read at problem
 * creation; default 0.25, i.e. cond ~ 4e6 -- the measured coefficient error is 1/17 .. 1/3600 of this worst-case bound,
 * <= ~1.5e-2 at the threshold; 0 = never refuse) gprhip_predict (means) and gprhip_train_stats return GPRHIP_EPRECISION
 * instead of results computed from such coefficients. */
int gprhip_condition(gprhip_problem* p, double* cond_km, double* coeff_error_bound);

/* Intermediates of the last evaluation, for parity tests (copied to host; sizes in doubles):
 *   "r" n, "is" n, "v" n, "w" n, "t" m;
 *   "km"  m*m : K_m as Inducing.calc_upper leaves it (lib/cov_se_iso.ml:56-87, lib/cov_se_fat.ml:110-142, without jitter
 *               or heteroskedastic noise), Fortran m x m, upper triangle valid, zeros below;
 *   "knm_rows" rows*m (rows = len / m <= the first row chunk): the first rows of K_nm recomputed with the kernel of the
 *               last evaluation (Inputs.calc_cross, lib/cov_se_iso.ml:128-159, lib/cov_se_fat.ml:224-256), Fortran
 *               rows x m (column-major, leading dimension rows); fp32-bulk problems return the rounded stored values;
 *   "w_mat" m*m : W of Trained.prepare_hyper (lib/fitc_gp.ml:1196-1203) after a gradient evaluation, Fortran m x m, symmetric;
 *   "x_rows" rows*m : the first rows of X (lib/fitc_gp.ml:1204-1206), Fortran rows x m -- fp64 problems whose training
 *               points fit one row chunk only (the chunk buffers are reused otherwise);
 *   "uinv", "rinv" m*m : U^-1 and R~^-1 as gprhip_predict, gprhip_covariances and the other posterior calls read them,
 *               Fortran m x m, upper triangle, zeros below -- after gprhip_eval, gprhip_eval_targets, or a
 *               gprhip_load_predictor with co-variance coefficients (GPRHIP_ESTATE otherwise).  A copy: the state is untouched.
 *   "rtil" m*m : R~ as stored (R = R~ U is the reference's r_mat), Fortran m x m, upper triangle, zeros below; "bvec" m : b =
 *               R~^-T c~ (= Q_n^T y~, lib/fitc_gp.ml:285-286) -- what gprhip_observe reads and updates, under the state
 *               conditions of "rinv" ("bvec": a state with one target vector; a loaded predictor forms b = R~ (U t) first, as
 *               its first gprhip_observe would).
 *   "pg_m" m*m : M = U^-1 (I - R~^-1 R~^-T) U^-T as the product G = K M of gprhip_predict_input_grad and gprhip_acquire reads
 *               it, Fortran m x m, full -- once a call of either has asked for a variance part with more than 64 inducing
 *               points or more than 16 point dimensions (stage "pg_m"), until the next evaluation or gprhip_load_predictor
 *               (GPRHIP_ESTATE otherwise).  With len >= mp*mp, mp = m rounded up to a multiple of 128, the padded
 *               mp x mp matrix as it is stored.  A copy: the state is untouched.
 *   "sp_a" m*ns : the weights A = t 1^T + U^-1 (R~^-1 Z) of the last gprhip_sample_paths or gprhip_sample_paths_refine call
 *               as its kernels read them, Fortran m x ns with ns the draws of that call (the problem remembers the count) --
 *               from that call until the next evaluation or gprhip_load_predictor (GPRHIP_ESTATE before any such call and
 *               after either).  With len >= mp*64 the padded block as it is stored, Fortran mp x 64: rows >= m and columns
 *               >= ns are zero.  A copy: the state is untouched.
 * Returns GPRHIP_EBADARG for an unknown name. */
int gprhip_debug_fetch(gprhip_problem* p, const char* name, double* out, int64_t len);

/* Timing of evaluations with HIP events on the problem's own stream.  level 0: none (default; GPRHIP_TIMING in the
 * environment sets the initial level); 1: one event pair around the dominant kernel alone (the pass-1 SYRK launch over
 * the shard's training points, reported as "kernel_p1_syrk_B"); 2: also a pair around every stage of the evaluation. */
int gprhip_set_timing(gprhip_problem* p, int level);

/* Timings of the last evaluation (milliseconds): fills up to `cap` entries of names/ms; returns the count. */
int gprhip_last_timings(gprhip_problem* p, const char** names, float* ms, int cap);

/* ---- Several hyper-parameter sets against one data set in one pass ---------------------------------------------------
 * A multi-start optimisation, a scan over sigma2 or a cross-validation over initialisations evaluates many
 * hyper-parameter sets against the same inputs and targets.  With at most 64 inducing points one evaluation is a chain of
 * eight short launches that leaves most of the device idle; a batch runs up to GPRHIP_MAX_BATCH such
 * evaluations ("lanes") through ONE chain of launches, the lanes side by side in the grid, with one upload and one wait.
 *
 *   gprhip_batch_create   `lanes` lanes (1 .. GPRHIP_MAX_BATCH) on problem p.  The batch borrows p's resident inputs and
 *                         targets (no copy: a later gprhip_set_inputs / gprhip_set_targets on p is seen by the next batch
 *                         evaluation) and p's device and stream; every lane owns its per-evaluation state.  All lane memory,
 *                         the scratch of the first evaluation included, is compared with the device's free memory before
 *                         anything is allocated: GPRHIP_EOOM leaves nothing behind.  Only problems the small path can take
 *                         are accepted -- fp64, m <= 64, d <= 16, GPRHIP_SMALL_PATH not 0: anything else is GPRHIP_EBADARG
 *                         (such a caller loops over gprhip_eval).  Without a device: GPRHIP_EHIP.
 *   gprhip_batch_eval     evaluates h[0 .. count) on lanes 0 .. count - 1 (1 <= count <= lanes).  res[j], column j of grad
 *                         (Fortran n_hypers x count, leading dimension ldg >= n_hypers; ignored when want_grad = 0) and
 *                         column j of coeffs (Fortran m x count, or NULL) are lane j's results, status[j] its own outcome:
 *                         GPRHIP_OK or GPRHIP_ENOTPOSDEF.  A refused lane leaves its outputs unspecified and does not
 *                         disturb the others; gprhip_last_error() then holds the first refused lane's message, in
 *                         gprhip_eval's wording.  The return value speaks for the call as a whole (arguments, HIP errors).
 *                         LANE j EQUALS gprhip_eval WITH h[j] ON A PLAIN PROBLEM OF THE SAME SHAPE AND DATA, BIT FOR BIT,
 *                         for every count and every position j: a lane runs the single evaluation's workgroups, block
 *                         assignment and in-order partial sums.
 *                         All lanes of a call share one option shape: tproj, log_hetero_skedasticity and
 *                         log_multiscales_m05 each given for all or for none, `variational` and `model_only` equal;
 *                         everything else is per lane.  GPRHIP_EBADARG: count out of range, mixed option shapes, reuse_v in
 *                         any lane, a negative sigma2, hypers the small path does not take (more than 64 input dimensions
 *                         in front of a projection, multiscales with d > 8).  GPRHIP_ESTATE: inputs not set, or targets not
 *                         set with model_only = 0.  Nothing is enqueued in a refused call, and the lanes keep their state.
 *   gprhip_batch_lane     lane j's problem, owned by the batch: after a batch evaluation gprhip_predict,
 *                         gprhip_co_variance_coeffs, gprhip_condition, gprhip_train_stats, gprhip_covariances and
 *                         gprhip_debug_fetch work on it exactly as after gprhip_eval (GPRHIP_ESTATE after a refused
 *                         factorisation).  Do not evaluate, set data on or destroy a lane's problem.  Lanes count .. lanes - 1
 *                         of a shorter evaluation keep the state of their last one.
 *   p itself is not touched: its evaluation and predictor state and the validity of reuse_v survive a batch evaluation.
 *   gprhip_set_timing(gprhip_batch_lane(b, 0), 2) times the batched stages ("batch_km_chol", "batch_p1", "batch_b_chol",
 *   "batch_p2", "batch_finish"); gprhip_last_timings on lane 0 reads them.  p's own timings are not disturbed.
 *   Order of destruction: either.  A batch that outlives its problem can only be destroyed (evaluating it is GPRHIP_ESTATE,
 *   and its lanes' problems are no longer usable). */
#define GPRHIP_MAX_BATCH 64
typedef struct gprhip_batch gprhip_batch;
int gprhip_batch_create(gprhip_problem* p, int lanes, gprhip_batch** out);
void gprhip_batch_destroy(gprhip_batch* b);
int gprhip_batch_lanes(const gprhip_batch* b);
gprhip_problem* gprhip_batch_lane(gprhip_batch* b, int j);
int gprhip_batch_eval(gprhip_batch* b, int count, const gprhip_hypers* h, int want_grad, gprhip_result* res, double* grad,
                      int64_t ldg, double* coeffs, int* status);

const char* gprhip_last_error(void);
const char* gprhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GPRHIP_H */
