// gprhip.hpp -- C++ host mirror of the reference's functor surface over the C ABI of gprhip.h.
//
// The reference is compiled OCaml:  module GP = Fitc_gp.Make_deriv (Cov_se_fat.Deriv)  gives  GP.FITC,
// GP.Variational_FITC, GP.FIC, GP.Variational_FIC, each with an Eval and a Deriv side (lib/fitc_gp.mli:83-135,
// lib/interfaces.ml Sigs.Eval :373-844, Sigs.Deriv :848-1154).  This header is that surface for a C++ caller:
//
//     using GP = gpr::Make_deriv<gpr::Cov_se_iso>;                 // Fitc_gp.Make_deriv (Cov_se_iso.Deriv)
//     auto kernel   = gpr::Cov_se_iso::Kernel::create({log_ell, log_sf2});
//     auto inducing = GP::FITC::Inducing::calc(kernel, inducing_points);
//     auto inputs   = GP::FITC::Inputs::calc(inducing, training_inputs);
//     auto model    = GP::FITC::Model::calc(inputs, sigma2);
//     auto trained  = GP::FITC::Trained::calc(model, targets);
//     double l      = GP::FITC::Trained::calc_log_evidence(trained);
//     auto hyper_t  = GP::FITC::Trained::prepare_hyper(trained);
//     double dl     = GP::FITC::Trained::calc_log_evidence(hyper_t, hyper);
//
// Inputs.t, Model.t, Trained.t and hyper_t are abstract in the reference signature (lib/interfaces.ml:433, :459,
// :514, :895-899, :944-948); here they are small value types sharing one device-resident problem.  The reference
// computes stage by stage; the device path is a two-pass streaming evaluation, so these objects are lazy and the
// evaluation runs when the first number is asked for.  Errors: the reference raises Failure / Invalid_argument;
// this header throws gpr::Failure carrying the library's message and status.
//
// Header-only, C++17, links against libgprhip.so.  Matrices are column-major like the reference's Bigarrays.
#ifndef GPRHIP_HPP
#define GPRHIP_HPP

#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gprhip.h"

namespace gpr {

struct Failure : std::runtime_error {
  int status;
  Failure(int st, const std::string& msg) : std::runtime_error(msg), status(st) {}
};
inline void check(int status) {
  if (status != GPRHIP_OK) throw Failure(status, gprhip_last_error());
}

using Vec = std::vector<double>;
// Column-major matrix (Lacaml.D.mat): element (r, c), 0-based, at a[c * rows + r].
struct Mat {
  int rows = 0, cols = 0;
  std::vector<double> a;
  Mat() = default;
  Mat(int r, int c, double v = 0.0) : rows(r), cols(c), a((size_t)r * c, v) {}
  double& operator()(int r, int c) { return a[(size_t)c * rows + r]; }
  double operator()(int r, int c) const { return a[(size_t)c * rows + r]; }
  const double* data() const { return a.data(); }
  double* data() { return a.data(); }
};
using MatP = std::shared_ptr<const Mat>;  // physical identity stands in for the reference's phys_equal checks

constexpr double cholesky_jitter = 1e-6;  // Utils.cholesky_jitter, lib/utils.ml:35

// One hyper-parameter of either covariance (Cov_se_iso.Hyper.t lib/cov_se_iso.ml:27-28, Cov_se_fat.Hyper.t
// lib/cov_se_fat.ml:258-284); ind / dim / big_dim / small_dim are 1-based like the reference.
struct Hyper {
  enum Kind { Log_ell, Log_sf2, Inducing_hyper, Proj, Log_hetero_skedasticity, Log_multiscale_m05 } kind;
  int ind = 0, dim = 0;  // Inducing_hyper{ind; dim}, Log_multiscale_m05{ind; dim}, Log_hetero_skedasticity dim
  int big_dim = 0, small_dim = 0;  // Proj{big_dim; small_dim}
};

// ---- Cov_se_iso (lib/cov_se_iso.ml) -----------------------------------------------------------------------
struct Cov_se_iso {
  static constexpr int cov_kind = GPRHIP_COV_SE_ISO;
  struct Params { double log_ell = 0.0, log_sf2 = 0.0; };  // :23-25; create_default_kernel_params :122-123
  struct Kernel {
    Params params;
    double inv_ell2 = 1.0, inv_ell2_05 = -0.5, log_sf2 = 0.0, sf2 = 1.0;
    static Kernel create(const Params& p) {  // :41-44
      Kernel k;
      k.params = p;
      k.inv_ell2 = std::exp(-2.0 * p.log_ell);
      k.inv_ell2_05 = -0.5 * k.inv_ell2;
      k.log_sf2 = p.log_sf2;
      k.sf2 = std::exp(p.log_sf2);
      return k;
    }
  };
  static int kernel_space_dim(const Kernel&, const Mat& inputs) { return inputs.rows; }
  static void fill(const Kernel& k, gprhip_hypers& h) {
    h.log_ell = k.params.log_ell;
    h.log_sf2 = k.params.log_sf2;
  }
  static int flags(const Kernel&) { return 0; }
  static std::vector<Hyper> get_all(const Kernel&, const Mat& inducing) {  // :188-202
    std::vector<Hyper> hs{{Hyper::Log_ell}, {Hyper::Log_sf2}};
    for (int ind = 1; ind <= inducing.cols; ++ind)
      for (int dim = 1; dim <= inducing.rows; ++dim) hs.push_back({Hyper::Inducing_hyper, ind, dim});
    return hs;
  }
  static double get_value(const Kernel& k, const Mat& inducing, const Hyper& h) {  // :204-207
    if (h.kind == Hyper::Log_ell) return k.params.log_ell;
    if (h.kind == Hyper::Log_sf2) return k.params.log_sf2;
    if (h.kind != Hyper::Inducing_hyper) throw Failure(GPRHIP_EBADARG, "Cov_se_iso.Hyper.get_value: foreign hyper");
    return inducing(h.dim - 1, h.ind - 1);
  }
  // :209-229 (the inducing matrix is copied only if one of its entries is set)
  static std::pair<Kernel, MatP> set_values(const Kernel& k, const MatP& inducing, const std::vector<Hyper>& hs,
                                            const Vec& values) {
    Params p = k.params;
    std::shared_ptr<Mat> z;
    for (size_t i = 0; i < hs.size(); ++i) {
      if (hs[i].kind == Hyper::Log_ell) p.log_ell = values[i];
      else if (hs[i].kind == Hyper::Log_sf2) p.log_sf2 = values[i];
      else {
        if (!z) z = std::make_shared<Mat>(*inducing);
        (*z)(hs[i].dim - 1, hs[i].ind - 1) = values[i];
      }
    }
    return {Kernel::create(p), z ? MatP(z) : inducing};
  }
  static int64_t index_of(const Kernel&, const Mat& inducing, const Hyper& h) {  // position in get_all
    if (h.kind == Hyper::Log_ell) return 0;
    if (h.kind == Hyper::Log_sf2) return 1;
    return 2 + (int64_t)(h.ind - 1) * inducing.rows + (h.dim - 1);
  }
};

// ---- Cov_se_fat (lib/cov_se_fat.ml) -----------------------------------------------------------------------
struct Cov_se_fat {
  static constexpr int cov_kind = GPRHIP_COV_SE_FAT;
  struct Params {  // :27-49
    int d = 0;
    double log_sf2 = 0.0;
    std::optional<Mat> tproj;                    // big_dim x d
    std::optional<Vec> log_hetero_skedasticity;  // m
    std::optional<Mat> log_multiscales_m05;      // d x m
    static Params create(Params p) {             // :38-48
      if (p.tproj && p.tproj->cols != p.d)
        throw Failure(GPRHIP_EBADARG, "Cov_se_fat.Params.create: tproj projection (" + std::to_string(p.tproj->cols) +
                                          ") disagrees with target dimension d (" + std::to_string(p.d) + ")");
      return p;
    }
  };
  struct Kernel {
    Params params;
    double sf2 = 1.0;
    static Kernel create(const Params& p) { return Kernel{p, std::exp(p.log_sf2)}; }  // :62-75
  };
  static int kernel_space_dim(const Kernel& k, const Mat&) { return k.params.d; }
  static void fill(const Kernel& k, gprhip_hypers& h) {
    h.log_sf2 = k.params.log_sf2;
    h.tproj = k.params.tproj ? k.params.tproj->data() : nullptr;
    h.log_hetero_skedasticity = k.params.log_hetero_skedasticity ? k.params.log_hetero_skedasticity->data() : nullptr;
    h.log_multiscales_m05 = k.params.log_multiscales_m05 ? k.params.log_multiscales_m05->data() : nullptr;
  }
  static int flags(const Kernel& k) {
    return (k.params.tproj ? 1 : 0) | (k.params.log_hetero_skedasticity ? 2 : 0) |
           (k.params.log_multiscales_m05 ? 4 : 0);
  }
  static std::vector<Hyper> get_all(const Kernel& k, const Mat& inducing) {  // :290-342
    const int d = k.params.d, m = inducing.cols;
    std::vector<Hyper> hs{{Hyper::Log_sf2}};
    for (int ind = 1; ind <= m; ++ind)
      for (int dim = 1; dim <= d; ++dim) hs.push_back({Hyper::Inducing_hyper, ind, dim});
    if (k.params.tproj)
      for (int big = 1; big <= k.params.tproj->rows; ++big)
        for (int small = 1; small <= d; ++small) hs.push_back({Hyper::Proj, 0, 0, big, small});
    if (k.params.log_hetero_skedasticity)
      for (int i = 1; i <= m; ++i) hs.push_back({Hyper::Log_hetero_skedasticity, 0, i});
    if (k.params.log_multiscales_m05)
      for (int ind = 1; ind <= m; ++ind)
        for (int dim = 1; dim <= d; ++dim) hs.push_back({Hyper::Log_multiscale_m05, ind, dim});
    return hs;
  }
  static double get_value(const Kernel& k, const Mat& inducing, const Hyper& h) {  // :344-362
    auto missing = [](const char* what) {
      return Failure(GPRHIP_EBADARG, std::string("Deriv.Hyper.option_get_value: ") + what + " not supported");
    };
    switch (h.kind) {
      case Hyper::Log_sf2: return k.params.log_sf2;
      case Hyper::Inducing_hyper: return inducing(h.dim - 1, h.ind - 1);
      case Hyper::Proj:
        if (!k.params.tproj) throw missing("tproj");
        return (*k.params.tproj)(h.big_dim - 1, h.small_dim - 1);
      case Hyper::Log_hetero_skedasticity:
        if (!k.params.log_hetero_skedasticity) throw missing("log_hetero_skedasticity");
        return (*k.params.log_hetero_skedasticity)[h.dim - 1];
      case Hyper::Log_multiscale_m05:
        if (!k.params.log_multiscales_m05) throw missing("log_multiscales_m05");
        return (*k.params.log_multiscales_m05)(h.dim - 1, h.ind - 1);
      default: throw Failure(GPRHIP_EBADARG, "Cov_se_fat.Hyper.get_value: foreign hyper");
    }
  }
  static std::pair<Kernel, MatP> set_values(const Kernel& k, const MatP& inducing, const std::vector<Hyper>& hs,
                                            const Vec& values) {  // :364-407
    Params p = k.params;
    std::shared_ptr<Mat> z;
    for (size_t i = 0; i < hs.size(); ++i) {
      const Hyper& h = hs[i];
      switch (h.kind) {
        case Hyper::Log_sf2: p.log_sf2 = values[i]; break;
        case Hyper::Inducing_hyper:
          if (!z) z = std::make_shared<Mat>(*inducing);
          (*z)(h.dim - 1, h.ind - 1) = values[i];
          break;
        case Hyper::Proj:
          if (!p.tproj) throw Failure(GPRHIP_EBADARG, "Deriv.Hyper.option_get_value: tproj not supported");
          (*p.tproj)(h.big_dim - 1, h.small_dim - 1) = values[i];
          break;
        case Hyper::Log_hetero_skedasticity:
          if (!p.log_hetero_skedasticity)
            throw Failure(GPRHIP_EBADARG, "Deriv.Hyper.option_get_value: log_hetero_skedasticity not supported");
          (*p.log_hetero_skedasticity)[h.dim - 1] = values[i];
          break;
        case Hyper::Log_multiscale_m05:
          if (!p.log_multiscales_m05)
            throw Failure(GPRHIP_EBADARG, "Deriv.Hyper.option_get_value: log_multiscales_m05 not supported");
          (*p.log_multiscales_m05)(h.dim - 1, h.ind - 1) = values[i];
          break;
        default: throw Failure(GPRHIP_EBADARG, "Cov_se_fat.Hyper.set_values: foreign hyper");
      }
    }
    return {Kernel::create(p), z ? MatP(z) : inducing};
  }
  static int64_t index_of(const Kernel& k, const Mat& inducing, const Hyper& h) {
    const int64_t d = k.params.d, m = inducing.cols;
    const int64_t nproj = k.params.tproj ? (int64_t)k.params.tproj->rows * d : 0;
    const int64_t nhet = k.params.log_hetero_skedasticity ? m : 0;
    switch (h.kind) {
      case Hyper::Log_sf2: return 0;
      case Hyper::Inducing_hyper: return 1 + (h.ind - 1) * d + (h.dim - 1);
      case Hyper::Proj: return 1 + d * m + (h.big_dim - 1) * d + (h.small_dim - 1);
      case Hyper::Log_hetero_skedasticity: return 1 + d * m + nproj + (h.dim - 1);
      case Hyper::Log_multiscale_m05: return 1 + d * m + nproj + nhet + (h.ind - 1) * d + (h.dim - 1);
      default: throw Failure(GPRHIP_EBADARG, "Cov_se_fat.Hyper.index_of: foreign hyper");
    }
  }
};

// Device-resident problem (RAII over gprhip_problem): one per (training inputs, m, d).
class Problem {
 public:
  Problem(int cov_kind, int64_t n, int D, int d, int m, int device = 0, int precision = GPRHIP_F64,
          int64_t chunk_rows = 0)
      : n(n), D(D), d(d), m(m) {
    check(gprhip_problem_create_ex(device, cov_kind, precision, n, D, d, m, chunk_rows, &p_));
  }
  ~Problem() { gprhip_problem_destroy(p_); }
  Problem(const Problem&) = delete;
  Problem& operator=(const Problem&) = delete;
  gprhip_problem* get() const { return p_; }
  const int64_t n;
  const int D, d, m;
  // identities are kept alive while they are remembered, so a recycled address can never match by accident
  std::shared_ptr<const void> state_owner;    // which evaluation's factors the device holds right now
  std::shared_ptr<const void> last_kernel;    // for Model.update_sigma2's re-use of K_nm, V, r
  std::shared_ptr<const void> last_inducing;

 private:
  gprhip_problem* p_ = nullptr;
};

struct Evaluation {  // everything one device evaluation returns
  double l1 = 0, l2 = 0, l = 0, dl_dsigma2 = 0;
  Vec grad;    // Hyper.get_all order
  Vec coeffs;  // Trained.calc_mean_coeffs
  bool has_grad = false;
};

// Several hyper-parameter sets against one problem's resident data in one pass (RAII over gprhip_batch; include/gprhip.h,
// "Several hyper-parameter sets ..."): eval() takes one gprhip_hypers per lane and returns one Evaluation and one status
// per lane; lane(j) is lane j's device problem for predictions.  The batch may be destroyed before or after its problem.
class Batch {
 public:
  Batch(Problem& p, int lanes) : m_(p.m) {
    check(gprhip_batch_create(p.get(), lanes, &b_));
  }
  ~Batch() { gprhip_batch_destroy(b_); }
  Batch(const Batch&) = delete;
  Batch& operator=(const Batch&) = delete;
  gprhip_batch* get() const { return b_; }
  int lanes() const { return gprhip_batch_lanes(b_); }
  gprhip_problem* lane(int j) const { return gprhip_batch_lane(b_, j); }
  // status[j] is GPRHIP_OK or GPRHIP_ENOTPOSDEF (that lane's Evaluation is then unspecified); anything else throws
  std::vector<Evaluation> eval(const std::vector<gprhip_hypers>& h, bool want_grad, std::vector<int>& status) {
    const int count = (int)h.size();
    const gprhip_hypers* h0 = count ? &h[0] : nullptr;
    const int flags = h0 ? (h0->tproj ? 1 : 0) | (h0->log_hetero_skedasticity ? 2 : 0) | (h0->log_multiscales_m05 ? 4 : 0) : 0;
    const int64_t nh = gprhip_n_hypers(lane(0), flags);  // (a lane's problem has the parent's shape)
    std::vector<gprhip_result> res(count ? count : 1);
    std::vector<double> grad((size_t)nh * (count ? count : 1)), coeffs((size_t)m_ * (count ? count : 1));
    status.assign(count ? count : 1, GPRHIP_OK);
    check(gprhip_batch_eval(b_, count, h0, want_grad ? 1 : 0, res.data(), grad.data(), nh, coeffs.data(), status.data()));
    status.resize(count);
    std::vector<Evaluation> out(count);
    for (int j = 0; j < count; ++j) {
      if (status[j] != GPRHIP_OK) continue;
      Evaluation& e = out[j];
      e.l1 = res[j].l1; e.l2 = res[j].l2; e.l = res[j].l; e.dl_dsigma2 = res[j].dl_dsigma2;
      e.has_grad = want_grad;
      if (want_grad) e.grad.assign(grad.begin() + (size_t)j * nh, grad.begin() + (size_t)j * nh + res[j].n_hypers);
      e.coeffs.assign(coeffs.begin() + (size_t)j * m_, coeffs.begin() + (size_t)(j + 1) * m_);
    }
    return out;
  }

 private:
  gprhip_batch* b_ = nullptr;
  int m_;
};

struct Evaluation_many {  // gprhip_eval_targets: k target vectors (the columns of an n x k matrix) on one model
  double l1 = 0, l_sum = 0, dl_dsigma2_sum = 0;
  Vec l;        // k values: Trained.calc_log_evidence per target
  Vec grad_sum; // gradient of l_sum, Hyper.get_all order
  Mat coeffs;   // m x k: Trained.calc_mean_coeffs per column
  bool has_grad = false;
};

struct Stats_t {  // Stats.t, lib/fitc_gp.ml:304-315
  int64_t n_samples;
  double target_variance, sse, mse, rmse, smse, msll, mad, maxad;
};

// Fitc_gp.Make_deriv (lib/fitc_gp.mli:120-135)
template <class Spec>
struct Make_deriv {
  using Kernel = typename Spec::Kernel;

  struct Inducing_t {  // Eval.Inducing.t
    Kernel kernel;
    MatP points;
  };
  struct Inputs_t {  // Eval.Inputs.t
    Inducing_t inducing;
    MatP points;
    std::shared_ptr<Problem> problem;  // null for inputs that are only predicted at
  };
  struct Model_t {  // Eval.Model.t / Deriv.Model.t
    Inputs_t inputs;
    double sigma2 = 0;
    bool variational = false;
    std::shared_ptr<Kernel> kernel_ref;  // identity of the kernel (shared by update_sigma2 copies)
    std::shared_ptr<std::map<bool, Evaluation>> ev = std::make_shared<std::map<bool, Evaluation>>();
    std::shared_ptr<int> id = std::make_shared<int>(0);  // identity of this model for the device-state bookkeeping
  };
  struct Trained_t {  // Eval.Trained.t / Deriv.Trained.t
    Model_t model;
    Vec targets;
    bool want_grad = false;
    std::shared_ptr<std::optional<Evaluation>> ev = std::make_shared<std::optional<Evaluation>>();
    std::shared_ptr<int> id = std::make_shared<int>(0);
  };
  struct Hyper_t {  // Deriv.Model.hyper_t / Deriv.Trained.hyper_t
    Evaluation ev;
    Kernel kernel;
    MatP inducing;
  };
  struct Variances_t { Vec variances; double sigma2; };
  struct Covariances_t { MatP points; Mat covariances; double sigma2; std::shared_ptr<Problem> problem; };
  // Mean_predictor.t / Co_variance_predictor.t built from stored numbers (lib/fitc_gp.ml:377-391, :429-447) rather
  // than from a model on the device -- the `test` flow of bin/ocaml_gpr.ml:373-413.  The device problem that serves
  // it is created on first use, sized for the batch it is asked about.
  struct Standalone_t {
    MatP inducing;
    std::optional<Vec> coeffs;
    std::optional<Kernel> kernel;
    std::optional<std::pair<Mat, Mat>> cov_coeffs;  // (chol_km, r_mat)
    std::shared_ptr<std::shared_ptr<Problem>> prob = std::make_shared<std::shared_ptr<Problem>>();
  };
  struct Cov_sampler_t { Vec means; Covariances_t covariances; double add_diag; };

  // one evaluation on the device: multim_f / multim_dcommon, lib/fitc_gp.ml:1601-1636
  static Evaluation run(const Model_t& model, const Vec* targets, bool want_grad, std::shared_ptr<const void> owner) {
    Problem& prob = *model.inputs.problem;
    const Kernel& k = model.inputs.inducing.kernel;
    const Mat& z = *model.inputs.inducing.points;
    if (targets) check(gprhip_set_targets(prob.get(), targets->data()));
    gprhip_hypers h{};
    Spec::fill(k, h);
    h.sigma2 = model.sigma2;
    h.inducing = z.data();
    h.variational = model.variational;
    h.model_only = targets ? 0 : 1;
    h.jitter = cholesky_jitter;
    // Model.update_sigma2 (lib/fitc_gp.ml:234-236): same kernel object and inducing matrix as the problem's
    // previous evaluation -> only sigma2 changed, K_nm / V / r stay on the device
    h.reuse_v = (prob.last_kernel == model.kernel_ref && prob.last_inducing == model.inputs.inducing.points);
    Evaluation ev;
    ev.grad.assign((size_t)std::max<int64_t>(1, gprhip_n_hypers(prob.get(), Spec::flags(k))), 0.0);
    ev.coeffs.assign((size_t)prob.m, 0.0);
    gprhip_result r{};
    check(gprhip_eval(prob.get(), &h, want_grad, &r, ev.grad.data(), ev.coeffs.data()));
    ev.l1 = r.l1; ev.l2 = r.l2; ev.l = r.l; ev.dl_dsigma2 = r.dl_dsigma2;
    ev.has_grad = want_grad;
    if (want_grad) ev.grad.resize((size_t)r.n_hypers);
    prob.last_kernel = model.kernel_ref;
    prob.last_inducing = model.inputs.inducing.points;
    prob.state_owner = std::move(owner);
    return ev;
  }

  // A gradient evaluation that also returns the D x n gradient of the log evidence with respect to the training inputs
  // (gprhip_eval_input_grad: an extension beyond the reference's signature; fp64 problems, no multiscales) -- what
  // gpr_amd/fitc_gp.py calls Deriv.Trained.calc_input_gradient (targets given) / Deriv.Model.calc_input_gradient (null).
  // `owner` as in run.
  static Evaluation run_input_grad(const Model_t& model, const Vec* targets, Mat& dl_dinputs, std::shared_ptr<const void> owner) {
    Problem& prob = *model.inputs.problem;
    const Kernel& k = model.inputs.inducing.kernel;
    const Mat& z = *model.inputs.inducing.points;
    if (targets) check(gprhip_set_targets(prob.get(), targets->data()));
    gprhip_hypers h{};
    Spec::fill(k, h);
    h.sigma2 = model.sigma2;
    h.inducing = z.data();
    h.variational = model.variational;
    h.model_only = targets ? 0 : 1;
    h.jitter = cholesky_jitter;
    h.reuse_v = (prob.last_kernel == model.kernel_ref && prob.last_inducing == model.inputs.inducing.points);
    Evaluation ev;
    ev.grad.assign((size_t)std::max<int64_t>(1, gprhip_n_hypers(prob.get(), Spec::flags(k))), 0.0);
    ev.coeffs.assign((size_t)prob.m, 0.0);
    dl_dinputs = Mat(prob.D, (int)prob.n);
    gprhip_result r{};
    check(gprhip_eval_input_grad(prob.get(), &h, &r, ev.grad.data(), ev.coeffs.data(), dl_dinputs.data(), prob.D, 0));
    ev.l1 = r.l1; ev.l2 = r.l2; ev.l = r.l; ev.dl_dsigma2 = r.dl_dsigma2;
    ev.has_grad = true;
    ev.grad.resize((size_t)r.n_hypers);
    prob.last_kernel = model.kernel_ref;
    prob.last_inducing = model.inputs.inducing.points;
    prob.state_owner = std::move(owner);
    return ev;
  }

  // Several target vectors on one model in one device evaluation (an extension beyond the reference's signature, whose
  // Trained.t holds one target vector); the Variational flag travels in the model, so the two helpers serve every variant
  // (what gpr_amd/fitc_gp.py calls Trained.calc_many).  `owner` as in run.
  static Evaluation_many run_many(const Model_t& model, const Mat& targets, bool want_grad, std::shared_ptr<const void> owner) {
    Problem& prob = *model.inputs.problem;
    const Kernel& k = model.inputs.inducing.kernel;
    const Mat& z = *model.inputs.inducing.points;
    check(gprhip_set_targets_many(prob.get(), targets.data(), targets.rows, targets.cols));
    gprhip_hypers h{};
    Spec::fill(k, h);
    h.sigma2 = model.sigma2;
    h.inducing = z.data();
    h.variational = model.variational;
    h.model_only = 0;
    h.jitter = cholesky_jitter;
    h.reuse_v = (prob.last_kernel == model.kernel_ref && prob.last_inducing == model.inputs.inducing.points);
    Evaluation_many ev;
    ev.grad_sum.assign((size_t)std::max<int64_t>(1, gprhip_n_hypers(prob.get(), Spec::flags(k))), 0.0);
    ev.coeffs = Mat((int)prob.m, targets.cols);
    ev.l.assign((size_t)targets.cols, 0.0);
    gprhip_targets_result r{};
    check(gprhip_eval_targets(prob.get(), &h, want_grad, &r, ev.l.data(), ev.grad_sum.data(), ev.coeffs.data()));
    for (double& v : ev.l) v += r.l1;  // (the call returns l2 per target)
    ev.l1 = r.l1; ev.l_sum = r.l_sum; ev.dl_dsigma2_sum = r.dl_dsigma2_sum;
    ev.has_grad = want_grad;
    if (want_grad) ev.grad_sum.resize((size_t)r.n_hypers);
    prob.last_kernel = model.kernel_ref;
    prob.last_inducing = model.inputs.inducing.points;
    prob.state_owner = std::move(owner);
    return ev;
  }
  // Means.calc per target column at the points of `in` (nt x k), from the state run_many left on the model's problem
  static Mat means_many(const Model_t& model, const Inputs_t& in, int k) {
    Mat means(in.points->cols, k);
    check(gprhip_predict_targets(model.inputs.problem->get(), in.points->data(), in.points->rows, in.points->cols, means.data()));
    return means;
  }

  template <bool Variational, int CovKind /* 0 FITC, 1 FIC */>
  struct Variant {
    struct Inducing {
      static Inducing_t calc(const Kernel& kernel, MatP points) { return {kernel, std::move(points)}; }
      static MatP get_points(const Inducing_t& i) { return i.points; }
    };
    struct Inputs {
      // Inputs.calc (lib/fitc_gp.ml:108-115).  `train` = these are training inputs: make them device-resident.
      static Inputs_t calc(const Inducing_t& inducing, MatP points, bool train = true, int device = 0,
                           int precision = GPRHIP_F64) {
        const int d = Spec::kernel_space_dim(inducing.kernel, *points);
        if (inducing.points->rows != d)
          throw Failure(GPRHIP_EBADARG, "Inputs.calc: inducing points and kernel space disagree about the dimension");
        Inputs_t in{inducing, points, nullptr};
        if (train) {
          in.problem = std::make_shared<Problem>(Spec::cov_kind, points->cols, points->rows, d,
                                                 inducing.points->cols, device, precision);
          check(gprhip_set_inputs(in.problem->get(), points->data(), points->rows));
        }
        return in;
      }
      // the same training inputs under new hyper-parameters (what the optimiser does every iteration)
      static Inputs_t recalc(const Inputs_t& old, const Inducing_t& inducing) {
        return {inducing, old.points, old.problem};
      }
    };
    struct Model {
      static Model_t calc(const Inputs_t& inputs, double sigma2) {
        if (sigma2 < 0.0) throw Failure(GPRHIP_EBADARG, "Model.check_sigma2: sigma2 < 0");  // lib/fitc_gp.ml:148-149
        if (!inputs.problem) throw Failure(GPRHIP_ESTATE, "Model.calc: inputs were not created as training inputs");
        Model_t m;
        m.inputs = inputs;
        m.sigma2 = sigma2;
        m.variational = Variational;
        m.kernel_ref = std::make_shared<Kernel>(inputs.inducing.kernel);
        return m;
      }
      static Model_t update_sigma2(const Model_t& model, double sigma2) {  // lib/fitc_gp.ml:234-236
        Model_t m = calc(model.inputs, sigma2);
        m.kernel_ref = model.kernel_ref;  // same kernel identity: the device keeps K_nm, V, r
        return m;
      }
      static const Evaluation& evaluation(const Model_t& m, bool want_grad) {
        auto it = m.ev->find(true);
        if (it != m.ev->end()) return it->second;
        it = m.ev->find(want_grad);
        if (it == m.ev->end()) it = m.ev->emplace(want_grad, run(m, nullptr, want_grad, m.id)).first;
        return it->second;
      }
      static void ensure_state(const Model_t& m) {
        if (m.inputs.problem->state_owner == m.id) return;
        (*m.ev)[false] = run(m, nullptr, false, m.id);
      }
      static double calc_log_evidence(const Model_t& m) { return evaluation(m, false).l1; }        // :238
      static double calc_log_evidence_sigma2(const Model_t& m) { return evaluation(m, true).dl_dsigma2; }  // :1121
      static Hyper_t prepare_hyper(const Model_t& m) {                                             // :1126-1136
        return {evaluation(m, true), m.inputs.inducing.kernel, m.inputs.inducing.points};
      }
      static double calc_log_evidence(const Hyper_t& ht, const Hyper& h) {
        return ht.ev.grad[(size_t)Spec::index_of(ht.kernel, *ht.inducing, h)];
      }
      static std::pair<Mat, Mat> calc_co_variance_coeffs(const Model_t& m) {  // :240
        ensure_state(m);
        const int mm = m.inputs.problem->m;
        Mat u(mm, mm), r(mm, mm);
        check(gprhip_co_variance_coeffs(m.inputs.problem->get(), u.data(), r.data()));
        return {u, r};
      }
      static double get_sigma2(const Model_t& m) { return m.sigma2; }
    };
    struct Trained {
      static Trained_t calc(const Model_t& model, const Vec& targets, bool want_grad = true) {
        if ((int64_t)targets.size() != model.inputs.problem->n)  // lib/fitc_gp.ml:283-284
          throw Failure(GPRHIP_EBADARG, "Trained.calc: Vec.dim targets (" + std::to_string(targets.size()) +
                                            ") <> n (" + std::to_string(model.inputs.problem->n) + ")");
        Trained_t t;
        t.model = model;
        t.targets = targets;
        t.want_grad = want_grad;
        return t;
      }
      static const Evaluation& evaluation(const Trained_t& t) {
        if (!*t.ev) *t.ev = run(t.model, &t.targets, t.want_grad, t.id);
        return **t.ev;
      }
      static void ensure_state(const Trained_t& t) {
        if (*t.ev && t.model.inputs.problem->state_owner == t.id) return;
        *t.ev = run(t.model, &t.targets, t.want_grad, t.id);
      }
      static double calc_log_evidence(const Trained_t& t) { return evaluation(t).l; }                 // :295
      static const Vec& calc_mean_coeffs(const Trained_t& t) { return evaluation(t).coeffs; }         // :294
      static double calc_log_evidence_sigma2(const Trained_t& t) { return evaluation(t).dl_dsigma2; } // :1187
      static Hyper_t prepare_hyper(const Trained_t& t) {                                              // :1192-1207
        if (!t.want_grad) throw Failure(GPRHIP_ESTATE, "Trained.prepare_hyper: created without derivatives");
        return {evaluation(t), t.model.inputs.inducing.kernel, t.model.inputs.inducing.points};
      }
      static double calc_log_evidence(const Hyper_t& ht, const Hyper& h) {                            // :1005-1021
        return ht.ev.grad[(size_t)Spec::index_of(ht.kernel, *ht.inducing, h)];
      }
      static Vec calc_means(const Trained_t& t) {                                                     // :296-297
        ensure_state(t);
        Vec means((size_t)t.model.inputs.problem->n);
        double sums[4];
        check(gprhip_train_stats(t.model.inputs.problem->get(), means.data(), sums));
        return means;
      }
    };
    struct Stats {
      static Stats_t calc(const Trained_t& t) {  // lib/fitc_gp.ml:353-373
        Trained::ensure_state(t);
        double s[4];
        check(gprhip_train_stats(t.model.inputs.problem->get(), nullptr, s));
        const double n = (double)t.targets.size();
        Stats_t st;
        st.n_samples = (int64_t)t.targets.size();
        st.target_variance = s[3] / n;
        st.sse = s[0];
        st.mse = s[0] / n;
        st.rmse = std::sqrt(st.mse);
        st.smse = st.mse / st.target_variance;
        const double pi = 3.14159265358979323846;
        st.msll = (-0.5 * std::log(2.0 * pi * st.target_variance) - 0.5) - Trained::evaluation(t).l / n;
        st.mad = s[1] / n;
        st.maxad = s[2];
        return st;
      }
    };
    // ---- prediction at new inputs from a trained model (Means / Variances / Covariances, :416-627)
    static Problem& problem_for(const Trained_t& t, const Inputs_t& in, const char* who) {
      if (in.inducing.points != t.model.inputs.inducing.points)  // phys_equal check, :419-424
        throw Failure(GPRHIP_EBADARG, std::string(who) + ": trained and inputs disagree about inducing points");
      Trained::ensure_state(t);
      return *t.model.inputs.problem;
    }
    static Problem& problem_for(const Model_t& m, const Inputs_t& in, const char* who) {
      if (in.inducing.points != m.inputs.inducing.points)
        throw Failure(GPRHIP_EBADARG, std::string(who) + ": co-variance predictor and inputs disagree about "
                                                           "inducing points");
      Model::ensure_state(m);
      return *m.inputs.problem;
    }
    static Problem& problem_for(const Standalone_t& sa, const Inputs_t& in, const char* who, double sigma2 = 0.0) {
      if (in.inducing.points != sa.inducing)
        throw Failure(GPRHIP_EBADARG, std::string(who) + ": predictor and inputs disagree about inducing points");
      const Kernel& k = sa.kernel ? *sa.kernel : in.inducing.kernel;
      const Mat& pts = *in.points;
      std::shared_ptr<Problem>& prob = *sa.prob;
      if (!prob || prob->D != pts.rows || prob->n < pts.cols)
        prob = std::make_shared<Problem>(Spec::cov_kind, std::max(pts.cols, 1024), pts.rows, sa.inducing->rows,
                                         sa.inducing->cols);
      gprhip_hypers h{};
      Spec::fill(k, h);
      h.sigma2 = sigma2;
      h.inducing = sa.inducing->data();
      h.jitter = cholesky_jitter;
      check(gprhip_load_predictor(prob->get(), &h, sa.coeffs ? sa.coeffs->data() : nullptr,
                                  sa.cov_coeffs ? sa.cov_coeffs->first.data() : nullptr,
                                  sa.cov_coeffs ? sa.cov_coeffs->second.data() : nullptr));
      prob->state_owner = sa.prob;
      return *prob;
    }
    static Problem& problem_of(const Trained_t& t, const Inputs_t& in, const char* who, double) {
      return problem_for(t, in, who);
    }
    static Problem& problem_of(const Model_t& m, const Inputs_t& in, const char* who, double) {
      return problem_for(m, in, who);
    }
    static Problem& problem_of(const Standalone_t& sa, const Inputs_t& in, const char* who, double sigma2) {
      return problem_for(sa, in, who, sigma2);
    }
    static std::shared_ptr<Problem> owner_problem(const Trained_t& t) { return t.model.inputs.problem; }
    static std::shared_ptr<Problem> owner_problem(const Model_t& m) { return m.inputs.problem; }
    static std::shared_ptr<Problem> owner_problem(const Standalone_t& sa) { return *sa.prob; }
    struct Mean_predictor {
      static const Trained_t& calc_trained(const Trained_t& t) { return t; }  // :380-384
      static Standalone_t calc(MatP inducing_points, const Vec& coeffs) {     // :386-391
        if ((size_t)inducing_points->cols != coeffs.size())
          throw Failure(GPRHIP_EBADARG, "Mean_predictor.calc: number of inducing points disagrees with dimension of "
                                        "coefficients");
        Standalone_t sa;
        sa.inducing = std::move(inducing_points);
        sa.coeffs = coeffs;
        return sa;
      }
    };
    struct Co_variance_predictor {
      static const Model_t& calc_model(const Model_t& m) { return m; }        // :438-444
      static Standalone_t calc(const Kernel& kernel, MatP inducing_points, const std::pair<Mat, Mat>& coeffs) {  // :446-447
        Standalone_t sa;
        sa.inducing = std::move(inducing_points);
        sa.kernel = kernel;
        sa.cov_coeffs = coeffs;
        return sa;
      }
    };
    struct Means {
      static Vec calc(const Standalone_t& mean_predictor, const Inputs_t& in) {
        Problem& p = problem_for(mean_predictor, in, "Means.calc");
        Vec means((size_t)in.points->cols);
        check(gprhip_predict(p.get(), in.points->data(), in.points->rows, in.points->cols, 0, means.data(), nullptr));
        return means;
      }
      static Vec calc(const Trained_t& mean_predictor, const Inputs_t& in) {  // :418-425
        Problem& p = problem_for(mean_predictor, in, "Means.calc");
        Vec means((size_t)in.points->cols);
        check(gprhip_predict(p.get(), in.points->data(), in.points->rows, in.points->cols, 0, means.data(), nullptr));
        return means;
      }
      // D x nt gradient of the means with respect to the test inputs (gprhip_predict_input_grad: an extension beyond the
      // reference's implemented surface; fp64 problems, no multiscales, at most 64 point dimensions on the kernel side)
      template <class Owner>
      static Mat calc_input_gradient(const Owner& mean_predictor, const Inputs_t& in) {
        Problem& p = problem_for(mean_predictor, in, "Means.calc_input_gradient");
        Mat g(in.points->rows, in.points->cols);
        check(gprhip_predict_input_grad(p.get(), in.points->data(), in.points->rows, in.points->cols, 0, nullptr, nullptr,
                                        g.data(), nullptr, in.points->rows, 0));
        return g;
      }
    };
    struct Variances {
      template <class Owner>
      static Variances_t calc(const Owner& cvp, double sigma2, const Inputs_t& in) {  // :498-518
        Problem& p = problem_of(cvp, in, "Variances.calc", sigma2);
        Variances_t v{Vec((size_t)in.points->cols), sigma2};
        check(gprhip_predict(p.get(), in.points->data(), in.points->rows, in.points->cols, 0, nullptr,
                             v.variances.data()));
        return v;
      }
      // D x nt gradient of the variances with respect to the test inputs (the same for predictive and latent variances)
      template <class Owner>
      static Mat calc_input_gradient(const Owner& cvp, double sigma2, const Inputs_t& in) {
        Problem& p = problem_of(cvp, in, "Variances.calc_input_gradient", sigma2);
        Mat g(in.points->rows, in.points->cols);
        check(gprhip_predict_input_grad(p.get(), in.points->data(), in.points->rows, in.points->cols, 0, nullptr, nullptr,
                                        nullptr, g.data(), in.points->rows, 0));
        return g;
      }
      static Vec get(const Variances_t& v, bool predictive = true) {  // :520-529
        Vec out = v.variances;
        if (predictive)
          for (double& x : out) x += v.sigma2;
        return out;
      }
    };
    // An acquisition criterion over the test inputs with its D x nt gradient and the best top_k candidates (gprhip_acquire:
    // an extension beyond the reference's implemented surface).  top_index holds -1 where fewer than top_k qualify.
    struct Acquired_t {
      Vec values;
      Mat dvalues;
      std::vector<int64_t> top_index;
      Vec top_values;
      Mat top_dvalues;
    };
    struct Refined_t {
      Mat x;         // D x ns
      Vec values;    // value and gradient at x
      Mat dvalues;
      std::vector<int> evals, accepted, status;
    };
    struct Acquisition {
      static Acquired_t calc(const Trained_t& trained, const Inputs_t& in, const gprhip_acquisition& acq, int top_k = 0) {
        Problem& p = problem_for(trained, in, "Acquisition.calc");
        const int k = top_k > 0 ? top_k : 0;
        Acquired_t a{Vec((size_t)in.points->cols), Mat(in.points->rows, in.points->cols), std::vector<int64_t>((size_t)k, -1),
                     Vec((size_t)k), Mat(in.points->rows, k > 0 ? k : 1)};
        check(gprhip_acquire(p.get(), &acq, in.points->data(), in.points->rows, in.points->cols, a.values.data(),
                             a.dvalues.data(), in.points->rows, nullptr, nullptr, top_k, k ? a.top_index.data() : nullptr,
                             k ? a.top_values.data() : nullptr, k ? a.top_dvalues.data() : nullptr, 0));
        return a;
      }
      // Max-value entropy search over the test inputs from the extreme values of 1 .. GPRHIP_MAX_EXTREMES drawn paths
      // (gprhip_acquire_max_value): maxima when `maximise`, else minima; the outputs as calc's.
      static Acquired_t calc_max_value(const Trained_t& trained, const Inputs_t& in, const Vec& extremes, bool maximise,
                                       double var_floor, int top_k = 0) {
        Problem& p = problem_for(trained, in, "Acquisition.calc_max_value");
        const int k = top_k > 0 ? top_k : 0;
        Acquired_t a{Vec((size_t)in.points->cols), Mat(in.points->rows, in.points->cols), std::vector<int64_t>((size_t)k, -1),
                     Vec((size_t)k), Mat(in.points->rows, k > 0 ? k : 1)};
        check(gprhip_acquire_max_value(p.get(), extremes.empty() ? nullptr : extremes.data(), (int)extremes.size(), maximise ? 1 : 0,
                                       var_floor, in.points->data(), in.points->rows, in.points->cols, a.values.data(),
                                       a.dvalues.data(), in.points->rows, nullptr, nullptr, top_k, k ? a.top_index.data() : nullptr,
                                       k ? a.top_values.data() : nullptr, k ? a.top_dvalues.data() : nullptr, 0));
        return a;
      }
      // The starts (D x ns, in.points) refined inside the box [lower, upper] by projected gradient ascent with Armijo
      // backtracking (gprhip_acquire_refine); scale: nullptr for all ones.  status holds GPRHIP_REFINE_ST_* per start.
      static Refined_t refine(const Trained_t& trained, const Inputs_t& in, const gprhip_acquisition& acq,
                              const gprhip_refine_options& opt, const Vec& lower, const Vec& upper, const Vec* scale = nullptr) {
        Problem& p = problem_for(trained, in, "Acquisition.refine");
        const size_t D = (size_t)in.points->rows, ns = (size_t)in.points->cols;
        if (lower.size() != D || upper.size() != D || (scale && scale->size() != D))
          throw std::invalid_argument("Acquisition.refine: lower, upper and scale take D entries each");
        Refined_t r{Mat(in.points->rows, in.points->cols), Vec(ns), Mat(in.points->rows, in.points->cols), std::vector<int>(ns),
                    std::vector<int>(ns), std::vector<int>(ns)};
        check(gprhip_acquire_refine(p.get(), &acq, &opt, lower.data(), upper.data(), scale ? scale->data() : nullptr,
                                    in.points->data(), in.points->rows, in.points->cols, r.x.data(), in.points->rows,
                                    r.values.data(), r.dvalues.data(), in.points->rows, r.evals.data(), r.accepted.data(),
                                    r.status.data(), nullptr, 0));
        return r;
      }
      // The same for max-value entropy search (gprhip_acquire_max_value_refine): the criterion of calc_max_value -- extremes,
      // maximise, var_floor -- climbed by the rule of refine.
      static Refined_t refine_max_value(const Trained_t& trained, const Inputs_t& in, const Vec& extremes, bool maximise,
                                        double var_floor, const gprhip_refine_options& opt, const Vec& lower, const Vec& upper,
                                        const Vec* scale = nullptr) {
        Problem& p = problem_for(trained, in, "Acquisition.refine_max_value");
        const size_t D = (size_t)in.points->rows, ns = (size_t)in.points->cols;
        if (lower.size() != D || upper.size() != D || (scale && scale->size() != D))
          throw std::invalid_argument("Acquisition.refine_max_value: lower, upper and scale take D entries each");
        Refined_t r{Mat(in.points->rows, in.points->cols), Vec(ns), Mat(in.points->rows, in.points->cols), std::vector<int>(ns),
                    std::vector<int>(ns), std::vector<int>(ns)};
        check(gprhip_acquire_max_value_refine(p.get(), extremes.empty() ? nullptr : extremes.data(), (int)extremes.size(),
                                              maximise ? 1 : 0, var_floor, &opt, lower.data(), upper.data(),
                                              scale ? scale->data() : nullptr, in.points->data(), in.points->rows, in.points->cols,
                                              r.x.data(), in.points->rows, r.values.data(), r.dvalues.data(), in.points->rows,
                                              r.evals.data(), r.accepted.data(), r.status.data(), nullptr, 0));
        return r;
      }
    };
    // New observations folded into the device state of a trained model or a model without a refit (gprhip_observe,
    // gprhip_posterior_save / _restore: an extension beyond the reference's implemented surface, whose objects are immutable).
    // MUTATING: every posterior call on that object reads the conditioned state afterwards; the object's targets, its
    // evidence and the resident training set are not touched, and the next evaluation on the shared problem forgets the
    // observations and drops the saved slot.  in.points: D x k, k <= GPRHIP_MAX_OBSERVE; a model takes no targets.
    struct Observe {
      static double observe(const Trained_t& trained, const Inputs_t& in, const Vec& targets) {
        Problem& p = problem_for(trained, in, "Observe.observe");
        if ((int64_t)targets.size() != in.points->cols)
          throw std::invalid_argument("Observe.observe: one target per new point");
        double dl = 0.0;
        check(gprhip_observe(p.get(), in.points->data(), in.points->rows, targets.data(), (int)in.points->cols, &dl, 0));
        return dl;  // the joint log density of the new targets given everything before them
      }
      static double observe(const Model_t& model, const Inputs_t& in) {
        Problem& p = problem_for(model, in, "Observe.observe");
        double dl = 0.0;
        check(gprhip_observe(p.get(), in.points->data(), in.points->rows, nullptr, (int)in.points->cols, &dl, 0));
        return dl;  // dl1 alone
      }
      // (no state is made here: a save or restore on an object whose state another evaluation has replaced is GPRHIP_ESTATE
      //  or acts on that other state -- the caller keeps save / observe / restore together)
      template <typename Owner> static void save(const Owner& o) { check(gprhip_posterior_save(o_problem(o).get())); }
      template <typename Owner> static void restore(const Owner& o) { check(gprhip_posterior_restore(o_problem(o).get())); }
      template <typename Owner> static int64_t count(const Owner& o) { return gprhip_observed_count(o_problem(o).get()); }

     private:
      static Problem& o_problem(const Trained_t& t) { return *t.model.inputs.problem; }
      static Problem& o_problem(const Model_t& m) { return *m.inputs.problem; }
    };
    // Posterior sample paths (gprhip_sample_paths: an extension beyond the reference's implemented surface).  A sampler keeps
    // the caller's m x ns standard normal draws z: the same sampler evaluates the same ns functions at any inputs.
    struct Path_sampler_t {
      const Trained_t* trained;
      Mat z;  // m x ns
    };
    struct Path_best_t {
      std::vector<int64_t> top_index;  // top_k x ns (-1 where fewer qualify)
      Vec top_values;                  // top_k x ns
      Vec top_dvalues;                 // D x top_k x ns: gradient of the path part at each winner
    };
    struct Path_sampler {
      static Path_sampler_t calc(const Trained_t& trained, const Mat& z) { return Path_sampler_t{&trained, z}; }
      // nt x ns samples; eps (nt x ns standard normal draws) or nullptr for the path part alone
      static Mat samples(const Path_sampler_t& s, const Inputs_t& in, const Mat* eps = nullptr, bool predictive = false) {
        Problem& p = problem_for(*s.trained, in, "Path_sampler.samples");
        Mat out(in.points->cols, s.z.cols);
        check(gprhip_sample_paths(p.get(), s.z.data(), s.z.rows, s.z.cols, in.points->data(), in.points->rows, in.points->cols,
                                  eps ? eps->data() : nullptr, eps ? eps->rows : 0, predictive ? 1 : 0, out.data(), out.rows, 1, 0,
                                  nullptr, nullptr, nullptr, 0));
        return out;
      }
      static Path_best_t best(const Path_sampler_t& s, const Inputs_t& in, int k, bool maximise = true) {
        Problem& p = problem_for(*s.trained, in, "Path_sampler.best");
        const size_t kk = (size_t)(k > 0 ? k : 0) * (size_t)s.z.cols;
        Path_best_t b{std::vector<int64_t>(kk, -1), Vec(kk), Vec(kk * (size_t)in.points->rows)};
        check(gprhip_sample_paths(p.get(), s.z.data(), s.z.rows, s.z.cols, in.points->data(), in.points->rows, in.points->cols,
                                  nullptr, 0, 0, nullptr, 0, maximise ? 1 : 0, k, b.top_index.data(), b.top_values.data(),
                                  b.top_dvalues.data(), 0));
        return b;
      }
      // The starts (D x ns, in.points) refined on the draws of the sampler (gprhip_sample_paths_refine): start i climbs
      // s f_{draw_of[i]} inside the box [lower, upper], s = +1 if maximise else -1; values / dvalues hold that objective and
      // its gradient, not the unsigned path.  scale: nullptr for all ones.
      static Refined_t refine(const Path_sampler_t& s, const Inputs_t& in, const std::vector<int>& draw_of,
                              const gprhip_refine_options& opt, const Vec& lower, const Vec& upper, bool maximise = true,
                              const Vec* scale = nullptr) {
        Problem& p = problem_for(*s.trained, in, "Path_sampler.refine");
        const size_t D = (size_t)in.points->rows, ns = (size_t)in.points->cols;
        if (lower.size() != D || upper.size() != D || (scale && scale->size() != D))
          throw std::invalid_argument("Path_sampler.refine: lower, upper and scale take D entries each");
        if (draw_of.size() != ns) throw std::invalid_argument("Path_sampler.refine: draw_of takes one entry per start");
        Refined_t r{Mat(in.points->rows, in.points->cols), Vec(ns), Mat(in.points->rows, in.points->cols), std::vector<int>(ns),
                    std::vector<int>(ns), std::vector<int>(ns)};
        check(gprhip_sample_paths_refine(p.get(), s.z.data(), s.z.rows, s.z.cols, maximise ? 1 : 0, &opt, lower.data(),
                                         upper.data(), scale ? scale->data() : nullptr, in.points->data(), in.points->rows,
                                         in.points->cols, draw_of.data(), r.x.data(), in.points->rows, r.values.data(),
                                         r.dvalues.data(), in.points->rows, r.evals.data(), r.accepted.data(), r.status.data(),
                                         nullptr, 0));
        return r;
      }
    };
    struct Covariances {  // FITC_covariances / FIC_covariances, :565-627
      template <class Owner>
      static Covariances_t calc(const Owner& cvp, double sigma2, const Inputs_t& in) {
        Problem& p = problem_of(cvp, in, CovKind ? "FIC_covariances.calc" : "FITC_covariances.calc", sigma2);
        Covariances_t c{in.points, Mat(in.points->cols, in.points->cols), sigma2,
                        owner_problem(cvp)};
        check(gprhip_covariances(p.get(), in.points->data(), in.points->rows, in.points->cols, CovKind, 0,
                                 c.covariances.data()));
        return c;
      }
      static Mat get(const Covariances_t& c, bool predictive = true) {  // :549-559
        Mat out = c.covariances;
        if (predictive)
          for (int i = 0; i < out.rows; ++i) out(i, i) += c.sigma2;
        return out;
      }
    };
    struct Cov_sampler {  // Common_cov_sampler, lib/fitc_gp.ml:656-697; the standard normal draws z are the caller's
      static Cov_sampler_t calc(const Vec& means, const Covariances_t& cov, bool predictive = true) {  // :659-675
        if ((int)means.size() != cov.covariances.rows)
          throw Failure(GPRHIP_EBADARG, "Cov_sampler: means and covariances disagree about input points");
        Cov_sampler_t s{means, cov, predictive ? cov.sigma2 : 0.0};
        Mat z0(cov.covariances.rows, 1);
        (void)samples(s, z0);  // factor now: a potrf failure surfaces in calc, as in the reference
        return s;
      }
      static Mat samples(const Cov_sampler_t& s, const Mat& z) {  // :685-697: means + cov_chol^T z, per column
        const int nt = s.covariances.covariances.rows;
        if (z.rows != nt) throw Failure(GPRHIP_EBADARG, "Cov_sampler.samples: z has the wrong number of rows");
        Mat out(nt, z.cols);
        check(gprhip_cov_samples(s.covariances.problem->get(), s.covariances.covariances.data(), nt, nt, s.add_diag,
                                 cholesky_jitter, s.means.data(), z.data(), z.cols, out.data()));
        return out;
      }
    };
    struct Optim {
      // Optim.calc_gradient (lib/fitc_gp.ml:1674-1694): [dl/dsigma2 * sigma2 (if learnt); dl/dhyper ...]
      static Vec calc_gradient(bool learn_sigma2, double sigma2, const std::vector<Hyper>& hypers,
                               const Trained_t& trained) {
        const Hyper_t ht = Trained::prepare_hyper(trained);
        Vec g;
        if (learn_sigma2) g.push_back(Trained::calc_log_evidence_sigma2(trained) * sigma2);
        for (const Hyper& h : hypers) g.push_back(Trained::calc_log_evidence(ht, h));
        return g;
      }
    };
    struct Test {
      // Deriv.Test.self_test (lib/fitc_gp.ml:1398-1462): forward finite difference (eps) of the model and trained
      // log evidence against the analytic derivative; throws like the reference's failwithf.  hyper == nullptr
      // checks sigma2.
      static void self_test(const Kernel& kernel, MatP inducing_points, MatP points, double sigma2,
                            const Vec& targets, const Hyper* hyper, double eps = 1e-8, double tol = 1e-2) {
        auto build = [&](const Kernel& k, MatP z, double s2) {
          auto ind = Inducing::calc(k, z);
          auto inp = Inputs::calc(ind, points);
          auto mod = Model::calc(inp, s2);
          return std::make_pair(mod, Trained::calc(mod, targets, true));
        };
        auto [mod1, tr1] = build(kernel, inducing_points, sigma2);
        double m1 = Model::evaluation(mod1, true).l1, t1 = Trained::evaluation(tr1).l, dm, dt, m2, t2;
        if (!hyper) {
          dm = Model::calc_log_evidence_sigma2(mod1);
          dt = Trained::calc_log_evidence_sigma2(tr1);
          auto [mod2, tr2] = build(kernel, inducing_points, sigma2 + eps);
          m2 = Model::calc_log_evidence(mod2);
          t2 = Trained::calc_log_evidence(tr2);
        } else {
          dm = Model::calc_log_evidence(Model::prepare_hyper(mod1), *hyper);
          dt = Trained::calc_log_evidence(Trained::prepare_hyper(tr1), *hyper);
          const double v = Spec::get_value(kernel, *inducing_points, *hyper);
          auto [k2, z2] = Spec::set_values(kernel, inducing_points, {*hyper}, {v + eps});
          auto [mod2, tr2] = build(k2, z2, sigma2);
          m2 = Model::calc_log_evidence(mod2);
          t2 = Trained::calc_log_evidence(tr2);
        }
        auto bad = [&](double before, double after, double deriv, const char* what) {
          const double fd = (after - before) / eps;
          if (!(std::fabs(fd - deriv) <= tol))  // is_bad_deriv, :1219-1221 (NaN-safe)
            throw Failure(GPRHIP_EBADARG, std::string("Gpr.Fitc_gp.Make_deriv.Test.self_test: finite difference (") +
                                              std::to_string(fd) + ") and derivative (" + std::to_string(deriv) +
                                              ") differ by more than " + std::to_string(tol) + " on " + what);
        };
        bad(m1, m2, dm, "model");
        bad(t1, t2, dt, "trained");
      }
    };
  };

  using FITC = Variant<false, 0>;
  using Variational_FITC = Variant<true, 0>;
  using FIC = Variant<false, 1>;
  using Variational_FIC = Variant<true, 1>;
};

}  // namespace gpr

#endif  // GPRHIP_HPP
