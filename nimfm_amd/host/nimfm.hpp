// nimfm_amd/host/nimfm.hpp -- header-only C++17 host mirror of nimfm's FM surface over the C ABI
// (include/nimfm_hip.h).  The reference's host language (Nim) is compiled code and no Nim toolchain
// exists in the build image; this header is the compiled-language counterpart of nim/nimfm_hip.nim:
// same names, argument meaning, defaults and error behaviour as the reference procs
// (citations relative to /root/reference/src/nimfm/):
//   FactorizationMachine            model/factorization_machine.nim:11-139, model/fm_base.nim:13-48
//   SGD<Loss>::fit / AdaGrad::fit   optimizer/sgd.nim:23-52,261-328, optimizer/adagrad.nim:20-44,137-203
// Errors of the library surface as std::invalid_argument (the reference's ValueError),
// nimfm::NotFittedError, or std::runtime_error.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <numeric>
#include <random>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <initializer_list>
#include <memory>
#include <vector>

#include "../../include/nimfm_hip.h"

namespace nimfm {

struct NotFittedError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void check(int32_t rc) {
  if (rc == NFM_OK) return;
  const std::string msg = nfm_last_error();
  if (rc == NFM_ERR_INVALID) throw std::invalid_argument(msg);
  if (rc == NFM_ERR_NOT_FITTED) throw NotFittedError(msg);
  throw std::runtime_error("libnimfm_hip error " + std::to_string(rc) + ": " + msg);
}

inline nfm_ctx* default_context() {
  static nfm_ctx* ctx = nullptr;
  if (!ctx) check(nfm_ctx_create(0, nullptr, &ctx));
  return ctx;
}

enum TaskKind { regression = NFM_TASK_REGRESSION, classification = NFM_TASK_CLASSIFICATION };
enum FitLowerKind { explicit_ = NFM_LOWER_EXPLICIT, augment = NFM_LOWER_AUGMENT, none = NFM_LOWER_NONE };
enum SchedulingKind { constant = NFM_SCHED_CONSTANT, optimal = NFM_SCHED_OPTIMAL, invscaling = NFM_SCHED_INVSCALING, pegasos = NFM_SCHED_PEGASOS };
struct Squared { static constexpr int id = NFM_LOSS_SQUARED; double param = 1.0; };
struct SquaredHinge { static constexpr int id = NFM_LOSS_SQUARED_HINGE; double param = 1.0; };
struct Logistic { static constexpr int id = NFM_LOSS_LOGISTIC; double param = 1.0; };
struct Huber { static constexpr int id = NFM_LOSS_HUBER; double param = 1.0; /* threshold */ };

// dataset.nim:10-16 + tensor/sparse.nim:9-12: CSR rows resident on the device
class CSRDataset {
 public:
  CSRDataset(const std::vector<double>& data, const std::vector<int64_t>& indices, const std::vector<int64_t>& indptr,
             int64_t nSamples, int64_t nFeatures)
      : n_(nSamples), d_(nFeatures) {
    if ((int64_t)indptr.size() != nSamples + 1) throw std::invalid_argument("len(indptr) != nSamples + 1");
    check(nfm_dataset_create_csr(default_context(), nSamples, nFeatures, indptr.data(), indices.data(), data.data(), nullptr,
                                 0, nullptr, &h_));
  }
  // a dataset made by one of the loaders below (the handle is adopted)
  explicit CSRDataset(nfm_dataset* h) : h_(h) {
    int64_t nnz = 0, nf = 0;
    check(nfm_dataset_shape(h_, &n_, &d_, &nnz, &nf));
  }
  CSRDataset(const CSRDataset&) = delete;
  ~CSRDataset() { nfm_dataset_destroy(h_); }
  std::vector<double> targets() const {  // the loaders' y
    std::vector<double> y((size_t)n_);
    check(nfm_dataset_get_targets(h_, y.data()));
    return y;
  }
  int64_t nSamples() const { return n_; }
  int64_t nFeatures() const { return d_; }
  nfm_dataset* handle() const { return h_; }
  // X[indicesRow] / X[a..<b] (dataset.nim:319-369) as a new dataset made on the device; checkIndicesRow's errors
  // (dataset.nim:307-316) come back as std::invalid_argument with the reference's texts
  CSRDataset operator[](const std::vector<int64_t>& indicesRow) const {
    nfm_dataset* h = nullptr;
    check(nfm_dataset_select_rows(h_, indicesRow.data(), (int64_t)indicesRow.size(), &h));
    return CSRDataset(h);
  }
  CSRDataset slice(int64_t begin, int64_t end) const {
    nfm_dataset* h = nullptr;
    check(nfm_dataset_slice_rows(h_, begin, end, &h));
    return CSRDataset(h);
  }
  // the reference's in-place procs (normalize): the object takes the new dataset's handle, the old arrays are freed
  void swapHandle(nfm_dataset* h) {
    int64_t nnz = 0, nf = 0;
    check(nfm_dataset_shape(h, &n_, &d_, &nnz, &nf));
    nfm_dataset_destroy(h_);
    h_ = h;
  }

 private:
  nfm_dataset* h_ = nullptr;
  int64_t n_, d_;
};

// loadSVMLightFile (dataset.nim:616-632): the text is parsed on the GPU, y comes back with the dataset
inline std::unique_ptr<CSRDataset> loadSVMLightFile(const std::string& f, std::vector<double>& y, int64_t nFeatures = -1) {
  nfm_dataset* h = nullptr;
  check(nfm_dataset_load_svmlight(default_context(), f.c_str(), nFeatures, &h));
  std::unique_ptr<CSRDataset> X(new CSRDataset(h));
  y = X->targets();
  return X;
}
// newStreamCSRDataset + loadStreamLabel (dataset.nim:170-174, 1007-1014): the whole file becomes resident
inline std::unique_ptr<CSRDataset> newStreamCSRDataset(const std::string& f, const std::string& fY = "") {
  nfm_dataset* h = nullptr;
  check(nfm_dataset_load_stream(default_context(), f.c_str(), fY.empty() ? nullptr : fY.c_str(), &h));
  return std::unique_ptr<CSRDataset>(new CSRDataset(h));
}

class FactorizationMachine {
 public:
  TaskKind task;
  int degree, nComponents;
  FitLowerKind fitLower;
  bool fitIntercept, fitLinear, warmStart;
  int randomState;
  double scale;
  bool isInitialized = false;
  std::vector<double> P;  // [nOrders][nComponents][nFeatures + nAugments]
  std::vector<double> lams, w;
  double intercept = 0.0;

  // newFactorizationMachine, model/factorization_machine.nim:43-78
  explicit FactorizationMachine(TaskKind task_, int degree_ = 2, int nComponents_ = 30, FitLowerKind fitLower_ = explicit_,
                                bool fitIntercept_ = true, bool fitLinear_ = true, bool warmStart_ = false,
                                int randomState_ = 1, double scale_ = 0.01)
      : task(task_), degree(degree_), nComponents(nComponents_), fitLower(fitLower_), fitIntercept(fitIntercept_),
        fitLinear(fitLinear_), warmStart(warmStart_), randomState(randomState_), scale(scale_) {
    if (degree < 1) throw std::invalid_argument("degree < 1.");
    if (nComponents < 1) throw std::invalid_argument("nComponents < 1.");
    lams.assign(nComponents, 1.0);
  }
  FactorizationMachine(const FactorizationMachine&) = delete;
  ~FactorizationMachine() { if (h_) nfm_model_destroy(h_); }

  int nAugments() const { return fitLower == augment ? (fitLinear ? degree - 2 : degree - 1) : 0; }  // :81-86
  int nOrders() const { return degree == 1 ? 0 : (fitLower == explicit_ ? degree - 1 : 1); }          // :89-97

  // init, :125-139 (std::mt19937_64 + normal_distribution stand in for Nim's RNG)
  void init(const CSRDataset& X, bool force = false) {
    if (force || !(warmStart && isInitialized)) {
      d_ = X.nFeatures();
      rng_.seed((uint64_t)randomState);
      std::normal_distribution<double> g(0.0, scale);
      w.assign(d_, 0.0);
      P.resize((size_t)nOrders() * nComponents * (d_ + nAugments()));
      for (auto& v : P) v = g(rng_);
      intercept = 0.0;
      dirty_ = true;
    }
    isInitialized = true;
  }
  void setParams(std::vector<double> P_, std::vector<double> w_, double b) {
    d_ = (int64_t)w_.size();
    if (P_.size() != (size_t)nOrders() * nComponents * (d_ + nAugments())) throw std::invalid_argument("bad P shape");
    P = std::move(P_); w = std::move(w_); intercept = b; isInitialized = true; dirty_ = true;
  }
  // decisionFunction, :100-122
  std::vector<double> decisionFunction(const CSRDataset& X) {
    if (!isInitialized) throw NotFittedError("Factorization machines is not fitted.");
    if (X.nFeatures() != d_) throw std::invalid_argument("Invalid nFeatures.");
    std::vector<double> out(X.nSamples());
    check(nfm_decision_function(push(), X.handle(), out.data()));
    return out;
  }
  // [nU][nV], row-major: [i][j] is decisionFunction (:100-122, kernels.nim:59-64) of row i of U followed by row j of V -- row
  // i * nV + j of hstack(U[rep], V[tile]), tensor/sparse.nim:671-698, which is never made.  Degree 2;
  // the library refuses everything else and names the pairs and decisionFunction as the way that remains.
  std::vector<double> crossDecisionFunction(const CSRDataset& U, const CSRDataset& V) {
    if (!isInitialized) throw NotFittedError("Factorization machines is not fitted.");
    std::vector<double> out((size_t)U.nSamples() * (size_t)V.nSamples());
    check(nfm_cross_decision_function(push(), U.handle(), V.handle(), out.data()));
    return out;
  }
  // per row of U the topK rows of V by descending crossDecisionFunction, then ascending id (NaN below every number): ids and
  // scores [nU][topK], the scores bit for bit crossDecisionFunction's.  1 <= topK <= min(nV, 256).  chunkItems: the items
  // one workgroup ranks, 0 = the library's choice; the result does not depend on it.
  std::pair<std::vector<int64_t>, std::vector<double>> recommend(const CSRDataset& U, const CSRDataset& V, int64_t topK, int64_t chunkItems = 0) {
    if (!isInitialized) throw NotFittedError("Factorization machines is not fitted.");
    const size_t n = topK >= 1 && topK <= 256 ? (size_t)U.nSamples() * (size_t)topK : 0;  // (out of range: refused before anything is written)
    std::vector<int64_t> ids(n);
    std::vector<double> scores(n);
    check(nfm_cross_topk(push(), U.handle(), V.handle(), topK, chunkItems, ids.data(), scores.data()));
    return {std::move(ids), std::move(scores)};
  }
  std::vector<int> predict(const CSRDataset& X) {  // fm_base.nim:18-20
    auto y = decisionFunction(X);
    std::vector<int> r(y.size());
    for (size_t i = 0; i < y.size(); ++i) r[i] = (y[i] > 0) - (y[i] < 0);
    return r;
  }
  double score(const CSRDataset& X, const std::vector<double>& y) {  // fm_base.nim:39-48, reduced on the device
    if (!isInitialized) throw NotFittedError("Factorization machines is not fitted.");
    if (X.nFeatures() != d_) throw std::invalid_argument("Invalid nFeatures.");
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    double out = 0.0;
    check(nfm_score(push(), X.handle(), &out));
    return out;
  }

  nfm_model* push() {  // device copy of the host parameters
    if (!h_ || hd_ != d_) {
      if (h_) nfm_model_destroy(h_);
      nfm_model_cfg c{NFM_KIND_FM, (int32_t)task, degree, nComponents, (int32_t)fitLower, fitIntercept, fitLinear, 0, d_, 0};
      check(nfm_model_create(default_context(), &c, &h_));
      hd_ = d_;
      dirty_ = true;
    }
    if (dirty_) {
      check(nfm_model_set_params(h_, P.empty() ? nullptr : P.data(), w.data(), intercept, lams.data()));
      dirty_ = false;
    }
    return h_;
  }
  void pull() { check(nfm_model_get_params(h_, P.empty() ? nullptr : P.data(), w.data(), &intercept)); dirty_ = false; }
  std::mt19937_64& rng() { return rng_; }

 private:
  nfm_model* h_ = nullptr;
  int64_t d_ = 0, hd_ = -1;
  bool dirty_ = true;
  std::mt19937_64 rng_;
};

namespace detail {
// the epoch loop shared by SGD and AdaGrad: optimizer/sgd.nim:294-328, adagrad.nim:164-203
template <class Opt>
void run_fit(Opt& self, nfm_opt* o, const CSRDataset& X, FactorizationMachine& fm,
             const std::function<void(Opt&, FactorizationMachine&)>& callback, bool callback_each_epoch) {
  const int64_t n = X.nSamples();
  std::vector<int64_t> indices(n);
  std::iota(indices.begin(), indices.end(), 0);
  bool isConverged = false;
  check(nfm_opt_set_it(o, self.it));
  if (self.verbose > 0) std::printf("Epoch   Violation    Loss         Regularization\n");
  for (int epoch = 0; epoch < self.maxIter; ++epoch) {
    double viol = 0.0, runningLoss = 0.0;
    const int64_t* perm = nullptr;
    if (self.shuffle) {
      std::shuffle(indices.begin(), indices.end(), fm.rng());
      perm = indices.data();
    }
    check(nfm_opt_epoch(o, X.handle(), perm, 0, n, &runningLoss, &viol));
    self.it += n;
    runningLoss /= (double)n;
    if (callback && callback_each_epoch) {
      check(nfm_opt_finalize(o));
      fm.pull();
      callback(self, fm);
    }
    bool isContinue = true;  // stoppingCriterion, sgd.nim:72-89
    if (std::isnan(runningLoss)) { std::printf("Loss is NaN. Use smaller learning rate.\n"); isContinue = false; }
    if (self.verbose > 0) {
      double psq = 0, wsq = 0, b = 0;
      check(nfm_model_sqnorms(fm.push(), &psq, &wsq));
      check(nfm_model_get_params(fm.push(), nullptr, nullptr, &b));
      std::printf("%-5d   %-10.4e   %-10.4e   %-10.4e\n", epoch + 1, viol, runningLoss,
                  0.5 * self.alpha0 * b * b + 0.5 * self.alpha * wsq + 0.5 * self.beta * psq);
    }
    if (viol < self.tol) {
      if (self.verbose > 0) std::printf("Converged at epoch %d.\n", epoch);
      isConverged = true;
      isContinue = false;
    }
    if (!isContinue) break;
  }
  if (!isConverged && self.verbose > 0) std::printf("Objective did not converge. Increase maxIter.\n");
  check(nfm_opt_finalize(o));
  fm.pull();
}
}  // namespace detail

template <class L = Squared>
class SGD {
 public:
  int maxIter; double eta0, alpha0, alpha, beta; L loss; SchedulingKind scheduling; double power;
  int verbose; double tol; bool shuffle; int nCalls; int64_t it = 1;
  int mode = NFM_MODE_SEQUENTIAL; int64_t batch = 8192;
  double touchCap = 1.0;  // mini-batch mode: nfm_opt_set_touch_cap (1 = the per-coordinate mean; about twice the touches per coordinate and batch)
  // newSGD, optimizer/sgd.nim:23-52
  explicit SGD(int maxIter_ = 100, double eta0_ = 0.01, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-3,
               L loss_ = L(), SchedulingKind scheduling_ = optimal, double power_ = 1.0, int verbose_ = 1, double tol_ = 1e-3,
               bool shuffle_ = true, int nCalls_ = -1)
      : maxIter(maxIter_), eta0(eta0_), alpha0(alpha0_), alpha(alpha_), beta(beta_), loss(loss_), scheduling(scheduling_),
        power(power_), verbose(verbose_), tol(tol_), shuffle(shuffle_), nCalls(nCalls_) {}
  ~SGD() { if (o_) nfm_opt_destroy(o_); }
  // fit, optimizer/sgd.nim:261-328; maxThreads != 0 = the Hogwild overload (sgd_multi.nim:40-42) -> mini-batch mode
  // maxThreads only SELECTS the mini-batch mode (a thread count is not a batch size); the mode's knobs are explicit:
  // miniBatchSize (0: this->batch), and across GPUs -- one process per GPU, X this rank's slice -- group + syncPeriod
  void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& fm, int maxThreads = 0,
           std::function<void(SGD&, FactorizationMachine&)> callback = nullptr, int64_t miniBatchSize = 0,
           int64_t syncPeriod = 0, nfm_dp* group = nullptr) {
    fm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    if (!fm.warmStart) it = 1;
    nfm_model* m = fm.push();
    const int md = (maxThreads != 0 || group) ? NFM_MODE_MINIBATCH : mode;
    const int64_t bsz = miniBatchSize > 0 ? miniBatchSize : batch;
    if (!o_ || m_ != m || md_ != md || b_ != bsz) {
      if (o_) nfm_opt_destroy(o_);
      nfm_sgd_cfg c{eta0, alpha0, alpha, beta, power, loss.param, L::id, (int32_t)scheduling, md, 0, bsz};
      check(nfm_sgd_create(m, &c, &o_));
      m_ = m; md_ = md; b_ = bsz; cap_ = 1.0;
    }
    if (md == NFM_MODE_MINIBATCH && cap_ != touchCap) { check(nfm_opt_set_touch_cap(o_, touchCap)); cap_ = touchCap; }
    if (md == NFM_MODE_MINIBATCH) check(nfm_opt_set_dp(o_, group, syncPeriod, 1));
    detail::run_fit<SGD>(*this, o_, X, fm, callback, nCalls <= 0 || md == NFM_MODE_MINIBATCH);
  }

 private:
  nfm_opt* o_ = nullptr; nfm_model* m_ = nullptr; int md_ = -1; int64_t b_ = -1; double cap_ = 1.0;
};

template <class L = Squared>
class AdaGrad {
 public:
  int maxIter; double eta0, alpha0, alpha, beta; L loss; double eps; int verbose; double tol; bool shuffle; int nCalls;
  int64_t it = 1; int mode = NFM_MODE_SEQUENTIAL; int64_t batch = 8192;
  double adaCross = 0.0;   // mini-batch mode: nfm_opt_set_ada_cross (weight of the batch's gradient cross products in g_norm; 0.1 at large batches)
  bool trackViol = true;   // adagrad.nim:99's sum |P_old - P_new| (the stopping criterion); false saves the stored-parameter round trip
  // newAdaGrad, optimizer/adagrad.nim:20-44
  explicit AdaGrad(int maxIter_ = 100, double eta0_ = 0.1, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-3,
                   L loss_ = L(), double eps_ = 1e-10, int verbose_ = 1, double tol_ = 1e-3, bool shuffle_ = true,
                   int nCalls_ = -1)
      : maxIter(maxIter_), eta0(eta0_), alpha0(alpha0_), alpha(alpha_), beta(beta_), loss(loss_), eps(eps_),
        verbose(verbose_), tol(tol_), shuffle(shuffle_), nCalls(nCalls_) {}
  ~AdaGrad() { if (o_) nfm_opt_destroy(o_); }
  void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& fm, int maxThreads = 0,
           std::function<void(AdaGrad&, FactorizationMachine&)> callback = nullptr, int64_t miniBatchSize = 0,
           int64_t syncPeriod = 0, nfm_dp* group = nullptr) {
    fm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    if (!fm.warmStart) it = 1;
    nfm_model* m = fm.push();
    const int md = (maxThreads != 0 || group) ? NFM_MODE_MINIBATCH : mode;
    const int64_t bsz = miniBatchSize > 0 ? miniBatchSize : batch;
    if (!o_ || m_ != m || md_ != md || b_ != bsz || tv_ != trackViol) {
      if (o_) nfm_opt_destroy(o_);
      nfm_adagrad_cfg c{eta0, alpha0, alpha, beta, eps, loss.param, L::id, md, trackViol ? 1 : 0, 0, bsz};
      check(nfm_adagrad_create(m, &c, &o_));
      m_ = m; md_ = md; b_ = bsz; tv_ = trackViol; cross_ = 0.0;
    }
    if (md == NFM_MODE_MINIBATCH && cross_ != adaCross) { check(nfm_opt_set_ada_cross(o_, adaCross)); cross_ = adaCross; }
    if (md == NFM_MODE_MINIBATCH) check(nfm_opt_set_dp(o_, group, syncPeriod, 1));
    detail::run_fit<AdaGrad>(*this, o_, X, fm, callback, true);
  }

 private:
  nfm_opt* o_ = nullptr; nfm_model* m_ = nullptr; int md_ = -1; int64_t b_ = -1; bool tv_ = true; double cross_ = 0.0;
};

// regularizer/{l1,l21,squaredl12,squaredl21}.nim: the penalties with a matrix proximal operator
struct L1 { static constexpr int id = NFM_REG_L1; bool transpose = false; };
struct L21 { static constexpr int id = NFM_REG_L21; bool transpose = false; };
struct SquaredL12 { static constexpr int id = NFM_REG_SQUAREDL12; bool transpose = true; /* squaredl12.nim:85 */ };
struct SquaredL21 { static constexpr int id = NFM_REG_SQUAREDL21; bool transpose = false; /* squaredl21.nim:15 */ };
// regularizer/omegati.nim: no matrix proximal operator (MBPSGD refuses it); PCD takes it, as it takes L1 and SquaredL12
struct OmegaTI { static constexpr int id = NFM_REG_OMEGATI; bool transpose = false; };
// regularizer/omegacs.nim: BCD hooks only (:31-85); PBCD takes it, at any degree, PCD and the matrix-prox solvers refuse it
struct OmegaCS { static constexpr int id = NFM_REG_OMEGACS; bool transpose = false; };

// reg.eval(P[order].T, degree) for the verbose lines (l1.nim:19-22, l21.nim:17-20, squaredl12.nim:72-82, squaredl21.nim:21-29,
// omegati.nim:17-26, omegacs.nim:15-28) on one order of P in either memory layout: component s of feature j is p[s * sk + j * sj], with no gaps.
// CD's family holds the model's [k][da] (sk = da, sj = 1), Katyusha's tilde the training layout [da][k] (sk = 1, sj = k).
struct OrderView {
  const double* p; int k; int64_t da, sk, sj;
  double at(int s, int64_t j) const { return p[s * sk + j * sj]; }
};
inline double regEval(const L1&, const OrderView& v, int) {
  double r = 0.0;
  for (int64_t t = 0; t < (int64_t)v.k * v.da; ++t) r += std::fabs(v.p[t]);  // in memory order
  return r;
}
inline double regEval(const SquaredL12& reg, const OrderView& v, int) {
  double r = 0.0;
  if (reg.transpose) {  // the l1 norm of every component, squared
    for (int s = 0; s < v.k; ++s) {
      double a = 0.0;
      for (int64_t j = 0; j < v.da; ++j) a += std::fabs(v.at(s, j));
      r += a * a;
    }
  } else {  // the l1 norm of every feature, squared
    for (int64_t j = 0; j < v.da; ++j) {
      double a = 0.0;
      for (int s = 0; s < v.k; ++s) a += std::fabs(v.at(s, j));
      r += a * a;
    }
  }
  return r;
}
inline double regEval(const OmegaTI&, const OrderView& v, int degree) {
  double r = 0.0;
  for (int s = 0; s < v.k; ++s) {
    std::vector<double> c((size_t)degree + 1, 0.0);
    c[0] = 1.0;
    for (int64_t j = 0; j < v.da; ++j)
      for (int t = 0; t < degree; ++t) c[degree - t] += c[degree - t - 1] * std::fabs(v.at(s, j));
    r += c[degree];
  }
  return r;
}
inline double rowNormSum(const OrderView& v) {
  double r = 0.0;
  for (int64_t j = 0; j < v.da; ++j) {
    double a = 0.0;
    for (int s = 0; s < v.k; ++s) a += v.at(s, j) * v.at(s, j);
    r += std::sqrt(a);
  }
  return r;
}
inline double regEval(const L21&, const OrderView& v, int) { return rowNormSum(v); }
// the ANOVA polynomial of the row norms, by recomputeCacheBCD's loop order (omegacs.nim:42-44)
inline double regEval(const OmegaCS&, const OrderView& v, int degree) {
  std::vector<double> c((size_t)degree + 1, 0.0);
  c[0] = 1.0;
  for (int64_t j = 0; j < v.da; ++j) {
    double a = 0.0;
    for (int s = 0; s < v.k; ++s) a += v.at(s, j) * v.at(s, j);
    const double nj = std::sqrt(a);
    for (int t = 0; t < degree; ++t) c[degree - t] += c[degree - t - 1] * nj;
  }
  return c[degree];
}
inline double regEval(const SquaredL21&, const OrderView& v, int) {
  const double r = rowNormSum(v);
  return r * r;
}
// the same on the model's layout, Po: [k][da]
template <class R>
double regEval(const R& reg, const double* Po, int k, int64_t da, int degree) { return regEval(reg, OrderView{Po, k, da, da, 1}, degree); }

namespace detail {
// indices[ii] with wrap-around and reshuffle (minibatch_psgd.nim:98-108,169-170, katyusha.nim:108-118,199-200) on the model's
// generator: the shuffle at the start, and again the moment ii reaches n
struct IndexStream {
  std::vector<int64_t> indices; bool shuffle; std::mt19937_64& rng; size_t ii = 0;
  IndexStream(int64_t n, bool shuffle_, std::mt19937_64& rng_) : indices((size_t)n), shuffle(shuffle_), rng(rng_) {
    std::iota(indices.begin(), indices.end(), 0);
    if (shuffle) std::shuffle(indices.begin(), indices.end(), rng);
  }
  void fill(std::vector<int64_t>& chunk) {
    for (int64_t& c : chunk) {
      c = indices[ii++];
      if (ii >= indices.size()) {
        ii = 0;
        if (shuffle) std::shuffle(indices.begin(), indices.end(), rng);
      }
    }
  }
};
// the default mini-batch size (minibatch_psgd.nim:160-163, katyusha.nim:203-206)
inline int64_t default_batch(const CSRDataset& X) {
  int64_t nnz = 0;
  check(nfm_dataset_shape(X.handle(), nullptr, nullptr, &nnz, nullptr));
  return std::max<int64_t>((X.nFeatures() * X.nSamples()) / std::max<int64_t>(nnz, 1), 1);
}
}  // namespace detail

// MBPSGD[L, R], optimizer/minibatch_psgd.nim:11-65,125-210
template <class L = Squared, class R = SquaredL12>
class MBPSGD {
 public:
  int maxIter; double eta0, alpha0, alpha, beta, gamma; L loss; R reg; int64_t miniBatchSize, maxIterInner;
  SchedulingKind scheduling; double power; int verbose; double tol; bool shuffle; int64_t it = 0;
  explicit MBPSGD(int maxIter_ = 100, double eta0_ = 0.1, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4,
                  double gamma_ = 1e-4, L loss_ = L(), R reg_ = R(), int64_t miniBatchSize_ = -1, int64_t maxIterInner_ = -1,
                  SchedulingKind scheduling_ = optimal, double power_ = 1.0, int verbose_ = 1, double tol_ = 1e-6,
                  bool shuffle_ = true)
      : maxIter(maxIter_), eta0(eta0_), alpha0(alpha0_), alpha(alpha_), beta(beta_), gamma(gamma_), loss(loss_), reg(reg_),
        miniBatchSize(miniBatchSize_), maxIterInner(maxIterInner_), scheduling(scheduling_), power(power_),
        verbose(verbose_), tol(tol_), shuffle(shuffle_) {}
  ~MBPSGD() { if (o_) nfm_opt_destroy(o_); }
  void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& sfm,
           std::function<void(MBPSGD&, FactorizationMachine&)> callback = nullptr) {
    sfm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    if (!sfm.warmStart) it = 1;  // :153-154
    const int64_t n = X.nSamples();
    const int64_t B = miniBatchSize > 0 ? miniBatchSize : detail::default_batch(X);  // :160-163
    int64_t inner = maxIterInner;
    if (inner <= 0) inner = std::max<int64_t>((n - 1) / B + 1, 1);  // :164-167
    nfm_model* m = sfm.push();
    if (!o_ || m_ != m || B_ != B) {
      if (o_) nfm_opt_destroy(o_);
      o_ = nullptr;
      nfm_mbpsgd_cfg c{eta0, alpha0, alpha, beta, gamma, power, loss.param, L::id, (int32_t)scheduling, R::id,
                       reg.transpose ? 1 : 0, B};
      check(nfm_mbpsgd_create(m, &c, &o_));
      m_ = m; B_ = B;
    }
    check(nfm_opt_set_it(o_, it));
    std::vector<int64_t> chunk((size_t)(B * inner));
    detail::IndexStream stream(n, shuffle, sfm.rng());
    if (verbose > 0) {
      std::printf("Minibatch size: %lld\nNumber of inner iteration: %lld\n", (long long)B, (long long)inner);
      std::printf("Epoch   Loss         Regularization\n");
    }
    double oldLossVal = INFINITY;
    bool isConverged = false;
    for (int t = 0; t < maxIter; ++t) {
      stream.fill(chunk);  // :98-108
      double ls = 0.0, viol = 0.0;
      check(nfm_opt_epoch(o_, X.handle(), chunk.data(), 0, (int64_t)chunk.size(), &ls, &viol));
      it += inner;
      const double runningLoss = ls / (double)(B * inner);  // :122
      if (callback) {
        check(nfm_opt_finalize(o_));
        sfm.pull();
        callback(*this, sfm);
      }
      if (std::isnan(runningLoss)) { std::printf("Loss is NaN. Use smaller learning rate.\n"); break; }
      if (verbose > 0) std::printf("%-5d   %-10.4e\n", t + 1, runningLoss);
      if (std::fabs(oldLossVal - runningLoss) < tol) {  // :201-204
        if (verbose > 0) std::printf("Converged at epoch %d.\n", t + 1);
        isConverged = true;
        break;
      }
      oldLossVal = runningLoss;
    }
    if (!isConverged && verbose > 0) std::printf("Objective did not converge. Increase maxIter.\n");
    check(nfm_opt_finalize(o_));
    sfm.pull();
  }

 private:
  nfm_opt* o_ = nullptr; nfm_model* m_ = nullptr; int64_t B_ = -1;
};

// PSGD[L, R], optimizer/psgd.nim:11-55,76-215: SGD in the reference's sample order with a sparsity regulariser whose effect
// on the rows a sample does not touch is caught up lazily.  The per-sample step with the regulariser's lazy hooks, the cache
// resets and finalize run on the device (nfm_psgd_create / nfm_psgd_begin_fit / nfm_opt_epoch / nfm_psgd_finalize); the epoch
// loop, the sample order, the nCalls split (:179-182), the callbacks and the stopping rule (:198-201) run here.
// R: L1 or L21.  The reference's default regulariser, SquaredL12, is this template's default too -- and the device has no PSGD
// step for SquaredL12 / SquaredL21 (it touches every parameter per sample): a default PSGD<> is refused at fit with an
// invalid_argument that names MBPSGD.  OmegaTI and OmegaCS have no SGD hooks.
template <class L = Squared, class R = SquaredL12>
class PSGD {
 public:
  int maxIter; double eta0, alpha0, alpha, beta, gamma; L loss; R reg; SchedulingKind scheduling; double power;
  int verbose; double tol; bool shuffle; int nCalls; int64_t it = 1;
  std::vector<double> lossSums;  // the running loss of every epoch before :186 divides it
  // newPSGD, optimizer/psgd.nim:23-55
  explicit PSGD(int maxIter_ = 100, double eta0_ = 0.01, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4,
                double gamma_ = 1e-4, L loss_ = L(), R reg_ = R(), SchedulingKind scheduling_ = optimal, double power_ = 1.0,
                int verbose_ = 1, double tol_ = 1e-3, bool shuffle_ = true, int nCalls_ = -1)
      : maxIter(maxIter_), eta0(eta0_), alpha0(alpha0_), alpha(alpha_), beta(beta_), gamma(gamma_), loss(loss_), reg(reg_),
        scheduling(scheduling_), power(power_), verbose(verbose_), tol(tol_), shuffle(shuffle_), nCalls(nCalls_) {}
  PSGD(const PSGD&) = delete;
  ~PSGD() { if (o_) nfm_opt_destroy(o_); }
  void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& sfm,
           std::function<void(PSGD&, FactorizationMachine&)> callback = nullptr) {
    if (R::id == NFM_REG_SQUAREDL12 || R::id == NFM_REG_SQUAREDL21)
      throw std::invalid_argument("PSGD on the device takes L1 or L21: the step of SquaredL12 / SquaredL21 touches every parameter per "
                                  "sample -- use MBPSGD<L, R>, which has their proximal operators");
    if (R::id != NFM_REG_L1 && R::id != NFM_REG_L21)
      throw std::invalid_argument("PSGD cannot be used for OmegaTI / OmegaCS: they have no SGD hooks -- use PCD (OmegaTI) or PBCD (OmegaCS)");
    if (sfm.nComponents > 128)
      throw std::invalid_argument("PSGD on the device supports nComponents <= 128: use MBPSGD<L, L1> or SGD for wider models");
    if (sfm.degree > 6) throw std::invalid_argument("PSGD on the device supports degree <= 6: use SGD beyond");
    sfm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    if (!sfm.warmStart) it = 1;  // :106-107
    const int64_t n = X.nSamples();
    nfm_model* m = sfm.push();
    if (!o_ || m_ != m) {
      if (o_) nfm_opt_destroy(o_);
      o_ = nullptr;
      nfm_mbpsgd_cfg c{eta0, alpha0, alpha, beta, gamma, power, loss.param, L::id, (int32_t)scheduling, R::id, 0, 1};
      check(nfm_psgd_create(m, &c, &o_));
      m_ = m;
    }
    check(nfm_opt_set_it(o_, it));
    check(nfm_psgd_begin_fit(o_, X.handle()));  // reg.initSGD, :112
    if (verbose > 0) std::printf("Epoch   Loss         Regularization\n");
    std::vector<int64_t> indices((size_t)n);
    std::iota(indices.begin(), indices.end(), 0);
    lossSums.clear();
    bool isConverged = false;
    double runningLossOld = 0.0;
    for (int epoch = 0; epoch < maxIter; ++epoch) {
      double runningLoss = 0.0;
      const int64_t* perm = nullptr;
      if (shuffle) {  // :120
        std::shuffle(indices.begin(), indices.end(), sfm.rng());
        perm = indices.data();
      }
      if (callback && nCalls > 0) {
        int64_t pos = 0;
        while (pos < n) {  // :179-182: the callback whenever it mod nCalls == 0, before inc(self.it)
          const int64_t to_next = (nCalls - it % nCalls) % nCalls + 1;
          const int64_t end = std::min(n, pos + to_next);
          double ls = 0.0, vs = 0.0;
          check(nfm_opt_epoch(o_, X.handle(), perm, pos, end, &ls, &vs));
          runningLoss += ls;
          it += end - pos;
          pos = end;
          if ((it - 1) % nCalls == 0) {
            check(nfm_psgd_finalize(o_));
            sfm.pull();
            --it;
            callback(*this, sfm);
            ++it;
          }
        }
      } else {
        double vs = 0.0;
        check(nfm_opt_epoch(o_, X.handle(), perm, 0, n, &runningLoss, &vs));
        it += n;
      }
      lossSums.push_back(runningLoss);
      runningLoss /= (double)n;  // :186
      if (callback && nCalls <= 0) {  // :190-192
        check(nfm_psgd_finalize(o_));
        sfm.pull();
        callback(*this, sfm);
      }
      if (std::isnan(runningLoss)) { std::printf("Loss is NaN. Use smaller learning rate.\n"); break; }  // :194-196
      if (std::fabs(runningLoss - runningLossOld) < tol) {  // :198-201
        if (verbose > 0) std::printf("Converged at epoch %d.\n", epoch);
        isConverged = true;
        break;
      }
      if (verbose > 0) {  // :203-207, on the working values (no finalize: it would move the caches)
        sfm.pull();
        double regVal = 0.5 * alpha0 * sfm.intercept * sfm.intercept;
        double wsq = 0.0, psq = 0.0;
        for (double v : sfm.w) wsq += v * v;
        for (double v : sfm.P) psq += v * v;
        regVal += 0.5 * alpha * wsq + 0.5 * beta * psq;
        const int64_t da = sfm.nOrders() * sfm.nComponents > 0 ? (int64_t)sfm.P.size() / (sfm.nOrders() * sfm.nComponents) : 0;
        for (int order = 0; order < sfm.nOrders(); ++order)
          regVal += gamma * regEval(reg, sfm.P.data() + (size_t)order * sfm.nComponents * da, sfm.nComponents, da, sfm.degree - order);
        std::printf("%-5d   %-10.4e   %-10.4e\n", epoch + 1, runningLoss, regVal);
      }
      runningLossOld = runningLoss;
    }
    if (!isConverged && verbose > 0) std::printf("Objective did not converge. Increase maxIter.\n");
    check(nfm_psgd_finalize(o_));  // :215
    sfm.pull();
  }

 private:
  nfm_opt* o_ = nullptr; nfm_model* m_ = nullptr;
};

namespace detail {
// The fit shared by the solvers that run one whole iteration per nfm_opt_epoch call, from checkTarget on: the CD family
// (cd.nim:128-186, pcd.nim:110-201, pbcd.nim:212-329) and the PGD family (pgd.nim:186-217, fista.nim:99-141,
// nmapgd.nim:221-268).  It owns the handle cache and the loop; the stopping rule, the verbose lines and the callback run here
// where the reference has them.  The per-class pieces:
//   create(m, &o)           makes the device optimizer o of the model m (kept while the model is: it carries CD's schedule, or
//                           t and NMAPGD's c, q and caches between warm-started fits)
//   begin(o)                nfm_cd_begin_fit / nfm_pgd_begin_fit
//   record(o, ls, viol, n)  -> the iteration's (viol, lossVal), which is also its history entry
//   regValue(fm, n)         the verbose line's regularisation (CD pulls the model for it, PGD has the library's figure)
//   callbackFirst           the callback before the verbose line, or after it (pcd.nim:188-192, pbcd.nim:302-314)
//   label(t)                "Converged at <label>." for the iteration of index t
// history, and iterations where the class has them, are cleared once the fit has begun.
template <class Opt>
auto clear_records(Opt& self, int) -> decltype(self.iterations.clear()) { self.history.clear(); self.iterations.clear(); }
template <class Opt>
void clear_records(Opt& self, long) { self.history.clear(); }
template <class Opt, class Label, class Create, class Begin, class Record, class RegValue>
void whole_iter_fit(Opt& self, nfm_opt*& o, nfm_model*& om, const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& fm,
                    const std::function<void(Opt&, FactorizationMachine&)>& callback, bool callbackFirst, Label label, Create create,
                    Begin begin, Record record, RegValue regValue) {
  check(nfm_dataset_set_targets(X.handle(), y.data()));
  nfm_model* m = fm.push();
  if (!o || om != m) {
    if (o) nfm_opt_destroy(o);
    o = nullptr;
    check(create(m, &o));
    om = m;
  }
  check(begin(o));
  const int64_t n = X.nSamples();
  if (self.verbose > 0) std::printf("Epoch   Violation    Loss         Regularization\n");
  clear_records(self, 0);
  bool isConverged = false;
  for (int t = 0; t < self.maxIter; ++t) {
    double ls = 0.0, vs = 0.0;
    check(nfm_opt_epoch(o, X.handle(), nullptr, 0, n, &ls, &vs));
    const std::pair<double, double> rec = record(o, ls, vs, n);
    self.history.push_back(rec);
    if (callback && callbackFirst) {
      fm.pull();
      callback(self, fm);
    }
    if (self.verbose > 0) std::printf("%-5d   %-10.4e   %-10.4e   %-10.4e\n", t + 1, rec.first, rec.second, regValue(fm, n));
    if (callback && !callbackFirst) {
      fm.pull();
      callback(self, fm);
    }
    if (rec.first < self.tol) {
      if (self.verbose > 0) std::printf("Converged at %s.\n", label(t).c_str());
      isConverged = true;
      break;
    }
  }
  if (!isConverged && self.verbose > 0) std::printf("Objective did not converge. Increase maxIter.\n");
  fm.pull();
}

// CD, PCD and PBCD: penalty(fm, nd) is the verbose line's regularisation times nSamples, on the pulled model
template <class Opt, class Create, class Penalty>
void cd_fit(Opt& self, nfm_opt*& o, nfm_model*& om, const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& fm,
            const std::function<void(Opt&, FactorizationMachine&)>& callback, bool callbackFirst, Create create, Penalty penalty) {
  whole_iter_fit(
      self, o, om, X, y, fm, callback, callbackFirst, [](int t) { return "iteration " + std::to_string(t + 1); }, create,
      [&](nfm_opt* h) { return nfm_cd_begin_fit(h, X.handle()); },  // cd.nim:128-153
      [](nfm_opt*, double ls, double viol, int64_t n) { return std::make_pair(viol, ls / (double)n); },
      [&](FactorizationMachine& f, int64_t n) {
        f.pull();
        return penalty(f, (double)n) / (double)n;
      });
}

// cd.nim:176-184: the L2 terms with the strengths scaled by nSamples
inline double cd_l2(const FactorizationMachine& fm, double alpha0, double alpha, double beta, double nd) {
  double pw = 0.0, pp = 0.0;
  for (double v : fm.w) pw += v * v;
  for (double v : fm.P) pp += v * v;
  return 0.5 * alpha0 * nd * fm.intercept * fm.intercept + 0.5 * alpha * nd * pw + 0.5 * beta * nd * pp;
}
}  // namespace detail

// CD[L], optimizer/cd.nim:6-25,128-186: coordinate descent.  The caches and every iteration run on the device as a level
// schedule over the features (nfm_cd_begin_fit, then one nfm_opt_epoch per iteration); the loop, the stopping rule, the
// verbose lines and the callback run here.
template <class L = Squared>
class CD {
 public:
  int maxIter; double alpha0, alpha, beta; L loss; int verbose; double tol;
  std::vector<std::pair<double, double>> history;  // (viol, mean loss) per iteration
  explicit CD(int maxIter_ = 100, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-3, L loss_ = L(), int verbose_ = 1,
              double tol_ = 1e-3)
      : maxIter(maxIter_), alpha0(alpha0_), alpha(alpha_), beta(beta_), loss(loss_), verbose(verbose_), tol(tol_) {}
  CD(const CD&) = delete;
  ~CD() { if (o_) nfm_opt_destroy(o_); }
  void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& fm,
           std::function<void(CD&, FactorizationMachine&)> callback = nullptr) {
    fm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    detail::cd_fit(
        *this, o_, m_, X, y, fm, callback, true,
        [&](nfm_model* m, nfm_opt** o) { return nfm_cd_create(m, alpha0, alpha, beta, L::id, loss.param, o); },
        [&](const FactorizationMachine& f, double nd) { return detail::cd_l2(f, alpha0, alpha, beta, nd); });
  }

 private:
  nfm_opt* o_ = nullptr; nfm_model* m_ = nullptr;
};

// PCD[L, R], optimizer/pcd.nim:9-35,110-201: proximal coordinate descent with R = L1, SquaredL12 (column-wise by default)
// or OmegaTI.  CD's device iteration with a proximal step per feature (nfm_pcd_create); the loop,
// the stopping rule, the verbose lines and the callback run here, the verbose line before the callback (:188-192).
template <class L = Squared, class R = SquaredL12>
class PCD {
 public:
  int maxIter; double alpha0, alpha, beta, gamma; L loss; R reg; int verbose; double tol;
  std::vector<std::pair<double, double>> history;  // (viol, mean loss) per iteration
  explicit PCD(int maxIter_ = 100, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4, double gamma_ = 1e-4,
               L loss_ = L(), R reg_ = R(), int verbose_ = 1, double tol_ = 1e-3)
      : maxIter(maxIter_), alpha0(alpha0_), alpha(alpha_), beta(beta_), gamma(gamma_), loss(loss_), reg(reg_), verbose(verbose_),
        tol(tol_) {}
  PCD(const PCD&) = delete;
  ~PCD() { if (o_) nfm_opt_destroy(o_); }
  void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& sfm,
           std::function<void(PCD&, FactorizationMachine&)> callback = nullptr) {
    sfm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    if (R::id == NFM_REG_SQUAREDL12 && sfm.degree != 2) throw std::invalid_argument("SquaredL12 supports only degree=2.");
    detail::cd_fit(
        *this, o_, m_, X, y, sfm, callback, false,
        [&](nfm_model* m, nfm_opt** o) {
          return nfm_pcd_create(m, alpha0, alpha, beta, gamma, L::id, loss.param, R::id, reg.transpose ? 1 : 0, o);
        },
        [&](const FactorizationMachine& f, double nd) {  // :176-189: gamma * n * reg.eval per order, then the L2 terms
          const int k = f.nComponents;
          const int64_t da = f.nOrders() * k > 0 ? (int64_t)f.P.size() / (f.nOrders() * k) : 0;
          double regVal = 0.0;
          for (int o = 0; o < f.nOrders(); ++o) regVal += gamma * nd * regEval(reg, f.P.data() + (size_t)o * k * da, k, da, f.degree - o);
          regVal += detail::cd_l2(f, alpha0, alpha, beta, nd);
          return regVal;
        });
  }

 private:
  nfm_opt* o_ = nullptr; nfm_model* m_ = nullptr;
};

// PBCD[L, R], optimizer/pbcd.nim:8-46,212-329 at maxSearch = 0: proximal block coordinate descent with R = L1, L21,
// SquaredL21 (the default) or OmegaCS (any degree).  A feature's whole row of P steps at once on the device (nfm_pbcd_create; DESIGN.md section
// 14); beta and gamma are not scaled by nSamples (:138,147,154).  The loop, the stopping rule, the verbose lines and the
// callback run here, the verbose line before the callback (:302-314).  shrink is stored and never read, as in the reference.
template <class L = Squared, class R = SquaredL21>
class PBCD {
 public:
  int maxIter; double alpha0, alpha, beta, gamma; L loss; R reg; int verbose; double tol, sigma, rho; int maxSearch;
  bool shrink, shuffle;
  std::vector<std::pair<double, double>> history;  // (viol, mean loss) per iteration
  explicit PBCD(int maxIter_ = 100, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4, double gamma_ = 1e-4,
                L loss_ = L(), R reg_ = R(), int verbose_ = 1, double tol_ = 1e-3, double sigma_ = 0.01, double rho_ = 0.5,
                int maxSearch_ = 0, bool shrink_ = false, bool shuffle_ = false)
      : maxIter(maxIter_), alpha0(alpha0_), alpha(alpha_), beta(beta_), gamma(gamma_), loss(loss_), reg(reg_), verbose(verbose_),
        tol(tol_), sigma(sigma_), rho(rho_), maxSearch(maxSearch_), shrink(shrink_), shuffle(shuffle_) {}
  PBCD(const PBCD&) = delete;
  ~PBCD() { if (o_) nfm_opt_destroy(o_); }
  void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& sfm,
           std::function<void(PBCD&, FactorizationMachine&)> callback = nullptr) {
    if (R::id == NFM_REG_SQUAREDL12) throw std::invalid_argument("PBCD cannot be used for squaredl12.");  // nimfm_sparsefm.nim:118
    if (R::id == NFM_REG_SQUAREDL21 && reg.transpose) throw std::invalid_argument("transpose=true is not supported for BCD.");
    if (maxSearch != 0) throw std::invalid_argument("maxSearch != 0 (the line search, pbcd.nim:80-109) is not supported");
    if (shuffle) throw std::invalid_argument("shuffle=true is not supported: the features step in the schedule's order");
    sfm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    if (R::id == NFM_REG_SQUAREDL21 && sfm.degree != 2) throw std::invalid_argument("SquaredL21 supports only degree=2.");
    detail::cd_fit(
        *this, o_, m_, X, y, sfm, callback, false,
        [&](nfm_model* m, nfm_opt** o) { return nfm_pbcd_create(m, alpha0, alpha, beta, gamma, L::id, loss.param, R::id, maxSearch, o); },
        [&](const FactorizationMachine& f, double nd) {  // :303-306: the UNSCALED strengths (cd_fit divides by nSamples)
          const int k = f.nComponents;
          const int64_t da = f.nOrders() * k > 0 ? (int64_t)f.P.size() / (f.nOrders() * k) : 0;
          double regVal = detail::cd_l2(f, alpha0, alpha, beta, 1.0);
          for (int o = 0; o < f.nOrders(); ++o) regVal += gamma * regEval(reg, f.P.data() + (size_t)o * k * da, k, da, f.degree - o);
          return regVal * nd;
        });
  }

 private:
  nfm_opt* o_ = nullptr; nfm_model* m_ = nullptr;
};

// predictAllWithGrad, optimizer/pgd.nim:70-103: yPred, dL and the gradient of the mean loss at sfm's parameters;
// gradP in the reference's training layout [nOrders][d + nAugments][k]
struct Grads { std::vector<double> P, w; double intercept = 0.0, loss = 0.0; };
template <class L = Squared>
inline Grads predictAllWithGrad(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& sfm,
                                std::vector<double>& yPred, std::vector<double>& dL, L loss = L()) {
  if (!sfm.isInitialized) throw NotFittedError("Factorization machines is not fitted.");
  if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
  check(nfm_dataset_set_targets(X.handle(), y.data()));
  nfm_model* m = sfm.push();
  nfm_mbpsgd_cfg c{0.1, 1e-6, 1e-3, 1e-4, 1e-4, 1.0, loss.param, L::id, (int32_t)optimal, NFM_REG_L1, 0, 1};
  nfm_opt* o = nullptr;
  check(nfm_mbpsgd_create(m, &c, &o));
  Grads g;
  g.P.assign(sfm.P.size(), 0.0);
  g.w.assign((size_t)X.nFeatures(), 0.0);
  yPred.assign((size_t)X.nSamples(), 0.0);
  dL.assign((size_t)X.nSamples(), 0.0);
  const int32_t rc = nfm_opt_predict_all_with_grad(o, X.handle(), yPred.data(), dL.data(), g.P.data(), g.w.data(), &g.intercept, &g.loss);
  nfm_opt_destroy(o);
  check(rc);
  g.loss /= (double)std::max<int64_t>(X.nSamples(), 1);
  return g;
}

namespace detail {
// PGD, FISTA and NMAPGD.  The algorithm -- gradient, line search, accept / restart and Z / V -- runs in the library with every
// parameter set resident on the device (nfm_pgd_create / nfm_pgd_begin_fit / nfm_opt_epoch); the
// stopping test is on the SQUARED distance.
struct PgdIter { double lossVal, regVal, viol, eta[2], start[2]; int trials[2], branch; double t, c, q; };
template <class Opt>
void pgd_fit(Opt& self, int32_t algo, double etaNm, int epochLabelOffset, nfm_opt*& o, nfm_model*& om, const CSRDataset& X,
             const std::vector<double>& y, FactorizationMachine& sfm, const std::function<void(Opt&, FactorizationMachine&)>& callback) {
  using R = decltype(self.reg);
  if (R::id == NFM_REG_OMEGATI) throw std::invalid_argument("OmegaTI has no matrix proximal operator");
  if (R::id == NFM_REG_OMEGACS) throw std::invalid_argument("OmegaCS has no matrix proximal operator");
  sfm.init(X);
  if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
  if ((R::id == NFM_REG_SQUAREDL12 || R::id == NFM_REG_SQUAREDL21) && sfm.degree != 2)  // initSGD, squaredl12.nim:103-105
    throw std::invalid_argument(R::id == NFM_REG_SQUAREDL12 ? "SquaredL12 supports only degree=2." : "SquaredL21 supports only degree=2.");
  PgdIter rec{};
  whole_iter_fit(
      self, o, om, X, y, sfm, callback, true,  // pgd.nim:197-199: the callback, then the verbose line
      [&](int t) { return "epoch " + std::to_string(t + epochLabelOffset); },
      [&](nfm_model* m, nfm_opt** h) {
        return nfm_pgd_create(m, algo, self.alpha0, self.alpha, self.beta, self.gamma, self.rho, self.sigma, etaNm,
                              decltype(self.loss)::id, self.loss.param, R::id, self.reg.transpose ? 1 : 0, self.maxSearch, h);
      },
      [&](nfm_opt* h) { return nfm_pgd_begin_fit(h, X.handle(), sfm.warmStart ? 1 : 0); },
      [&](nfm_opt* h, double, double, int64_t) {
        double r[NFM_PGD_IT_COUNT];
        check(nfm_pgd_last_iter(h, r));
        rec = PgdIter{r[NFM_PGD_IT_LOSS], r[NFM_PGD_IT_REG], r[NFM_PGD_IT_VIOL], {r[NFM_PGD_IT_ETA], r[NFM_PGD_IT_ETA_V]},
                      {r[NFM_PGD_IT_START], r[NFM_PGD_IT_START_V]}, {(int)r[NFM_PGD_IT_TRIALS], (int)r[NFM_PGD_IT_TRIALS_V]},
                      (int)r[NFM_PGD_IT_BRANCH], r[NFM_PGD_IT_T], r[NFM_PGD_IT_C], r[NFM_PGD_IT_Q]};
        self.iterations.push_back(rec);
        return std::make_pair(rec.viol, rec.lossVal);
      },
      [&](FactorizationMachine&, int64_t) { return rec.regVal; });
}
}  // namespace detail

#define NIMFM_PGD_HOST(NAME, ALGO, LABEL, ETA_DECL, ETA_USE)                                                                             \
  template <class L = Squared, class R = SquaredL12>                                                                                     \
  class NAME {                                                                                                                           \
   public:                                                                                                                               \
    int maxIter; double alpha0, alpha, beta, gamma; L loss; R reg; double rho, sigma; int maxSearch; ETA_DECL int verbose; double tol;   \
    std::vector<std::pair<double, double>> history; /* (viol, lossVal) per iteration */                                                  \
    std::vector<detail::PgdIter> iterations;        /* nfm_pgd_last_iter of every iteration */                                           \
    NAME(const NAME&) = delete;                                                                                                          \
    ~NAME() { if (o_) nfm_opt_destroy(o_); }                                                                                             \
    void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& sfm,                                               \
             std::function<void(NAME&, FactorizationMachine&)> callback = nullptr) {                                                     \
      detail::pgd_fit(*this, ALGO, ETA_USE, LABEL, o_, m_, X, y, sfm, callback);                                                         \
    }                                                                                                                                    \
   private:                                                                                                                              \
    nfm_opt* o_ = nullptr; nfm_model* m_ = nullptr;                                                                                      \
   public:

// PGD[L, R], optimizer/pgd.nim:10-42,149-217 ("Converged at epoch" prints `epoch`, not `epoch + 1`, :209 -- kept)
NIMFM_PGD_HOST(PGD, NFM_PGD_ALGO_PGD, 0, , 0.5)
  explicit PGD(int maxIter_ = 100, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4, double gamma_ = 1e-4, L loss_ = L(),
               R reg_ = R(), double rho_ = 0.5, double sigma_ = 1.0, int maxSearch_ = -1, int verbose_ = 1, double tol_ = 1e-6)
      : maxIter(maxIter_), alpha0(alpha0_), alpha(alpha_), beta(beta_), gamma(gamma_), loss(loss_), reg(reg_), rho(rho_), sigma(sigma_),
        maxSearch(maxSearch_), verbose(verbose_), tol(tol_) {}
};
// FISTA[L, R], optimizer/fista.nim:10-43,52-141; t stays on the optimizer for a warm-started model
NIMFM_PGD_HOST(FISTA, NFM_PGD_ALGO_FISTA, 1, , 0.5)
  explicit FISTA(int maxIter_ = 100, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4, double gamma_ = 1e-4, L loss_ = L(),
                 R reg_ = R(), double rho_ = 0.5, double sigma_ = 1.0, int maxSearch_ = -1, int verbose_ = 1, double tol_ = 1e-6)
      : maxIter(maxIter_), alpha0(alpha0_), alpha(alpha_), beta(beta_), gamma(gamma_), loss(loss_), reg(reg_), rho(rho_), sigma(sigma_),
        maxSearch(maxSearch_), verbose(verbose_), tol(tol_) {}
};
// NMAPGD[L, R], optimizer/nmapgd.nim:10-46,174-268; alpha0 is accepted and ignored (:44 stores alpha0: alpha); eta is the
// non-monotonicity, not a step size; t, c, q and the caches stay on the optimizer for a warm-started model
NIMFM_PGD_HOST(NMAPGD, NFM_PGD_ALGO_NMAPGD, 1, double eta;, this->eta)
  explicit NMAPGD(int maxIter_ = 100, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4, double gamma_ = 1e-4, L loss_ = L(),
                  R reg_ = R(), double rho_ = 0.5, double sigma_ = 0.01, int maxSearch_ = -1, double eta_ = 0.5, int verbose_ = 1,
                  double tol_ = 1e-5)
      : maxIter(maxIter_), alpha0(alpha0_), alpha(alpha_), beta(beta_), gamma(gamma_), loss(loss_), reg(reg_), rho(rho_), sigma(sigma_),
        maxSearch(maxSearch_), eta(eta_), verbose(verbose_), tol(tol_) {}
};
#undef NIMFM_PGD_HOST

// Katyusha[L, R], optimizer/katyusha.nim:11-53,156-269.  The seven parameter sets, the variance-reduced mini-batch gradient
// and the dense updates of the inner loop stay on the device (nfm_katyusha_create / nfm_katyusha_begin_fit / one nfm_opt_epoch
// per outer iteration); the index stream (:108-118), the stopping test on viol, the per-epoch callback
// and the verbose lines run here.  After every outer iteration the model holds what finalize (:56-73) gives the user.
// nCalls > 0 is refused; beta <= 0, alpha <= 0 with fitLinear, alpha0 <= 0 with fitIntercept and eta <= 0 throw
// std::invalid_argument (nfm_katyusha_create) where the reference returns NaN parameters.  history: (viol, lossVal).
template <class L = Squared, class R = SquaredL12>
class Katyusha {
 public:
  int maxIter; double eta, alpha0, alpha, beta, gamma; L loss; R reg; int64_t miniBatchSize; double tau1, tau2; int verbose;
  double tol; bool shuffle; int nCalls;
  std::vector<std::pair<double, double>> history;  // (viol, lossVal) per outer iteration
  explicit Katyusha(int maxIter_ = 100, double eta_ = 0.1, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-4,
                    double gamma_ = 1e-4, L loss_ = L(), R reg_ = R(), int64_t miniBatchSize_ = -1, double tau1_ = 0.5,
                    double tau2_ = -1.0, int verbose_ = 1, double tol_ = 1e-6, bool shuffle_ = true, int nCalls_ = -1)
      : maxIter(maxIter_), eta(eta_), alpha0(alpha0_), alpha(alpha_), beta(beta_), gamma(gamma_), loss(loss_), reg(reg_),
        miniBatchSize(miniBatchSize_), tau1(tau1_), tau2(tau2_), verbose(verbose_), tol(tol_), shuffle(shuffle_), nCalls(nCalls_) {}
  Katyusha(const Katyusha&) = delete;
  ~Katyusha() { if (o_) nfm_opt_destroy(o_); }
  nfm_opt* handle() const { return o_; }
  void fit(const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& sfm,
           std::function<void(Katyusha&, FactorizationMachine&)> callback = nullptr) {
    if (R::id == NFM_REG_OMEGATI) throw std::invalid_argument("OmegaTI has no matrix proximal operator");
    if (R::id == NFM_REG_OMEGACS) throw std::invalid_argument("OmegaCS has no matrix proximal operator");
    if (nCalls > 0)
      throw std::invalid_argument("Katyusha: nCalls > 0 (a callback inside the inner loop) is not supported; nCalls <= 0 calls the callback once per epoch");
    sfm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    const int64_t n = X.nSamples();
    const int64_t B = miniBatchSize > 0 ? miniBatchSize : detail::default_batch(X);  // :203-206
    const int64_t inner = (n - 1) / B + 1;                                           // :207
    nfm_model* m = sfm.push();
    if (o_) nfm_opt_destroy(o_);  // nothing is carried between fits
    o_ = nullptr;
    check(nfm_katyusha_create(m, eta, alpha0, alpha, beta, gamma, tau1, tau2, L::id, loss.param, R::id, reg.transpose ? 1 : 0, B, &o_));
    check(nfm_katyusha_begin_fit(o_, X.handle()));
    std::vector<int64_t> chunk((size_t)(B * inner));
    detail::IndexStream stream(n, shuffle, sfm.rng());
    if (verbose > 0) {
      std::printf("Minibatch size: %lld\nNumber of inner iteration: %lld\n", (long long)B, (long long)inner);
      std::printf("%-*s   %-10s   %-10s   Regularization\n", (int)std::to_string(maxIter).size(), "Epoch", "Violation", "Loss");
    }
    history.clear();
    bool isConverged = false;
    const int k = sfm.nComponents, no = sfm.nOrders();
    const int64_t da = X.nFeatures() + sfm.nAugments();
    std::vector<double> tP((size_t)no * da * k), tw((size_t)X.nFeatures());
    for (int t = 0; t < maxIter; ++t) {
      stream.fill(chunk);  // :108-118
      double ls = 0.0, viol = 0.0;
      check(nfm_opt_epoch(o_, X.handle(), chunk.data(), 0, (int64_t)chunk.size(), &ls, &viol));
      const double lossVal = ls / (double)n;  // :241-244: the loss at the snapshot the epoch started from
      history.emplace_back(viol, lossVal);
      if (callback) {  // :237-239: the finalized model
        sfm.pull();
        callback(*this, sfm);
      }
      if (std::isnan(lossVal)) { std::printf("Loss is NaN. Use smaller learning rate.\n"); break; }
      if (verbose > 0) {  // :249-253: regVal on tilde
        double tb = 0.0, wsq = 0.0, psq = 0.0;
        check(nfm_katyusha_snapshot(o_, tP.empty() ? nullptr : tP.data(), tw.data(), &tb));
        for (double v : tw) wsq += v * v;
        for (double v : tP) psq += v * v;
        double regVal = 0.5 * alpha0 * tb * tb + 0.5 * alpha * wsq + 0.5 * beta * psq;
        for (int o = 0; o < no; ++o) regVal += gamma * regEval(reg, OrderView{tP.data() + (size_t)o * da * k, k, da, 1, k}, sfm.degree - o);
        std::printf("%-*d   %-10.4e   %-10.4e   %-10.4e\n", std::max(5, (int)std::to_string(maxIter).size()), t + 1, viol, lossVal, regVal);
      }
      if (viol < tol) {  // :255-258
        if (verbose > 0) std::printf("Converged at epoch %d.\n", t + 1);
        isConverged = true;
        break;
      }
    }
    if (!isConverged && verbose > 0) std::printf("Objective did not converge. Increase maxIter.\n");
    sfm.pull();  // :269: finalize's model, already in the handle
  }

 private:
  nfm_opt* o_ = nullptr;
};

// ---- ConvexFactorizationMachine and Hazan's algorithm ----
// model/convex_factorization_machine.nim:6-84: P [nComponents][nFeatures] row-major, lams [nComponents], w, intercept;
// nComponents = lams.size() grows from 0 to maxComponents
class ConvexFactorizationMachine {
 public:
  TaskKind task;
  int maxComponents;
  bool fitIntercept, fitLinear, ignoreDiag, warmStart;
  bool isInitialized = false;
  std::vector<double> P, lams, w;
  double intercept = 0.0;

  // newConvexFactorizationMachine, :25-46
  explicit ConvexFactorizationMachine(TaskKind task_, int maxComponents_ = 30, bool fitIntercept_ = true, bool fitLinear_ = true,
                                      bool ignoreDiag_ = true, bool warmStart_ = false)
      : task(task_), maxComponents(maxComponents_), fitIntercept(fitIntercept_), fitLinear(fitLinear_), ignoreDiag(ignoreDiag_),
        warmStart(warmStart_) {
    if (maxComponents < 1) throw std::invalid_argument("maxComponents < 1.");
  }
  ConvexFactorizationMachine(const ConvexFactorizationMachine&) = delete;
  ~ConvexFactorizationMachine() { if (h_) nfm_model_destroy(h_); }

  int nComponents() const { return (int)lams.size(); }
  // init, :49-60
  void init(const CSRDataset& X, bool force = false) {
    if (force || !(warmStart && isInitialized)) {
      d_ = X.nFeatures();
      w.assign(d_, 0.0);
      P.clear();
      lams.clear();
      intercept = 0.0;
      dirty_ = true;
    }
    isInitialized = true;
  }
  void setParams(std::vector<double> P_, std::vector<double> lams_, std::vector<double> w_, double b) {
    d_ = (int64_t)w_.size();
    if (P_.size() != lams_.size() * (size_t)d_ || (int)lams_.size() > maxComponents) throw std::invalid_argument("bad P shape");
    P = std::move(P_); lams = std::move(lams_); w = std::move(w_); intercept = b; isInitialized = true; dirty_ = true;
  }
  // decisionFunction, :63-84
  std::vector<double> decisionFunction(const CSRDataset& X) {
    if (!isInitialized) throw NotFittedError("Factorization machines is not fitted.");
    if (X.nFeatures() != d_) throw std::invalid_argument("Invalid nFeatures.");
    std::vector<double> out(X.nSamples());
    check(nfm_decision_function(push(), X.handle(), out.data()));
    return out;
  }
  double score(const CSRDataset& X, const std::vector<double>& y) {  // fm_base.nim:39-48
    if (!isInitialized) throw NotFittedError("Factorization machines is not fitted.");
    if (X.nFeatures() != d_) throw std::invalid_argument("Invalid nFeatures.");
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    double out = 0.0;
    check(nfm_score(push(), X.handle(), &out));
    return out;
  }
  nfm_model* push() {
    if (!h_ || hd_ != d_) {
      if (h_) nfm_model_destroy(h_);
      h_ = nullptr;
      check(nfm_cfm_create(default_context(), (int32_t)task, maxComponents, fitIntercept, fitLinear, ignoreDiag, d_, &h_));
      hd_ = d_;
      dirty_ = true;
    }
    if (dirty_) {
      check(nfm_cfm_set_params(h_, nComponents(), P.empty() ? nullptr : P.data(), lams.empty() ? nullptr : lams.data(), w.data(), intercept));
      dirty_ = false;
    }
    return h_;
  }
  void pull() {
    int32_t nc = 0;
    std::vector<double> Pm((size_t)maxComponents * d_), lm((size_t)maxComponents);
    check(nfm_cfm_get_params(h_, &nc, Pm.data(), lm.data(), w.data(), &intercept));
    P.assign(Pm.begin(), Pm.begin() + (size_t)nc * d_);
    lams.assign(lm.begin(), lm.begin() + nc);
    dirty_ = false;
  }

 private:
  nfm_model* h_ = nullptr;
  int64_t d_ = 0, hd_ = -1;
  bool dirty_ = true;
};

// Nim's global generator as the library restates it (nfm_rng_*): randomize(seed), then the uniform draws of the power
// method's start vector
struct NimRand {
  uint64_t state[2] = {0x69B4C98CB8530805ull, 0xFED1DD3004688D68ull};
  void randomize(int64_t seed) { check(nfm_rng_randomize(seed, state)); }
  std::vector<double> rand(int64_t n, double max = 1.0) {
    std::vector<double> out((size_t)n);
    check(nfm_rng_rand_uniform(state, n, max, out.data()));
    return out;
  }
};
inline NimRand& globalRand() {
  static NimRand r;
  return r;
}

// ---- datasets made from datasets on the device (include/nimfm_hip.h) ----
enum NormKind { l1 = 0, l2 = 1, linfty = 2 };  // tensor/sparse.nim:37-38
namespace detail {
inline CSRDataset stack(int32_t (*entry)(nfm_dataset* const*, int64_t, nfm_dataset**), const std::vector<const CSRDataset*>& dataseq) {
  if (dataseq.empty()) throw std::invalid_argument("no datasets to stack");
  std::vector<nfm_dataset*> hs;
  for (const CSRDataset* X : dataseq) hs.push_back(X->handle());
  nfm_dataset* h = nullptr;
  check(entry(hs.data(), (int64_t)hs.size(), &h));
  return CSRDataset(h);
}
}  // namespace detail
// vstack / hstack (tensor/sparse.nim:564-581, 613-633 / :671-698, 719-750)
inline CSRDataset vstack(const std::vector<const CSRDataset*>& dataseq) { return detail::stack(nfm_dataset_vstack, dataseq); }
inline CSRDataset hstack(const std::vector<const CSRDataset*>& dataseq) { return detail::stack(nfm_dataset_hstack, dataseq); }
// normalize (dataset.nim:398-403): in place, as the reference
inline void normalize(CSRDataset& X, int axis = 1, NormKind norm = l2) {
  nfm_dataset* h = nullptr;
  check(nfm_dataset_normalize(X.handle(), axis, (int32_t)norm, &h));
  X.swapHandle(h);
}
// shuffle (dataset.nim:372-395): (X[indices], y[indices]); without indices the forward draw from the global generator
template <class U>
inline std::pair<CSRDataset, std::vector<U>> shuffle(const CSRDataset& X, const std::vector<U>& y, const std::vector<int64_t>& indices) {
  if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("X.nSamples != len(y)");
  nfm_dataset* h = nullptr;
  check(nfm_dataset_select_rows(X.handle(), indices.data(), (int64_t)indices.size(), &h));
  std::vector<U> ys(indices.size());
  for (size_t ii = 0; ii < indices.size(); ++ii) ys[ii] = y[(size_t)indices[ii]];
  return std::pair<CSRDataset, std::vector<U>>(std::piecewise_construct, std::forward_as_tuple(h), std::forward_as_tuple(std::move(ys)));
}
template <class U>
inline std::pair<CSRDataset, std::vector<U>> shuffle(const CSRDataset& X, const std::vector<U>& y) {
  if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("X.nSamples != len(y)");
  std::vector<int64_t> indices(y.size());
  std::iota(indices.begin(), indices.end(), (int64_t)0);
  check(nfm_rng_shuffle_forward(globalRand().state, indices.data(), (int64_t)indices.size()));
  return shuffle(X, y, indices);
}
// loadUserItemRatingFile (dataset.nim:840-900): the text is parsed on the GPU; X takes the new dataset
inline void loadUserItemRatingFile(const std::string& f, CSRDataset& X, std::vector<double>& y) {
  nfm_dataset* h = nullptr;
  check(nfm_dataset_load_user_item(default_context(), f.c_str(), &h));
  X.swapHandle(h);
  y = X.targets();
}

// ---- column-major datasets (include/nimfm_hip.h) ----
// dataset.nim:18-22 + tensor/sparse.nim:14-17: CSC columns resident on the device, beside the row twin the library makes
// of them.  It IS a CSRDataset to everything that takes rows: decisionFunction, predict, score and the fit of CD, PCD,
// PBCD, Hazan and GreedyCD (the reference's ColDataset solvers) run on the twin, bit-equal to the same call on
// toCSRDataset(X); the row-wise solvers, X[indices], shuffle and the dumps are refused by the library (std::runtime_error
// naming toCSRDataset), where the reference does not compile.
class CSCDataset : public CSRDataset {
 public:
  // newCSCDataset (dataset.nim:124-129): indptr has nFeatures + 1 entries, indices are sample ids
  CSCDataset(const std::vector<double>& data, const std::vector<int64_t>& indices, const std::vector<int64_t>& indptr,
             int64_t nSamples, int64_t nFeatures)
      : CSRDataset(create(data, indices, indptr, nSamples, nFeatures)) {}
  // a column-major dataset made by the library (the handle is adopted)
  explicit CSCDataset(nfm_dataset* h) : CSRDataset(h) {
    int32_t layout = NFM_LAYOUT_CSR;
    check(nfm_dataset_layout(h, &layout));
    if (layout != NFM_LAYOUT_CSC) throw std::invalid_argument("the handle is a row-major dataset");
  }
  // X[a..<b] (tensor/sparse.nim:300-330)
  CSCDataset slice(int64_t begin, int64_t end) const {
    nfm_dataset* h = nullptr;
    check(nfm_dataset_slice_rows(handle(), begin, end, &h));
    return CSCDataset(h);
  }
  // the column arrays in the reference's widths
  void toHost(std::vector<int64_t>& indptr, std::vector<int64_t>& indices, std::vector<double>& data) const {
    int64_t n = 0, d = 0, nnz = 0, nf = 0;
    check(nfm_dataset_shape(handle(), &n, &d, &nnz, &nf));
    indptr.assign((size_t)d + 1, 0);
    indices.assign((size_t)nnz, 0);
    data.assign((size_t)nnz, 0.0);
    check(nfm_dataset_get_csc(handle(), indptr.data(), indices.data(), data.data()));
  }

 private:
  static nfm_dataset* create(const std::vector<double>& data, const std::vector<int64_t>& indices, const std::vector<int64_t>& indptr,
                             int64_t nSamples, int64_t nFeatures) {
    if ((int64_t)indptr.size() != nFeatures + 1) throw std::invalid_argument("len(indptr) != nFeatures + 1");
    nfm_dataset* h = nullptr;
    check(nfm_dataset_create_csc(default_context(), nSamples, nFeatures, indptr.data(), indices.data(), data.data(), nullptr, &h));
    return h;
  }
};
// toCSCDataset / toCSRDataset (tensor/sparse.nim:510-527 / :490-507) on the device; the targets are carried over
inline CSCDataset toCSCDataset(const CSRDataset& X) {
  nfm_dataset* h = nullptr;
  check(nfm_dataset_to_csc(X.handle(), &h));
  return CSCDataset(h);
}
inline CSRDataset toCSRDataset(const CSRDataset& X) {
  nfm_dataset* h = nullptr;
  check(nfm_dataset_to_csr(X.handle(), &h));
  return CSRDataset(h);
}
// vstack / hstack of CSCDatasets (tensor/sparse.nim:583-610 / :701-716): vstack({&A, &B}).  (A list of pointers, not a
// vector: a braced list of CSRDataset pointers must keep choosing the row-major overloads above.)  normalize(X, axis, norm)
// above serves both layouts.
namespace detail {
inline CSCDataset stack_csc(int32_t (*entry)(nfm_dataset* const*, int64_t, nfm_dataset**), std::initializer_list<const CSCDataset*> dataseq) {
  if (dataseq.size() == 0) throw std::invalid_argument("no datasets to stack");
  std::vector<nfm_dataset*> hs;
  for (const CSCDataset* X : dataseq) hs.push_back(X->handle());
  nfm_dataset* h = nullptr;
  check(entry(hs.data(), (int64_t)hs.size(), &h));
  return CSCDataset(h);
}
}  // namespace detail
inline CSCDataset vstack(std::initializer_list<const CSCDataset*> dataseq) { return detail::stack_csc(nfm_dataset_vstack, dataseq); }
inline CSCDataset hstack(std::initializer_list<const CSCDataset*> dataseq) { return detail::stack_csc(nfm_dataset_hstack, dataseq); }
// the loaders as CSC (dataset.nim:643-693, 903-992): the row loader's GPU parse followed by the transposition; the rating
// loader with the CSC overload's line rule (lines of fewer than 5 characters are skipped)
inline std::unique_ptr<CSCDataset> loadSVMLightFileCSC(const std::string& f, std::vector<double>& y, int64_t nFeatures = -1) {
  std::unique_ptr<CSRDataset> rows = loadSVMLightFile(f, y, nFeatures);
  nfm_dataset* h = nullptr;
  check(nfm_dataset_to_csc(rows->handle(), &h));
  return std::unique_ptr<CSCDataset>(new CSCDataset(h));
}
inline std::unique_ptr<CSCDataset> loadUserItemRatingFileCSC(const std::string& f, std::vector<double>& y) {
  nfm_dataset* hr = nullptr;
  check(nfm_dataset_load_user_item_lines(default_context(), f.c_str(), 1, &hr));
  CSRDataset rows(hr);
  y = rows.targets();
  nfm_dataset* h = nullptr;
  check(nfm_dataset_to_csc(rows.handle(), &h));
  return std::unique_ptr<CSCDataset>(new CSCDataset(h));
}

// ---- a dataset on the device -> its text file (include/nimfm_hip.h) ----
namespace detail {
template <class U>
inline void dump(int32_t (*entry)(nfm_dataset*, const char*, const double*, int32_t, int64_t), const std::string& f, const CSRDataset& X,
                 const std::vector<U>& y, int64_t chunkBytes) {
  if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("X.nSamples != len(y).");
  const std::vector<double> yd(y.begin(), y.end());
  check(entry(X.handle(), f.c_str(), yd.data(), std::is_integral<U>::value ? 1 : 0, chunkBytes));
}
}  // namespace detail
// dumpSVMLightFile (dataset.nim:793-805) / dumpFFMFile (dataset.nim:825-837), formatted on the GPU.  y: seq[float64], or
// seq[int] (any integer type), which is written as integers as the reference writes it; without y: the dataset's targets
template <class U>
inline void dumpSVMLightFile(const std::string& f, const CSRDataset& X, const std::vector<U>& y, int64_t chunkBytes = 0) {
  detail::dump(nfm_dataset_dump_svmlight, f, X, y, chunkBytes);
}
inline void dumpSVMLightFile(const std::string& f, const CSRDataset& X, int64_t chunkBytes = 0) {
  check(nfm_dataset_dump_svmlight(X.handle(), f.c_str(), nullptr, 0, chunkBytes));
}
template <class U>
inline void dumpFFMFile(const std::string& f, const CSRDataset& X, const std::vector<U>& y, int64_t chunkBytes = 0) {
  detail::dump(nfm_dataset_dump_ffm, f, X, y, chunkBytes);
}
inline void dumpFFMFile(const std::string& f, const CSRDataset& X, int64_t chunkBytes = 0) {
  check(nfm_dataset_dump_ffm(X.handle(), f.c_str(), nullptr, 0, chunkBytes));
}
// the same bytes in memory (the field-aware form for a field-aware dataset): the counterpart of the loaders' parse
inline std::string formatText(const CSRDataset& X, int64_t chunkBytes = 0) {
  int64_t len = 0;
  check(nfm_dataset_format_text(X.handle(), nullptr, 0, chunkBytes, nullptr, 0, &len));
  std::string out((size_t)len, '\0');
  check(nfm_dataset_format_text(X.handle(), nullptr, 0, chunkBytes, len ? &out[0] : nullptr, len, &len));
  return out;
}

// ---- the binary stream files, written and transposed on the device (include/nimfm_hip.h) ----
// newStreamCSCDataset + loadStreamLabel (dataset.nim:176-179, 1007-1014): the STREAMCSC file becomes resident as a whole
inline std::unique_ptr<CSCDataset> newStreamCSCDataset(const std::string& f, const std::string& fY = "") {
  nfm_dataset* h = nullptr;
  check(nfm_dataset_load_stream_csc(default_context(), f.c_str(), fY.empty() ? nullptr : fY.c_str(), &h));
  return std::unique_ptr<CSCDataset>(new CSCDataset(h));
}
// transposeFile (dataset.nim:1100-1199): the reference's result at a cache that holds every entry; cacheSize is ignored
inline void transposeFile(const std::string& fIn, const std::string& fOut, int cacheSize = 200, int64_t chunkBytes = 0) {
  (void)cacheSize;
  check(nfm_transpose_file(default_context(), fIn.c_str(), fOut.c_str(), chunkBytes));
}
// convertFFMFile (dataset.nim:1202-1299): ids shifted by the smallest index, fields as the text has them
inline void convertFFMFile(const std::string& fIn, const std::string& fOutX, const std::string& fOutY) {
  check(nfm_convert_ffm(default_context(), fIn.c_str(), fOutX.c_str(), fOutY.c_str()));
}
// X as the stream file of its kind (CSRDataset: STREAMCSR / STREAMCSRFIELD, CSCDataset: STREAMCSC), packed on the GPU
inline void dumpStreamFile(const std::string& f, const CSRDataset& X, int64_t chunkBytes = 0) {
  check(nfm_dataset_dump_stream(X.handle(), f.c_str(), chunkBytes));
}
inline std::string formatStream(const CSRDataset& X, int64_t chunkBytes = 0) {
  int64_t len = 0;
  check(nfm_dataset_format_stream(X.handle(), chunkBytes, nullptr, 0, &len));
  std::string out((size_t)len, '\0');
  check(nfm_dataset_format_stream(X.handle(), chunkBytes, len ? &out[0] : nullptr, len, &len));
  return out;
}
// loadStreamLabel (dataset.nim:1007-1014), the one-argument form: the raw float64 values of a label file
inline std::vector<double> loadStreamLabel(const std::string& fIn) {
  std::vector<double> y;
  FILE* f = fopen(fIn.c_str(), "rb");
  if (!f) throw std::invalid_argument(fIn + " cannot be read.");
  double v;
  while (fread(&v, sizeof v, 1, f) == 1) y.push_back(v);
  fclose(f);
  return y;
}

// newHazan(...).fit(X, y, cfm), optimizer/hazan.nim:22-46,59-225.  The outer loop, the nTol rule, the verbose line and the
// callback run here; one nfm_hazan_iter call is one outer iteration and returns its record (history).  The reference's cg has
// no working iteration cap (tensor.nim:992); the library's ends after 1000 iterations and when curv is 0 or not finite.
class Hazan {
 public:
  struct Record { double loss, trace; int slot; double step; int64_t powerIters, cgIters; double eval; int nComponents; };
  int maxIter; double eta; int verbose; double tol; int nTol; int64_t maxIterPower; double tolPower; bool optimal_;
  int64_t it = 0;
  std::vector<Record> history;
  // replaces the d draws of 2 * rand(1.0) - 1.0 per outer iteration (tensor.nim:920-921) when set
  std::function<std::vector<double>(int64_t)> powerInit;

  explicit Hazan(int maxIter_ = 100, double eta_ = 1000.0, int verbose_ = 2, double tol_ = 1e-7, int nTol_ = 10, int64_t maxIterPower_ = 1000,
                 double tolPower_ = 1e-7, bool optimal__ = true)
      : maxIter(maxIter_), eta(eta_), verbose(verbose_), tol(tol_), nTol(nTol_), maxIterPower(maxIterPower_), tolPower(tolPower_),
        optimal_(optimal__) {}
  Hazan(const Hazan&) = delete;
  ~Hazan() { if (o_) nfm_opt_destroy(o_); }

  void fit(const CSRDataset& X, const std::vector<double>& y, ConvexFactorizationMachine& cfm,
           std::function<void(Hazan&, ConvexFactorizationMachine&)> callback = nullptr) {
    cfm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    if (o_) nfm_opt_destroy(o_);
    o_ = nullptr;
    check(nfm_hazan_create(cfm.push(), eta, maxIterPower, tolPower, optimal_, &o_));
    double lossOld = 0.0;
    check(nfm_hazan_begin_fit(o_, X.handle(), &lossOld));
    if (!cfm.warmStart) it = 0;  // :87-88
    const int64_t d = X.nFeatures();
    int nc = cfm.nComponents(), ntol = 0;
    bool isConverged = false;
    history.clear();
    double rec[NFM_HAZAN_REC_COUNT];
    for (int t = 0; t < maxIter; ++t) {
      if (!optimal_ && nc >= cfm.maxComponents) break;  // :137-138
      std::vector<double> start;
      if (powerInit) {
        start = powerInit(d);
      } else {
        start = globalRand().rand(d, 1.0);
        for (auto& v : start) v = 2 * v - 1.0;
      }
      if ((int64_t)start.size() != d) throw std::invalid_argument("powerInit must return nFeatures values");
      check(nfm_hazan_iter(o_, X.handle(), it, start.data(), rec));
      history.push_back(Record{rec[NFM_HAZAN_REC_LOSS], rec[NFM_HAZAN_REC_TRACE], (int)rec[NFM_HAZAN_REC_SLOT], rec[NFM_HAZAN_REC_STEP],
                               (int64_t)rec[NFM_HAZAN_REC_POWER_ITERS], (int64_t)rec[NFM_HAZAN_REC_CG_ITERS], rec[NFM_HAZAN_REC_EVAL],
                               (int)rec[NFM_HAZAN_REC_N_COMPONENTS]});
      nc = history.back().nComponents;
      if (callback) {  // :198-199
        cfm.pull();
        callback(*this, cfm);
      }
      const double lossNew = history.back().loss;
      if (verbose > 0)  // :203-209
        std::printf("Epoch: %*lld   MSE/2: %1.4e   Trace Norm: %1.4e\n", (int)std::to_string(maxIter).size(), (long long)it, lossNew / 2.0,
                    history.back().trace);
      if (lossOld - lossNew < tol) {  // :211-219
        if (++ntol >= nTol) {
          if (verbose > 0) std::printf("Converged at iteration %lld.\n", (long long)(it + 1));
          isConverged = true;
          break;
        }
      } else {
        ntol = 0;
      }
      lossOld = lossNew;
      ++it;
    }
    if (!isConverged && verbose > 0) std::printf("Objective did not converge. Increase maxIter.\n");
    cfm.pull();
  }
  nfm_opt* handle() const { return o_; }

 private:
  nfm_opt* o_ = nullptr;
};

// newGreedyCD(...).fit(X, y, cfm), optimizer/greedy_cd.nim:25-30,415-500 at refitFully = false.  The
// outer and the inner loop, both stopping tests, the refit schedule, the verbose lines and the callback run here; the library
// keeps yPred, dL, K, P, lams, w and the power method's vectors and hands back one record per step.  The power method's start
// vector is drawn only in the inner iterations that add a base, as the reference draws it.  refitFully = true (ADMM, Newton-CG,
// two dsyev calls) stays with the reference: fit throws std::invalid_argument.  sigma, maxIterADMM, tolADMM and
// maxIterLineSearch belong to it: accepted and unused.
template <class L = Squared>
class GreedyCD {
 public:
  struct Inner { int it; bool added; int slot; double lam; int64_t powerIters; double eval; int nComponents; double objective; int nStored;
                 bool refit, checked; };
  struct Outer { double loss, reg, objOld; int nComponents; std::vector<Inner> inner; };
  int maxIter; double alpha0, alpha, beta; L loss; int maxIterInner, nRefitting; bool refitFully; int verbose; double tol;
  int64_t maxIterPower; double tolPower, sigma; int maxIterADMM; double tolADMM; int maxIterLineSearch;
  std::vector<Outer> history;
  // replaces the d draws of 2 * rand(1.0) - 1.0 of an inner iteration that adds a base when set
  std::function<std::vector<double>(int64_t)> powerInit;

  explicit GreedyCD(int maxIter_ = 10, double alpha0_ = 1e-6, double alpha_ = 1e-3, double beta_ = 1e-5, L loss_ = L{}, int maxIterInner_ = 10,
                    int nRefitting_ = 10, bool refitFully_ = false, int verbose_ = 1, double tol_ = 1e-7, int64_t maxIterPower_ = 100,
                    double tolPower_ = 1e-7, double sigma_ = 1e-4, int maxIterADMM_ = 100, double tolADMM_ = 1e-4, int maxIterLineSearch_ = 100)
      : maxIter(maxIter_), alpha0(alpha0_), alpha(alpha_), beta(beta_), loss(loss_), maxIterInner(maxIterInner_), nRefitting(nRefitting_),
        refitFully(refitFully_), verbose(verbose_), tol(tol_), maxIterPower(maxIterPower_), tolPower(tolPower_), sigma(sigma_),
        maxIterADMM(maxIterADMM_), tolADMM(tolADMM_), maxIterLineSearch(maxIterLineSearch_) {
    if (nRefitting < 1) throw std::invalid_argument("nRefitting < 1.");  // the reference would divide by zero (:384)
  }
  GreedyCD(const GreedyCD&) = delete;
  ~GreedyCD() { if (o_) nfm_opt_destroy(o_); }

  void fit(const CSRDataset& X, const std::vector<double>& y, ConvexFactorizationMachine& cfm,
           std::function<void(GreedyCD&, ConvexFactorizationMachine&)> callback = nullptr) {
    if (nRefitting < 1) throw std::invalid_argument("nRefitting < 1.");
    cfm.init(X);
    if ((int64_t)y.size() != X.nSamples()) throw std::invalid_argument("len(y) != nSamples");
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    if (o_) nfm_opt_destroy(o_);
    o_ = nullptr;
    check(nfm_gcd_create(cfm.push(), alpha0, alpha, beta, L::id, loss.param, maxIterPower, tolPower, refitFully, &o_));
    double lossOld = 0.0, regOld = 0.0;
    const int32_t rc = nfm_gcd_begin_fit(o_, X.handle(), &lossOld, &regOld);  // :419-457
    if (rc == NFM_ERR_UNSUPPORTED && refitFully) throw std::invalid_argument(nfm_last_error());
    check(rc);
    const int64_t d = X.nFeatures();
    bool isConverged = false;
    history.clear();
    double rec[NFM_GCD_REC_COUNT];
    const int width = (int)std::to_string(maxIterInner).size();
    for (int it = 0; it < maxIter; ++it) {
      if (verbose > 0) std::printf("Outer Iteration %d\n", it + 1);
      check(nfm_gcd_outer_begin(o_, X.handle(), rec));  // :464-469 and fitZ's head :332-336
      int nc = (int)rec[NFM_GCD_REC_N_COMPONENTS];
      double objOld = rec[NFM_GCD_REC_OBJECTIVE];
      Outer outer{0.0, 0.0, objOld, nc, {}};
      for (int itIn = 0; itIn < maxIterInner; ++itIn) {  // fitZ, :347-412
        std::vector<double> start;
        if (nc < cfm.maxComponents) {
          if (powerInit) {
            start = powerInit(d);
          } else {
            start = globalRand().rand(d, 1.0);
            for (auto& v : start) v = 2 * v - 1.0;
          }
          if ((int64_t)start.size() != d) throw std::invalid_argument("powerInit must return nFeatures values");
        }
        const bool refit = (itIn + 1) % nRefitting == 0;
        check(nfm_gcd_inner(o_, X.handle(), start.empty() ? nullptr : start.data(), refit, rec));
        Inner r{itIn, rec[NFM_GCD_REC_ADDED] != 0.0, (int)rec[NFM_GCD_REC_SLOT], rec[NFM_GCD_REC_LAM], (int64_t)rec[NFM_GCD_REC_POWER_ITERS],
                rec[NFM_GCD_REC_EVAL], (int)rec[NFM_GCD_REC_N_COMPONENTS], rec[NFM_GCD_REC_OBJECTIVE], (int)rec[NFM_GCD_REC_N_STORED], refit, false};
        nc = r.nComponents;
        r.checked = r.added || refit || itIn == maxIterInner - 1;  // :392
        outer.inner.push_back(r);
        if (r.checked) {
          if (verbose > 1)
            std::printf("   Iteration: %*d   Objective: %1.4e   Decreasing: %1.4e\n", width, itIn + 1, r.objective, objOld - r.objective);
          if (std::fabs(r.objective - objOld) < tol) {
            if (verbose > 1) std::printf("   Converged at iteration %d.\n", itIn + 1);
            break;
          }
          objOld = r.objective;
        }
      }
      // :474-476; yPred is rebuilt (:493-497) when another outer iteration may follow: nothing reads it before that
      check(nfm_gcd_outer_end(o_, X.handle(), it < maxIter - 1, &outer.loss, &outer.reg));
      outer.nComponents = nc;
      history.push_back(outer);
      if (callback) {  // :478-479
        cfm.pull();
        callback(*this, cfm);
      }
      if (verbose > 0) std::printf("   Loss: %1.4e   Reg: %1.4e\n", outer.loss, outer.reg);
      if (std::fabs(outer.loss + outer.reg - lossOld - regOld) < tol) {
        if (verbose > 0) std::printf("Converged at iteration %d.\n", it + 1);
        isConverged = true;
        break;
      }
      lossOld = outer.loss;
      regOld = outer.reg;
    }
    if (!isConverged && verbose > 0) std::printf("Objective did not converge. Increase maxIter.\n");
    cfm.pull();
  }
  nfm_opt* handle() const { return o_; }

 private:
  nfm_opt* o_ = nullptr;
};

}  // namespace nimfm
