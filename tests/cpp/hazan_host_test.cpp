// tests/cpp/hazan_host_test.cpp -- ConvexFactorizationMachine and Hazan of nimfm_amd/host/nimfm.hpp (optimizer/hazan.nim): fit is
// nfm_hazan_create, nfm_hazan_begin_fit and one nfm_hazan_iter per outer iteration with the same start vectors, bit for bit;
// the callback runs once per outer iteration; decisionFunction is the C ABI's; what is refused throws.
// Built by tests/test_cpp_hazan.py; needs a GPU to run.
#include <cstdio>
#include <random>

#include "../../nimfm_amd/host/nimfm.hpp"

using namespace nimfm;

static int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                               \
    }                                                           \
  } while (0)

int main() {
  const int64_t n = 90, d = 12, m = 4;
  const int maxc = 3, iters = 5;
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::vector<int64_t> indptr(n + 1), indices;
  std::vector<double> data, y(n);
  for (int64_t i = 0; i < n; ++i) {
    indptr[i] = (int64_t)indices.size();
    for (int64_t t = 0; t < m; ++t) {  // distinct, ascending column ids
      indices.push_back((i + t) % (d / m) + t * (d / m));
      data.push_back(U(rng));
    }
    y[i] = U(rng);
  }
  indptr[n] = (int64_t)indices.size();
  CSRDataset X(data, indices, indptr, n, d);

  for (int optimal = 0; optimal < 2; ++optimal)
    for (int ignoreDiag = 0; ignoreDiag < 2; ++ignoreDiag) {
      // the host class after randomize(1) against the C ABI driven by hand with the same draws
      ConvexFactorizationMachine a(regression, maxc, true, true, ignoreDiag != 0), b(regression, maxc, true, true, ignoreDiag != 0);
      Hazan opt(iters, 2.0, 0, -100.0, 10, 50, 0.0, optimal != 0);
      int calls = 0;
      globalRand().randomize(1);
      opt.fit(X, y, a, [&](Hazan&, ConvexFactorizationMachine& m_) { ++calls; CHECK(m_.nComponents() >= 1); });
      b.init(X);
      check(nfm_dataset_set_targets(X.handle(), y.data()));
      nfm_opt* o = nullptr;
      check(nfm_hazan_create(b.push(), 2.0, 50, 0.0, optimal, &o));
      double loss0 = 0.0;
      check(nfm_hazan_begin_fit(o, X.handle(), &loss0));
      NimRand r;
      r.randomize(1);
      size_t done = 0;
      int nc = 0;
      for (int t = 0; t < iters; ++t) {
        if (!optimal && nc >= maxc) break;
        std::vector<double> start = r.rand(d, 1.0);
        for (auto& v : start) v = 2 * v - 1.0;
        double rec[NFM_HAZAN_REC_COUNT];
        check(nfm_hazan_iter(o, X.handle(), t, start.data(), rec));
        CHECK(done < opt.history.size() && rec[NFM_HAZAN_REC_LOSS] == opt.history[done].loss && rec[NFM_HAZAN_REC_STEP] == opt.history[done].step);
        CHECK(done < opt.history.size() && (int)rec[NFM_HAZAN_REC_SLOT] == opt.history[done].slot);
        nc = (int)rec[NFM_HAZAN_REC_N_COMPONENTS];
        ++done;
      }
      b.pull();
      nfm_opt_destroy(o);
      CHECK(done == opt.history.size() && calls == (int)done);
      CHECK(optimal ? (int)done == iters : (int)done == maxc);  // optimal = false breaks once the basis is full
      CHECK(opt.it == (int64_t)done);
      CHECK(a.P == b.P && a.lams == b.lams && a.w == b.w && a.intercept == b.intercept);
      CHECK(a.nComponents() == maxc && (int64_t)a.P.size() == maxc * d);
      CHECK(a.decisionFunction(X) == b.decisionFunction(X));
      // the rmse of the fitted model is the last record's loss (||residual||^2 / n), recomputed from the parameters
      CHECK(loss0 > 0.0 && std::fabs(a.score(X, y) - std::sqrt(opt.history.back().loss)) < 1e-9 * std::sqrt(opt.history.back().loss));
    }

  // refusals
  {
    bool threw = false;
    try { ConvexFactorizationMachine bad(regression, 0); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    FactorizationMachine fm(regression, 2, 2);
    fm.init(X);
    nfm_opt* o = nullptr;
    CHECK(nfm_hazan_create(fm.push(), 1000.0, 10, 1e-7, 1, &o) == NFM_ERR_UNSUPPORTED);
    ConvexFactorizationMachine c(regression, 2);
    c.init(X);
    CHECK(nfm_cd_create(c.push(), 1e-6, 1e-3, 1e-3, NFM_LOSS_SQUARED, 1.0, &o) == NFM_ERR_UNSUPPORTED);
    nfm_sgd_cfg sc{0.01, 1e-6, 1e-3, 1e-3, 1.0, 1.0, NFM_LOSS_SQUARED, NFM_SCHED_OPTIMAL, NFM_MODE_SEQUENTIAL, 0, 1};
    CHECK(nfm_sgd_create(c.push(), &sc, &o) == NFM_ERR_UNSUPPORTED);
    ConvexFactorizationMachine unfitted(regression, 2);
    threw = false;
    try { unfitted.decisionFunction(X); } catch (const NotFittedError&) { threw = true; }
    CHECK(threw);
  }
  if (failures) return 1;
  std::printf("hazan host ok\n");
  return 0;
}
