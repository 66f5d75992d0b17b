// tests/cpp/gcd_host_test.cpp -- GreedyCD of nimfm_amd/host/nimfm.hpp (optimizer/greedy_cd.nim at refitFully = false): fit is
// nfm_gcd_create, nfm_gcd_begin_fit and per outer iteration nfm_gcd_outer_begin, the nfm_gcd_inner calls and nfm_gcd_outer_end
// with the same start vectors, bit for bit; the start vector is drawn only while a base is added; the callback runs once per
// outer iteration; what is refused throws.
// Built by tests/test_cpp_gcd.py; needs a GPU to run.
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
  const int maxc = 3, iters = 3, inner = 4, nrefit = 2;
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

  for (int ignoreDiag = 0; ignoreDiag < 2; ++ignoreDiag) {
    // the host class after randomize(1) against the C ABI driven by hand with the same draws
    ConvexFactorizationMachine a(regression, maxc, true, true, ignoreDiag != 0), b(regression, maxc, true, true, ignoreDiag != 0);
    GreedyCD<Squared> opt(iters, 1e-6, 1e-3, 1e-5, Squared{}, inner, nrefit, false, 0, 0.0, 50, 0.0);
    int calls = 0;
    globalRand().randomize(1);
    opt.fit(X, y, a, [&](GreedyCD<Squared>&, ConvexFactorizationMachine& m_) { ++calls; CHECK(m_.nComponents() >= 1); });
    b.init(X);
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    nfm_opt* o = nullptr;
    check(nfm_gcd_create(b.push(), 1e-6, 1e-3, 1e-5, NFM_LOSS_SQUARED, 1.0, 50, 0.0, 0, &o));
    double loss0 = 0.0, reg0 = 0.0;
    check(nfm_gcd_begin_fit(o, X.handle(), &loss0, &reg0));
    CHECK(loss0 > 0.0 && reg0 == 0.0);
    NimRand r;
    r.randomize(1);
    int draws = 0;
    double rec[NFM_GCD_REC_COUNT];
    for (int t = 0; t < iters; ++t) {
      check(nfm_gcd_outer_begin(o, X.handle(), rec));
      int nc = (int)rec[NFM_GCD_REC_N_COMPONENTS];
      CHECK(t < (int)opt.history.size() && rec[NFM_GCD_REC_OBJECTIVE] == opt.history[t].objOld);
      for (int s = 0; s < inner; ++s) {
        std::vector<double> start;
        if (nc < maxc) {
          start = r.rand(d, 1.0);
          for (auto& v : start) v = 2 * v - 1.0;
          ++draws;
        }
        check(nfm_gcd_inner(o, X.handle(), start.empty() ? nullptr : start.data(), (s + 1) % nrefit == 0, rec));
        nc = (int)rec[NFM_GCD_REC_N_COMPONENTS];
        const auto& h = opt.history[t].inner[s];
        CHECK(rec[NFM_GCD_REC_OBJECTIVE] == h.objective && (int)rec[NFM_GCD_REC_SLOT] == h.slot && rec[NFM_GCD_REC_LAM] == h.lam);
        CHECK((rec[NFM_GCD_REC_ADDED] != 0.0) == h.added && nc == h.nComponents && (int)rec[NFM_GCD_REC_N_STORED] == h.nStored);
        CHECK(h.refit == ((s + 1) % nrefit == 0) && h.checked == (h.added || h.refit || s == inner - 1));
      }
      double lo = 0.0, re = 0.0;
      check(nfm_gcd_outer_end(o, X.handle(), t < iters - 1, &lo, &re));
      CHECK(lo == opt.history[t].loss && re == opt.history[t].reg && (int)opt.history[t].inner.size() == inner);
    }
    b.pull();
    // the calls of an outer iteration come in order; a start vector is due exactly while a base is added
    CHECK(nfm_gcd_inner(o, X.handle(), nullptr, 0, rec) == NFM_ERR_INVALID);
    nfm_opt_destroy(o);
    CHECK((int)opt.history.size() == iters && calls == iters && draws == maxc);  // the basis filled up: no draw after that
    CHECK(a.P == b.P && a.lams == b.lams && a.w == b.w && a.intercept == b.intercept);
    CHECK(a.nComponents() == maxc && (int64_t)a.P.size() == maxc * d);
    CHECK(a.decisionFunction(X) == b.decisionFunction(X));
    CHECK(opt.history.back().loss < loss0);
    // the rmse of the fitted model against the last outer objective (sum 0.5 r^2 / n), recomputed from the parameters
    CHECK(std::fabs(a.score(X, y) - std::sqrt(2.0 * opt.history.back().loss)) < 1e-9);
  }

  // a second loss through the template, as classification
  {
    std::vector<double> yc(n);
    for (int64_t i = 0; i < n; ++i) yc[i] = y[i] > 0 ? 1.0 : -1.0;
    ConvexFactorizationMachine c(classification, maxc);
    GreedyCD<Logistic> opt(2, 1e-6, 1e-3, 1e-5, Logistic{}, inner, nrefit, false, 0, 0.0, 50, 0.0);
    globalRand().randomize(1);
    opt.fit(X, yc, c);
    CHECK(opt.history.size() == 2 && opt.history[1].loss < opt.history[0].loss && c.nComponents() == maxc);
  }

  // refusals
  {
    bool threw = false;
    ConvexFactorizationMachine c(regression, 2);
    try {
      GreedyCD<Squared> full(1, 1e-6, 1e-3, 1e-5, Squared{}, 10, 10, true, 0);
      full.fit(X, y, c);
    } catch (const std::invalid_argument& e) {
      threw = std::string(e.what()).find("dsyev") != std::string::npos;
    }
    CHECK(threw);
    threw = false;
    try { GreedyCD<Squared> bad(1, 1e-6, 1e-3, 1e-5, Squared{}, 10, 0); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    FactorizationMachine fm(regression, 2, 2);
    fm.init(X);
    nfm_opt* o = nullptr;
    CHECK(nfm_gcd_create(fm.push(), 1e-6, 1e-3, 1e-5, NFM_LOSS_SQUARED, 1.0, 10, 1e-7, 0, &o) == NFM_ERR_UNSUPPORTED);
    c.init(X);
    check(nfm_gcd_create(c.push(), 1e-6, 1e-3, 1e-5, NFM_LOSS_SQUARED, 1.0, 10, 1e-7, 0, &o));
    double ls = 0.0, vs = 0.0, rec[NFM_GCD_REC_COUNT];
    CHECK(nfm_opt_epoch(o, X.handle(), nullptr, 0, n, &ls, &vs) == NFM_ERR_INVALID);
    CHECK(nfm_gcd_outer_begin(o, X.handle(), rec) == NFM_ERR_INVALID);  // before begin_fit
    nfm_opt_destroy(o);
  }
  if (failures) return 1;
  std::printf("gcd host ok\n");
  return 0;
}
