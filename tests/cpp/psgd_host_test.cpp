// tests/cpp/psgd_host_test.cpp -- PSGD of nimfm_amd/host/nimfm.hpp (optimizer/psgd.nim with L1 / L21): fit is nfm_psgd_create,
// nfm_psgd_begin_fit, one nfm_opt_epoch per epoch (or per nCalls piece, with nfm_psgd_finalize before every callback) and
// nfm_psgd_finalize, bit for bit; `it` persists between warm-started fits; what is refused throws.
// Built by tests/test_cpp_psgd.py; needs a GPU to run.
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

template <class R>
static void against_the_abi(const CSRDataset& X, const std::vector<double>& y, int degree, int nCalls) {
  const int64_t n = X.nSamples();
  const int epochs = 3;
  FactorizationMachine a(regression, degree, 5, explicit_, true, true, true), b(regression, degree, 5, explicit_, true, true, true);
  PSGD<Squared, R> opt(epochs, 0.05, 1e-6, 1e-3, 1e-4, 1e-3, Squared{}, R{}, optimal, 1.0, 0, 0.0, false, nCalls);
  int calls = 0;
  std::vector<int64_t> its;
  if (nCalls != 0)
    opt.fit(X, y, a, [&](PSGD<Squared, R>& o, FactorizationMachine&) { ++calls; its.push_back(o.it); });
  else
    opt.fit(X, y, a);
  b.init(X);
  check(nfm_dataset_set_targets(X.handle(), y.data()));
  nfm_opt* o = nullptr;
  nfm_mbpsgd_cfg c{0.05, 1e-6, 1e-3, 1e-4, 1e-3, 1.0, 1.0, NFM_LOSS_SQUARED, NFM_SCHED_OPTIMAL, R::id, 0, 1};
  check(nfm_psgd_create(b.push(), &c, &o));
  check(nfm_psgd_begin_fit(o, X.handle()));
  int64_t it = 1;
  int want_calls = 0;
  for (int e = 0; e < epochs; ++e) {
    double sum = 0.0;
    if (nCalls > 0) {
      int64_t pos = 0;
      while (pos < n) {
        const int64_t end = std::min(n, pos + (nCalls - it % nCalls) % nCalls + 1);
        double ls = 0.0, vs = 1.0;
        check(nfm_opt_epoch(o, X.handle(), nullptr, pos, end, &ls, &vs));
        CHECK(vs == 0.0);
        sum += ls;
        it += end - pos;
        pos = end;
        if ((it - 1) % nCalls == 0) {
          check(nfm_psgd_finalize(o));
          CHECK(want_calls < (int)its.size() && its[want_calls] == it - 1);
          ++want_calls;
        }
      }
    } else {
      double vs = 1.0;
      check(nfm_opt_epoch(o, X.handle(), nullptr, 0, n, &sum, &vs));
      CHECK(vs == 0.0);
      it += n;
      if (nCalls < 0) {
        check(nfm_psgd_finalize(o));
        ++want_calls;
      }
    }
    CHECK(e < (int)opt.lossSums.size() && opt.lossSums[e] == sum);
  }
  check(nfm_psgd_finalize(o));
  b.pull();
  int64_t it_lib = 0;
  check(nfm_opt_get_it(o, &it_lib));
  CHECK(it_lib == it && opt.it == it && it == 1 + epochs * n);
  CHECK(nCalls == 0 || calls == want_calls);
  CHECK(a.P == b.P && a.w == b.w && a.intercept == b.intercept);
  CHECK(a.decisionFunction(X) == b.decisionFunction(X));
  bool any = false, finite = true;
  for (double v : a.P) { any = any || v != 0.0; finite = finite && std::isfinite(v); }
  CHECK(any && finite);
  // a warm-started fit goes on counting; the caches start afresh (begin_fit), so it equals the by-hand continuation
  opt.fit(X, y, a);
  CHECK(opt.it == 1 + 2 * epochs * n);
  nfm_opt_destroy(o);
}

template <class Opt>
static bool refuses(Opt& opt, const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& fm, const char* needle) {
  try {
    opt.fit(X, y, fm);
  } catch (const std::invalid_argument& e) {
    return std::string(e.what()).find(needle) != std::string::npos;
  }
  return false;
}

int main() {
  const int64_t n = 70, d = 12, m = 4;
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

  against_the_abi<L1>(X, y, 2, 0);    // no callback
  against_the_abi<L21>(X, y, 3, -1);  // a callback per epoch
  against_the_abi<L1>(X, y, 3, 25);   // a callback whenever it mod 25 == 0
  against_the_abi<L21>(X, y, 2, 25);

  // refusals: the template's default regulariser is the reference's, SquaredL12
  {
    FactorizationMachine fm(regression, 2, 3);
    PSGD<> dflt(1);
    CHECK(refuses(dflt, X, y, fm, "MBPSGD"));
    PSGD<Squared, SquaredL21> s21(1);
    CHECK(refuses(s21, X, y, fm, "MBPSGD"));
    PSGD<Squared, OmegaTI> ti(1);
    CHECK(refuses(ti, X, y, fm, "no SGD hooks"));
    PSGD<Squared, OmegaCS> cs(1);
    CHECK(refuses(cs, X, y, fm, "no SGD hooks"));
    FactorizationMachine wide(regression, 2, 129);
    PSGD<Squared, L1> l1(1, 0.01, 1e-6, 1e-3, 1e-4, 1e-4, Squared{}, L1{}, optimal, 1.0, 0);
    CHECK(refuses(l1, X, y, wide, "nComponents <= 128"));
    // the C ABI's own refusals
    fm.init(X);
    nfm_opt* o = nullptr;
    nfm_mbpsgd_cfg c{0.01, 1e-6, 1e-3, 1e-4, 1e-4, 1.0, 1.0, NFM_LOSS_SQUARED, NFM_SCHED_OPTIMAL, NFM_REG_SQUAREDL12, 1, 1};
    CHECK(nfm_psgd_create(fm.push(), &c, &o) == NFM_ERR_UNSUPPORTED && std::string(nfm_last_error()).find("newMBPSGD") != std::string::npos);
    c.reg = NFM_REG_OMEGACS;
    CHECK(nfm_psgd_create(fm.push(), &c, &o) == NFM_ERR_UNSUPPORTED);
    wide.init(X);
    c.reg = NFM_REG_L1;
    CHECK(nfm_psgd_create(wide.push(), &c, &o) == NFM_ERR_UNSUPPORTED);
    check(nfm_psgd_create(fm.push(), &c, &o));
    double ls = 0.0, vs = 0.0;
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    CHECK(nfm_opt_epoch(o, X.handle(), nullptr, 0, n, &ls, &vs) == NFM_ERR_INVALID);  // before begin_fit
    CHECK(nfm_psgd_finalize(o) == NFM_ERR_INVALID);
    nfm_opt_destroy(o);
  }
  if (failures) return 1;
  std::printf("psgd host ok\n");
  return 0;
}
