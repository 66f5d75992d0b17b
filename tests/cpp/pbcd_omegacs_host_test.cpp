// tests/cpp/pbcd_omegacs_host_test.cpp -- PBCD<L, OmegaCS> of nimfm_amd/host/nimfm.hpp (optimizer/pbcd.nim at maxSearch = 0
// with regularizer/omegacs.nim's BCD hooks): at degrees 2 and 3 fit is nfm_pbcd_create, nfm_cd_begin_fit and one nfm_opt_epoch
// per iteration, bit for bit from the same starting model; the solvers without a step for OmegaCS throw before any device
// work; regEval's values are printed for tests/test_cpp_pbcd_omegacs.py to hold against the Python host's eval.
// Built by tests/test_cpp_pbcd_omegacs.py; needs a GPU to run.
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

template <class Opt>
static bool refuses(Opt& opt, const CSRDataset& X, const std::vector<double>& y, FactorizationMachine& fm) {
  try {
    opt.fit(X, y, fm);
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

int main() {
  const int64_t n = 120, d = 30, m = 4;
  const int k = 3, iters = 3;
  const double gamma = 1e-3;
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::vector<int64_t> indptr(n + 1), indices;
  std::vector<double> data, y(n);
  for (int64_t i = 0; i < n; ++i) {
    indptr[i] = (int64_t)indices.size();
    for (int64_t t = 0; t < m; ++t) {  // distinct, ascending column ids
      indices.push_back((i * 7 + t * (d / m) + (int64_t)(rng() % (uint64_t)(d / m))) % (d / m) + t * (d / m));
      data.push_back(U(rng));
    }
    y[i] = U(rng);
  }
  indptr[n] = (int64_t)indices.size();
  CSRDataset X(data, indices, indptr, n, d);

  for (int degree = 2; degree <= 3; ++degree) {
    PBCD<Squared, OmegaCS> opt(iters, 1e-6, 1e-3, 1e-4, gamma, Squared(), OmegaCS(), 0, 0.0);
    FactorizationMachine a(regression, degree, k), b(regression, degree, k);
    int calls = 0;
    opt.fit(X, y, a, [&](auto&, FactorizationMachine&) { ++calls; });
    b.init(X);
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    nfm_opt* o = nullptr;
    check(nfm_pbcd_create(b.push(), 1e-6, 1e-3, 1e-4, gamma, NFM_LOSS_SQUARED, 1.0, NFM_REG_OMEGACS, 0, &o));
    check(nfm_cd_begin_fit(o, X.handle()));
    std::vector<std::pair<double, double>> hist;
    for (int t = 0; t < iters; ++t) {
      double ls = 0.0, viol = 0.0;
      check(nfm_opt_epoch(o, X.handle(), nullptr, 0, n, &ls, &viol));
      hist.emplace_back(viol, ls / (double)n);
    }
    b.pull();
    nfm_opt_destroy(o);
    CHECK(calls == iters && opt.history.size() == (size_t)iters && opt.history == hist);
    CHECK(a.P == b.P && a.w == b.w && a.intercept == b.intercept);
    bool moved = false;
    FactorizationMachine c(regression, degree, k);
    c.init(X);
    for (size_t t = 0; t < a.P.size(); ++t) moved = moved || a.P[t] != c.P[t];
    CHECK(moved);
  }
  {  // the verbose line's regularisation rests on regEval: the ANOVA polynomial of the row norms
    const double P34[4] = {3.0, 0.0, 4.0, 2.0};  // [k = 2][da = 2]: rows (3, 4) and (0, 2), norms 5 and 2
    CHECK(regEval(OmegaCS(), P34, 2, 2, 1) == 7.0 && regEval(OmegaCS(), P34, 2, 2, 2) == 10.0);
    double Po[15];  // [k = 3][da = 5]; tests/test_cpp_pbcd_omegacs.py builds the same values
    for (int t = 0; t < 15; ++t) Po[t] = ((t * 7) % 11 - 5) / 8.0;
    for (int degree = 1; degree <= 4; ++degree) std::printf("regeval %d %.17g\n", degree, regEval(OmegaCS(), Po, 3, 5, degree));
  }
  {  // refusals: OmegaCS has BCD hooks only
    FactorizationMachine fm(regression, 2, k);
    PGD<Squared, OmegaCS> pgd;
    CHECK(refuses(pgd, X, y, fm));
    FISTA<Squared, OmegaCS> fista;
    CHECK(refuses(fista, X, y, fm));
    NMAPGD<Squared, OmegaCS> nmapgd;
    CHECK(refuses(nmapgd, X, y, fm));
    Katyusha<Squared, OmegaCS> kat;
    CHECK(refuses(kat, X, y, fm));
    PBCD<Squared, OmegaCS> search(iters, 1e-6, 1e-3, 1e-4, gamma, Squared(), OmegaCS(), 0, 0.0, 0.01, 0.5, 2);
    CHECK(refuses(search, X, y, fm));
  }
  if (failures == 0) std::printf("pbcd omegacs host ok\n");
  return failures == 0 ? 0 : 1;
}
