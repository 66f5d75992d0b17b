// tests/cpp/katyusha_host_test.cpp -- Katyusha<L, R> of nimfm_amd/host/nimfm.hpp (optimizer/katyusha.nim): fit is
// nfm_katyusha_create, nfm_katyusha_begin_fit and one nfm_opt_epoch per outer iteration over the same index stream, bit for
// bit from the same starting model; the callback runs once per outer iteration; what is refused throws.
// Built by tests/test_cpp_katyusha.py; needs a GPU to run.
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
  const int64_t n = 120, d = 30, m = 4, B = 32;  // four inner iterations, 128 positions per epoch: the stream wraps
  const int k = 3, iters = 3;
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

  // the host class (shuffle = false: the identity stream with wrap-around) against the C ABI driven by hand (perm == NULL)
  auto same = [&](auto& opt, int32_t reg, int32_t transpose, double tau1, double tau2) {
    FactorizationMachine a(regression, 2, k), b(regression, 2, k);
    int calls = 0;
    opt.fit(X, y, a, [&](auto&, FactorizationMachine&) { ++calls; });
    b.init(X);
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    nfm_opt* o = nullptr;
    check(nfm_katyusha_create(b.push(), 0.1, 1e-6, 1e-3, 1e-4, 1e-2, tau1, tau2, NFM_LOSS_SQUARED, 1.0, reg, transpose, B, &o));
    check(nfm_katyusha_begin_fit(o, X.handle()));
    const int64_t need = B * ((n - 1) / B + 1);
    std::vector<std::pair<double, double>> hist;
    for (int t = 0; t < iters; ++t) {
      double ls = 0.0, viol = 0.0;
      check(nfm_opt_epoch(o, X.handle(), nullptr, (int64_t)t * need, (int64_t)(t + 1) * need, &ls, &viol));
      hist.emplace_back(viol, ls / (double)n);
    }
    b.pull();
    nfm_opt_destroy(o);
    CHECK(calls == iters && opt.history.size() == (size_t)iters && opt.history == hist);
    CHECK(a.P == b.P && a.w == b.w && a.intercept == b.intercept);
  };
  Katyusha<Squared, L1> k1(iters, 0.1, 1e-6, 1e-3, 1e-4, 1e-2, Squared(), L1(), B, 0.5, -1.0, 0, 0.0, false);
  same(k1, NFM_REG_L1, 0, 0.5, -1.0);
  Katyusha<Squared, SquaredL12> k12(iters, 0.1, 1e-6, 1e-3, 1e-4, 1e-2, Squared(), SquaredL12(), B, -1.0, 0.2, 1, 0.0, false);  // verbose lines
  same(k12, NFM_REG_SQUAREDL12, 1, -1.0, 0.2);
  Katyusha<Squared, SquaredL21> k21(iters, 0.1, 1e-6, 1e-3, 1e-4, 1e-2, Squared(), SquaredL21(), B, 0.5, -1.0, 0, 0.0, false);
  same(k21, NFM_REG_SQUAREDL21, 0, 0.5, -1.0);
  {  // defaults of the reference's constructor
    Katyusha<> q;
    CHECK(q.maxIter == 100 && q.eta == 0.1 && q.alpha0 == 1e-6 && q.alpha == 1e-3 && q.beta == 1e-4 && q.gamma == 1e-4);
    CHECK(q.miniBatchSize == -1 && q.tau1 == 0.5 && q.tau2 == -1.0 && q.tol == 1e-6 && q.shuffle && q.nCalls == -1 && q.reg.transpose);
  }
  {  // refusals
    FactorizationMachine fm(regression, 2, k), cubic(regression, 3, k);
    Katyusha<Squared, SquaredL12> sq12(iters);
    CHECK(refuses(sq12, X, y, cubic));
    Katyusha<Squared, OmegaTI> ti;
    CHECK(refuses(ti, X, y, fm));
    Katyusha<Squared, L1> calls(iters, 0.1, 1e-6, 1e-3, 1e-4, 1e-4, Squared(), L1(), -1, 0.5, -1.0, 0, 1e-6, true, 5);
    CHECK(refuses(calls, X, y, fm));
    Katyusha<Squared, L1> beta0(iters, 0.1, 1e-6, 1e-3, 0.0);
    CHECK(refuses(beta0, X, y, fm));
    Katyusha<Squared, L1> alpha0(iters, 0.1, 1e-6, 0.0);
    CHECK(refuses(alpha0, X, y, fm));
    Katyusha<Squared, L1> icpt0(iters, 0.1, 0.0);
    CHECK(refuses(icpt0, X, y, fm));
    Katyusha<Squared, L1> eta0(iters, 0.0);
    CHECK(refuses(eta0, X, y, fm));
  }
  if (failures == 0) std::printf("katyusha host ok\n");
  return failures == 0 ? 0 : 1;
}
