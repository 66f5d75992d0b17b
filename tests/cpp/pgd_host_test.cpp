// tests/cpp/pgd_host_test.cpp -- PGD<L, R>, FISTA<L, R> and NMAPGD<L, R> of nimfm_amd/host/nimfm.hpp (optimizer/pgd.nim,
// fista.nim, nmapgd.nim): fit is nfm_pgd_create, nfm_pgd_begin_fit and one nfm_opt_epoch per iteration, bit for bit from the
// same starting model; the callback runs once per iteration; what the reference refuses throws before any device work.
// Built by tests/test_cpp_pgd.py; needs a GPU to run.
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
  const int k = 3, iters = 4;
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

  // the host class against the C ABI driven by hand
  auto same = [&](auto& opt, int32_t algo, int32_t reg, int32_t transpose, double sigma) {
    FactorizationMachine a(regression, 2, k), b(regression, 2, k);
    int calls = 0;
    opt.fit(X, y, a, [&](auto&, FactorizationMachine&) { ++calls; });
    b.init(X);
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    nfm_opt* o = nullptr;
    check(nfm_pgd_create(b.push(), algo, 1e-6, 1e-3, 1e-4, 1e-3, 0.5, sigma, 0.5, NFM_LOSS_SQUARED, 1.0, reg, transpose, -1, &o));
    check(nfm_pgd_begin_fit(o, X.handle(), 0));
    std::vector<std::pair<double, double>> hist;
    bool recs = opt.iterations.size() == (size_t)iters;
    for (int t = 0; t < iters; ++t) {
      double ls = 0.0, viol = 0.0, r[NFM_PGD_IT_COUNT];
      check(nfm_opt_epoch(o, X.handle(), nullptr, 0, n, &ls, &viol));
      check(nfm_pgd_last_iter(o, r));
      hist.emplace_back(r[NFM_PGD_IT_VIOL], r[NFM_PGD_IT_LOSS]);
      if (recs) {
        const auto& q = opt.iterations[t];
        recs = q.trials[0] == (int)r[NFM_PGD_IT_TRIALS] && q.trials[1] == (int)r[NFM_PGD_IT_TRIALS_V] && q.branch == (int)r[NFM_PGD_IT_BRANCH] &&
               q.eta[0] == r[NFM_PGD_IT_ETA] && q.start[0] == r[NFM_PGD_IT_START] && q.regVal == r[NFM_PGD_IT_REG] && q.t == r[NFM_PGD_IT_T] &&
               q.c == r[NFM_PGD_IT_C] && viol == r[NFM_PGD_IT_VIOL] && ls == r[NFM_PGD_IT_LOSS] * (double)n;
      }
    }
    b.pull();
    nfm_opt_destroy(o);
    CHECK(recs);
    CHECK(calls == iters && opt.history.size() == (size_t)iters && opt.history == hist);
    CHECK(a.P == b.P && a.w == b.w && a.intercept == b.intercept);
  };
  PGD<Squared, L1> pgd(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L1(), 0.5, 1.0, -1, 0, 0.0);
  same(pgd, NFM_PGD_ALGO_PGD, NFM_REG_L1, 0, 1.0);
  FISTA<Squared, L21> fista(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L21(), 0.5, 1.0, -1, 0, 0.0);
  same(fista, NFM_PGD_ALGO_FISTA, NFM_REG_L21, 0, 1.0);
  NMAPGD<Squared, SquaredL12> nm(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), SquaredL12(), 0.5, 0.01, -1, 0.5, 0, 0.0);  // the default R
  same(nm, NFM_PGD_ALGO_NMAPGD, NFM_REG_SQUAREDL12, 1, 0.01);
  NMAPGD<Squared, SquaredL21> nm21(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), SquaredL21(), 0.5, 0.01, -1, 0.5, 0, 0.0);
  same(nm21, NFM_PGD_ALGO_NMAPGD, NFM_REG_SQUAREDL21, 0, 0.01);
  {  // defaults of the reference's constructors
    PGD<> p;
    FISTA<> f;
    NMAPGD<> q;
    CHECK(p.sigma == 1.0 && p.tol == 1e-6 && p.maxSearch == -1 && p.rho == 0.5 && p.reg.transpose);
    CHECK(f.sigma == 1.0 && f.tol == 1e-6);
    CHECK(q.sigma == 0.01 && q.tol == 1e-5 && q.eta == 0.5);
  }
  {  // a warm-started model keeps t on the optimizer
    FactorizationMachine w(regression, 2, k, explicit_, true, true, true);
    FISTA<Squared, L1> one(1, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L1(), 0.5, 1.0, -1, 0, 0.0);
    one.fit(X, y, w);
    const double t1 = one.iterations.back().t;
    one.fit(X, y, w);
    CHECK(t1 == 1.0 && one.iterations.back().t > t1);
  }
  {  // refusals
    FactorizationMachine fm(regression, 2, k), cubic(regression, 3, k);
    PGD<Squared, SquaredL12> sq12(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), SquaredL12(), 0.5, 1.0, -1, 0, 0.0);
    CHECK(refuses(sq12, X, y, cubic));
    FISTA<Squared, SquaredL21> sq21(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), SquaredL21(), 0.5, 1.0, -1, 0, 0.0);
    CHECK(refuses(sq21, X, y, cubic));
    NMAPGD<Squared, OmegaTI> ti;
    CHECK(refuses(ti, X, y, fm));
    PGD<Squared, L1> rho(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L1(), 1.0, 1.0, -1, 0, 0.0);  // rho outside (0, 1): NFM_ERR_INVALID
    CHECK(refuses(rho, X, y, fm));
  }
  if (failures == 0) std::printf("pgd host ok\n");
  return failures == 0 ? 0 : 1;
}
