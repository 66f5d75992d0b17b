// tests/cpp/pbcd_host_test.cpp -- PBCD<L, R> of nimfm_amd/host/nimfm.hpp (optimizer/pbcd.nim at maxSearch = 0): fit is
// nfm_pbcd_create, nfm_cd_begin_fit and one nfm_opt_epoch per iteration, bit for bit from the same starting model; the
// callback runs once per iteration; what the reference refuses (and the line search, and shuffling) throws before any
// device work.  Built by tests/test_cpp_pbcd.py; needs a GPU to run.
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

  auto same = [&](auto& opt, int32_t reg) {
    FactorizationMachine a(regression, 2, k), b(regression, 2, k);
    int calls = 0;
    opt.fit(X, y, a, [&](auto&, FactorizationMachine&) { ++calls; });
    b.init(X);
    check(nfm_dataset_set_targets(X.handle(), y.data()));
    nfm_opt* o = nullptr;
    check(nfm_pbcd_create(b.push(), 1e-6, 1e-3, 1e-4, 1e-3, NFM_LOSS_SQUARED, 1.0, reg, 0, &o));
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
  };
  PBCD<Squared, L1> l1(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L1(), 0, 0.0);
  same(l1, NFM_REG_L1);
  PBCD<Squared, L21> l21(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L21(), 0, 0.0);
  same(l21, NFM_REG_L21);
  PBCD<Squared, SquaredL21> sq(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), SquaredL21(), 0, 0.0);  // the default R
  same(sq, NFM_REG_SQUAREDL21);
  {  // the verbose line's regularisation rests on regEval: row norms summed (L21), that sum squared (SquaredL21)
    const double Po[4] = {3.0, 0.0, 4.0, 2.0};  // [k = 2][da = 2]: rows (3, 4) and (0, 2)
    CHECK(regEval(L21(), Po, 2, 2, 2) == 7.0 && regEval(SquaredL21(), Po, 2, 2, 2) == 49.0);
  }
  {  // refusals
    FactorizationMachine fm(regression, 2, k), cubic(regression, 3, k);
    PBCD<Squared, SquaredL12> sq12;
    CHECK(refuses(sq12, X, y, fm));
    SquaredL21 tr;
    tr.transpose = true;
    PBCD<Squared, SquaredL21> trp(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), tr, 0, 0.0);
    CHECK(refuses(trp, X, y, fm));
    PBCD<Squared, SquaredL21> deg3(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), SquaredL21(), 0, 0.0);
    CHECK(refuses(deg3, X, y, cubic));
    PBCD<Squared, L21> search(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L21(), 0, 0.0, 0.01, 0.5, 2);
    CHECK(refuses(search, X, y, fm));
    PBCD<Squared, L21> shuf(iters, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L21(), 0, 0.0, 0.01, 0.5, 0, false, true);
    CHECK(refuses(shuf, X, y, fm));
    PBCD<Squared, L21> shrink(1, 1e-6, 1e-3, 1e-4, 1e-3, Squared(), L21(), 0, 0.0, 0.01, 0.5, 0, true, false);
    CHECK(!refuses(shrink, X, y, fm));  // accepted and ignored
  }
  if (failures == 0) std::printf("pbcd host ok\n");
  return failures == 0 ? 0 : 1;
}
