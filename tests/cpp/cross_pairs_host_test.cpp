// tests/cpp/cross_pairs_host_test.cpp -- crossDecisionFunctionAt, recommendAmong and rankingScoreAmong of nimfm_amd/host/nimfm.hpp
//  agree with the dense members by bits.  Built by tests/test_cpp_cross_pairs.py; needs a GPU to run.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../nimfm_amd/host/nimfm.hpp"

using namespace nimfm;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

typedef std::vector<int64_t> I;
typedef std::vector<double> D;

int main() {  // the sets of cross_host_test.cpp: 3 users over 4 columns, 5 items over 3 columns
  CSRDataset U(D{1.0, -2.0, 0.5, 1.5, 0.25}, I{3, 0, 1, 2, 0}, I{0, 2, 2, 5}, 3, 4);
  CSRDataset V(D{1.0, 0.5, -1.0, 2.0, 0.5, -1.0, 0.75, 0.5}, I{0, 1, 2, 2, 1, 2, 0, 0}, I{0, 1, 3, 4, 6, 8}, 5, 3);
  const int64_t nV = 5, d = 7, k = 3;
  FactorizationMachine fm(regression, 2, (int)k, augment, true, false);
  D P((size_t)k * (d + 1)), w(d, 0.0);
  for (size_t t = 0; t < P.size(); ++t) P[t] = 0.1 * std::sin(1.0 + 0.7 * (double)t);
  fm.setParams(P, w, 0.375);
  // candidates: user 0 an unsorted row with item 3 twice, user 1 none, user 2 one item; seen: their complement
  const I ci{3, 0, 3, 4, 2}, cp{0, 4, 4, 5};
  CSRDataset cand(D(ci.size(), 1.0), ci, cp, 3, nV), seen(D{1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0},
                                                             I{1, 2, 0, 1, 2, 3, 4, 0, 1, 3, 4}, I{0, 2, 7, 11}, 3, nV);
  CSRDataset held(D{1.0, 1.0, 1.0}, I{3, 1, 2}, I{0, 1, 2, 3}, 3, nV);
  const D cross = fm.crossDecisionFunction(U, V), at = fm.crossDecisionFunctionAt(U, V, cand);
  CHECK(at.size() == ci.size());
  for (int64_t i = 0; i < 3; ++i)
    for (int64_t e = cp[i]; e < cp[i + 1] && (size_t)e < at.size(); ++e) CHECK(std::memcmp(&at[e], &cross[i * nV + ci[e]], sizeof(double)) == 0);
  for (int64_t K : {1, 4}) {
    auto among = fm.recommendAmong(U, V, K, cand), unseen = fm.recommend(U, V, seen, K);
    CHECK(among.first == unseen.first && among.second.size() == unseen.second.size() &&
          std::memcmp(among.second.data(), unseen.second.data(), sizeof(double) * unseen.second.size()) == 0);
    CHECK(among.first[1 * K] == -1 && std::isnan(among.second[1 * K]) && among.first[2 * K] == 2);
    auto a = fm.rankingScoreAmong(U, V, held, K, cand), b = fm.rankingScore(U, V, held, K, &seen);
    CHECK(std::memcmp(&a, &b, sizeof(a)) == 0 && a.nUsers == 3 && a.hitRate > 0.0);
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("cross pairs host ok\n");
  return 0;
}
