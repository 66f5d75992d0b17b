// tests/cpp/cross_host_test.cpp -- crossDecisionFunction and recommend of nimfm_amd/host/nimfm.hpp are the
// C ABI's: every pair's score is decisionFunction of the pair's joined row, made here with operator[] and hstack, within the
// project's bound for decisionFunction against an independently ordered sum; recommend is the top K, by (-score, id), of
// exactly those bits; what is refused names the way that remains.  Built by tests/test_cpp_cross.py; needs a GPU to run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

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

typedef std::vector<int64_t> I;
typedef std::vector<double> D;

template <class F>
static std::string message_of(F f) {
  try {
    f();
  } catch (const std::exception& e) {
    return e.what();
  }
  return "(no exception)";
}

int main() {
  // U: 3 users over 4 columns (an empty row, unsorted ids); V: 5 items over 3 columns (a repeated id; items 1 and 3 identical)
  CSRDataset U(D{1.0, -2.0, 0.5, 1.5, 0.25}, I{3, 0, 1, 2, 0}, I{0, 2, 2, 5}, 3, 4);
  CSRDataset V(D{1.0, 0.5, -1.0, 2.0, 0.5, -1.0, 0.75, 0.5}, I{0, 1, 2, 2, 1, 2, 0, 0}, I{0, 1, 3, 4, 6, 8}, 5, 3);
  const int64_t nU = 3, nV = 5, d = 7, k = 3;
  FactorizationMachine fm(regression, 2, (int)k, augment, true, false);  // the dummy feature: nAugments = 1
  D P((size_t)k * (d + 1)), w(d, 0.0);
  for (size_t t = 0; t < P.size(); ++t) P[t] = 0.1 * std::sin(1.0 + 0.7 * (double)t);
  fm.setParams(P, w, 0.375);

  const D cross = fm.crossDecisionFunction(U, V);
  CHECK((int64_t)cross.size() == nU * nV);
  I rep, tile;
  for (int64_t i = 0; i < nU; ++i)
    for (int64_t j = 0; j < nV; ++j) {
      rep.push_back(i);
      tile.push_back(j);
    }
  CSRDataset Ur = U[rep], Vt = V[tile];
  CSRDataset pairs = hstack({&Ur, &Vt});
  const D want = fm.decisionFunction(pairs);
  for (size_t t = 0; t < want.size(); ++t) CHECK(std::fabs(cross[t] - want[t]) <= 1e-12 + 1e-9 * std::fabs(want[t]));

  // recommend: the top K of those bits by (-score, id); the identical items 1 and 3 in id order
  for (int64_t K : {1, 2, 5})
    for (int64_t chunk : {0, 1}) {
      auto top = fm.recommend(U, V, K, chunk);
      CHECK((int64_t)top.first.size() == nU * K && (int64_t)top.second.size() == nU * K);
      for (int64_t i = 0; i < nU; ++i) {
        I order{0, 1, 2, 3, 4};
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return cross[i * nV + a] > cross[i * nV + b]; });
        for (int64_t r = 0; r < K; ++r) {
          CHECK(top.first[i * K + r] == order[r]);
          CHECK(std::memcmp(&top.second[i * K + r], &cross[i * nV + order[r]], sizeof(double)) == 0);
        }
      }
    }
  for (int64_t i = 0; i < nU; ++i) CHECK(std::memcmp(&cross[i * nV + 1], &cross[i * nV + 3], sizeof(double)) == 0);

  // refusals
  CHECK(message_of([&] { fm.recommend(U, V, 6); }).find("crossDecisionFunction") != std::string::npos);
  CHECK(message_of([&] { fm.recommend(U, V, 0); }).find("min(nV, 256) = 5") != std::string::npos);
  CHECK(message_of([&] { fm.crossDecisionFunction(U, U); }).find("Invalid nFeatures.") != std::string::npos);
  FactorizationMachine f3(regression, 3, 2, none);
  f3.setParams(D(2 * 7, 0.5), D(7, 0.0), 0.0);
  const std::string m3 = message_of([&] { f3.crossDecisionFunction(U, V); });
  CHECK(m3.find("degree 2") != std::string::npos && m3.find("decisionFunction") != std::string::npos);

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("cross host ok\n");
  return 0;
}
