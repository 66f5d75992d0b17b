// tests/cpp/dataset_ops_host_test.cpp -- the dataset ops of nimfm_amd/host/nimfm.hpp (X[indices], slice, shuffle, vstack, hstack,
// normalize, loadUserItemRatingFile) are the C ABI's calls: the arrays read back are the ones computed here by hand, the
// reference's error texts come back as std::invalid_argument, normalize works in place.
// Built by tests/test_cpp_dataset_ops.py; needs a GPU to run.
#include <cmath>
#include <cstdio>
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

struct Host {
  std::vector<int64_t> indptr, indices;
  std::vector<double> data;
  int64_t n = 0, d = 0;
};
static Host read_back(const CSRDataset& X) {
  Host H;
  int64_t nnz = 0, nf = 0;
  check(nfm_dataset_shape(X.handle(), &H.n, &H.d, &nnz, &nf));
  H.indptr.resize((size_t)H.n + 1);
  H.indices.resize((size_t)nnz);
  H.data.resize((size_t)nnz);
  check(nfm_dataset_get_csr(X.handle(), H.indptr.data(), H.indices.data(), H.data.data(), nullptr));
  return H;
}
template <class F>
static std::string message_of(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "(no exception)";
}

int main() {
  // the reference's 4 x 6 literal (tests/test_dataset.nim:124-128)
  const std::vector<double> data{1.0, -4.2, -3.0, -5.0, 103.2}, y{-1.0, 2.0, -10.0, 5.2};
  const std::vector<int64_t> indices{2, 4, 0, 3, 5}, indptr{0, 2, 3, 3, 5};
  CSRDataset X(data, indices, indptr, 4, 6);
  check(nfm_dataset_set_targets(X.handle(), y.data()));

  CSRDataset S = X[{3, 1, 3}];
  Host h = read_back(S);
  CHECK(h.n == 3 && h.d == 6 && (h.indptr == std::vector<int64_t>{0, 2, 3, 5}) && (h.indices == std::vector<int64_t>{3, 5, 0, 3, 5}));
  CHECK((h.data == std::vector<double>{-5.0, 103.2, -3.0, -5.0, 103.2}) && (S.targets() == std::vector<double>{5.2, 2.0, 5.2}));
  CSRDataset T = X.slice(1, 4);
  h = read_back(T);
  CHECK(h.n == 3 && (h.indptr == std::vector<int64_t>{0, 1, 1, 3}) && (h.indices == std::vector<int64_t>{0, 3, 5}) &&
        (T.targets() == std::vector<double>{2.0, -10.0, 5.2}));
  CHECK(message_of([&] { X[std::vector<int64_t>{}]; }) == "Invalid slice: nSamples < 1.");
  CHECK(message_of([&] { X[{0, 4}]; }) == "max(indicesRow) 4 >= 4.");
  CHECK(message_of([&] { X[{-1, 2}]; }) == "min(indicesRow) -1 < 0.");
  CHECK(message_of([&] { X.slice(2, 2); }) == "Invalid slice: nSamples < 1.");

  CSRDataset V = vstack({&X, &T, &X});
  h = read_back(V);
  CHECK(h.n == 11 && h.d == 6 && h.indptr.back() == 13 && h.indptr[4] == 5 && h.indptr[7] == 8 && h.indices[5] == 0 && h.data[12] == 103.2);
  CHECK(V.targets().size() == 11 && V.targets()[4] == 2.0 && V.targets()[10] == 5.2);
  CSRDataset Hs = hstack({&X, &X});
  h = read_back(Hs);
  CHECK(h.n == 4 && h.d == 12 && (h.indptr == std::vector<int64_t>{0, 4, 6, 6, 10}) &&
        (h.indices == std::vector<int64_t>{2, 4, 8, 10, 0, 6, 3, 5, 9, 11}) && (Hs.targets() == y));
  CHECK(message_of([&] { vstack({&X, &Hs}); }) == "All matrics must have the same shape[1].");
  CHECK(message_of([&] { hstack({&X, &T}); }) == "All matrics must have the same shape[0].");

  // normalize in place: l2 per row, then linfty per column of a fresh copy
  CSRDataset N = X.slice(0, 4);
  normalize(N);
  h = read_back(N);
  const double r0 = std::sqrt((0.0 + 1.0 * 1.0) + -4.2 * -4.2), r3 = std::sqrt((0.0 + -5.0 * -5.0) + 103.2 * 103.2);
  CHECK((h.data == std::vector<double>{1.0 / r0, -4.2 / r0, -3.0 / 3.0, -5.0 / r3, 103.2 / r3}) && (h.indices == indices) && N.nSamples() == 4);
  CSRDataset C = vstack({&X, &X});
  normalize(C, 0, linfty);
  h = read_back(C);
  CHECK(h.data.size() == 10 && h.data[0] == 1.0 && h.data[1] == -1.0 && h.data[4] == 1.0 && h.data[9] == 1.0);
  normalize(C, 1, l1);  // the object keeps working after the swap
  h = read_back(C);
  CHECK(h.data[0] == 0.5 && h.data[1] == -0.5 && h.data[2] == -1.0);
  CHECK(read_back(X).data == data);  // the input is untouched

  // shuffle: explicit indices, then the forward draw (a permutation, reproducible from the seed)
  auto sh = shuffle(X, y, std::vector<int64_t>{2, 0, 3});
  CHECK(sh.first.nSamples() == 3 && (sh.second == std::vector<double>{-10.0, -1.0, 5.2}) && (read_back(sh.first).indptr == std::vector<int64_t>{0, 0, 2, 4}));
  globalRand().randomize(5);
  auto a = shuffle(X, y);
  globalRand().randomize(5);
  auto b = shuffle(X, y);
  std::vector<double> sorted = a.second;
  std::sort(sorted.begin(), sorted.end());
  CHECK(a.second == b.second && (sorted == std::vector<double>{-10.0, -1.0, 2.0, 5.2}) && a.first.targets() == a.second);
  CHECK(message_of([&] { shuffle(X, std::vector<double>{1.0}); }) == "X.nSamples != len(y)");

  // loadUserItemRatingFile: smallest id 5 keeps base 1
  const char* path = "/tmp/nimfm_dataset_ops_host_test_ratings.txt";
  FILE* f = std::fopen(path, "w");
  std::fputs("5::7::3::978300760\n9::5::4.5::978300761\n", f);
  std::fclose(f);
  std::vector<double> yr;
  CSRDataset R = X.slice(0, 1);
  loadUserItemRatingFile(path, R, yr);
  std::remove(path);
  h = read_back(R);
  CHECK(h.n == 2 && h.d == 9 + 7 && (h.indices == std::vector<int64_t>{4, 15, 8, 13}) && (h.data == std::vector<double>{1, 1, 1, 1}) &&
        (yr == std::vector<double>{3.0, 4.5}));
  if (failures == 0) std::printf("dataset ops host ok\n");
  return failures != 0;
}
