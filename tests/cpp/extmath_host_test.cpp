// tests/cpp/extmath_host_test.cpp -- matmul, mvmul, vmmul of nimfm_amd/host/nimfm.hpp are the C ABI's: the
// reference's argument order on both layouts, the result shapes, and std::invalid_argument with the reference's texts for a shape
// mismatch.  The operands are identities and ones on the reference's 4 x 6 literal, so every expected number is a stored
// value or an exact sum; the kernels' bits are tests/test_gpu_extmath.py's.
// Built by tests/test_cpp_extmath.py; needs a GPU to run.
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

typedef std::vector<int64_t> I;
typedef std::vector<double> D;

template <class F>
static std::string invalid_argument_of(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  } catch (const std::exception& e) {
    return std::string("(another exception) ") + e.what();
  }
  return "(no exception)";
}
static Matrix identity(int64_t n) {
  Matrix E(n, n);
  for (int64_t i = 0; i < n; ++i) E(i, i) = 1.0;
  return E;
}

int main() {
  // the reference's 4 x 6 literal (tests/test_dataset.nim:124-128)
  const D data{1.0, -4.2, -3.0, -5.0, 103.2};
  const I indices{2, 4, 0, 3, 5}, indptr{0, 2, 3, 3, 5};
  CSRDataset X(data, indices, indptr, 4, 6);
  CSCDataset Xc = toCSCDataset(X);
  const D dense{0, 0, 1.0, 0, -4.2, 0, /**/ -3.0, 0, 0, 0, 0, 0, /**/ 0, 0, 0, 0, 0, 0, /**/ 0, 0, 0, -5.0, 0, 103.2};

  for (const CSRDataset* S : {static_cast<const CSRDataset*>(&X), static_cast<const CSRDataset*>(&Xc)}) {
    Matrix R = matmul(*S, identity(6));  // S . I
    CHECK(R.rows == 4 && R.cols == 6 && R.data == dense);
    Matrix L = matmul(identity(4), *S);  // I . S
    CHECK(L.rows == 4 && L.cols == 6 && L.data == dense);
    Matrix two(6, 2);  // the columns 2 and 5 of S
    two(2, 0) = 1.0;
    two(5, 1) = 1.0;
    CHECK((matmul(*S, two).data == D{1.0, 0, 0, 0, 0, 0, 0, 103.2}));
    Matrix pick(1, 4);  // the row 3 of S
    pick(0, 3) = 1.0;
    CHECK((matmul(pick, *S).data == D{0, 0, 0, -5.0, 0, 103.2}));
    CHECK((mvmul(*S, D{1, 1, 1, 1, 1, 1}) == D{1.0 + -4.2, -3.0, 0.0, -5.0 + 103.2}));
    CHECK((vmmul(D{1, 1, 1, 1}, *S) == D{-3.0, 0.0, 1.0, -5.0, -4.2, 103.2}));
    CHECK((vmmul(D{0, 2, 0, 0}, *S) == D{-6.0, 0, 0, 0, 0, 0}));

    CHECK(invalid_argument_of([&] { matmul(*S, identity(5)); }) == "S.shape[1] 6 != D.shape[0] 5.");
    CHECK(invalid_argument_of([&] { mvmul(*S, D{1, 1, 1, 1}); }) == "shape[1] 6 != len(vec)4.");
    CHECK(invalid_argument_of([&] { vmmul(D{1, 1, 1, 1, 1, 1}, *S); }) == "len(vec)6 != shape[0] 4.");
  }
  CHECK(invalid_argument_of([&] { matmul(identity(6), X); }) == "D.shape[1] 6 != shape[0] 4.");
  CHECK(invalid_argument_of([&] { matmul(identity(6), Xc); }) == "D.shape[1] 6 != S.shape[0] 4.");

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("extmath host ok\n");
  return 0;
}
