// tests/cpp/csc_host_test.cpp -- the column-major dataset of nimfm_amd/host/nimfm.hpp (CSCDataset, toCSCDataset, toCSRDataset,
// slice, vstack, hstack, normalize, decisionFunction and CD's fit on it) is the C ABI's: the arrays read back are the ones
// computed here by hand from the reference's 4 x 6 literal, a consumer of rows gives on it what it gives on toCSRDataset of
// it, bit for bit, and what needs rows in storage order is refused with a message that names the way out.
// Built by tests/test_cpp_csc.py; needs a GPU to run.
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

struct Cols {
  I indptr, indices;
  D data;
};
static Cols cols_of(const CSCDataset& X) {
  Cols c;
  X.toHost(c.indptr, c.indices, c.data);
  return c;
}
static Cols rows_of(const CSRDataset& X) {
  Cols c;
  int64_t n = 0, d = 0, nnz = 0, nf = 0;
  check(nfm_dataset_shape(X.handle(), &n, &d, &nnz, &nf));
  c.indptr.resize((size_t)n + 1);
  c.indices.resize((size_t)nnz);
  c.data.resize((size_t)nnz);
  check(nfm_dataset_get_csr(X.handle(), c.indptr.data(), c.indices.data(), c.data.data(), nullptr));
  return c;
}
template <class F>
static std::string message_of(F f) {
  try {
    f();
  } catch (const std::exception& e) {
    return e.what();
  }
  return "(no exception)";
}
static bool same_bits(const D& a, const D& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

int main() {
  // the reference's 4 x 6 literal (tests/test_dataset.nim:124-128)
  const D data{1.0, -4.2, -3.0, -5.0, 103.2}, y{-1.0, 2.0, -10.0, 5.2};
  const I indices{2, 4, 0, 3, 5}, indptr{0, 2, 3, 3, 5};
  CSRDataset X(data, indices, indptr, 4, 6);
  check(nfm_dataset_set_targets(X.handle(), y.data()));

  CSCDataset Xc = toCSCDataset(X);
  Cols c = cols_of(Xc);
  CHECK(Xc.nSamples() == 4 && Xc.nFeatures() == 6 && Xc.targets() == y);
  CHECK((c.indptr == I{0, 1, 1, 2, 3, 4, 5}) && (c.indices == I{1, 0, 3, 0, 3}) && (c.data == D{-3.0, 1.0, -5.0, -4.2, 103.2}));
  CSRDataset Xr = toCSRDataset(Xc);
  Cols r = rows_of(Xr);
  CHECK(r.indptr == indptr && r.indices == indices && r.data == data && Xr.targets() == y);

  // newCSCDataset from the same arrays is the same dataset
  CSCDataset Xn(c.data, c.indices, c.indptr, 4, 6);
  Cols cn = cols_of(Xn);
  CHECK(cn.indptr == c.indptr && cn.indices == c.indices && cn.data == c.data);

  // X[1..<4]: ids rebased, targets sliced
  CSCDataset S = Xc.slice(1, 4);
  Cols s = cols_of(S);
  CHECK(S.nSamples() == 3 && (s.indptr == I{0, 1, 1, 1, 2, 2, 3}) && (s.indices == I{0, 2, 2}) && (s.data == D{-3.0, -5.0, 103.2}));
  CHECK((S.targets() == D{2.0, -10.0, 5.2}));

  // hstack: arrays concatenated; vstack: per column the parts' columns, ids offset; its indptr has nFeatures + 1 entries
  CSCDataset H = hstack({&Xc, &Xc});
  Cols h = cols_of(H);
  CHECK(H.nSamples() == 4 && H.nFeatures() == 12 && (h.indptr == I{0, 1, 1, 2, 3, 4, 5, 6, 6, 7, 8, 9, 10}));
  CHECK((h.indices == I{1, 0, 3, 0, 3, 1, 0, 3, 0, 3}) && H.targets() == y);
  CSCDataset V = vstack({&Xc, &Xc});
  Cols v = cols_of(V);
  CHECK(V.nSamples() == 8 && V.nFeatures() == 6 && (v.indptr == I{0, 2, 2, 4, 6, 8, 10}) && (v.indices == I{1, 5, 0, 4, 3, 7, 0, 4, 3, 7}));
  CHECK((v.data == D{-3.0, -3.0, 1.0, 1.0, -5.0, -5.0, -4.2, -4.2, 103.2, 103.2}) && V.targets().size() == 8);

  // normalize in place: every column of the literal holds one entry, so l1 per column leaves the signs
  CSCDataset N = toCSCDataset(X);
  normalize(N, 0, l1);
  CHECK((cols_of(N).data == D{-1.0, 1.0, -1.0, -1.0, 1.0}) && cols_of(N).indices == c.indices);
  CSCDataset M = toCSCDataset(X);
  normalize(M, 1, linfty);  // per sample: row 0 by 4.2, row 1 by 3, row 3 by 103.2
  CHECK((cols_of(M).data == D{-3.0 / 3.0, 1.0 / 4.2, -5.0 / 103.2, -4.2 / 4.2, 103.2 / 103.2}));

  // consumers of rows: the CSCDataset gives what toCSRDataset of it gives
  FactorizationMachine fa(regression, 2, 4, explicit_, true, true, false, 3), fb(regression, 2, 4, explicit_, true, true, false, 3);
  fa.init(Xc);
  fb.init(Xr);
  CHECK(same_bits(fa.decisionFunction(Xc), fb.decisionFunction(Xr)));
  CHECK(fa.score(Xc, y) == fb.score(Xr, y));
  CD<Squared> ca(2, 1e-6, 1e-3, 1e-3, Squared(), 0, 0.0), cb(2, 1e-6, 1e-3, 1e-3, Squared(), 0, 0.0);
  ca.fit(Xc, y, fa);
  cb.fit(Xr, y, fb);
  CHECK(same_bits(fa.P, fb.P) && same_bits(fa.w, fb.w) && fa.intercept == fb.intercept && ca.history == cb.history);
  FactorizationMachine f0(regression, 2, 4, explicit_, true, true, false, 3);
  f0.init(Xr);
  CHECK(!same_bits(fa.P, f0.P));

  // what needs rows in storage order names the way out
  CHECK(message_of([&] { Xc[{0, 1}]; }).find("toCSRDataset") != std::string::npos);
  CHECK(message_of([&] { dumpSVMLightFile("/dev/null", Xc, y); }).find("toCSRDataset") != std::string::npos);
  SGD<Squared> sgd(1);
  sgd.verbose = 0;
  CHECK(message_of([&] { sgd.fit(Xc, y, f0); }).find("toCSRDataset") != std::string::npos);
  CHECK(message_of([&] { hstack(std::vector<const CSRDataset*>{&Xc, &X}); }).find("cannot be stacked together") != std::string::npos);

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("csc host ok\n");
  return 0;
}
