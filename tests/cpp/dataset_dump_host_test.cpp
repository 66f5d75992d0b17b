// tests/cpp/dataset_dump_host_test.cpp -- dumpSVMLightFile / dumpFFMFile / formatText of nimfm_amd/host/nimfm.hpp are the C ABI's
// calls: the files hold the bytes written here by hand, integer targets are written as integers, the refusals come back as
// std::invalid_argument with the reference's text.
// Built by tests/test_cpp_dataset_dump.py; needs a GPU to run.
#include <cstdio>
#include <fstream>
#include <sstream>
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

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream s;
  s << f.rdbuf();
  return s.str();
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

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string p = dir + "/nimfm_dataset_dump_host_test.txt";
  // the reference's 4 x 6 literal (tests/test_dataset.nim:124-128)
  const std::vector<double> data{1.0, -4.2, -3.0, -5.0, 103.2}, y{-1.0, 2.0, -10.0, 5.2};
  const std::vector<int64_t> indices{2, 4, 0, 3, 5}, indptr{0, 2, 3, 3, 5};
  CSRDataset X(data, indices, indptr, 4, 6);
  const std::string want = "-1.0 3:1.0 5:-4.2\n2.0 1:-3.0\n-10.0\n5.2 4:-5.0 6:103.2";

  dumpSVMLightFile(p, X, y);
  CHECK(slurp(p) == want);
  dumpSVMLightFile(p, X, y, 8);  // a row per piece
  CHECK(slurp(p) == want);
  dumpSVMLightFile(p, X, std::vector<int>{-1, 1, 1, -1});
  CHECK(slurp(p) == "-1 3:1.0 5:-4.2\n1 1:-3.0\n1\n-1 4:-5.0 6:103.2");
  CHECK(message_of([&] { dumpSVMLightFile(p, X); }) == "X.nSamples != len(y).");  // no targets yet
  CHECK(message_of([&] { dumpSVMLightFile(p, X, std::vector<double>{1.0}); }) == "X.nSamples != len(y).");
  check(nfm_dataset_set_targets(X.handle(), y.data()));
  dumpSVMLightFile(p, X);
  CHECK(slurp(p) == want);
  CHECK(formatText(X) == want && formatText(X, 16) == want);
  CHECK(message_of([&] { dumpFFMFile(p, X, y); }) != "(no exception)");
  CHECK(message_of([&] { dumpSVMLightFile(dir + "/no/such/dir/x.txt", X, y); }).find("cannot be written") != std::string::npos);

  // a dataset made on the device dumps as its upload does
  CSRDataset S = X[{3, 1, 3}];
  dumpSVMLightFile(p, S);
  CHECK(slurp(p) == "5.2 4:-5.0 6:103.2\n2.0 1:-3.0\n5.2 4:-5.0 6:103.2");

  // field-aware
  const std::vector<int64_t> fields{0, 1, 1, 0, 2};
  nfm_dataset* h = nullptr;
  check(nfm_dataset_create_csr(default_context(), 4, 6, indptr.data(), indices.data(), data.data(), fields.data(), 3, y.data(), &h));
  CSRDataset F(h);
  const std::string want_ffm = "-1.0 1:3:1.0 2:5:-4.2\n2.0 2:1:-3.0\n-10.0\n5.2 1:4:-5.0 3:6:103.2";
  dumpFFMFile(p, F);
  CHECK(slurp(p) == want_ffm);
  dumpFFMFile(p, F, std::vector<int64_t>{0, 0, 7, 0}, 1);
  CHECK(slurp(p) == "0 1:3:1.0 2:5:-4.2\n0 2:1:-3.0\n7\n0 1:4:-5.0 3:6:103.2");
  CHECK(formatText(F) == want_ffm);
  CHECK(message_of([&] { dumpSVMLightFile(p, F); }) != "(no exception)");
  std::remove(p.c_str());
  if (failures == 0) std::printf("dataset dump host ok\n");
  return failures != 0;
}
