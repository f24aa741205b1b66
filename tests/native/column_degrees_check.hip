// column_degrees_check.hip — k_column_degrees alone (csrc/kernels.hip, linked directly)
// through launch_column_degrees (TEST ONLY; run by tests/test_gpu_constraint_degrees.py).
// A column is E segments of n felts in the library's bit-reversed layout: element m*n + p
// holds coefficient m*n + rev(p). Cases, at (n, E) = (128, 4) [two blocks of 256] and
// (2^11, 2) [16 blocks]: one non-zero coefficient at index 0, 1, 63, 64, n - 1, n and
// E*n - 1; two non-zeros whose higher index sits at the lower memory position; an all-zero
// column; ten columns in one launch, zero and non-zero alternating. The expected degree of
// every column is a plain host scan of the same array. Prints one line per case and the
// mismatch count, and exits non-zero unless that is 0.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../zk_stark_project_amd/csrc/zkp_internal.hpp"

using namespace fp;

void launch_fail(int code, const char* what) { throw std::runtime_error(std::string(what) + " " + std::to_string(code)); }

#define CK(x)                                                 \
  do {                                                        \
    hipError_t e_ = (x);                                      \
    if (e_ != hipSuccess) {                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      exit(2);                                                \
    }                                                         \
  } while (0)

static uint32_t rev(uint32_t p, uint32_t bits) {
  uint32_t r = 0;
  for (uint32_t b = 0; b < bits; b++) r |= ((p >> b) & 1u) << (bits - 1 - b);
  return r;
}

struct Shape {
  uint32_t logn, logE;
  uint64_t n() const { return 1ull << logn; }
  uint64_t M() const { return 1ull << (logn + logE); }
  // the memory position of coefficient d
  uint64_t pos(uint64_t d) const { return (d & ~(n() - 1)) | rev((uint32_t)(d & (n() - 1)), logn); }
};

static int cases = 0, mismatches = 0;

// `cols` columns of sh.M() felts each: the launch against a host scan
static void run(hipStream_t st, Prof& pf, const Shape& sh, const std::vector<felt>& h, uint32_t cols, const char* what) {
  const uint64_t M = sh.M();
  std::vector<long long> want(cols, -1), got(cols, 0);
  for (uint32_t k = 0; k < cols; k++)
    for (uint64_t e = 0; e < M; e++)
      if (h[k * M + e].lo | h[k * M + e].hi) {
        const uint32_t p = (uint32_t)(e & (sh.n() - 1));
        const long long d = (long long)(e - p + rev(p, sh.logn));
        if (d > want[k]) want[k] = d;
      }
  felt* d;
  long long* dd;
  CK(hipMalloc(&d, h.size() * sizeof(felt)));
  CK(hipMalloc(&dd, cols * 8));
  CK(hipMemcpy(d, h.data(), h.size() * sizeof(felt), hipMemcpyHostToDevice));
  CK(hipMemsetAsync(dd, 0xff, cols * 8, st));
  launch_column_degrees(pf, st, d, sh.logn, sh.logE, cols, dd);
  CK(hipStreamSynchronize(st));
  CK(hipMemcpy(got.data(), dd, cols * 8, hipMemcpyDeviceToHost));
  CK(hipFree(d));
  CK(hipFree(dd));
  int bad = 0;
  for (uint32_t k = 0; k < cols; k++) bad += got[k] != want[k];
  printf("n=2^%u E=%u %-28s want[0]=%lld got[0]=%lld %s\n", sh.logn, 1u << sh.logE, what, want[0], got[0],
         bad ? "MISMATCH" : "ok");
  cases++;
  mismatches += bad;
}

int main() {
  setvbuf(stdout, NULL, _IONBF, 0);
  hipStream_t st;
  CK(hipStreamCreate(&st));
  Prof pf;
  const felt v = make(0x1234, 0x1);
  for (const Shape sh : {Shape{7, 2}, Shape{11, 1}}) {
    const uint64_t n = sh.n(), M = sh.M();
    for (uint64_t d : {(uint64_t)0, (uint64_t)1, (uint64_t)63, (uint64_t)64, n - 1, n, M - 1}) {
      std::vector<felt> h(M, zero());
      h[sh.pos(d)] = v;
      run(st, pf, sh, h, 1, ("single coefficient " + std::to_string(d)).c_str());
    }
    {
      // memory positions 1 and 2 of segment 0 hold coefficients n/2 and n/4
      std::vector<felt> h(M, zero());
      h[1] = v;
      h[2] = make(1, 0);
      run(st, pf, sh, h, 1, "higher index at lower position");
    }
    {
      std::vector<felt> h(M, zero());
      run(st, pf, sh, h, 1, "all zero");
    }
    {
      // a value whose low word alone, then whose high word alone is non-zero; zero columns between
      std::vector<felt> h(10 * M, zero());
      for (uint32_t k = 1; k < 10; k += 2) {
        h[k * M + sh.pos(k * 37 % M)] = make(0, 1);
        h[k * M + sh.pos((k * 101 + n) % M)] = make(1, 0);
      }
      run(st, pf, sh, h, 10, "ten columns, alternating");
    }
  }
  printf("%d cases, %d mismatches\n", cases, mismatches);
  return mismatches ? 1 : 0;
}
