// deep_inv_check.hip — the DEEP inverse table of launch_deep_denominators
// (csrc/kernels.hip, linked directly) against one Fermat inversion per point
// (TEST ONLY; run by tests/test_gpu_deep_denominators.py).
// The table holds 1 / (x_q - z) of every LDE point, coset-major; k_deep takes
// the second denominator from the previous row: 1 / (x_q - z w_n) = w_n^-1 *
// table[q^-], q^- = the cyclic predecessor of q within its coset. Both are
// checked at every point, the row t = 0 of every coset included, for trace
// lengths 8 (one group of 8 per coset, no w_{n/8} table), 16, 64 and 2^11 (the
// table's first full 2048-point block per coset) over 2, 8 and 32 cosets.
// z is fixed and off every domain. Prints one line per case and the mismatch
// count, and exits non-zero unless that is 0.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../zk_stark_project_amd/csrc/zkp_internal.hpp"
#include "../../zk_stark_project_amd/csrc/host_stark.hpp"

using namespace fp;
using namespace zkh;

void launch_fail(int code, const char* what) { throw std::runtime_error(std::string(what) + " " + std::to_string(code)); }

#define CK(x)                                                 \
  do {                                                        \
    hipError_t e_ = (x);                                      \
    if (e_ != hipSuccess) {                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      exit(2);                                                \
    }                                                         \
  } while (0)

template <typename T>
static T* up(const std::vector<T>& h) {
  T* d;
  CK(hipMalloc(&d, h.size() * sizeof(T) + 16));
  CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

// stage-major table of a 2^logN domain: level t at [2^t - 1, 2^(t+1) - 1) holds w_{2^(t+1)}^j
static std::vector<felt> stage_table(uint32_t logN) {
  std::vector<felt> t((size_t)1 << logN);
  for (uint32_t lev = 0; lev < logN; lev++) {
    const felt w = root_of_unity(lev + 1);
    felt acc = one();
    for (uint64_t j = 0; j < (1ull << lev); j++) {
      t[((1ull << lev) - 1) + j] = acc;
      acc = mul(acc, w);
    }
  }
  return t;
}

int main() {
  setvbuf(stdout, NULL, _IONBF, 0);
  hipStream_t st;
  CK(hipStreamCreate(&st));
  // the launch inverts its one total product on a second stream, joined by an event
  hipStream_t st2;
  hipEvent_t ev;
  CK(hipStreamCreate(&st2));
  CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  Prof pf;
  const felt z = make(0x0123456789abcdefull, 0x0fedcba987654321ull);
  const felt w8 = root_of_unity(3), w8_2 = sqr(w8);
  const DeepRoots roots{w8, w8_2, mul(w8_2, w8)};
  long long bad = 0;
  int cases = 0;
  for (const uint32_t logn : {3u, 4u, 6u, 11u})
    for (const uint32_t logB : {1u, 3u, 5u}) {
      const uint32_t B = 1u << logB, logN = logn + logB;
      const uint64_t n = 1ull << logn, count = (uint64_t)B * n;
      const felt wn = root_of_unity(logn), wN = root_of_unity(logN), g = felt_u64(3);
      if (eq(pow_u64(z, 1ull << logN), pow_u64(g, 1ull << logN))) {
        printf("z lies on the domain\n");
        return 2;
      }
      // the prover's inputs: coset offsets and their 8th powers, the twiddle table, z's squarings
      std::vector<felt> cx(B), cx8(B), pw(2 * (size_t)logn), zz = {z, mul(z, wn)};
      for (uint32_t j = 0; j < B; j++) {
        cx[j] = mul(g, pow_u64(wN, j));
        cx8[j] = pow_u64(cx[j], 8);
      }
      felt a = zz[0], b = zz[1];
      for (uint32_t l = 0; l < logn; l++) { pw[l] = a; pw[logn + l] = b; a = sqr(a); b = sqr(b); }
      felt *dcx = up(cx), *dcx8 = up(cx8), *dpw = up(pw), *dzz = up(zz), *dtw = up(stage_table(logN));
      felt *scratch, *table;
      CK(hipMalloc(&scratch, deep_den_scratch(count) * 16));
      CK(hipMalloc(&table, count * 16));
      CK(hipMemset(table, 0, count * 16));
      const PointMap pm{dcx, dtw + ((1ull << (logn - 1)) - 1), logn};
      const PointMap pm8{dcx8, logn > 3 ? dtw + ((1ull << (logn - 4)) - 1) : nullptr, logn - 3};
      launch_deep_denominators(pf, st, st2, ev, pm, pm8, roots, count, dzz, dpw, scratch, table);
      CK(hipStreamSynchronize(st));
      std::vector<felt> got(count);
      CK(hipMemcpy(got.data(), table, count * 16, hipMemcpyDeviceToHost));
      const felt ginv = inv(wn);
      long long mz = 0, mzg = 0;
      for (uint32_t j = 0; j < B; j++) {
        felt x = cx[j];
        for (uint64_t t = 0; t < n; t++, x = mul(x, wn)) {
          const uint64_t q = (uint64_t)j * n + t, qp = t ? q - 1 : q + n - 1;
          if (!eq(got[q], inv(sub(x, zz[0])))) mz++;
          if (!eq(mul(ginv, got[qp]), inv(sub(x, zz[1])))) mzg++;
        }
      }
      cases++;
      bad += mz + mzg;
      printf("n=2^%u cosets=%u: %lld mismatches at z, %lld at z*w_n of %llu points\n", logn, B, mz, mzg,
             (unsigned long long)count);
      for (felt* p : {dcx, dcx8, dpw, dzz, dtw, scratch, table}) CK(hipFree(p));
    }
  printf("%d cases, %lld mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
