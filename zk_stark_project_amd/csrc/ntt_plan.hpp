// ntt_plan.hpp — the pass plan of a transform: which stages each kernel launch
// of launch_ntt (ntt.hip) runs, and in what block shape. Plain C++17 with no HIP
// dependency, so a CPU build can check it (tests/native/plan_dump.cpp).
#pragma once
#include <stdint.h>

// One pass: stages [s0, s0 + K) over groups of 2^K elements 2^lo apart
// (lo = s0 for DIT, logn - s0 - K for DIF), 2^logT groups per block of which
// runs of 2^logTl are contiguous in memory.
struct NttPass {
  uint32_t s0, K, lo;
  uint32_t lognt;  // log2 of the block's threads: 8, or 9 (radix-8 passes of 9 stages)
  uint32_t logT, logTl;
  bool small;      // lo == 0: the pass over the transform's smallest stages 0..2
};

struct NttPlan {
  uint32_t n = 0;
  NttPass pass[4];
  const NttPass* begin() const { return pass; }
  const NttPass* end() const { return pass + n; }
};

// Passes of <= 8 stages over `stages` stages, sizes in Ks: whole radix-8 rounds
// (multiples of 3) first where the rest still fits, largest pass last.
inline uint32_t ntt_split_stages(uint32_t stages, uint32_t Ks[4]) {
  const uint32_t KMAX = 8;
  const uint32_t npass = (stages + KMAX - 1) / KMAX;
  uint32_t rem = stages;
  for (uint32_t p = 0; p < npass; p++) {
    const uint32_t left = npass - p;
    uint32_t k = (rem + left - 1) / left;
    if (left > 1) {
      const uint32_t k3 = k / 3 * 3;  // round down to whole radix-8 rounds if the rest still fits
      if (k3 >= 3 && rem - k3 <= KMAX * (left - 1)) k = k3;
    }
    Ks[p] = k;
    rem -= k;
  }
  return npass;
}

// The passes of a 2^logn transform (1 <= logn <= 32; otherwise none) over
// `batches` arrays. logn < 11: radix-2 passes (k_ntt_pass, 4096 elements per
// block). logn >= 11: radix-8 register-blocked passes (k_ntt8) of 2048 elements
// per 256-thread block, or 4096 per 512-thread block:
//   2^11       one 11-stage pass: one HBM read and write per array instead of 6 + 5
//              stages' two
//   2^17-2^20  11 stages in the lo = 0 pass (first for DIT, last for DIF) and the
//              other 6-9 in one more: a third less HBM traffic than three passes
//   otherwise  ntt_split_stages
// The measurements behind these choices are cited in launch_ntt.
inline NttPlan ntt_plan(uint32_t logn, bool dit, uint32_t batches) {
  NttPlan pl;
  if (logn == 0 || logn > 32) return pl;
  const bool radix2 = logn < 11;
  uint32_t Ks[4] = {0, 0, 0, 0};
  if (logn == 11) {
    pl.n = 1;
    Ks[0] = 11;
  } else if (logn >= 17 && logn <= 20) {
    pl.n = 2;
    Ks[0] = dit ? 11 : logn - 11;
    Ks[1] = dit ? logn - 11 : 11;
  } else {
    pl.n = ntt_split_stages(logn, Ks);
  }
  uint32_t s0 = 0;
  for (uint32_t p = 0; p < pl.n; s0 += Ks[p], p++) {
    NttPass& ps = pl.pass[p];
    ps.s0 = s0;
    ps.K = Ks[p];
    ps.lo = dit ? s0 : logn - s0 - ps.K;
    ps.small = ps.lo == 0;
    // 9 stages (2^20 only) in 512-thread blocks, rows of 8 felts = whole 128-B lines,
    // when there are >= 8 arrays; fewer keep 256 threads (see launch_ntt)
    ps.lognt = !radix2 && ps.K == 9 && batches >= 8 ? 9 : 8;
    const uint32_t loge = radix2 ? 12 : ps.lognt + 3, logG = logn - ps.K;
    ps.logT = loge - ps.K < logG ? loge - ps.K : logG;
    ps.logTl = ps.logT < ps.lo ? ps.logT : ps.lo;
  }
  return pl;
}
