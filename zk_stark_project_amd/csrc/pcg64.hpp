// pcg64.hpp — numpy's PCG64 (PCG XSL-RR 128/64) as an indexed stream, for gfx950 and host.
//
// np.random.default_rng(seed).integers(0, 2**64, shape, uint64) is the generator's raw
// output, so the TrainingUpdate masks (prover.py build_trace) are values of this stream:
//   s_0 = state, s_{j+1} = s_j * MUL + inc (mod 2^128), value e = out(s_{e+1}),
//   out(s) = rotr64((s >> 64) ^ (s & (2^64 - 1)), s >> 122).
// The step is an affine map, so k steps are one: (a, c) o (a, c) = (a^2, c * (a + 1)), and
// square-and-multiply over the doubled pairs reaches any index in log2(index) products.
#pragma once
#include "felt.hpp"

namespace pcg {

struct u128 {
  uint64_t lo, hi;
};

constexpr uint64_t MUL_LO = 0x4385DF649FCCF645ull, MUL_HI = 0x2360ED051FC65DA4ull;
// doubled pairs a device jump reads: indices below 2^30 (120 masks x 2^23 rows = 2^29.9)
constexpr uint32_t JUMP_BITS = 30;

ZKP_HD uint64_t mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
ZKP_HD u128 mul(u128 a, u128 b) { return {a.lo * b.lo, mulhi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo}; }
ZKP_HD u128 add(u128 a, u128 b) {
  const uint64_t lo = a.lo + b.lo;
  return {lo, a.hi + b.hi + (lo < a.lo)};
}
// s * a + c: one step with (MUL, inc), 2^j steps with the j-th doubled pair
ZKP_HD u128 affine(u128 s, u128 a, u128 c) { return add(mul(s, a), c); }
ZKP_HD uint64_t out(u128 s) {
  const uint64_t x = s.hi ^ s.lo;
  const uint32_t r = (uint32_t)(s.hi >> 58);
  return (x >> r) | (x << ((64 - r) & 63));
}

// pair j = 2^j steps of the generator with increment inc
inline void doubled_pairs(u128 inc, uint32_t count, u128* a, u128* c) {
  a[0] = {MUL_LO, MUL_HI};
  c[0] = inc;
  for (uint32_t j = 1; j < count; j++) {
    a[j] = mul(a[j - 1], a[j - 1]);
    c[j] = mul(c[j - 1], add(a[j - 1], {1, 0}));
  }
}

// s_k from s_0 for k < 2^JUMP_BITS: every lane runs every pair and keeps the ones of its
// own bits (a, c: uniform reads on the device)
ZKP_HD u128 jump(u128 s, const u128* __restrict__ a, const u128* __restrict__ c, uint32_t k) {
  for (uint32_t j = 0; j < JUMP_BITS; j++) {
    const u128 t = affine(s, a[j], c[j]);
    const bool take = (k >> j) & 1;
    s.lo = take ? t.lo : s.lo;
    s.hi = take ? t.hi : s.hi;
  }
  return s;
}

}  // namespace pcg
