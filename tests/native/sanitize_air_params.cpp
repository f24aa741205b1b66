// Host ASan/UBSan driver (TEST ONLY) for programs with public inputs: the binding and
// validation code of zkp_air_register_params (csrc/air_program.hpp), zkp_air_check_trace_pub
// and the verifier's pub path (csrc/verifier.cpp). Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all; every array it passes is an
// exactly-sized heap block, so a read past an end aborts the run.
// Usage: sanitize_air_params <case_dir>   (a MiMC proof: proof.bin, pub.bin, meta.txt)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/zkp.h"

static std::vector<uint8_t> slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
template <class T>
static T* heap(const std::vector<T>& v) {  // an exactly-sized copy
  T* p = (T*)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
static zkp_felt fe(uint64_t v) { return zkp_felt{v, 0}; }
static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
      failures++;                                                 \
    }                                                             \
  } while (0)

// width 1: next - cur - pub[0] = 0 (a counter with the step from pub); one single, one
// periodic-over-n and one sequence assertion, bound or concrete
struct Counter {
  std::vector<uint8_t> degrees{1};
  std::vector<uint64_t> ops{ZKP_AIR_OP(ZKP_OP_SUB, 0, ZKP_AIR_OPERAND(ZKP_SRC_NEXT, 0), ZKP_AIR_OPERAND(ZKP_SRC_CUR, 0)),
                            ZKP_AIR_OP(ZKP_OP_SUB, 0, ZKP_AIR_OPERAND(ZKP_SRC_REG, 0), ZKP_AIR_OPERAND(ZKP_SRC_PUB, 0)),
                            ZKP_AIR_OP(ZKP_OP_EMIT, 0, ZKP_AIR_OPERAND(ZKP_SRC_REG, 0), 0)};
  std::vector<zkp_air_assertion> asserts{{0, 0, 0, fe(0)}};
  std::vector<zkp_air_strided_assertion> strided{{0, 0, 3, 16, fe(0), nullptr}, {0, 4, 1, 4, fe(0), nullptr}};
  std::vector<zkp_air_binding> binds{{ZKP_BIND_ASSERTION, 0, 1}, {ZKP_BIND_STRIDED, 0, 2}, {ZKP_BIND_STRIDED, 1, 3}};
  uint32_t num_pub = 7;
  int reg(int* id) {
    uint8_t* d = heap(degrees);
    uint64_t* o = heap(ops);
    zkp_air_assertion* a = heap(asserts);
    zkp_air_strided_assertion* s = heap(strided);
    zkp_air_binding* b = heap(binds);
    zkp_air_program p{};
    p.width = 1;
    p.num_constraints = 1;
    p.degrees = d;
    p.num_assertions = (uint32_t)asserts.size();
    p.assertions = a;
    p.num_registers = 1;
    p.num_ops = (uint32_t)ops.size();
    p.ops = o;
    const int rc = zkp_air_register_params(&p, s, (uint32_t)strided.size(), num_pub, b, (uint32_t)binds.size(), id);
    free(d), free(o), free(a), free(s), free(b);
    return rc;
  }
};

static void registration_and_check() {
  int id = 0;
  Counter ok;
  EXPECT(ok.reg(&id) == ZKP_OK);
  // the trace 5, 8, 11, ... over 16 rows; pub = [step, T[0], T[3], T[1], T[5], T[9], T[13]]
  const uint64_t n = 16;
  std::vector<zkp_felt> t(n), pub;
  for (uint64_t r = 0; r < n; r++) t[r] = fe(5 + 3 * r);
  for (uint64_t v : {3ull, 5ull, 14ull, 8ull, 20ull, 32ull, 44ull}) pub.push_back(fe(v));
  uint64_t row;
  uint32_t con, asr;
  auto check = [&](const std::vector<zkp_felt>& pv, const std::vector<zkp_felt>& tv) {
    zkp_felt *pp = heap(pv), *tp = heap(tv);
    const int rc = zkp_air_check_trace_pub(id, pp, pv.size(), tp, 1, n, &row, &con, &asr);
    free(pp), free(tp);
    return rc;
  };
  EXPECT(check(pub, t) == ZKP_OK && row == UINT64_MAX);
  for (size_t i = 0; i < pub.size(); i++) {  // every pub element decides something
    std::vector<zkp_felt> w = pub;
    w[i].lo += 1;
    EXPECT(check(w, t) == ZKP_OK && row != UINT64_MAX);
  }
  std::vector<zkp_felt> shorter(pub.begin(), pub.end() - 1), longer = pub, big = pub;
  longer.push_back(fe(0));
  big[6] = zkp_felt{~0ull, ~0ull};
  EXPECT(check(shorter, t) == ZKP_ERR_PUB_INPUTS);
  EXPECT(check(longer, t) == ZKP_ERR_PUB_INPUTS);
  EXPECT(check(big, t) == ZKP_ERR_PUB_INPUTS);
  EXPECT(check({}, t) == ZKP_ERR_PUB_INPUTS);
  EXPECT(zkp_air_check_trace(id, t.data(), 1, n, &row, &con, &asr) == ZKP_ERR_PUB_INPUTS);
  EXPECT(zkp_air_unregister(id) == ZKP_OK);
  // refusals: each names bindings[i] or ops[pc]
  auto refused = [&](Counter c, const char* field) {
    int rid = -1;
    EXPECT(c.reg(&rid) == ZKP_ERR_ARGUMENT);
    EXPECT(strstr(zkp_air_last_error(), field) != nullptr);
  };
  Counter c;
  c = Counter(); c.num_pub = 0; refused(c, "num_pub");
  c = Counter(); c.num_pub = ZKP_AIR_MAX_PUB + 1; refused(c, "num_pub");
  c = Counter(); c.binds[0].pub_offset = 7; refused(c, "bindings[0]");
  c = Counter(); c.binds[2].pub_offset = 4; refused(c, "bindings[2]");  // 4 values from 4 end at 8
  c = Counter(); c.binds[2].pub_offset = ~0ull; refused(c, "bindings[2]");
  c = Counter(); c.binds[1].index = 2; refused(c, "bindings[1]");
  c = Counter(); c.binds[0].index = 1; refused(c, "bindings[0]");
  c = Counter(); c.binds[1].kind = 2; refused(c, "bindings[1]");
  c = Counter(); c.binds.push_back({ZKP_BIND_STRIDED, 1, 0}); refused(c, "bindings[3]");
  c = Counter(); c.asserts[0].value = fe(1); refused(c, "bindings[0]");
  c = Counter(); c.ops[1] = ZKP_AIR_OP(ZKP_OP_SUB, 0, ZKP_AIR_OPERAND(ZKP_SRC_REG, 0), ZKP_AIR_OPERAND(ZKP_SRC_PUB, 7));
  refused(c, "ops[1]");
  c = Counter(); c.binds.pop_back(); refused(c, "strided[1]");  // an unbound sequence without values
  // limits: the largest pub, a sequence bound at the last legal offset
  c = Counter();
  c.num_pub = ZKP_AIR_MAX_PUB;
  c.binds[2].pub_offset = ZKP_AIR_MAX_PUB - 4;
  EXPECT(c.reg(&id) == ZKP_OK);
  {
    std::vector<zkp_felt> bigpub(ZKP_AIR_MAX_PUB, fe(0));
    bigpub[0] = fe(3);
    bigpub[1] = fe(5);
    bigpub[2] = fe(14);
    for (int i = 0; i < 4; i++) bigpub[ZKP_AIR_MAX_PUB - 4 + i] = fe(8 + 12 * i);
    EXPECT(check(bigpub, t) == ZKP_OK && row == UINT64_MAX);
    bigpub[ZKP_AIR_MAX_PUB - 1].lo += 1;
    EXPECT(check(bigpub, t) == ZKP_OK && row == 13);
  }
  EXPECT(zkp_air_unregister(id) == ZKP_OK);
}

// MiMC with both assertion values from pub, the result as a single / a bound sequence of one
// value / a bound periodic assertion over the stride n
static int mimc_id(uint64_t n, int form) {
  std::vector<uint8_t> degrees{7};
  std::vector<uint32_t> cycles{64};
  std::vector<zkp_felt> k;
  for (uint64_t j = 0; j < 64; j++) k.push_back(fe((j + 1) * 1000000ull));
  const uint64_t R0 = ZKP_AIR_OPERAND(ZKP_SRC_REG, 0), R1 = ZKP_AIR_OPERAND(ZKP_SRC_REG, 1),
                 R2 = ZKP_AIR_OPERAND(ZKP_SRC_REG, 2);
  std::vector<uint64_t> ops{
      ZKP_AIR_OP(ZKP_OP_ADD, 0, ZKP_AIR_OPERAND(ZKP_SRC_CUR, 0), ZKP_AIR_OPERAND(ZKP_SRC_PERIODIC, 0)),  // u
      ZKP_AIR_OP(ZKP_OP_MUL, 1, R0, R0),                                                                 // u^2
      ZKP_AIR_OP(ZKP_OP_MUL, 2, R1, R0),                                                                 // u^3
      ZKP_AIR_OP(ZKP_OP_MUL, 1, R1, R1),                                                                 // u^4
      ZKP_AIR_OP(ZKP_OP_MUL, 1, R1, R2),                                                                 // u^7
      ZKP_AIR_OP(ZKP_OP_SUB, 0, ZKP_AIR_OPERAND(ZKP_SRC_NEXT, 0), R1),
      ZKP_AIR_OP(ZKP_OP_EMIT, 0, R0, 0)};
  std::vector<zkp_air_assertion> asserts{{0, 0, 0, fe(0)}};
  std::vector<zkp_air_strided_assertion> strided;
  std::vector<zkp_air_binding> binds{{ZKP_BIND_ASSERTION, 0, 0}};
  if (form == 0) {
    asserts.push_back({0, 0, n - 1, fe(0)});
    binds.push_back({ZKP_BIND_ASSERTION, 1, 1});
  } else {
    strided.push_back({0, form == 1 ? 1u : 0u, n - 1, n, fe(0), nullptr});
    binds.push_back({ZKP_BIND_STRIDED, 0, 1});
  }
  uint8_t* d = heap(degrees);
  uint32_t* cy = heap(cycles);
  zkp_felt* kv = heap(k);
  uint64_t* o = heap(ops);
  zkp_air_assertion* a = heap(asserts);
  zkp_air_strided_assertion* s = heap(strided);
  zkp_air_binding* b = heap(binds);
  zkp_air_program p{};
  p.width = 1;
  p.num_constraints = 1;
  p.degrees = d;
  p.num_periodic = 1;
  p.periodic_cycles = cy;
  p.periodic_values = kv;
  p.num_assertions = (uint32_t)asserts.size();
  p.assertions = a;
  p.num_registers = 3;
  p.num_ops = (uint32_t)ops.size();
  p.ops = o;
  int id = -1;
  EXPECT(zkp_air_register_params(&p, s, (uint32_t)strided.size(), 2, b, (uint32_t)binds.size(), &id) == ZKP_OK);
  free(d), free(cy), free(kv), free(o), free(a), free(s), free(b);
  return id;
}

int main(int argc, char** argv) {
  registration_and_check();
  long verified = 0;
  for (int ai = 1; ai < argc; ai++) {
    const std::string dir = argv[ai];
    std::vector<uint8_t> proof = slurp(dir + "/proof.bin"), pubb = slurp(dir + "/pub.bin");
    zkp_proof_options o{};
    int air = 0;
    FILE* m = fopen((dir + "/meta.txt").c_str(), "r");
    if (!m || fscanf(m, "%d %u %u %u %u %u %u %u %u", &air, &o.num_queries, &o.blowup_factor, &o.grinding_factor,
                     &o.field_extension, &o.fri_folding_factor, &o.fri_remainder_max_degree,
                     &o.batching_constraints, &o.batching_deep) != 9 || air != ZKP_AIR_MIMC || pubb.size() != 32) {
      fprintf(stderr, "bad MiMC case in %s\n", dir.c_str());
      return 2;
    }
    fclose(m);
    const uint64_t n = 1ull << proof[3];  // the context's log2 of the trace length
    std::vector<zkp_felt> pub(2);
    memcpy(pub.data(), pubb.data(), 32);
    for (int form = 0; form < 3; form++) {
      const int id = mimc_id(n, form);
      auto verify = [&](const std::vector<zkp_felt>& pv, const std::vector<uint8_t>& pr) {
        zkp_felt* pp = heap(pv);
        uint8_t* bp = heap(pr);
        const int rc = zkp_verify((zkp_air_id)id, bp, pr.size(), pp, pv.size(), &o);
        free(pp), free(bp);
        verified++;
        return rc;
      };
      EXPECT(verify(pub, proof) == ZKP_VERIFY_OK);
      EXPECT(verify({pub[0]}, proof) == ZKP_VERIFY_PUB_INPUTS);
      EXPECT(verify({pub[0], pub[1], pub[1]}, proof) == ZKP_VERIFY_PUB_INPUTS);
      EXPECT(verify({pub[0], zkp_felt{~0ull, ~0ull}}, proof) == ZKP_VERIFY_PUB_INPUTS);
      for (int at = 0; at < 2; at++) {
        std::vector<zkp_felt> w = pub;
        w[at].lo ^= 1;
        EXPECT(verify(w, proof) == ZKP_VERIFY_INCONSISTENT_OOD);
      }
      uint64_t rng = 0x9e3779b97f4a7c15ull + form;
      long rejected = 0;
      for (int i = 0; i < 300; i++) {  // bit flips across the proof: parsed without a bad read
        rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
        std::vector<uint8_t> bad = proof;
        bad[rng % bad.size()] ^= (uint8_t)(1u << (rng >> 60 & 7));
        rejected += verify(pub, bad) != ZKP_VERIFY_OK;
      }
      EXPECT(rejected > 280);
      EXPECT(zkp_air_unregister(id) == ZKP_OK);
    }
  }
  printf("checked %ld verifications, %d failures\n", verified, failures);
  return failures ? 1 : 0;
}
