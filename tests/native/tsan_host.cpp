// Host ThreadSanitizer driver (TEST ONLY) for the host-only entries of csrc/verifier.cpp:
// zkp_air_register / _strided / _params, zkp_air_unregister, zkp_air_check_trace / _pub,
// zkp_air_last_error and zkp_verify under built-in and registered ids, called from eight
// threads at once. Built with -fsanitize=thread (host code only) and run on its own.
//
// Every thread has a fixed script of calls (worker()): what it registers, checks, verifies
// and which registration it has refused depend on its thread number and the iteration alone,
// and no status depends on the value of an id (ids are never reused). main() runs the eight
// scripts one after another first, which gives the single-threaded statuses, then all eight
// at once, and compares every status. A data race is ThreadSanitizer's to report (exit 66).
// Usage: tsan_host <mimc_case_dir> <global_update_case_dir>   (proof.bin, pub.bin, meta.txt)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/zkp.h"

static constexpr int THREADS = 8, ITERS = 12;
static constexpr uint64_t ROWS = 16;  // the counter programs' trace length

static std::vector<uint8_t> slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static zkp_felt fe(uint64_t v) { return zkp_felt{v, 0}; }

struct Case {
  int air = 0;
  zkp_proof_options opts{};
  std::vector<uint8_t> proof;
  std::vector<zkp_felt> pub;
  bool load(const std::string& dir, int want_air) {
    proof = slurp(dir + "/proof.bin");
    const std::vector<uint8_t> pubb = slurp(dir + "/pub.bin");
    pub.resize(pubb.size() / 16);
    if (!pubb.empty()) memcpy(pub.data(), pubb.data(), pub.size() * 16);
    FILE* m = fopen((dir + "/meta.txt").c_str(), "r");
    zkp_proof_options& o = opts;
    const bool ok = m && fscanf(m, "%d %u %u %u %u %u %u %u %u", &air, &o.num_queries, &o.blowup_factor,
                                &o.grinding_factor, &o.field_extension, &o.fri_folding_factor,
                                &o.fri_remainder_max_degree, &o.batching_constraints, &o.batching_deep) == 9;
    if (m) fclose(m);
    return ok && air == want_air && !proof.empty();
  }
};

// width 1: next - cur - step = 0 with T[0] = 5. kind 0: step a constant, zkp_air_register;
// kind 1: the same and T[3] as a strided assertion, zkp_air_register_strided; kind 2: step = pub[0],
// T[0] = pub[1] and T[3] = pub[2], zkp_air_register_params.
// `refuse`: 0 = a valid program, else 1 + the index of a field made invalid (REFUSED below).
static const char* const REFUSED[THREADS] = {"width",          "num_registers", "degrees[0]", "constants[0]",
                                             "ops[0]",         "assertions[0]", "strided[0]", "bindings[0]"};
static int register_counter(int kind, uint64_t step, int refuse, int* id) {
  const uint64_t step_src = kind == 2 ? ZKP_AIR_OPERAND(ZKP_SRC_PUB, 0) : ZKP_AIR_OPERAND(ZKP_SRC_CONST, 0);
  uint8_t degrees[1] = {1};
  zkp_felt consts[1] = {fe(step)};
  uint64_t ops[3] = {ZKP_AIR_OP(ZKP_OP_SUB, 0, ZKP_AIR_OPERAND(ZKP_SRC_NEXT, 0), ZKP_AIR_OPERAND(ZKP_SRC_CUR, 0)),
                     ZKP_AIR_OP(ZKP_OP_SUB, 0, ZKP_AIR_OPERAND(ZKP_SRC_REG, 0), step_src),
                     ZKP_AIR_OP(ZKP_OP_EMIT, 0, ZKP_AIR_OPERAND(ZKP_SRC_REG, 0), 0)};
  zkp_air_assertion asserts[1] = {{0, 0, 0, kind == 2 ? fe(0) : fe(5)}};
  zkp_air_strided_assertion strided[1] = {{0, 0, 3, ROWS, kind == 2 ? fe(0) : fe(5 + 3 * step), nullptr}};
  zkp_air_binding binds[2] = {{ZKP_BIND_ASSERTION, 0, 1}, {ZKP_BIND_STRIDED, 0, 2}};
  zkp_air_program p{};
  p.width = 1;
  p.num_constraints = 1;
  p.degrees = degrees;
  p.num_constants = 1;
  p.constants = consts;
  p.num_assertions = 1;
  p.assertions = asserts;
  p.num_registers = 1;
  p.num_ops = 3;
  p.ops = ops;
  switch (refuse) {
    case 1: p.width = 0; break;
    case 2: p.num_registers = 0; break;
    case 3: degrees[0] = 0; break;
    case 4: consts[0] = zkp_felt{~0ull, ~0ull}; break;
    case 5: ops[0] |= 1ull << 50; break;
    case 6: asserts[0].column = 1; break;
    case 7: strided[0].stride = 3; break;   // kind 1 or 2
    case 8: binds[0].index = 1; break;      // kind 2
    default: break;
  }
  if (kind == 0) return zkp_air_register(&p, id);
  if (kind == 1) return zkp_air_register_strided(&p, strided, 1, id);
  return zkp_air_register_params(&p, strided, 1, 3, binds, 2, id);
}

// MiMC (next = (cur + k_j)^7, 64 round constants) for the oracle's proof: kind 0 with the two
// assertion values concrete (zkp_air_register), kind 1 with both from pub (zkp_air_register_params)
static int register_mimc(uint64_t n, const std::vector<zkp_felt>& pub, int kind, int* id) {
  uint8_t degrees[1] = {7};
  uint32_t cycles[1] = {64};
  std::vector<zkp_felt> k;
  for (uint64_t j = 0; j < 64; j++) k.push_back(fe((j + 1) * 1000000ull));
  const uint64_t R0 = ZKP_AIR_OPERAND(ZKP_SRC_REG, 0), R1 = ZKP_AIR_OPERAND(ZKP_SRC_REG, 1),
                 R2 = ZKP_AIR_OPERAND(ZKP_SRC_REG, 2);
  uint64_t ops[7] = {ZKP_AIR_OP(ZKP_OP_ADD, 0, ZKP_AIR_OPERAND(ZKP_SRC_CUR, 0), ZKP_AIR_OPERAND(ZKP_SRC_PERIODIC, 0)),
                     ZKP_AIR_OP(ZKP_OP_MUL, 1, R0, R0),
                     ZKP_AIR_OP(ZKP_OP_MUL, 2, R1, R0),
                     ZKP_AIR_OP(ZKP_OP_MUL, 1, R1, R1),
                     ZKP_AIR_OP(ZKP_OP_MUL, 1, R1, R2),
                     ZKP_AIR_OP(ZKP_OP_SUB, 0, ZKP_AIR_OPERAND(ZKP_SRC_NEXT, 0), R1),
                     ZKP_AIR_OP(ZKP_OP_EMIT, 0, R0, 0)};
  zkp_air_assertion asserts[2] = {{0, 0, 0, kind ? fe(0) : pub[0]}, {0, 0, n - 1, kind ? fe(0) : pub[1]}};
  zkp_air_binding binds[2] = {{ZKP_BIND_ASSERTION, 0, 0}, {ZKP_BIND_ASSERTION, 1, 1}};
  zkp_air_program p{};
  p.width = 1;
  p.num_constraints = 1;
  p.degrees = degrees;
  p.num_periodic = 1;
  p.periodic_cycles = cycles;
  p.periodic_values = k.data();
  p.num_assertions = 2;
  p.assertions = asserts;
  p.num_registers = 3;
  p.num_ops = 7;
  p.ops = ops;
  return kind ? zkp_air_register_params(&p, nullptr, 0, 2, binds, 2, id) : zkp_air_register(&p, id);
}

static std::atomic<long> g_unexpected{0};  // statuses that are known without the single-threaded run
#define EXPECT(cond)                                     \
  do {                                                   \
    if (!(cond)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      g_unexpected++;                                    \
    }                                                    \
  } while (0)

struct Shared {
  Case mimc, gu;
  uint64_t mimc_n = 0;
  int mimc_id = -1;  // registered before the threads start, used by all of them
};

// Thread `tid`'s script. Every status (and every reported row) goes to `log` in call order.
static void worker(const Shared& sh, int tid, std::vector<int64_t>& log) {
  uint64_t rng = 0x9e3779b97f4a7c15ull * (tid + 1);
  auto next = [&] {
    rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
    return rng;
  };
  auto verify = [&](int air, const Case& c, const std::vector<uint8_t>& proof, const std::vector<zkp_felt>& pub) {
    log.push_back(zkp_verify((zkp_air_id)air, proof.data(), proof.size(), pub.data(), pub.size(), &c.opts));
  };
  auto flipped = [&](const Case& c) {
    std::vector<uint8_t> bad = c.proof;
    const uint64_t r = next();
    bad[r % bad.size()] ^= (uint8_t)(1u << (r >> 60 & 7));
    return bad;
  };
  for (int it = 0; it < ITERS; it++) {
    // a distinct program per (thread, iteration), its trace checked valid and with one cell off
    const int kind = (tid + it) % 3;
    const uint64_t step = 1 + 100 * tid + it;
    int id = -1;
    log.push_back(register_counter(kind, step, 0, &id));
    EXPECT(log.back() == ZKP_OK);
    std::vector<zkp_felt> t(ROWS), pub;
    for (uint64_t r = 0; r < ROWS; r++) t[r] = fe(5 + step * r);
    if (kind == 2) pub = {fe(step), fe(5), fe(5 + 3 * step)};
    uint64_t row = 0;
    uint32_t con = 0, asr = 0;
    auto check = [&](const std::vector<zkp_felt>& tv, const std::vector<zkp_felt>& pv) {
      log.push_back(kind == 2 ? zkp_air_check_trace_pub(id, pv.data(), pv.size(), tv.data(), 1, ROWS, &row, &con, &asr)
                              : zkp_air_check_trace(id, tv.data(), 1, ROWS, &row, &con, &asr));
      log.back() = (int64_t)(((uint64_t)log.back() * 1000003u + row) * 1000003u + con * 65537ull + asr);  // one entry per call
    };
    check(t, pub);
    EXPECT(row == UINT64_MAX);
    std::vector<zkp_felt> bad = t;
    bad[1 + (tid + it) % (ROWS - 1)].lo += 1;
    check(bad, pub);
    EXPECT(row != UINT64_MAX);
    if (kind == 2) {
      std::vector<zkp_felt> wrong = pub;
      wrong[2].lo += 1;  // the bound strided value
      check(t, wrong);
      log.push_back(zkp_air_check_trace(id, t.data(), 1, ROWS, &row, &con, &asr));  // the entry without pub
    }
    // a refused registration: this thread's own field is the one named
    const int field = tid % THREADS;
    int rid = -1;
    log.push_back(register_counter(field >= 7 ? 2 : field == 6 ? 1 : kind, step, 1 + field, &rid));
    EXPECT(log.back() == ZKP_ERR_ARGUMENT);
    log.push_back(strstr(zkp_air_last_error(), REFUSED[field]) != nullptr);
    EXPECT(log.back() == 1);
    // the verifier: built-in ids, the shared MiMC id, a MiMC id of this iteration's own
    verify(ZKP_AIR_MIMC, sh.mimc, sh.mimc.proof, sh.mimc.pub);
    verify(ZKP_AIR_MIMC, sh.mimc, flipped(sh.mimc), sh.mimc.pub);
    verify(ZKP_AIR_GLOBAL_UPDATE, sh.gu, sh.gu.proof, sh.gu.pub);
    verify(ZKP_AIR_GLOBAL_UPDATE, sh.gu, flipped(sh.gu), sh.gu.pub);
    verify(sh.mimc_id, sh.mimc, sh.mimc.proof, sh.mimc.pub);
    verify(sh.mimc_id, sh.mimc, flipped(sh.mimc), sh.mimc.pub);
    int own = -1;
    log.push_back(register_mimc(sh.mimc_n, sh.mimc.pub, (tid + it) & 1, &own));
    verify(own, sh.mimc, sh.mimc.proof, sh.mimc.pub);
    EXPECT(log.back() == ZKP_VERIFY_OK);
    verify(own, sh.mimc, flipped(sh.mimc), sh.mimc.pub);
    std::vector<zkp_felt> other = sh.mimc.pub;
    other[1].lo ^= 1;
    verify(own, sh.mimc, sh.mimc.proof, other);
    verify(id, sh.mimc, sh.mimc.proof, sh.mimc.pub);  // the counter's id: another AIR
    log.push_back(zkp_air_unregister(own));
    verify(own, sh.mimc, sh.mimc.proof, sh.mimc.pub);  // freed
    EXPECT(log.back() == ZKP_VERIFY_PUB_INPUTS);
    log.push_back(zkp_air_unregister(id));
    log.push_back(zkp_air_unregister(id));  // twice
    log.push_back(strstr(zkp_air_last_error(), "air_id") != nullptr);
    check(t, pub);  // freed
  }
}

int main(int argc, char** argv) {
  Shared sh;
  if (argc != 3 || !sh.mimc.load(argv[1], ZKP_AIR_MIMC) || !sh.gu.load(argv[2], ZKP_AIR_GLOBAL_UPDATE) ||
      sh.mimc.pub.size() != 2) {
    fprintf(stderr, "usage: tsan_host <mimc_case_dir> <global_update_case_dir>\n");
    return 2;
  }
  sh.mimc_n = 1ull << sh.mimc.proof[3];  // the context's log2 of the trace length
  if (register_mimc(sh.mimc_n, sh.mimc.pub, 0, &sh.mimc_id) != ZKP_OK) {
    fprintf(stderr, "MiMC program refused: %s\n", zkp_air_last_error());
    return 2;
  }
  std::vector<std::vector<int64_t>> want(THREADS), got(THREADS);
  for (int t = 0; t < THREADS; t++) worker(sh, t, want[t]);
  long failures = 0, calls = 0;
  // the single-threaded run itself: the valid proofs verify
  {
    const std::vector<zkp_felt>& pub = sh.mimc.pub;
    if (zkp_verify(ZKP_AIR_MIMC, sh.mimc.proof.data(), sh.mimc.proof.size(), pub.data(), pub.size(), &sh.mimc.opts) ||
        zkp_verify((zkp_air_id)sh.mimc_id, sh.mimc.proof.data(), sh.mimc.proof.size(), pub.data(), pub.size(),
                   &sh.mimc.opts) ||
        zkp_verify(ZKP_AIR_GLOBAL_UPDATE, sh.gu.proof.data(), sh.gu.proof.size(), sh.gu.pub.data(), sh.gu.pub.size(),
                   &sh.gu.opts)) {
      fprintf(stderr, "a valid proof was rejected single-threaded\n");
      failures++;
    }
  }
  std::vector<std::thread> threads;
  for (int t = 0; t < THREADS; t++) threads.emplace_back([&, t] { worker(sh, t, got[t]); });
  for (auto& th : threads) th.join();
  for (int t = 0; t < THREADS; t++) {
    calls += (long)got[t].size();
    if (got[t].size() != want[t].size()) {
      fprintf(stderr, "thread %d: %zu statuses, %zu single-threaded\n", t, got[t].size(), want[t].size());
      failures++;
      continue;
    }
    for (size_t i = 0; i < got[t].size(); i++)
      if (got[t][i] != want[t][i]) {
        fprintf(stderr, "thread %d, status %zu: %lld, single-threaded %lld\n", t, i, (long long)got[t][i],
                (long long)want[t][i]);
        failures++;
      }
  }
  if (zkp_air_unregister(sh.mimc_id) != ZKP_OK) failures++;
  failures += g_unexpected.load();
  printf("checked %ld calls, %ld failures\n", calls, failures);
  return failures ? 1 : 0;
}
