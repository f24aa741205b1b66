// abi.cpp — the context, device-memory, stateless-stage and statistics entry points
// of include/zkp.h (the proofs are in prover.cpp, the sharded ones in
// prover_shard.cpp, the stage sessions in session.cpp).
#include "prover_internal.hpp"

#include <mutex>

using namespace zkpi;

namespace {
// gfx950 check once per device and process (hipGetDeviceProperties queries every
// attribute of the device: milliseconds, paid again by every context otherwise)
bool device_is_gfx950(int device) {
  static std::mutex mu;
  static std::map<int, bool> known;
  std::lock_guard<std::mutex> lk(mu);
  auto it = known.find(device);
  if (it != known.end()) return it->second;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return false;
  const bool ok = strncmp(prop.gcnArchName, "gfx950", 6) == 0;
  known[device] = ok;
  return ok;
}

// a TrainingUpdate state: 60 cells of a (value, sign) pair, half the trace's width
constexpr uint32_t TU_STATE = TU_W / 2;

// zkp_build_training_update_traces, and zkp_build_training_update_trace as its batch of
// one. Every refusal comes before the first upload and names the client in zkp_last_error.
int tu_build(zkp_ctx* ctx, const zkp_training_client* cl, uint32_t K, uint64_t bs, uint64_t n) {
  HIP_CHECK(hipSetDevice(ctx->device));
  ctx->err.clear();
  auto refuse = [&](int code, uint32_t k, const char* what) {
    ctx->err = "client " + std::to_string(k) + ": " + what;
    return code;
  };
  for (uint32_t k = 0; k < K; k++)
    if (!cl[k].initial_state || !cl[k].d_trace_out || (bs && (!cl[k].x_batch || !cl[k].x_sign || !cl[k].y_batch)))
      return refuse(ZKP_ERR_ARGUMENT, k, "null initial_state, d_trace_out or batch pointer");
  if (n < 16 || (n & (n - 1)) || n <= bs || n > (1ull << MAX_LOG_TRACE)) return (int)ZKP_ERR_TRACE_SHAPE;
  auto canon = [](const zkp_felt* v, uint64_t cnt) {
    for (uint64_t i = 0; i < cnt; i++)
      if (ge_p(make(v[i].lo, v[i].hi))) return false;
    return true;
  };
  for (uint32_t k = 0; k < K; k++)
    if (ge_p(make(cl[k].learning_rate.lo, cl[k].learning_rate.hi)) ||
        ge_p(make(cl[k].precision.lo, cl[k].precision.hi)) || !canon(cl[k].initial_state, TU_STATE) ||
        !canon(cl[k].x_batch, bs * TU_FE) || !canon(cl[k].x_sign, bs * TU_FE) || !canon(cl[k].y_batch, bs * TU_AC))
      return refuse(ZKP_ERR_ARGUMENT, k, "a felt >= p");
  const uint64_t out_bytes = (uint64_t)TU_W * n * 16;
  std::vector<std::pair<uintptr_t, uint32_t>> outs(K);
  for (uint32_t k = 0; k < K; k++) outs[k] = {(uintptr_t)cl[k].d_trace_out, k};
  std::sort(outs.begin(), outs.end());
  for (uint32_t i = 1; i < K; i++)
    if (outs[i].first - outs[i - 1].first < out_bytes)
      return refuse(ZKP_ERR_ARGUMENT, std::max(outs[i].second, outs[i - 1].second),
                    "d_trace_out overlaps another client's trace");

  // one packed upload: [descriptors | initial states (K x 120) | batches (K x bs x 24)]
  const uint64_t batch_felts = bs * (2 * TU_FE + TU_AC);
  const size_t off_init = (size_t)K * sizeof(TuClient), off_batch = off_init + (size_t)K * TU_STATE * 16;
  const size_t packed_bytes = off_batch + (size_t)K * batch_felts * 16;
  uint64_t mask_clients = 0;
  for (uint32_t k = 0; k < K; k++) mask_clients += cl[k].masks != nullptr;
  uint64_t* dm = ctx->buf<uint64_t>("tu_masks", mask_clients * n * TU_STATE);
  uint8_t* dp = ctx->buf<uint8_t>("tu_packed", packed_bytes);
  felt* ds = ctx->buf<felt>("tu_states", (size_t)K * (bs + 1) * TU_STATE);
  felt* dfl = ctx->buf<felt>("tu_first_last", (size_t)K * 2 * TU_STATE);
  std::vector<uint8_t> packed(packed_bytes);
  uint64_t mi = 0;
  for (uint32_t k = 0; k < K; k++) {
    const zkp_training_client& c = cl[k];
    TuClient d{};
    d.out = (felt*)c.d_trace_out;
    // divisors of signed.rs div_generic (0 is accepted: winterfell inv(0) = 0)
    d.pr_inv = inv(make(c.precision.lo, c.precision.hi));
    d.lr_inv = inv(make(c.learning_rate.lo, c.learning_rate.hi));
    if (c.masks) {
      d.masks = dm + mi++ * n * TU_STATE;
    } else {
      d.pcg_state = {c.pcg_state[0], c.pcg_state[1]};
      pcg::doubled_pairs({c.pcg_inc[0], c.pcg_inc[1]}, pcg::JUMP_BITS, d.pcg_mul, d.pcg_inc);
    }
    memcpy(packed.data() + k * sizeof(TuClient), &d, sizeof d);
    memcpy(packed.data() + off_init + (size_t)k * TU_STATE * 16, c.initial_state, TU_STATE * 16);
    if (bs) {
      uint8_t* b = packed.data() + off_batch + (size_t)k * batch_felts * 16;  // [x | x_sign | y]
      memcpy(b, c.x_batch, bs * TU_FE * 16);
      memcpy(b + bs * TU_FE * 16, c.x_sign, bs * TU_FE * 16);
      memcpy(b + 2 * bs * TU_FE * 16, c.y_batch, bs * TU_AC * 16);
    }
  }
  ctx->upload(dp, packed.data(), packed_bytes);
  mi = 0;
  for (uint32_t k = 0; k < K; k++)
    if (cl[k].masks) ctx->upload(dm + mi++ * n * TU_STATE, cl[k].masks, n * TU_STATE * 8);
  const TuClient* dcl = (const TuClient*)dp;
  const felt* dinit = (const felt*)(dp + off_init);
  // the unmasked states: rows 1..bs by the chain kernel, which also writes row 0; without
  // samples a client's states are its initial state, where it was uploaded
  if (bs)  // mse_prime divides by f64_to_felt(6.0) (helper.rs:245-269)
    launch_tu_states(ctx->prof, ctx->stream, dcl, K, dinit, (const felt*)(dp + off_batch), ds, (uint32_t)bs,
                     inv(felt_u64(TU_AC * 1000000ull)));
  const felt* states = bs ? ds : dinit;
  launch_tu_write(ctx->prof, ctx->stream, dcl, K, states, bs, n, dfl);
  // what the clients asked back: copied into one pinned block, one synchronisation
  bool want_fl = false, want_raw = false;
  for (uint32_t k = 0; k < K; k++) {
    want_fl |= cl[k].first_last != nullptr;
    want_raw |= cl[k].raw_states != nullptr;
  }
  const size_t fl_bytes = (size_t)K * 2 * TU_STATE * 16, raw_bytes = (size_t)K * (bs + 1) * TU_STATE * 16;
  uint8_t* hp = (uint8_t*)ctx->pinned((want_fl ? fl_bytes : 0) + (want_raw ? raw_bytes : 0));
  uint8_t* hraw = hp + (want_fl ? fl_bytes : 0);
  if (want_fl) HIP_CHECK(hipMemcpyAsync(hp, dfl, fl_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (want_raw) HIP_CHECK(hipMemcpyAsync(hraw, states, raw_bytes, hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  for (uint32_t k = 0; k < K; k++) {
    if (cl[k].first_last) memcpy(cl[k].first_last, hp + (size_t)k * 2 * TU_STATE * 16, 2 * TU_STATE * 16);
    if (cl[k].raw_states)
      memcpy(cl[k].raw_states, hraw + (size_t)k * (bs + 1) * TU_STATE * 16, (bs + 1) * TU_STATE * 16);
  }
  ctx->collect_prof();
  ctx->free_retired();  // buffers a larger batch or trace outgrew (no proof's finish follows)
  return 0;
}
}  // namespace

extern "C" {

int zkp_ctx_create(int device, zkp_ctx** out) {
  if (!out) return ZKP_ERR_ARGUMENT;
  *out = nullptr;
  // phase wall times, kept in the context's statistics as host_ctx_* rows
  using clk = std::chrono::steady_clock;
  auto t = clk::now();
  std::vector<std::pair<const char*, double>> phases;
  auto lap = [&](const char* name) {
    const auto now = clk::now();
    phases.emplace_back(name, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  };
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= device || device < 0) return ZKP_ERR_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKP_ERR_DEVICE;
  if (!device_is_gfx950(device)) return ZKP_ERR_DEVICE;  // code objects are gfx950-only
  lap("host_ctx_device_check");
  zkp_ctx* c = new_ctx(device);
  if (!c) return ZKP_ERR_DEVICE;
  lap("host_ctx_streams");
  // the kernels' code objects, the streams' hardware queues and the pinned staging
  // buffers, ahead of the first proof (a process's first proof was ≈ 4x a warm one)
  preload_kernels_module();
  preload_merkle_module();
  preload_ntt_module();
  lap("host_ctx_code_objects");
  try {
    c->pinned(1u << 20);
    lap("host_ctx_pinned");
    const felt zero[1]{};
    c->upload(c->buf<felt>("ring_warm", 1), zero, 16);
    drain_streams(c);  // this context's streams only (not other contexts' proofs in flight)
    lap("host_ctx_first_copy");
  } catch (const ZkpFail& f) {
    delete c;
    return f.code;
  }
  for (auto& ph : phases) {
    auto& st = c->stats[ph.first];
    st.launches += 1;
    st.ms += ph.second;
  }
  *out = c;
  return ZKP_OK;
}

void zkp_ctx_destroy(zkp_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (zkp_ctx* sc : ctx->session_pool) {  // idle session contexts (stage sessions)
    drain_streams(sc);
    delete sc;
  }
  ctx->session_pool.clear();
  drain_streams(ctx);
  delete ctx;
}

int zkp_ctx_trim(zkp_ctx* ctx) {
  if (!ctx) return ZKP_ERR_ARGUMENT;
  (void)hipSetDevice(ctx->device);
  for (zkp_ctx* sc : ctx->session_pool) {
    drain_streams(sc);
    delete sc;
  }
  ctx->session_pool.clear();
  return ZKP_OK;
}

const char* zkp_last_error(const zkp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void zkp_free(void* p) { free(p); }

int zkp_device_alloc(zkp_ctx* ctx, uint64_t bytes, void** d_ptr) {
  return guarded(ctx, [&] {
    if (!d_ptr) return (int)ZKP_ERR_ARGUMENT;
    HIP_CHECK(hipSetDevice(ctx->device));
    HIP_CHECK(hipMalloc(d_ptr, bytes ? bytes : 16));
    ctx->user_allocs.push_back(*d_ptr);
    return 0;
  });
}

int zkp_device_free(zkp_ctx* ctx, void* d_ptr) {
  return guarded(ctx, [&] {
    auto it = std::find(ctx->user_allocs.begin(), ctx->user_allocs.end(), d_ptr);
    if (it == ctx->user_allocs.end()) return (int)ZKP_ERR_ARGUMENT;
    ctx->user_allocs.erase(it);
    HIP_CHECK(hipFree(d_ptr));
    return 0;
  });
}

int zkp_copy_to_device(zkp_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes) {
  return guarded(ctx, [&] {
    HIP_CHECK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();
    return 0;
  });
}

int zkp_copy_to_host(zkp_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes) {
  return guarded(ctx, [&] {
    ctx->download(h_dst, d_src, bytes);
    return 0;
  });
}

int zkp_trace_lde_commit(zkp_ctx* ctx, const zkp_felt* trace, uint32_t w, uint64_t n, uint32_t blowup,
                         zkp_felt* lde_out, uint8_t root[32]) {
  return guarded(ctx, [&] {
    HIP_CHECK(hipSetDevice(ctx->device));
    if (!trace || !root) return (int)ZKP_ERR_ARGUMENT;
    if (n < 8 || (n & (n - 1)) || w == 0 || w > 255) return (int)ZKP_ERR_TRACE_SHAPE;
    if (blowup < 2 || (blowup & (blowup - 1)) || blowup > 128) return (int)ZKP_ERR_INVALID_OPTIONS;
    uint32_t logn = ilog2(n), logB = ilog2(blowup);
    if (logn + logB > MAX_LOG_DOMAIN) return (int)ZKP_ERR_TRACE_SHAPE;
    uint64_t N = n * blowup;
    felt* d = ctx->buf<felt>("trace_in", (size_t)w * n);
    ctx->upload(d, trace, (size_t)w * n * 16);
    felt* coef = ctx->buf<felt>("coef", (size_t)w * n);
    felt* lde = ctx->buf<felt>("tlde", (size_t)w * N);
    ctx->ensure_coset(logn, logB, 1);
    const uint32_t logN = logn + logB;
    NttBatch ib{d, coef, nullptr, n, n, 1, 1, w};
    launch_ntt(ctx->prof, ctx->stream, ib, logn, false, ctx->itws(logN), logN);
    NttBatch lb{coef, lde, ctx->S(logn, logB), n, n, blowup, blowup, w * blowup};
    launch_ntt(ctx->prof, ctx->stream, lb, logn, true, ctx->tws(logN), logN);
    TreeShard tr;
    commit_rows(ctx, ctx->self_comm(), 0, lde, n, w, logB, logn, false, "ttree", tr, root);
    if (lde_out) {
      std::vector<felt> h((size_t)w * N);
      ctx->download(h.data(), lde, h.size() * 16);
      for (uint32_t c = 0; c < w; c++)
        for (uint64_t i = 0; i < N; i++) {
          felt v = h[((size_t)c * blowup + (i & (blowup - 1))) * n + (i >> logB)];
          lde_out[(size_t)c * N + i].lo = v.lo;
          lde_out[(size_t)c * N + i].hi = v.hi;
        }
    }
    ctx->collect_prof();
    return 0;
  });
}

int zkp_merkle_commit_rows(zkp_ctx* ctx, const zkp_felt* cols, uint32_t w, uint64_t rows, uint8_t root[32]) {
  return guarded(ctx, [&] {
    HIP_CHECK(hipSetDevice(ctx->device));
    if (!cols || !root) return (int)ZKP_ERR_ARGUMENT;
    if (rows < 2 || (rows & (rows - 1)) || w == 0 || w > 255) return (int)ZKP_ERR_TRACE_SHAPE;
    felt* d = ctx->buf<felt>("mrows", (size_t)w * rows);
    ctx->upload(d, cols, (size_t)w * rows * 16);
    uint32_t* tree = ctx->buf<uint32_t>("mtree", (size_t)16 * rows);
    launch_merkle_lde(ctx->prof, ctx->stream, d, w, 0, rows, tree, rows);
    ctx->download(root, tree + 8, 32);
    ctx->collect_prof();
    return 0;
  });
}

int zkp_grind(zkp_ctx* ctx, const uint8_t seed[32], uint32_t bits, uint64_t* nonce) {
  return guarded(ctx, [&] {
    HIP_CHECK(hipSetDevice(ctx->device));
    if (!seed || !nonce || bits > 64) return (int)ZKP_ERR_ARGUMENT;
    uint32_t sw[8];
    for (int i = 0; i < 8; i++)
      sw[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) |
              ((uint32_t)seed[4 * i + 3] << 24);
    // one launch to the minimum nonce (k_grind_all), as zkp_prove's device query tail
    unsigned long long* dres = ctx->buf<unsigned long long>("grind_res", 1);
    uint32_t* dseed = ctx->buf<uint32_t>("grind_seed", 8);
    ctx->upload(dseed, sw, 32);
    HIP_CHECK(hipMemsetAsync(dres, 0xff, 8, ctx->stream));
    // chunks of 2^32 nonces (≈ 40 ms of full-chip BLAKE3 each), the host checking
    // between them, up to 2^40 (≈ 11 s): the first chunk with a hit holds the minimum.
    // bits <= 32 expects 2^bits tries, so the first chunk nearly always ends it
    unsigned long long res = ~0ull;
    for (uint64_t base = 1; base <= (1ull << 40) && res == ~0ull; base += 1ull << 32) {
      launch_grind_all(ctx->prof, ctx->stream, dseed, base, base + (1ull << 32) - 1, bits, dres);
      ctx->download(&res, dres, 8);
    }
    if (res == ~0ull) return (int)ZKP_ERR_NONCE;
    *nonce = res;
    ctx->collect_prof();
    return 0;
  });
}

int zkp_build_global_update_trace(zkp_ctx* ctx, const zkp_felt* raw_global, const zkp_felt* blinding,
                                  const zkp_felt* local_updates, uint64_t ndev, zkp_felt k, uint64_t n,
                                  void* d_trace_out, zkp_felt* final_state) {
  return guarded(ctx, [&] {
    HIP_CHECK(hipSetDevice(ctx->device));
    if (!raw_global || !blinding || !d_trace_out || (ndev && !local_updates)) return (int)ZKP_ERR_ARGUMENT;
    if (n < 8 || (n & (n - 1)) || n < ndev + 2) return (int)ZKP_ERR_TRACE_SHAPE;
    const felt kf = make(k.lo, k.hi);
    if (ge_p(kf)) return (int)ZKP_ERR_PUB_INPUTS;  // k = 0 is accepted: winterfell inv(0) = 0
    auto canon = [](const zkp_felt* v, uint64_t cnt) {
      for (uint64_t i = 0; i < cnt; i++)
        if (ge_p(make(v[i].lo, v[i].hi))) return false;
      return true;
    };
    if (!canon(raw_global, GU_D) || !canon(blinding, GU_D) || !canon(local_updates, ndev * GU_D))
      return (int)ZKP_ERR_ARGUMENT;
    // masked global model (prover.rs:68-79): raw + blinding
    std::vector<felt> hm(2 * GU_D);
    for (uint32_t c = 0; c < GU_D; c++) {
      hm[c] = add(make(raw_global[c].lo, raw_global[c].hi), make(blinding[c].lo, blinding[c].hi));
      hm[GU_D + c] = make(raw_global[c].lo, raw_global[c].hi);
    }
    felt* dm = ctx->buf<felt>("gu_masked_raw", 2 * GU_D);
    ctx->upload(dm, hm.data(), hm.size() * 16);
    felt* dl = ctx->buf<felt>("gu_local", ndev ? ndev * GU_D : 1);
    if (ndev) HIP_CHECK(hipMemcpyAsync(dl, local_updates, ndev * GU_D * 16, hipMemcpyHostToDevice, ctx->stream));
    const uint64_t tiles = (n + 4095) / 4096;
    felt* tb = ctx->buf<felt>("gu_tiles", tiles * GU_D);
    launch_gu_trace(ctx->prof, ctx->stream, dm, dm + GU_D, dl, ndev, inv(kf), n, tb, (felt*)d_trace_out);
    if (final_state)  // row ndev + 1 of the S columns (the state get_pub_inputs reads, prover.rs:168-172)
      HIP_CHECK(hipMemcpy2DAsync(final_state, 16, (const felt*)d_trace_out + ndev + 1, n * 16, 16, GU_D,
                                 hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    ctx->collect_prof();
    return 0;
  });
}

int zkp_build_training_update_trace(zkp_ctx* ctx, const zkp_felt* initial_state, const zkp_felt* x_batch,
                                    const zkp_felt* x_sign, const zkp_felt* y_batch, uint64_t bs,
                                    zkp_felt learning_rate, zkp_felt precision, const uint64_t* masks, uint64_t n,
                                    void* d_trace_out, zkp_felt* first_last, zkp_felt* raw_states) {
  return guarded(ctx, [&] {
    if (!masks) return (int)ZKP_ERR_ARGUMENT;  // this entry takes host masks only
    zkp_training_client c{};
    c.initial_state = initial_state;
    c.x_batch = x_batch;
    c.x_sign = x_sign;
    c.y_batch = y_batch;
    c.learning_rate = learning_rate;
    c.precision = precision;
    c.masks = masks;
    c.d_trace_out = d_trace_out;
    c.first_last = first_last;
    c.raw_states = raw_states;
    return tu_build(ctx, &c, 1, bs, n);
  });
}

int zkp_build_training_update_traces(zkp_ctx* ctx, const zkp_training_client* clients, uint32_t num_clients,
                                     uint64_t bs, uint64_t n) {
  return guarded(ctx, [&] {
    if (!clients || num_clients == 0 || num_clients > ZKP_TU_MAX_CLIENTS) {
      ctx->err = "clients must be non-null and 1.." + std::to_string(ZKP_TU_MAX_CLIENTS) + " in number";
      return (int)ZKP_ERR_ARGUMENT;
    }
    return tu_build(ctx, clients, num_clients, bs, n);
  });
}

int zkp_pcg64_masks(const uint64_t state[2], const uint64_t inc[2], uint64_t first_index, uint64_t count,
                    uint64_t* out) {
  if (!state || !inc || (count && !out)) return ZKP_ERR_ARGUMENT;
  // s_first_index by square-and-multiply over the doubled pairs, made as they are needed
  pcg::u128 s{state[0], state[1]}, a{pcg::MUL_LO, pcg::MUL_HI}, c{inc[0], inc[1]};
  const pcg::u128 step_a = a, step_c = c;
  for (uint64_t k = first_index; k; k >>= 1) {
    if (k & 1) s = pcg::affine(s, a, c);
    c = pcg::mul(c, pcg::add(a, {1, 0}));
    a = pcg::mul(a, a);
  }
  for (uint64_t i = 0; i < count; i++) {
    s = pcg::affine(s, step_a, step_c);
    out[i] = pcg::out(s);
  }
  return ZKP_OK;
}

int zkp_set_profiling(zkp_ctx* ctx, int enabled) {
  return guarded(ctx, [&] {
    ctx->prof.enabled = enabled != 0;
    return 0;
  });
}

int zkp_set_profiling_kernel(zkp_ctx* ctx, const char* kernel_name) {
  return guarded(ctx, [&] {
    ctx->prof.only = kernel_name ? kernel_name : "";
    return 0;
  });
}

int zkp_kernel_stats(zkp_ctx* ctx, const char* kernel_name, uint64_t* launches, double* total_ms) {
  return guarded(ctx, [&] {
    if (!kernel_name || !launches || !total_ms) return (int)ZKP_ERR_ARGUMENT;
    auto it = ctx->stats.find(kernel_name);
    *launches = it == ctx->stats.end() ? 0 : it->second.launches;
    *total_ms = it == ctx->stats.end() ? 0.0 : it->second.ms;
    return 0;
  });
}

int zkp_reset_stats(zkp_ctx* ctx) {
  return guarded(ctx, [&] {
    ctx->stats.clear();
    return 0;
  });
}

int zkp_kernel_stats_table(zkp_ctx* ctx, char** table) {
  return guarded(ctx, [&] {
    if (!table) return (int)ZKP_ERR_ARGUMENT;
    std::string s;
    char line[256];
    for (auto& kv : ctx->stats) {
      snprintf(line, sizeof line, "%s %llu %.6f %.0f\n", kv.first.c_str(), (unsigned long long)kv.second.launches,
               kv.second.ms, kv.second.bytes);
      s += line;
    }
    *table = (char*)malloc(s.size() + 1);
    memcpy(*table, s.c_str(), s.size() + 1);
    return 0;
  });
}

// zkp_air_check_trace on a trace in device memory (k_check_program). Every status is
// decided on the host, in zkp_air_check_trace's order, before the first HIP call.
int zkp_air_check_trace_device(zkp_ctx* ctx, int air_id, const void* d_trace_cols, uint32_t width, uint64_t n,
                               uint64_t* bad_row, uint32_t* bad_constraint, uint32_t* bad_assertion) {
  return zkp_air_check_trace_device_pub(ctx, air_id, nullptr, 0, d_trace_cols, width, n, bad_row, bad_constraint,
                                        bad_assertion);
}

// With public inputs (zkp_air_register_params) the cached image holds no value of pub: the
// pub table and the singles' values go up per call, and a bound strided assertion's cells
// read the pub table (ProgStridedCells::pub1).
int zkp_air_check_trace_device_pub(zkp_ctx* ctx, int air_id, const zkp_felt* pub_elems, uint64_t n_pub,
                                   const void* d_trace_cols, uint32_t width, uint64_t n, uint64_t* bad_row,
                                   uint32_t* bad_constraint, uint32_t* bad_assertion) {
  if (!ctx || !d_trace_cols || !bad_row || !bad_constraint || !bad_assertion || (n_pub && !pub_elems))
    return ZKP_ERR_ARGUMENT;
  return guarded(ctx, [&] {
    if (air_id == ZKP_AIR_MIMC || air_id == ZKP_AIR_GLOBAL_UPDATE || air_id == ZKP_AIR_TRAINING_UPDATE)
      return (int)ZKP_ERR_UNSUPPORTED_AIR;
    if (n < 8 || (n & (n - 1)) || width == 0 || width > 255) return (int)ZKP_ERR_TRACE_SHAPE;
    AirDesc air;
    std::vector<felt> pub(n_pub);
    for (uint64_t i = 0; i < n_pub; i++) pub[i] = make(pub_elems[i].lo, pub_elems[i].hi);
    const int rc = build_air(air, air_id, width, n, pub);
    if (rc) return rc;
    if (!air.prog->num_pub && n_pub) return (int)ZKP_ERR_PUB_INPUTS;
    if (n > (1ull << MAX_LOG_TRACE)) return (int)ZKP_ERR_TRACE_SHAPE;  // the result key holds 23 bits of row
    const airp::Program& pr = *air.prog;
    HIP_CHECK(hipSetDevice(ctx->device));
    // the check's device image, in 16-byte units: the code sections (ProgCodeLayout) with the
    // raw periodic values, then [assertion columns | assertion steps | assertion values]. It
    // depends on the program alone; a context keeps the last id's (ids are never reused).
    const ProgCodeLayout lay(pr, 1);
    const size_t A = pr.a_col.size(), o_col = lay.end();
    // Strided assertions append [cell descriptors (3 units each) | sequence values]; their
    // cell counts and block runs depend on n, so the tag carries it too.
    static_assert(sizeof(ProgStridedCells) == 48, "three 16-byte units");
    const std::vector<airp::Strided>& sv = pr.strided;
    const size_t S = sv.size();
    size_t seq_felts = 0;
    for (const airp::Strided& a : sv) seq_felts += a.pub < 0 ? a.values.size() : 0;  // bound ones are read from pub
    const size_t o_step = o_col + (A + 3) / 4, o_val = o_step + (A + 3) / 4, o_sdesc = o_val + A,
                 o_svals = o_sdesc + 3 * S, total = o_svals + seq_felts;
    uint64_t strided_blocks = 0;
    for (const airp::Strided& a : sv) strided_blocks += (n / a.stride + 63) / 64;
    felt* dimg = ctx->buf<felt>("check_image", total);
    std::vector<felt>& tag = ctx->host_cache["check_image_tag"];
    const felt want = make((uint64_t)air_id | (S ? n << 32 : 0), total);
    if (tag.size() != 1 || !eq(tag[0], want)) {
      tag.clear();
      std::vector<felt> img(total, zero());
      lay.write(img.data());
      for (size_t p = 0; p < pr.periodic.size(); p++)
        memcpy(img.data() + lay.tab[p], pr.periodic[p].data(), pr.periodic[p].size() * 16);
      uint32_t* steps = reinterpret_cast<uint32_t*>(img.data() + o_step);
      for (size_t k = 0; k < A; k++) steps[k] = (uint32_t)pr.a_step[k];  // < n <= 2^23 (build_air)
      if (A) {
        memcpy(img.data() + o_col, pr.a_col.data(), A * 4);
        if (!pr.num_pub) memcpy(img.data() + o_val, pr.a_val.data(), A * 16);
      }
      ProgStridedCells* cells = reinterpret_cast<ProgStridedCells*>(img.data() + o_sdesc);
      uint32_t blk = 0, voff = 0;
      for (size_t j = 0; j < S; j++) {
        const uint32_t count = (uint32_t)(n / sv[j].stride);
        const bool bound = sv[j].pub >= 0;
        cells[j] = ProgStridedCells{sv[j].col, (uint32_t)sv[j].first, (uint32_t)sv[j].stride, count, blk,
                                    sv[j].sequence() ? voff : 0xffffffffu, bound ? (uint32_t)sv[j].pub + 1 : 0, 0,
                                    bound ? zero() : sv[j].val};
        if (sv[j].sequence() && !bound) {
          memcpy(img.data() + o_svals + voff, sv[j].values.data(), (size_t)count * 16);
          voff += count;
        }
        blk += (count + 63) / 64;
      }
      // singles alone: at most 224 KiB, staged in the pinned ring. Sequence values can take it
      // past the ring's 1 MiB (upload() then copies from `img` itself), so wait for that copy
      ctx->upload(dimg, img.data(), total * 16);
      if (total * 16 > (1u << 20)) ctx->sync();
      tag.assign(1, want);
    }
    ProgCheckArgs ca{};
    ca.code = lay.code(dimg);
    ca.nassert = (uint32_t)A;
    ca.a_col = reinterpret_cast<const uint32_t*>(dimg + o_col);
    ca.a_step = reinterpret_cast<const uint32_t*>(dimg + o_step);
    ca.a_val = dimg + o_val;
    if (pr.num_pub) {
      // the instance's values: the pub table (larger than the ring's 1 MiB it is copied from
      // `pr.pub`, which lives until the download below has synchronised) and the singles' values
      felt* dpub = ctx->buf<felt>("check_pub", pr.num_pub);
      ctx->upload(dpub, pr.pub.data(), (size_t)pr.num_pub * 16);
      ca.code.pub = dpub;
      felt* dval = ctx->buf<felt>("check_aval", A);
      if (A) ctx->upload(dval, pr.a_val.data(), A * 16);
      ca.a_val = dval;
    }
    ca.n = n;
    ca.nstrided = (uint32_t)S;
    ca.sdesc = reinterpret_cast<const ProgStridedCells*>(dimg + o_sdesc);
    ca.svals = dimg + o_svals;
    unsigned long long* dres = ctx->buf<unsigned long long>("check_result", 2);
    HIP_CHECK(hipMemsetAsync(dres, 0xff, 16, ctx->stream));
    launch_check_program(ctx->prof, ctx->stream, ca, width, (const felt*)d_trace_cols, dres, strided_blocks);
    unsigned long long res[2];
    ctx->download(res, dres, 16);  // the call's one stream synchronise
    ctx->collect_prof();
    ctx->free_retired();
    // the host check's precedence: a failing transition wins over any assertion
    *bad_row = UINT64_MAX;
    *bad_constraint = UINT32_MAX;
    *bad_assertion = UINT32_MAX;
    if (res[0] != ~0ull) {
      *bad_row = res[0] >> 10;
      *bad_constraint = (uint32_t)(res[0] & 1023);
    } else if (res[1] != ~0ull) {
      *bad_row = res[1] & 0xffffffffull;
      *bad_assertion = (uint32_t)(res[1] >> 32);
    }
    return 0;
  });
}

// Each transition constraint's actual degree on a trace in device memory (include/zkp.h).
// Every refusal is degrees_plan's (host_stark.hpp) or the capacity check, before the first
// HIP call. Every buffer is this entry's own ("deg_*"); the domain tables it shares with
// proofs (twiddles, S, Si) depend on the shape alone and are only ever filled with the same values.
int zkp_air_constraint_degrees_device(zkp_ctx* ctx, int air_id, const zkp_felt* pub_elems, uint64_t n_pub,
                                      const void* d_trace_cols, uint32_t width, uint64_t n, uint64_t* degrees,
                                      uint32_t capacity, zkp_air_degree_report* report) {
  return guarded(ctx, [&] {  // a null ctx returns ZKP_ERR_ARGUMENT there
    if (!d_trace_cols || !degrees || !report || (n_pub && !pub_elems)) {
      ctx->err = "d_trace_cols, degrees, report or (with n_pub set) pub_elems: null";
      return (int)ZKP_ERR_ARGUMENT;
    }
    DegreesPlan pl;
    const int rc = degrees_plan(air_id, pub_elems, n_pub, width, n, pl, ctx->err);
    if (rc) return rc;
    const airp::Program& pr = *pl.air.prog;
    if (capacity < pr.num_t) {
      ctx->err = "capacity: below num_constraints (" + std::to_string(pr.num_t) + ")";
      return (int)ZKP_ERR_ARGUMENT;
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    const uint32_t E = pl.E, logE = ilog2(E), logn = ilog2(n), logN = logn + logE;
    const uint64_t M = n * E;
    ctx->ensure_coset(logn, logE, logE);
    // the image: the code sections with each periodic column over the E*n domain (as the
    // evaluation image's at scale ce); a context keeps the last (id, n, E)'s
    const ProgCodeLayout lay(pr, E);
    const size_t total = lay.end();
    felt* dimg = ctx->buf<felt>("deg_image", total);
    std::vector<felt>& tag = ctx->host_cache["deg_image_tag"];
    const felt want[2] = {make((uint64_t)air_id, logn), make(logE, total)};
    if (tag.size() != 2 || !eq(tag[0], want[0]) || !eq(tag[1], want[1])) {
      tag.clear();
      std::vector<felt> img(total, zero());
      lay.write(img.data());
      const felt g = felt_u64(3);
      for (size_t p = 0; p < pr.periodic.size(); p++) {
        const size_t cyc = pr.periodic[p].size();
        std::vector<felt> kc = pr.periodic[p];
        host_interpolate(kc, one());
        const std::vector<felt> kv = host_evaluate(kc, cyc * E, pow_u64(g, n / cyc));
        memcpy(img.data() + lay.tab[p], kv.data(), kv.size() * 16);
      }
      ctx->upload(dimg, img.data(), total * 16);
      if (total * 16 > (1u << 20)) ctx->sync();  // past the ring's size the copy reads `img` itself
      tag.assign(want, want + 2);
    }
    ProgCode code = lay.code(dimg);
    if (pr.num_pub) {  // the instance's pub table (pr.pub lives until the download below has synchronised)
      felt* dpub = ctx->buf<felt>("deg_pub", pr.num_pub);
      ctx->upload(dpub, pr.pub.data(), (size_t)pr.num_pub * 16);
      code.pub = dpub;
    }
    // 1. the columns' coefficients, then their values on the E cosets g w_N^j <w_n> (the trace LDE's route)
    felt* coef = ctx->buf<felt>("deg_coef", (size_t)width * n);
    felt* ext = ctx->buf<felt>("deg_ext", (size_t)width * M);
    NttBatch ib{(const felt*)d_trace_cols, coef, nullptr, n, n, 1, 1, width};
    launch_ntt(ctx->prof, ctx->stream, ib, logn, false, ctx->itws(logN), logN);
    NttBatch lb{coef, ext, ctx->S(logn, logE), n, n, E, E, width * E};
    launch_ntt(ctx->prof, ctx->stream, lb, logn, true, ctx->tws(logN), logN);
    // the cross-coset DFT's constants, all E segments kept (shape-only)
    const std::string dkey = "deg_dft_" + std::to_string(logn) + "_" + std::to_string(logE);
    felt* dcoefs = ctx->buf<felt>(dkey + "_coefs", (size_t)E + E / 2);
    uint32_t* dblk = ctx->buf<uint32_t>(dkey + "_blk", E);
    if (!ctx->have_cached(dkey)) {
      const std::vector<felt> dc = comp_dft_consts(n, logE, E);
      std::vector<uint32_t> blk(E);
      for (uint32_t u = 0; u < E; u++) blk[u] = u;
      ctx->upload(dcoefs, dc.data(), dc.size() * 16);
      ctx->upload(dblk, blk.data(), blk.size() * 4);
    }
    const uint32_t K = std::min(pl.K, pr.num_t);
    felt* vals = ctx->buf<felt>("deg_vals", (size_t)K * M);
    felt* cf = ctx->buf<felt>("deg_coefs", (size_t)K * M);
    long long* ddeg = ctx->buf<long long>("deg_result", pr.num_t);
    HIP_CHECK(hipMemsetAsync(ddeg, 0xff, (size_t)pr.num_t * 8, ctx->stream));
    for (uint32_t i0 = 0; i0 < pr.num_t; i0 += K) {
      const uint32_t k = std::min(K, pr.num_t - i0);
      // 2. the chunk's raw constraint values; 3. each one's coefficients by the composition's
      // route: per-coset inverse NTTs (in place), then the E-point DFT with its twists per column
      launch_program_columns(ctx->prof, ctx->stream, code, ext, width, logn, logE, i0, k, vals);
      NttBatch cb{vals, vals, nullptr, n, n, 1, 1, k * E};
      launch_ntt(ctx->prof, ctx->stream, cb, logn, false, ctx->itws(logN), logN);
      for (uint32_t c = 0; c < k; c++)
        launch_comp_dft(ctx->prof, ctx->stream, vals + (size_t)c * M, dblk, ctx->Si(logn, logE, logE), dcoefs, E, E,
                        logn, 0, n, cf + (size_t)c * M);
      // 4. the top non-zero coefficient of each
      launch_column_degrees(ctx->prof, ctx->stream, cf, logn, logE, k, ddeg + i0);
    }
    std::vector<uint64_t> h(pr.num_t);
    ctx->download(h.data(), ddeg, (size_t)pr.num_t * 8);  // the call's one stream synchronise
    ctx->collect_prof();
    ctx->free_retired();
    zkp_air_degree_report r{};
    r.num_constraints = pr.num_t;
    r.eval_blowup = E;
    r.columns = pl.air.comp_cols();
    r.max_degree = ZKP_DEGREE_ZERO;
    r.first_under = UINT32_MAX;
    for (uint32_t i = 0; i < pr.num_t; i++) {
      degrees[i] = h[i];
      if (h[i] == ZKP_DEGREE_ZERO) continue;
      if (r.max_degree == ZKP_DEGREE_ZERO || h[i] > r.max_degree) r.max_degree = h[i];
      if (r.first_under == UINT32_MAX && h[i] > (uint64_t)pr.degrees[i] * (n - 1)) r.first_under = i;
    }
    r.columns_needed = 1;
    r.proof_fits = 1;
    if (r.max_degree != ZKP_DEGREE_ZERO) {
      // the quotient by the transition divisor (degree n - 1) has max_degree - (n - 1) + 1 coefficients
      if (r.max_degree + 2 > n) r.columns_needed = (uint32_t)((r.max_degree + 2 - n + n - 1) / n);
      if (r.columns_needed < 1) r.columns_needed = 1;
      r.proof_fits = r.max_degree <= ((uint64_t)r.columns + 1) * n - 2;
    }
    *report = r;
    return 0;
  });
}

// Host-side MiMC AIR trace builder (trace construction, like TraceTable building
// in the reference; not part of the proving hot path).
int zkp_build_mimc_trace(const uint8_t seed[16], uint64_t n, zkp_felt* out) {
  if (!seed || !out || n == 0) return ZKP_ERR_ARGUMENT;
  felt v = from_u128_bytes(seed);
  if (ge_p(v)) v = sub(v, make(P_LO, P_HI));
  for (uint64_t i = 0; i < n; i++) {
    out[i].lo = v.lo;
    out[i].hi = v.hi;
    felt u = add(v, felt_u64((i % 64 + 1) * 1000000ull));
    felt u2 = sqr(u), u3 = mul(u2, u), u6 = sqr(u3);
    v = mul(u6, u);
  }
  return 0;
}

}  // extern "C"
