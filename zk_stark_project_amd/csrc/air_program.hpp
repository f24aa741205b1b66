// air_program.hpp — caller-defined AIRs (include/zkp.h, zkp_air_program): the
// validated copy of a constraint program, the process-wide table of registered
// ids, and the host interpreter that the verifier (OOD frame) and
// zkp_air_check_trace (trace rows) share. The device runs the same op stream in
// run_program (kernels.hip). Pure host code: no HIP calls.
#pragma once
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/zkp.h"
#include "felt.hpp"
#include "zkp_internal.hpp"  // op_code, op_dst, op_a, op_b, src_kind, src_index

namespace airp {
using namespace fp;

// a strided assertion (zkp_air_strided_assertion): T[col][first + stride*i] = val (periodic,
// `values` empty) or values[i] (sequence)
struct Strided {
  uint32_t col = 0;
  uint64_t first = 0, stride = 0;
  felt val = {};
  std::vector<felt> values;
  uint32_t nvals = 0;  // a sequence's num_values; `values` is empty while it is bound and not yet instantiated
  int64_t pub = -1;    // zkp_air_register_params: the value(s) are pub[pub ...]; -1 = concrete
  bool sequence() const { return nvals != 0; }
  felt value_at(uint64_t i) const { return values.empty() ? val : values[i]; }
};

// a registered program: the caller's arrays copied, the single assertions sorted by
// (step, column), the strided ones by (stride, first, column)
struct Program {
  std::vector<Strided> strided;
  size_t num_assertions() const { return a_col.size() + strided.size(); }
  uint32_t width = 0, num_t = 0, base_degree = 0, nreg = 0;
  std::vector<uint8_t> degrees;
  std::vector<felt> consts;
  std::vector<std::vector<felt>> periodic;  // column p: its cycle of values
  std::vector<uint32_t> a_col;
  std::vector<uint64_t> a_step;
  std::vector<felt> a_val;
  std::vector<uint64_t> ops;
  // zkp_air_register_params: a_pub[k] = the pub offset of stored single assertion k, or -1.
  // `pub` is empty in the registered program and holds the instance's public inputs in the
  // copy that instantiate() makes, where every bound value is filled in.
  uint32_t num_pub = 0;
  std::vector<int64_t> a_pub;
  std::vector<felt> pub;
  uint32_t max_cycle() const {
    uint32_t m = 0;
    for (auto& c : periodic) m = std::max<uint32_t>(m, (uint32_t)c.size());
    return m;
  }
};

// Checks every rule of zkp_air_program that does not depend on the trace length and
// fills `out`; returns the empty string, or a message naming the failing field.
inline std::string validate(const zkp_air_program* p, Program& out, uint32_t num_pub = 0,
                            std::vector<uint32_t>* single_order = nullptr) {
  auto idx = [](const char* what, size_t i, const std::string& why) {
    return std::string(what) + "[" + std::to_string(i) + "]: " + why;
  };
  if (!p) return "program: null";
  if (p->width < 1 || p->width > 255) return "width: must be 1..255";
  if (p->num_constraints < 1 || p->num_constraints > ZKP_AIR_MAX_CONSTRAINTS) return "num_constraints: must be 1..1024";
  if (!p->degrees) return "degrees: null";
  out.width = p->width;
  out.num_t = p->num_constraints;
  out.base_degree = 0;
  out.degrees.assign(p->degrees, p->degrees + p->num_constraints);
  for (uint32_t i = 0; i < p->num_constraints; i++) {
    if (p->degrees[i] < 1 || p->degrees[i] > ZKP_AIR_MAX_DEGREE) return idx("degrees", i, "must be 1..17");
    out.base_degree = std::max<uint32_t>(out.base_degree, p->degrees[i]);
  }
  if (p->num_constants > ZKP_AIR_MAX_CONSTANTS) return "num_constants: at most 256";
  if (p->num_constants && !p->constants) return "constants: null";
  out.consts.resize(p->num_constants);
  for (uint32_t i = 0; i < p->num_constants; i++) {
    out.consts[i] = make(p->constants[i].lo, p->constants[i].hi);
    if (ge_p(out.consts[i])) return idx("constants", i, "not a canonical field element");
  }
  if (p->num_periodic > ZKP_AIR_MAX_PERIODIC) return "num_periodic: at most 8";
  if (p->num_periodic && (!p->periodic_cycles || !p->periodic_values)) return "periodic_cycles / periodic_values: null";
  out.periodic.resize(p->num_periodic);
  size_t off = 0;
  for (uint32_t c = 0; c < p->num_periodic; c++) {
    const uint32_t cyc = p->periodic_cycles[c];
    if (cyc < 2 || cyc > ZKP_AIR_MAX_CYCLE || (cyc & (cyc - 1)))
      return idx("periodic_cycles", c, "must be a power of two in 2..1024");
    out.periodic[c].resize(cyc);
    for (uint32_t j = 0; j < cyc; j++) {
      const zkp_felt v = p->periodic_values[off + j];
      out.periodic[c][j] = make(v.lo, v.hi);
      if (ge_p(out.periodic[c][j])) return idx("periodic_values", off + j, "not a canonical field element");
    }
    off += cyc;
  }
  if (p->num_assertions > ZKP_AIR_MAX_ASSERTIONS) return "num_assertions: at most 1024";
  if (p->num_assertions && !p->assertions) return "assertions: null";
  {
    std::vector<uint32_t> order(p->num_assertions);
    for (uint32_t i = 0; i < p->num_assertions; i++) {
      order[i] = i;
      const zkp_air_assertion& a = p->assertions[i];
      if (a.column >= p->width) return idx("assertions", i, "column outside the trace width");
      if (ge_p(make(a.value.lo, a.value.hi))) return idx("assertions", i, "value not a canonical field element");
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
      const zkp_air_assertion &a = p->assertions[x], &b = p->assertions[y];
      return a.step != b.step ? a.step < b.step : a.column < b.column;
    });
    uint32_t steps = 0;
    for (uint32_t k = 0; k < p->num_assertions; k++) {
      const zkp_air_assertion& a = p->assertions[order[k]];
      if (k && out.a_step.back() == a.step && out.a_col.back() == a.column)
        return idx("assertions", order[k], "duplicate (column, step)");
      if (!k || out.a_step.back() != a.step) steps++;
      if (steps > ZKP_AIR_MAX_ASSERTION_STEPS) return idx("assertions", order[k], "more than 4 distinct steps");
      out.a_col.push_back(a.column);
      out.a_step.push_back(a.step);
      out.a_val.push_back(make(a.value.lo, a.value.hi));
    }
    out.a_pub.assign(p->num_assertions, -1);
    if (single_order) *single_order = order;  // stored position k holds the caller's assertions[order[k]]
  }
  out.num_pub = num_pub;
  if (p->num_registers < 1 || p->num_registers > ZKP_AIR_MAX_REGISTERS) return "num_registers: must be 1..32";
  if (p->num_ops < 1 || p->num_ops > ZKP_AIR_MAX_OPS) return "num_ops: must be 1..8192";
  if (!p->ops) return "ops: null";
  out.nreg = p->num_registers;
  out.ops.assign(p->ops, p->ops + p->num_ops);
  // the walk: operand ranges, registers written before they are read, the EMIT
  // count, and each constraint's syntactic degree against its declared one
  constexpr uint32_t DEG_CAP = 1u << 16;  // saturation (a chain of squarings doubles it per op)
  uint32_t rdeg[ZKP_AIR_MAX_REGISTERS];
  bool rset[ZKP_AIR_MAX_REGISTERS] = {};
  uint32_t emitted = 0;
  for (uint32_t pc = 0; pc < p->num_ops; pc++) {
    const uint64_t op = p->ops[pc];
    std::string err;
    auto operand = [&](uint32_t o, uint32_t& deg) {
      const uint32_t k = src_kind(o), i = src_index(o);
      deg = 0;
      switch (k) {
        case ZKP_SRC_REG:
          if (i >= p->num_registers) err = "register operand outside num_registers";
          else if (!rset[i]) err = "register read before it is written";
          else deg = rdeg[i];
          break;
        case ZKP_SRC_CUR:
        case ZKP_SRC_NEXT:
          if (i >= p->width) err = "trace column outside the width";
          deg = 1;
          break;
        case ZKP_SRC_PERIODIC:
          if (i >= p->num_periodic) err = "periodic column outside num_periodic";
          break;
        case ZKP_SRC_CONST:
          if (i >= p->num_constants) err = "constant outside num_constants";
          break;
        case ZKP_SRC_PUB:
          if (!num_pub) err = "unknown operand kind";  // the entries without public inputs
          else if (i >= num_pub) err = "public input outside num_pub";
          break;
        default:
          err = "unknown operand kind";
      }
    };
    if (op >> 48) return idx("ops", pc, "bits 48..63 must be zero");
    const uint32_t code = op_code(op);
    uint32_t da = 0, db = 0;
    if (code == ZKP_OP_EMIT) {
      if (op_dst(op) || op_b(op)) return idx("ops", pc, "EMIT takes one operand");
      operand(op_a(op), da);
      if (!err.empty()) return idx("ops", pc, err);
      if (emitted >= p->num_constraints) return idx("ops", pc, "more EMITs than num_constraints");
      if (da > p->degrees[emitted])
        return idx("degrees", emitted, "the constraint's degree in the code (" + std::to_string(da) +
                                           ") exceeds the declared degree");
      emitted++;
      continue;
    }
    if (code != ZKP_OP_ADD && code != ZKP_OP_SUB && code != ZKP_OP_MUL) return idx("ops", pc, "unknown opcode");
    operand(op_a(op), da);
    if (err.empty()) operand(op_b(op), db);
    if (!err.empty()) return idx("ops", pc, err);
    const uint32_t dst = op_dst(op);
    if (dst >= p->num_registers) return idx("ops", pc, "destination register outside num_registers");
    rdeg[dst] = std::min(DEG_CAP, code == ZKP_OP_MUL ? da + db : std::max(da, db));
    rset[dst] = true;
  }
  if (emitted != p->num_constraints) return "ops: fewer EMITs than num_constraints";
  return "";
}

// The strided assertions of zkp_air_register_strided against a program that validate()
// has filled: every rule that does not depend on the trace length. Returns the empty
// string, or a message naming strided[i].
inline std::string validate_strided(const zkp_air_strided_assertion* s, uint32_t count, Program& out,
                                    const std::vector<int64_t>* bound = nullptr) {
  auto idx = [](size_t i, const std::string& why) { return "strided[" + std::to_string(i) + "]: " + why; };
  if (!count) return "";
  if (!s) return "strided: null";
  if ((uint64_t)count + out.a_col.size() > ZKP_AIR_MAX_ASSERTIONS)
    return idx(ZKP_AIR_MAX_ASSERTIONS - out.a_col.size(), "more than 1024 assertions, single and strided together");
  uint64_t seq_values = 0;
  std::vector<uint32_t> order(count);
  for (uint32_t i = 0; i < count; i++) {
    order[i] = i;
    const zkp_air_strided_assertion& a = s[i];
    if (a.stride < 2 || (a.stride & (a.stride - 1))) return idx(i, "stride must be a power of two >= 2");
    if (a.first_step >= a.stride) return idx(i, "first_step must be below the stride");
    if (a.column >= out.width) return idx(i, "column outside the trace width");
    if (a.num_values & (a.num_values - 1)) return idx(i, "num_values must be a power of two");
    if (!a.num_values) {
      if (ge_p(make(a.value.lo, a.value.hi))) return idx(i, "value not a canonical field element");
      continue;
    }
    const bool is_bound = bound && (*bound)[i] >= 0;  // its values come from pub (validate_bindings)
    if (!a.values && !is_bound) return idx(i, "values: null");
    seq_values += a.num_values;
    if (seq_values > ZKP_AIR_MAX_SEQUENCE_VALUES) return idx(i, "more than 2^18 sequence values in the program");
    for (uint32_t j = 0; j < a.num_values && !is_bound; j++)
      if (ge_p(make(a.values[j].lo, a.values[j].hi)))
        return idx(i, "values[" + std::to_string(j) + "] not a canonical field element");
  }
  // two assertions over one cell (independent of the trace length)
  for (uint32_t i = 0; i < count; i++) {
    for (uint32_t j = 0; j < i; j++) {
      const uint64_t m = std::min(s[i].stride, s[j].stride);
      if (s[i].column == s[j].column && (s[i].first_step & (m - 1)) == (s[j].first_step & (m - 1)))
        return idx(i, "overlaps strided[" + std::to_string(j) + "]");
    }
    for (size_t k = 0; k < out.a_col.size(); k++)
      if (out.a_col[k] == s[i].column && (out.a_step[k] & (s[i].stride - 1)) == s[i].first_step)
        return idx(i, "overlaps the single assertion at step " + std::to_string(out.a_step[k]));
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    const zkp_air_strided_assertion &a = s[x], &b = s[y];
    if (a.stride != b.stride) return a.stride < b.stride;
    return a.first_step != b.first_step ? a.first_step < b.first_step : a.column < b.column;
  });
  uint32_t groups = 0;
  for (uint32_t k = 0; k < count; k++) {
    const zkp_air_strided_assertion& a = s[order[k]];
    if (!k || out.strided.back().stride != a.stride || out.strided.back().first != a.first_step) groups++;
    if (groups > ZKP_AIR_MAX_STRIDED_GROUPS) return idx(order[k], "more than 4 distinct (stride, first_step) groups");
    Strided d;
    d.col = a.column;
    d.first = a.first_step;
    d.stride = a.stride;
    d.val = a.num_values ? zero() : make(a.value.lo, a.value.hi);
    d.nvals = a.num_values;
    d.pub = bound ? (*bound)[order[k]] : -1;
    for (uint32_t j = 0; j < a.num_values && d.pub < 0; j++) d.values.push_back(make(a.values[j].lo, a.values[j].hi));
    out.strided.push_back(std::move(d));
  }
  return "";
}

// The bindings of zkp_air_register_params, before the assertions are sorted: every rule of
// include/zkp.h. single[i] / strided[i] receive the pub offset of the caller's assertions[i] /
// strided[i], or -1. Returns the empty string, or a message naming bindings[i].
inline std::string validate_bindings(const zkp_air_program* p, const zkp_air_strided_assertion* s, uint32_t num_strided,
                                     uint32_t num_pub, const zkp_air_binding* b, uint32_t count,
                                     std::vector<int64_t>& single, std::vector<int64_t>& strided) {
  auto idx = [](size_t i, const std::string& why) { return "bindings[" + std::to_string(i) + "]: " + why; };
  single.assign(p->num_assertions, -1);
  strided.assign(num_strided, -1);
  if (count && !b) return "bindings: null";
  if (num_strided && !s) return "strided: null";
  for (uint32_t i = 0; i < count; i++) {
    uint64_t run = 1;
    if (b[i].kind == ZKP_BIND_ASSERTION) {
      if (b[i].index >= p->num_assertions) return idx(i, "index outside the assertions");
      if (single[b[i].index] >= 0) return idx(i, "the assertion is bound twice");
      const zkp_felt v = p->assertions[b[i].index].value;
      if (v.lo | v.hi) return idx(i, "a bound assertion's own value must be zero");
    } else if (b[i].kind == ZKP_BIND_STRIDED) {
      if (b[i].index >= num_strided) return idx(i, "index outside the strided assertions");
      if (strided[b[i].index] >= 0) return idx(i, "the assertion is bound twice");
      const zkp_air_strided_assertion& a = s[b[i].index];
      if (a.value.lo | a.value.hi) return idx(i, "a bound assertion's own value must be zero");
      if (a.values) return idx(i, "a bound sequence's own values must be null");
      if (a.num_values) run = a.num_values;
    } else {
      return idx(i, "unknown kind");
    }
    if (b[i].pub_offset >= num_pub || run > num_pub - b[i].pub_offset)
      return idx(i, "pub_offset (or the sequence's run from it) ends past num_pub");
    (b[i].kind == ZKP_BIND_ASSERTION ? single : strided)[b[i].index] = (int64_t)b[i].pub_offset;
  }
  return "";
}

// The instance of a program with public inputs that `pub` states (num_pub canonical felts,
// checked by the caller): a copy that carries pub and every bound value.
inline std::shared_ptr<const Program> instantiate(const Program& pr, const std::vector<felt>& pub) {
  auto b = std::make_shared<Program>(pr);
  b->pub = pub;
  for (size_t k = 0; k < b->a_pub.size(); k++)
    if (b->a_pub[k] >= 0) b->a_val[k] = pub[b->a_pub[k]];
  for (Strided& s : b->strided) {
    if (s.pub < 0) continue;
    if (s.sequence()) s.values.assign(pub.begin() + s.pub, pub.begin() + s.pub + s.nvals);
    else s.val = pub[s.pub];
  }
  return b;
}

// The program on one frame: out[i] = constraint i (per[p] = periodic column p at the
// frame's point). The canonical field ops of felt.hpp, as on the device.
inline void evaluate(const Program& pr, const felt* cur, const felt* nxt, const felt* per, felt* out) {
  felt reg[ZKP_AIR_MAX_REGISTERS];
  auto fetch = [&](uint32_t o) {
    const uint32_t i = src_index(o);
    switch (src_kind(o)) {
      case ZKP_SRC_REG: return reg[i];
      case ZKP_SRC_CUR: return cur[i];
      case ZKP_SRC_NEXT: return nxt[i];
      case ZKP_SRC_PERIODIC: return per[i];
      case ZKP_SRC_PUB: return pr.pub[i];
      default: return pr.consts[i];
    }
  };
  uint32_t e = 0;
  for (uint64_t op : pr.ops) {
    const felt a = fetch(op_a(op));
    if (op_code(op) == ZKP_OP_EMIT) {
      out[e++] = a;
      continue;
    }
    const felt b = fetch(op_b(op));
    reg[op_dst(op)] = op_code(op) == ZKP_OP_MUL ? mul(a, b) : op_code(op) == ZKP_OP_ADD ? add(a, b) : sub(a, b);
  }
}

// Each constraint's syntactic degree with every periodic operand counted as 1 (validate()
// counts it as 0): ADD / SUB -> max, MUL -> sum, saturated at 255. A product of that many
// trace and periodic columns over n rows has degree at most bound * (n - 1), so the bound
// sizes the domain on which a constraint's actual degree can be measured without aliasing
// (zkp_air_constraint_degrees_device). `pr` has passed validate().
inline std::vector<uint8_t> degree_bounds(const Program& pr) {
  uint32_t rdeg[ZKP_AIR_MAX_REGISTERS] = {};
  auto deg = [&](uint32_t o) -> uint32_t {
    switch (src_kind(o)) {
      case ZKP_SRC_REG: return rdeg[src_index(o)];
      case ZKP_SRC_CUR:
      case ZKP_SRC_NEXT:
      case ZKP_SRC_PERIODIC: return 1;
      default: return 0;
    }
  };
  std::vector<uint8_t> out;
  for (uint64_t op : pr.ops) {
    const uint32_t da = deg(op_a(op));
    if (op_code(op) == ZKP_OP_EMIT) {
      out.push_back((uint8_t)da);
      continue;
    }
    const uint32_t db = deg(op_b(op));
    rdeg[op_dst(op)] = std::min(255u, op_code(op) == ZKP_OP_MUL ? da + db : std::max(da, db));
  }
  return out;
}

// ---- the process-wide table (ids from ZKP_AIR_FIRST_ID, never reused)
struct Registry {
  std::mutex mu;
  std::map<int, std::shared_ptr<const Program>> table;
  int next_id = ZKP_AIR_FIRST_ID;
};
inline Registry& registry() {
  static Registry r;
  return r;
}
inline std::shared_ptr<const Program> lookup(int id) {
  if (id < ZKP_AIR_FIRST_ID) return nullptr;
  Registry& r = registry();
  std::lock_guard<std::mutex> lk(r.mu);
  auto it = r.table.find(id);
  return it == r.table.end() ? nullptr : it->second;
}
inline int insert(std::shared_ptr<const Program> p) {
  Registry& r = registry();
  std::lock_guard<std::mutex> lk(r.mu);
  const int id = r.next_id++;
  r.table[id] = std::move(p);
  return id;
}
inline bool erase(int id) {
  Registry& r = registry();
  std::lock_guard<std::mutex> lk(r.mu);
  return r.table.erase(id) != 0;
}
inline std::string& last_error() {
  static thread_local std::string e;
  return e;
}

}  // namespace airp
