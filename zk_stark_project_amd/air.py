"""AIR descriptions mirrored from the reference (public inputs + metadata).

The constraint arithmetic itself runs on the GPU (csrc/kernels.hip);
these classes carry what `Air::new` / `get_assertions` / `to_elements` carry
in the reference so callers build identical public inputs.
"""
from __future__ import annotations

from dataclasses import dataclass, field

from .field import P
from .helper import AC, FE

AIR_MIMC = 1
AIR_GLOBAL_UPDATE = 2
AIR_TRAINING_UPDATE = 3

D_STATE = AC * FE + AC  # 60 (src/aggregation/air.rs:94)


@dataclass
class Assertion:
    """winterfell `Assertion::single(column, step, value)`."""
    column: int
    step: int
    value: int


# --------------------------------------------------------------------- MiMC
@dataclass
class MimcInputs:
    """Public inputs of the builder-defined MiMC AIR."""
    seed: int
    result: int

    def to_elements(self):
        return [self.seed % P, self.result % P]


class MimcAir:
    """x' = (x + K)^7 with K the 64-cycle periodic column `get_round_constants()`
    (src/helper.rs:213-217, 404-406); assertions at rows 0 and n-1."""
    AIR_ID = AIR_MIMC
    WIDTH = 1
    TRANSITION_DEGREE = 7
    CYCLE = 64

    def __init__(self, trace_length: int, pub_inputs: MimcInputs, options):
        if trace_length < 64 or trace_length & (trace_length - 1):
            raise ValueError("MiMC AIR needs a power-of-two trace length >= 64")
        self.trace_length = trace_length
        self.pub_inputs = pub_inputs
        self.options = options

    def get_assertions(self):
        return [Assertion(0, 0, self.pub_inputs.seed),
                Assertion(0, self.trace_length - 1, self.pub_inputs.result)]


# --------------------------------------------------------------- aggregation
@dataclass
class GlobalUpdateInputs:
    """src/aggregation/air.rs:14-81."""
    global_w: list
    global_b: list
    new_global_w: list
    new_global_b: list
    k: int
    digest: int
    steps: int

    def to_elements(self):
        """air.rs:57-81 — 123 elements; k is element 120."""
        e = []
        for i in range(AC):
            for j in range(FE):
                e.append(self.global_w[i][j])
        for i in range(AC):
            e.append(self.global_b[i])
        for i in range(AC):
            for j in range(FE):
                e.append(self.new_global_w[i][j])
        for i in range(AC):
            e.append(self.new_global_b[i])
        e.append(self.k)
        e.append(self.digest)
        e.append(self.steps % P)
        return e

    def to_bytes(self) -> bytes:
        """`Serializable::write_into` (air.rs:33-55): the same 123 felts, 16 B LE each."""
        return b"".join(int(v).to_bytes(16, "little") for v in self.to_elements())


class GlobalUpdateAir:
    """src/aggregation/air.rs:89-151: width 2d = 120, d = 60 degree-1 transition
    constraints `k*next[i] - k*cur[i] - next[i+d]`, 2d assertions at row steps-1."""
    AIR_ID = AIR_GLOBAL_UPDATE
    WIDTH = 2 * D_STATE
    TRANSITION_DEGREE = 1
    CYCLE = 0

    def __init__(self, trace_length: int, pub_inputs: GlobalUpdateInputs, options):
        self.trace_length = trace_length
        self.pub_inputs = pub_inputs
        self.options = options

    def get_assertions(self):
        final = [self.pub_inputs.new_global_w[i][j] for i in range(AC) for j in range(FE)]
        final += list(self.pub_inputs.new_global_b)
        last = self.pub_inputs.steps - 1
        out = [Assertion(i, last, final[i]) for i in range(D_STATE)]
        out += [Assertion(i, last, 0) for i in range(D_STATE, 2 * D_STATE)]
        return out


# ------------------------------------------------------------------ training
TU_STATE = 2 * (AC * FE + AC)   # 120: flattened [v, s] pairs (src/training/prover.rs:98-103)
TU_WIDTH = 2 * TU_STATE         # 240: masked state || masks


@dataclass
class TrainingUpdateInputs:
    """src/training/air.rs:18-99."""
    initial_masked: list
    final_masked: list
    steps: int
    x_batch: list        # BS x FE
    y_batch: list        # BS x AC
    learning_rate: int
    precision: int
    batch_size: int

    def to_elements(self):
        """air.rs:74-98: initial || final || f64(steps) || f64(bs) || x || y || lr || precision."""
        from .helper import f64_to_felt
        e = list(self.initial_masked) + list(self.final_masked)
        e.append(f64_to_felt(float(self.steps)))
        e.append(f64_to_felt(float(self.batch_size)))
        for row in self.x_batch:
            e.extend(row)
        for row in self.y_batch:
            e.extend(row)
        e.append(self.learning_rate)
        e.append(self.precision)
        return e

    def to_bytes(self) -> bytes:
        """`Serializable::write_into` (air.rs:38-70): the same elements, 16 B LE each."""
        return b"".join(int(v).to_bytes(16, "little") for v in self.to_elements())


class TrainingUpdateAir:
    """src/training/air.rs:101-292: width 240, 240 degree-1 transition constraints
    that evaluate to zero (current_step() == 0), masked state asserted
    at row 0 and row trace_length - 1 (240 assertions)."""
    AIR_ID = AIR_TRAINING_UPDATE
    WIDTH = TU_WIDTH
    TRANSITION_DEGREE = 1
    CYCLE = 0

    def __init__(self, trace_length: int, pub_inputs: TrainingUpdateInputs, options):
        if len(pub_inputs.x_batch) != pub_inputs.batch_size or len(pub_inputs.y_batch) != pub_inputs.batch_size:
            raise ValueError("batch data does not match batch_size in public inputs")  # air.rs:120-123
        self.trace_length = trace_length
        self.pub_inputs = pub_inputs
        self.options = options

    def get_assertions(self):
        half = self.WIDTH // 2
        last = self.trace_length - 1
        out = [Assertion(i, 0, self.pub_inputs.initial_masked[i]) for i in range(half)]
        out += [Assertion(i, last, self.pub_inputs.final_masked[i]) for i in range(half)]
        return out


# ------------------------------------------------------- caller-defined AIRs
# A constraint program (include/zkp.h `zkp_air_program`): the transition constraints
# as a straight-line program of field operations that the device runs at every point
# of the constraint-evaluation domain, periodic columns, and single-row assertions.
OP_ADD, OP_SUB, OP_MUL, OP_EMIT = 0, 1, 2, 3
SRC_REG, SRC_CUR, SRC_NEXT, SRC_PERIODIC, SRC_CONST, SRC_PUB = 0, 1, 2, 3, 4, 5
MAX_REGISTERS, MAX_OPS = 32, 8192
MAX_PUB, MAX_PUB_OPERAND = 1 << 19, 1 << 13


class Expr:
    """A node of an AirProgram's expression graph (`+ - *`, `** k` for small k)."""
    __slots__ = ("prog", "id", "kind", "a", "b")

    def __init__(self, prog, id_, kind, a, b):
        self.prog, self.id, self.kind, self.a, self.b = prog, id_, kind, a, b

    def _other(self, o):
        if isinstance(o, Expr):
            if o.prog is not self.prog:
                raise ValueError("expressions of two different programs")
            return o
        return self.prog.const(o)

    def __add__(self, o):
        return self.prog._op("add", self, self._other(o))

    def __radd__(self, o):
        return self.prog._op("add", self._other(o), self)

    def __sub__(self, o):
        return self.prog._op("sub", self, self._other(o))

    def __rsub__(self, o):
        return self.prog._op("sub", self._other(o), self)

    def __mul__(self, o):
        return self.prog._op("mul", self, self._other(o))

    def __rmul__(self, o):
        return self.prog._op("mul", self._other(o), self)

    def __neg__(self):
        return self.prog._op("sub", self.prog.const(0), self)

    def __pow__(self, k):
        if not isinstance(k, int) or k < 1 or k > 64:
            raise ValueError("power must be an integer in 1..64")
        out, base = None, self
        while k:  # square and multiply
            if k & 1:
                out = base if out is None else out * base
            k >>= 1
            if k:
                base = base * base
        return out


class _Columns:
    def __init__(self, prog, kind):
        self.prog, self.kind = prog, kind

    def __getitem__(self, c):
        c = int(c)
        if not 0 <= c < self.prog.width:
            raise IndexError(f"column {c} outside the trace width {self.prog.width}")
        return self.prog._leaf(self.kind, c)


class CompiledProgram:
    """The op stream of an AirProgram after register allocation."""

    def __init__(self, ops, num_registers):
        self.ops, self.num_registers = ops, num_registers


class RegisteredAir:
    """A registered constraint program: `.AIR_ID` is accepted wherever a built-in id is
    (Context.prove, prove_device, verify, verify_status, Session, Channel,
    prove_by_stages). The id is freed by close() or when the object is collected."""

    def __init__(self, air_id, program):
        self.AIR_ID = air_id
        self.WIDTH = program.width
        self.num_constraints = len(program.constraints)
        self.degrees = [d for _, d in program.constraints]  # the declared degrees
        self.num_assertions = len(program.assertions) + len(program.strided_assertions)
        self.num_coeffs = self.num_constraints + self.num_assertions  # composition coefficients
        self.num_pub = program.num_pub  # 0: concrete values; else every proof's pub has this length

    def __int__(self):
        return self.AIR_ID

    __index__ = __int__

    def check_trace(self, trace, pub=None):
        from . import _native
        return _native.air_check_trace(self.AIR_ID, trace, pub)

    def check_trace_device(self, ctx, d_trace, n):
        """Context.check_trace_device for this id: the trace (WIDTH x n) is in device memory."""
        return ctx.check_trace_device(self.AIR_ID, d_trace, self.WIDTH, n)

    def check_trace_device_pub(self, ctx, pub, d_trace, n):
        """The same for an id with public inputs, against the instance `pub` states."""
        return ctx.check_trace_device_pub(self.AIR_ID, pub, d_trace, self.WIDTH, n)

    def constraint_degrees_device(self, ctx, d_trace, n, pub=None):
        """Context.constraint_degrees_device for this id: the DegreeReport of the trace
        (WIDTH x n, in device memory); `pub` for an id with public inputs."""
        return ctx.constraint_degrees_device(self, d_trace, self.WIDTH, n, pub)

    def degree_bounds(self):
        """zkp_air_degree_bounds: per constraint, the syntactic degree with periodic operands counted as 1."""
        from . import _native
        return _native.air_degree_bounds(self.AIR_ID)

    def close(self):
        if self.AIR_ID is not None:
            from . import _native
            aid, self.AIR_ID = self.AIR_ID, None
            _native.air_unregister(aid)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AirProgram:
    """Builder of a constraint program over a trace of `width` columns.

        p = AirProgram(1)
        K = p.periodic([(j + 1) * 10**6 for j in range(64)])
        p.constraint(p.next[0] - (p.cur[0] + K) ** 7, degree=7)
        p.assertion(0, 0, seed); p.assertion(0, n - 1, result)
        air = p.register()          # air.AIR_ID

    Values are concrete for one instance (what `Air::new` derives from the public
    inputs), or come from each proof's public inputs: `p.pub(i)` is an expression leaf,
    `assertion(col, step, pub=i)`, `periodic_assertion(..., pub=i)` and
    `sequence_assertion(..., pub_offset=o, count=k)` bind assertion values, and the program
    registers once (zkp_air_register_params) for every instance; `num_pub` is the length of
    pub (by default one past the highest index used). bind(pub) gives the concrete program
    of one instance. Equal subexpressions are shared; registers are allocated by a linear scan
    over last uses. evaluate() is a pure-Python evaluation of the same constraints."""

    def __init__(self, width: int):
        self.width = int(width)
        self.cur, self.next = _Columns(self, "cur"), _Columns(self, "next")
        self._nodes = []       # creation order = a topological order
        self._intern = {}
        self.constants = []    # the constant pool
        self._const_index = {}
        self.periodic_columns = []
        self.constraints = []  # (Expr, degree)
        self.assertions = []   # (column, step, value)
        self.strided_assertions = []  # (column, first_step, stride, value | [values])
        self.bound = {}          # index into assertions -> pub index
        self.strided_bound = {}  # index into strided_assertions -> (pub offset, count or None)
        self._num_pub = None     # set_num_pub(); None: one past the highest pub index used
        self._pub_top = 0

    # -- expression nodes
    def _leaf(self, kind, index):
        key = (kind, index)
        if key not in self._intern:
            self._intern[key] = Expr(self, len(self._nodes), kind, index, None)
            self._nodes.append(self._intern[key])
        return self._intern[key]

    def _op(self, kind, a, b):
        if kind in ("add", "mul") and b.id < a.id:
            a, b = b, a  # commutative: one node for x*y and y*x
        key = (kind, a.id, b.id)
        if key not in self._intern:
            self._intern[key] = Expr(self, len(self._nodes), kind, a, b)
            self._nodes.append(self._intern[key])
        return self._intern[key]

    def const(self, v) -> Expr:
        v = int(v) % P
        if v not in self._const_index:
            self._const_index[v] = len(self.constants)
            self.constants.append(v)
        return self._leaf("const", self._const_index[v])

    def _use_pub(self, i, run=1):
        i = int(i)
        if i < 0 or run < 1 or i + run > MAX_PUB:
            raise IndexError(f"public input {i} (run {run}) outside 0..{MAX_PUB}")
        self._pub_top = max(self._pub_top, i + run)
        return i

    def pub(self, i) -> Expr:
        """Public input i of the proof's `pub` (degree 0, like a constant)."""
        i = self._use_pub(i)
        if i >= MAX_PUB_OPERAND:
            raise IndexError(f"a public input used as an operand must have an index below {MAX_PUB_OPERAND}")
        return self._leaf("pub", i)

    def set_num_pub(self, n: int):
        """The length every proof's `pub` must have (pub may be longer than what the program
        reads: the whole of it seeds the coin)."""
        self._num_pub = int(n)

    @property
    def num_pub(self) -> int:
        return self._pub_top if self._num_pub is None else self._num_pub

    def periodic(self, values) -> Expr:
        """A periodic column: `values` repeats along the trace (a power-of-two cycle in 2..1024)."""
        self.periodic_columns.append([int(v) % P for v in values])
        return self._leaf("periodic", len(self.periodic_columns) - 1)

    def constraint(self, expr, degree: int):
        """A transition constraint `expr == 0` on every row but the last; `degree` is its
        declared degree in trace-column factors (TransitionConstraintDegree::new)."""
        if not isinstance(expr, Expr):
            expr = self.const(expr)
        self.constraints.append((expr, int(degree)))

    def assertion(self, column: int, step: int, value: int = None, pub: int = None):
        """`Assertion::single(column, step, value)`; with pub=i the value is pub[i] of each proof."""
        if (value is None) == (pub is None):
            raise ValueError("an assertion takes a value or pub=, not both")
        if pub is not None:
            self.bound[len(self.assertions)] = self._use_pub(pub)
        self.assertions.append((int(column), int(step), 0 if pub is not None else int(value) % P))

    def periodic_assertion(self, column: int, first_step: int, stride: int, value: int = None, pub: int = None):
        """`Assertion::periodic(column, first_step, stride, value)`: the column holds `value` (or
        pub[pub]) at first_step + stride * i for every i < n / stride (stride a power of two >= 2)."""
        if (value is None) == (pub is None):
            raise ValueError("an assertion takes a value or pub=, not both")
        if pub is not None:
            self.strided_bound[len(self.strided_assertions)] = (self._use_pub(pub), None)
        self.strided_assertions.append((int(column), int(first_step), int(stride),
                                        0 if pub is not None else int(value) % P))

    def sequence_assertion(self, column: int, first_step: int, stride: int, values=None, pub_offset: int = None,
                           count: int = None):
        """`Assertion::sequence(column, first_step, stride, values)`: the column holds values[i] at
        first_step + stride * i; len(values) = n / stride, a power of two. With pub_offset=o,
        count=k the values are pub[o .. o + k)."""
        if (values is None) == (pub_offset is None):
            raise ValueError("a sequence takes values or pub_offset= and count=, not both")
        if pub_offset is not None:
            if count is None or int(count) < 1:
                raise ValueError("a bound sequence states count=")
            self.strided_bound[len(self.strided_assertions)] = (self._use_pub(pub_offset, int(count)), int(count))
            self.strided_assertions.append((int(column), int(first_step), int(stride), 0))
            return
        self.strided_assertions.append((int(column), int(first_step), int(stride), [int(v) % P for v in values]))

    def bind(self, pub) -> "AirProgram":
        """The concrete program of the instance `pub`: every pub leaf a constant, every bound
        assertion its value. It registers through the entries without public inputs; a proof
        under it equals, byte for byte, the proof under this program's id with the same pub."""
        pub = [int(v) % P for v in pub]
        if len(pub) != self.num_pub:
            raise ValueError(f"pub has {len(pub)} elements, the program takes {self.num_pub}")
        out = AirProgram(self.width)
        made = {}
        for nd in self._nodes:
            if nd.kind in ("cur", "next"):
                made[nd.id] = out._leaf(nd.kind, nd.a)
            elif nd.kind == "periodic":
                while len(out.periodic_columns) <= nd.a:
                    out.periodic(self.periodic_columns[len(out.periodic_columns)])
                made[nd.id] = out._leaf("periodic", nd.a)
            elif nd.kind == "const":
                made[nd.id] = out.const(self.constants[nd.a])
            elif nd.kind == "pub":
                made[nd.id] = out.const(pub[nd.a])
            else:
                made[nd.id] = out._op(nd.kind, made[nd.a.id], made[nd.b.id])
        while len(out.periodic_columns) < len(self.periodic_columns):
            out.periodic(self.periodic_columns[len(out.periodic_columns)])
        for e, d in self.constraints:
            out.constraint(made[e.id], d)
        for i, (c, s, v) in enumerate(self.assertions):
            out.assertion(c, s, pub[self.bound[i]] if i in self.bound else v)
        for i, (c, f, st, v) in enumerate(self.strided_assertions):
            if i in self.strided_bound:
                o, k = self.strided_bound[i]
                v = pub[o] if k is None else pub[o:o + k]
            if isinstance(v, list):
                out.sequence_assertion(c, f, st, v)
            else:
                out.periodic_assertion(c, f, st, v)
        return out

    def sorted_assertions(self):
        """The single assertions in the order their composition coefficients are drawn: (step, column)."""
        return sorted(self.assertions, key=lambda a: (a[1], a[0]))

    def sorted_strided_assertions(self):
        """The strided assertions in the order their coefficients are drawn, after the singles':
        (stride, first_step, column)."""
        return sorted(self.strided_assertions, key=lambda a: (a[2], a[1], a[0]))

    # -- the spec
    def evaluate(self, cur_row, next_row, row_index: int = 0, periodic=None, pub=None):
        """Every constraint's value on the frame (cur_row, next_row) at trace row `row_index`
        (periodic columns take values[row_index % cycle]); big-int arithmetic mod P. Off the
        trace domain, `periodic` gives the periodic columns' values at the frame's point.
        `pub`: the instance's public inputs, for a program that reads them."""
        per = list(periodic) if periodic is not None else [c[row_index % len(c)] for c in self.periodic_columns]
        return self._evaluate(cur_row, next_row, per, pub)

    def _evaluate(self, cur_row, next_row, per, pub=None):
        val = [0] * len(self._nodes)
        for nd in self._nodes:
            if nd.kind == "cur":
                v = int(cur_row[nd.a])
            elif nd.kind == "next":
                v = int(next_row[nd.a])
            elif nd.kind == "periodic":
                v = per[nd.a]
            elif nd.kind == "const":
                v = self.constants[nd.a]
            elif nd.kind == "pub":
                v = int(pub[nd.a])
            elif nd.kind == "add":
                v = val[nd.a.id] + val[nd.b.id]
            elif nd.kind == "sub":
                v = val[nd.a.id] - val[nd.b.id]
            else:
                v = val[nd.a.id] * val[nd.b.id]
            val[nd.id] = v % P
        return [val[e.id] for e, _ in self.constraints]

    # -- code generation
    def compile(self) -> CompiledProgram:
        """Ops in dependency order, each constraint's EMIT right after its value; registers
        from a linear scan over last uses (a register is free again after its last read)."""
        leaf = {"cur": SRC_CUR, "next": SRC_NEXT, "periodic": SRC_PERIODIC, "const": SRC_CONST, "pub": SRC_PUB}
        code = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL}
        order, placed = [], set()   # ("op", node) / ("emit", node)
        for root, _ in self.constraints:
            stack = [(root, False)]
            while stack:
                nd, done = stack.pop()
                if nd.kind in leaf or nd.id in placed:
                    continue
                if done:
                    placed.add(nd.id)
                    order.append(("op", nd))
                else:
                    stack.append((nd, True))
                    stack.append((nd.b, False))
                    stack.append((nd.a, False))
            order.append(("emit", root))
        last_use = {}
        for i, (what, nd) in enumerate(order):
            for src in ((nd,) if what == "emit" else (nd.a, nd.b)):
                if src.kind not in leaf:
                    last_use[src.id] = i
        free = list(range(MAX_REGISTERS - 1, -1, -1))
        reg, used, ops = {}, 0, []

        def operand(src):
            if src.kind in leaf:
                return (leaf[src.kind] << 13) | src.a
            return (SRC_REG << 13) | reg[src.id]
        for i, (what, nd) in enumerate(order):
            srcs = (nd,) if what == "emit" else (nd.a, nd.b)
            enc = [operand(s) for s in srcs]
            for s in set(x.id for x in srcs if x.kind not in leaf):
                if last_use[s] == i:
                    free.append(reg.pop(s))
            if what == "emit":
                ops.append(OP_EMIT | (enc[0] << 16))
                continue
            if nd.id not in last_use:
                continue  # (unreachable: every placed op feeds an op or an EMIT)
            if not free:
                raise ValueError(f"the program needs more than {MAX_REGISTERS} registers")
            r = free.pop()
            reg[nd.id] = r
            used = max(used, r + 1)
            ops.append(code[nd.kind] | (r << 8) | (enc[0] << 16) | (enc[1] << 32))
        if len(ops) > MAX_OPS:
            raise ValueError(f"the program has {len(ops)} ops, more than {MAX_OPS}")
        return CompiledProgram(ops, max(used, 1))

    def register(self) -> RegisteredAir:
        """zkp_air_register_strided, or zkp_air_register_params for a program that reads public
        inputs: validates the program and returns its id holder."""
        from . import _native
        cp = self.compile()
        bindings = seq_counts = None
        if self.num_pub:
            bindings = [(_native.BIND_ASSERTION, i, o) for i, o in sorted(self.bound.items())]
            bindings += [(_native.BIND_STRIDED, i, o) for i, (o, _) in sorted(self.strided_bound.items())]
            seq_counts = {i: k for i, (_, k) in self.strided_bound.items() if k is not None}
        aid = _native.air_register(self.width, [d for _, d in self.constraints], self.constants,
                                   self.periodic_columns, self.assertions, cp.num_registers, cp.ops,
                                   self.strided_assertions, self.num_pub, bindings, seq_counts)
        return RegisteredAir(aid, self)

    def check_trace(self, trace, pub=None):
        """zkp_air_check_trace on a (width, n, 2) uint64 column-major trace: None when every
        transition and assertion holds, else (row, constraint, assertion). `pub`: the instance,
        for a program that reads public inputs."""
        with self.register() as air:
            return air.check_trace(trace, pub)

    def check_trace_device(self, ctx, trace, pub=None):
        """The same check on the device (Context.check_trace on a host trace)."""
        with self.register() as air:
            return ctx.check_trace_pub(air, pub, trace)

    def constraint_degrees(self, ctx, trace, pub=None):
        """Context.constraint_degrees on a host (width, n, 2) uint64 trace: every constraint's
        actual degree on that trace, as a DegreeReport (registers and frees an id)."""
        with self.register() as air:
            return ctx.constraint_degrees(air, trace, pub)

    def degree_bounds(self):
        """zkp_air_degree_bounds of this program: per constraint, the syntactic degree with every
        periodic operand counted as 1 (host only; registers and frees an id)."""
        with self.register() as air:
            return air.degree_bounds()
