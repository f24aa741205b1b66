"""Programs with public inputs (zkp_air_register_params) shared by test_air_params.py and
test_gpu_air_params.py. The yardstick of both files is the concrete path: for a program P
and a pub vector v, everything under P's one id with pub_elems = v must equal what
P.bind(v), registered through the entries without public inputs, gives with the same v."""
from air_program_cases import power_periodic
from zk_stark_project_amd import AirProgram
from zk_stark_project_amd.field import P

ZKP_ERR_PUB_INPUTS, ZKP_ERR_UNSUPPORTED_AIR, ZKP_ERR_ARGUMENT = 4, 8, 9
VERIFY_PUB_INPUTS, VERIFY_INCONSISTENT_OOD = 35, 36

FORMS = ["a", "b", "both", "emit"]


def pub_power_trace(d, n, c, start=(2, 9)):
    """power_program's trace with a constant added: next0 = cur0^d + P1 + c, next1 = cur1 + cur0 * P2."""
    p1, p2 = power_periodic(n)
    c0, c1 = [start[0] % P], [start[1] % P]
    for r in range(n - 1):
        c0.append((pow(c0[r], d, P) + p1[r % 2] + c) % P)
        c1.append((c1[r] + c0[r] * p2[r % len(p2)]) % P)
    return [c0, c1]


def pub_power_program(d, n, form="b", first=True, concrete_start=False, extra_pub=0):
    """power_program with its constant and assertion values from pub. pub = [c or -c, 0, the five
    asserted values] with the constant's slot first, or the whole layout reversed so that the
    constant is pub[num_pub - 1] (`first` False). `form` is where the PUB operand stands: operand
    a of a SUB, operand b, both operands of a MUL, or the operand of an EMIT. concrete_start
    keeps row 0's two values concrete (one group then mixes them with no bound value; row n/2
    and n-1 stay bound). extra_pub slots that nothing reads follow."""
    num = 7 + extra_pub
    at = (lambda i: i) if first else (lambda i: num - 1 - i)
    p1, p2 = power_periodic(n)
    p = AirProgram(2)
    P1, P2 = p.periodic(p1), p.periodic(p2)
    step = p.cur[0] ** d + P1
    if form == "a":
        p.constraint(p.pub(at(0)) - (step - p.next[0]), degree=d)        # pub[at 0] = -c
    else:
        p.constraint((p.next[0] - step) - p.pub(at(0)), degree=d)        # pub[at 0] = c
    second = p.next[1] - (p.cur[1] + p.cur[0] * P2)
    if form == "both":
        second = second + p.pub(at(1)) * p.pub(at(0))                     # 0 * c
    p.constraint(second, degree=1)
    if form == "emit":
        p.constraint(p.pub(at(1)), degree=1)                              # the constant 0
    cells = [(0, 0), (1, 0), (1, n // 2), (0, n - 1), (1, n - 1)]
    start = pub_power_trace(d, 8, 0)
    for k, (col, row) in enumerate(cells):
        if concrete_start and row == 0:
            p.assertion(col, row, start[col][0])
        else:
            p.assertion(col, row, pub=at(2 + k))
    p.set_num_pub(num)
    return p


def pub_power_instance(p, d, n, c, form="b", first=True):
    """-> (trace columns, pub) of the instance with constant c."""
    cols = pub_power_trace(d, n, c)
    num = p.num_pub
    at = (lambda i: i) if first else (lambda i: num - 1 - i)
    pub = [(31 * i + 5) % P for i in range(num)]  # slots nothing reads still seed the coin
    pub[at(0)] = (-c) % P if form == "a" else c % P
    pub[at(1)] = 0
    for k, (col, row) in enumerate([(0, 0), (1, 0), (1, n // 2), (0, n - 1), (1, n - 1)]):
        pub[at(2 + k)] = cols[col][row]
    return cols, pub


def pub_strided_program(n, seqs, periodic=(), singles=True, num_pub=None):
    """Width 3 over pub_power_trace(3, n, c) plus a third column x2' = 100 - x2 (period 2):
    constant from pub[0], then bound strided assertions. seqs = [(column, first, stride)], each
    a bound sequence of n / stride values; periodic = [(column, first, stride)] bound periodic
    ones (column 2 with an even stride, or stride = n). Values are laid out in pub in that
    order after pub[0]; singles at row 0 on the columns no strided assertion touches there."""
    p1, p2 = power_periodic(n)
    p = AirProgram(3)
    P1, P2 = p.periodic(p1), p.periodic(p2)
    p.constraint((p.next[0] - (p.cur[0] ** 3 + P1)) - p.pub(0), degree=3)
    p.constraint(p.next[1] - (p.cur[1] + p.cur[0] * P2), degree=1)
    p.constraint(p.next[2] - (100 - p.cur[2]), degree=1)
    off = 1
    layout = []
    for col, first, stride in seqs:
        k = n // stride
        p.sequence_assertion(col, first, stride, pub_offset=off, count=k)
        layout.append((col, first, stride, k))
        off += k
    for col, first, stride in periodic:
        p.periodic_assertion(col, first, stride, pub=off)
        layout.append((col, first, stride, 1))
        off += 1
    if singles:
        touched = {(c, f % s) for c, f, s, _ in layout}
        for col in range(3):
            if not any(c == col and f == 0 for c, f in touched):
                p.assertion(col, 0, pub=off)
                layout.append((col, 0, n, 1))
                off += 1
    if num_pub is not None:
        p.set_num_pub(num_pub)
    p.layout = layout
    return p


def pub_strided_instance(p, n, c):
    cols = pub_power_trace(3, n, c)
    c2 = [(4 + c) % P]
    for r in range(n - 1):
        c2.append((100 - c2[r]) % P)
    cols.append(c2)
    pub = [c % P]
    for col, first, stride, k in p.layout:
        pub += [cols[col][first + stride * i] for i in range(k)]
    pub += [(17 * i + 3) % P for i in range(p.num_pub - len(pub))]
    return cols, pub


def training_update_params_program(n, num_pub) -> AirProgram:
    """TrainingUpdate once for every client and round: 240 constant-0 constraints, the masked
    state asserted at row 0 from pub[i] and at row n - 1 from pub[120 + i]; num_pub = the
    full to_elements() length, so the coin seed is the built-in id's."""
    p = AirProgram(240)
    for _ in range(240):
        p.constraint(p.const(0), degree=1)
    for i in range(120):
        p.assertion(i, 0, pub=i)
        p.assertion(i, n - 1, pub=120 + i)
    p.set_num_pub(num_pub)
    return p
