"""The fold-by-16 IDENTITY machine, written a second time -- the first is zktls_amd/csrc/fri16_chip.hip (the machine and its key) and fri16_rows.cuh
(fri16_identity_rows_kernel, the traces of AIR16 and SCALARS16).  It is the head machine of tests/fri16_head_air.py with the AIR identity at zeta inside.
Written from docs/PROTOCOL.md and step (a) of the shard verifier for a version-3 proof without lookup pairs (tests/pyverify.py checks the same identity).

Statement (the public values are the inner proof's own; the key holds what the head machine's key holds): everything the head machine states, and with G = W / 4
groups a, b, c, d = loc[4 g .. 4 g + 3], dn = nxt[4 g + 3]:
    c1 = c - a^2 b - (g + 1),   c2 = sel_trans (dn - a b - c - (2 g + 3)),   c3 = sel_first (d - (5 g + 7)),   acc <- ((acc alpha + c1) alpha + c2) alpha + c3 from 0
    sel_trans = zeta - 1 / g_N,   sel_first = (zeta^N - 1) / (zeta - 1),   zeta^N by n = H - b squarings
    quot = sum_{k < 2} (a_k zeta^N + b_k) sum_e X^e opq[4 k + e],   acc = quot (zeta^N - 1)
where alpha, zeta and the opened values are the ones the transcript chain draws and absorbs.  STILL OUTSIDE: lookups, version-7 and version-8 inner proofs, roots
leaving the key, the wiring into the shard verifier.

Thirteen tables: the head machine's eleven by its numbers, 11 AIR16, 12 SCALARS16.  Changed among the eleven: P2TH's interaction table (one more send, alpha from
row A - 1, multiplicity in preprocessed column 61; in the key zeta's multiplicity is 2), OPENED16's preprocessed width (12: H0 at 8, H1 at 9, the multiplicities of
two more sends that carry the row's two halves under its row number) and with it its program's and table's column numbers, and the table count.
11 AIR16      preprocessed ACT FIRST NOTFIRST LAST K1 K2 K3 KL0 KL1 KN1 0 0; main A B C D DN ALPHA SELT SELF A2 AB ACCIN U1 U2 ACCO, four columns each
12 SCALARS16  preprocessed FIRST KQ[4] 0 0 0; main ALPHA ZETA ZP_1 .. ZP_n INVF SELF SELT QZ_0 .. QZ_7 QK0 QK1 QUO ACC; 2^7 rows, every row the first"""
import types

import numpy as np

import fri16_air as A
import fri16_head_air as HA
import fri16_transcript_air as TA
import oracle_lib as O
import pyref
import recursion_air as RA
from recursion_air import ev, eb, eadd, esub, emul, egate, ec, escale, pv

P = O.P
V = O.air_var
AIR16, SCALARS16 = 11, 12
NAMES = HA.NAMES + ["AIR16", "SCALARS16"]
CHANGED = [HA.P2TH, HA.OPENED16]                                                # among the head's eleven: the interaction tables of both, OPENED16's widths
BUS_OH0, BUS_OH1, BUS_ALPHA, BUS_KA, BUS_KSELT, BUS_KSELF, BUS_ACC = range(94, 101)
PH_AM, OPN_PRE, OQ_H0, OQ_H1 = 61, 12, 8, 9
AIR_PRE, AP_ACT, AP_FIRST, AP_NOTFIRST, AP_LAST, AP_K1, AP_K2, AP_K3, AP_KL0, AP_KL1, AP_KN1 = 12, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
AIR_COLS = ["A", "B", "C", "D", "DN", "ALPHA", "SELT", "SELF", "A2", "AB", "ACCIN", "U1", "U2", "ACCO"]
AI = {name: 4 * i for i, name in enumerate(AIR_COLS)}
AIR_MAIN = 4 * len(AIR_COLS)
SC_PRE, SP_FIRST, SP_KQ, SC_LOG_ROWS = 8, 0, 1, 7
ZETA_RECEIVERS = 2                                                              # QUERY16H and SCALARS16


def scalars_cols(n):
    """SCALARS16's main columns -> ({name: first of its four columns}, width)"""
    names = ["ALPHA", "ZETA"] + ["ZP%d" % i for i in range(1, n + 1)] + ["INVF", "SELF", "SELT"] + ["QZ%d" % j for j in range(8)] + ["QK0", "QK1", "QUO", "ACC"]
    return {name: 4 * i for i, name in enumerate(names)}, 4 * len(names)


def log_rows(R, F, b, Q, W, NP):
    return HA.log_rows(R, F, b, Q, W, NP) + [A.lg(W // 4, 6), SC_LOG_ROWS]


def shape_ok(R, F, b, Q, pow_bits, W, NP):
    """the head machine's inner proofs, but the shapes at which nine of the thirteen tables would have one height"""
    if not HA.OA.shape_ok(R, F, b, Q, pow_bits, W) or not 1 <= NP <= HA.MAX_NP:
        return False
    lr = log_rows(R, F, b, Q, W, NP)
    return max(lr.count(h) for h in lr) <= HA.MAX_SAME_HEIGHT


def order(R, F, b, Q, W, NP):
    lr = log_rows(R, F, b, Q, W, NP)
    return sorted(range(13), key=lambda i: (-lr[i], i))


def main_widths(lf, n):
    return HA.main_widths(lf) + [AIR_MAIN, scalars_cols(n)[1]]


PRE_WIDTHS = HA.PRE_WIDTHS[:HA.OPENED16] + [OPN_PRE, AIR_PRE, SC_PRE]


# ---------------------------------------------------------------- programs
def _ext(out, name, sel, e):
    for c in range(4):
        out.append((name, sel, e[c]))


def air16_constraints():
    M0, ALL, TRANS = AIR_PRE, O.SEL_ALL, O.SEL_TRANSITION
    e = lambda name, nxt=False: ev(M0 + AI[name], nxt)
    first, nf = pv(AP_FIRST), pv(AP_NOTFIRST, True)
    out = []
    for name in ("ALPHA", "SELT", "SELF"):
        _ext(out, "%s' = %s" % (name, name), TRANS, egate(nf, esub(e(name, True), e(name))))
    _ext(out, "A2 = A A", ALL, esub(e("A2"), emul(e("A"), e("A"))))
    _ext(out, "AB = A B", ALL, esub(e("AB"), emul(e("A"), e("B"))))
    al = e("ALPHA")
    _ext(out, "ACCIN = 0 on the first row", ALL, egate(first, e("ACCIN")))
    _ext(out, "U1", ALL, esub(e("U1"), eadd(emul(e("ACCIN"), al), esub(esub(e("C"), emul(e("A2"), e("B"))), eb(pv(AP_K1))))))
    _ext(out, "U2", ALL, esub(e("U2"), eadd(emul(e("U1"), al), emul(e("SELT"), esub(esub(esub(e("DN"), e("AB")), e("C")), eb(pv(AP_K2)))))))
    _ext(out, "ACCO", ALL, esub(e("ACCO"), eadd(emul(e("U2"), al), emul(e("SELF"), esub(e("D"), eb(pv(AP_K3)))))))
    _ext(out, "ACCIN' = ACCO", TRANS, egate(nf, esub(e("ACCIN", True), e("ACCO"))))
    return out


def zps_consts(n):
    return RA.zps_consts(types.SimpleNamespace(n=n))


def scalars16_constraints(n):
    M0, ALL = SC_PRE, O.SEL_ALL
    m, width = scalars_cols(n)
    e = lambda name, nxt=False: ev(M0 + m[name], nxt)
    out = []
    prev = e("ZETA")
    for i in range(1, n + 1):
        _ext(out, "squaring", ALL, esub(e("ZP%d" % i), emul(prev, prev)))
        prev = e("ZP%d" % i)
    znn = prev
    wni = pow(pyref.two_adic_generator(n), -1, P)
    _ext(out, "(ZETA - 1) INVF = 1", ALL, esub(emul(esub(e("ZETA"), ec(1)), e("INVF")), ec(1)))
    _ext(out, "SELF", ALL, esub(e("SELF"), emul(esub(znn, ec(1)), e("INVF"))))
    _ext(out, "SELT", ALL, esub(e("SELT"), esub(e("ZETA"), ec(wni))))
    for k in range(2):
        q = ec(0)
        for t in range(4):
            basis = [0, 0, 0, 0]
            basis[t] = 1
            q = eadd(q, emul(ec(basis), e("QZ%d" % (4 * k + t))))
        _ext(out, "QK%d" % k, ALL, esub(e("QK%d" % k), q))
    (a0, b0), (a1, b1) = zps_consts(n)
    z0, z1 = eadd(escale(znn, a0), ec(b0)), eadd(escale(znn, a1), ec(b1))
    _ext(out, "QUO", ALL, esub(e("QUO"), eadd(emul(z0, e("QK0")), emul(z1, e("QK1")))))
    _ext(out, "ACC = QUO (ZP_n - 1)", ALL, esub(e("ACC"), emul(e("QUO"), esub(znn, ec(1)))))
    for col in range(0, width, 4):
        _ext(out, "every row repeats row 0", O.SEL_TRANSITION, esub(ev(M0 + col, True), ev(M0 + col)))
    return out


def _shift_var(v, at, by):
    kind, col = v >> 30, v & ((1 << 30) - 1)
    return v if kind == 2 or col < at else (kind << 30) | (col + by)


def opened16_constraints():
    """the head machine's, its main columns four places on"""
    return [(name, sel, [(c, [_shift_var(v, HA.OPN_PRE, OPN_PRE - HA.OPN_PRE) for v in vs]) for c, vs in poly]) for name, sel, poly in HA.opened16_constraints()]


def constraint_names(table, W=0, NP=0, log_n=0, pow_bits=0):
    if table == AIR16:
        return [n for n, _, _ in air16_constraints()]
    if table == SCALARS16:
        return [n for n, _, _ in scalars16_constraints(log_n)]
    return HA.constraint_names(table, W, NP, log_n, pow_bits)


def programs(R, F, b, pow_bits, W, NP):
    """by table number"""
    n = 4 * R + F
    hp = HA.programs(R, F, b, pow_bits, W, NP)
    hp[HA.OPENED16] = HA._program(OPN_PRE + HA.OP_MAIN, opened16_constraints(), NP)
    return hp + [HA._program(AIR_PRE + AIR_MAIN, air16_constraints(), NP), HA._program(SC_PRE + scalars_cols(n)[1], scalars16_constraints(n), NP)]


def interactions(R, lf, n):
    """by table number"""
    hp = HA.interactions(R, lf)
    S, Rv = O.SEND, O.RECEIVE
    e4 = lambda c: [c, c + 1, c + 2, c + 3]
    ent = lambda tab: [(int(s), int(m), int(bus), [int(c) for c in cols]) for s, m, bus, cols in TA._entries(tab)]
    o = HA.PTH_PRE + HA.P2.OUTE(7)
    p2th = ent(hp[HA.P2TH]) + [(S, PH_AM, BUS_ALPHA, [o + 7, o + 6, o + 5, o + 4])]
    sh = lambda c: c + (OPN_PRE - HA.OPN_PRE) if c >= HA.OPN_PRE else c
    M0 = OPN_PRE
    opened = [(s, m, bus, [sh(c) for c in cols]) for s, m, bus, cols in ent(hp[HA.OPENED16])]
    opened += [(S, OQ_H0, BUS_OH0, [HA.OQ_ROW] + e4(M0 + HA.OP_V)), (S, OQ_H1, BUS_OH1, [HA.OQ_ROW] + e4(M0 + HA.OP_V + 4))]
    M0 = AIR_PRE
    air = [(Rv, AP_ACT, bus, [key] + e4(M0 + AI[name])) for bus, key, name in ((BUS_OH0, AP_KL0, "A"), (BUS_OH1, AP_KL0, "B"), (BUS_OH0, AP_KL1, "C"), (BUS_OH1, AP_KL1, "D"),
                                                                               (BUS_OH1, AP_KN1, "DN"))]
    air += [(Rv, AP_FIRST, bus, e4(M0 + AI[name])) for bus, name in ((BUS_KA, "ALPHA"), (BUS_KSELT, "SELT"), (BUS_KSELF, "SELF"))]
    air += [(S, AP_LAST, BUS_ACC, e4(M0 + AI["ACCO"]))]
    M0 = SC_PRE
    m, _ = scalars_cols(n)
    sc = [(Rv, SP_FIRST, BUS_ALPHA, e4(M0 + m["ALPHA"])), (Rv, SP_FIRST, HA.BUS_ZETA, e4(M0 + m["ZETA"]))]
    for i in range(4):
        sc += [(Rv, SP_FIRST, BUS_OH0, [SP_KQ + i] + e4(M0 + m["QZ%d" % (2 * i)])), (Rv, SP_FIRST, BUS_OH1, [SP_KQ + i] + e4(M0 + m["QZ%d" % (2 * i + 1)]))]
    sc += [(Rv, SP_FIRST, BUS_ACC, e4(M0 + m["ACC"]))]
    sc += [(S, SP_FIRST, bus, e4(M0 + m[name])) for bus, name in ((BUS_KA, "ALPHA"), (BUS_KSELT, "SELT"), (BUS_KSELF, "SELF"))]
    out = list(hp)
    out[HA.P2TH], out[HA.OPENED16] = O.interaction_table(p2th), O.interaction_table(opened)
    return out + [O.interaction_table(air), O.interaction_table(sc)]


# ---------------------------------------------------------------- the identity in plain integers
def _sub_base(e, k):
    return [(e[0] - k) % P] + list(e[1:])


def selectors(zeta, n):
    """-> (ZP_1 .. ZP_n, INVF, SELF, SELT)"""
    zeta = [int(c) for c in zeta]
    zp, cur = [], zeta
    for _ in range(n):
        cur = pyref.ext_mul(cur, cur)
        zp.append([int(c) for c in cur])
    d = _sub_base(zeta, 1)
    invf = [int(c) for c in pyref.ext_inv(d)] if any(d) else [0, 0, 0, 0]
    self_ = pyref.ext_mul(_sub_base(zp[-1], 1), invf)
    selt = _sub_base(zeta, pow(pyref.two_adic_generator(n), -1, P))
    return zp, invf, [int(c) for c in self_], selt


def air16_main(opened, alpha, zeta, W, n, lr=None):
    """AIR16's main trace -> (trace [2^lr][56], ACCO of the last group)"""
    lr = A.lg(W // 4, 6) if lr is None else lr
    alpha = [int(c) for c in alpha]
    op = [[int(c) for c in e] for e in opened]
    _, _, self_, selt = selectors(zeta, n)
    mul, add, sub = pyref.ext_mul, A.e_add, A.e_sub
    t = np.zeros((1 << lr, AIR_MAIN), dtype=np.uint64)
    acc = [0, 0, 0, 0]
    for g in range(W // 4):
        a, b, c, d, dn = op[4 * g], op[4 * g + 1], op[4 * g + 2], op[4 * g + 3], op[W + 4 * g + 3]
        a2, ab = mul(a, a), mul(a, b)
        u1 = add(mul(acc, alpha), _sub_base(sub(c, mul(a2, b)), g + 1))
        u2 = add(mul(u1, alpha), mul(selt, _sub_base(sub(sub(dn, ab), c), 2 * g + 3)))
        acco = add(mul(u2, alpha), mul(self_, _sub_base(d, 5 * g + 7)))
        for name, val in zip(AIR_COLS, (a, b, c, d, dn, alpha, selt, self_, a2, ab, acc, u1, u2, acco)):
            t[g, AI[name]:AI[name] + 4] = [int(x) for x in val]
        acc = [int(x) for x in acco]
    return t.astype(np.uint32), acc


def scalars16_main(opened, alpha, zeta, W, n, acc=None):
    """SCALARS16's main trace, one row repeated -> (trace [2^7][4 (17 + n)], QUO (zeta^N - 1)); acc: what the ACC column holds (default: that product)"""
    m, width = scalars_cols(n)
    op = [[int(c) for c in e] for e in opened]
    zp, invf, self_, selt = selectors(zeta, n)
    mul, add = pyref.ext_mul, A.e_add
    row = np.zeros(width, dtype=np.uint64)
    put = lambda name, val: row.__setitem__(slice(m[name], m[name] + 4), [int(x) for x in val])
    put("ALPHA", alpha), put("ZETA", zeta), put("INVF", invf), put("SELF", self_), put("SELT", selt)
    for i in range(n):
        put("ZP%d" % (i + 1), zp[i])
    qz = op[2 * W:2 * W + 8]
    qk = []
    for k in range(2):
        q = [0, 0, 0, 0]
        for t in range(4):
            basis = [0, 0, 0, 0]
            basis[t] = 1
            put("QZ%d" % (4 * k + t), qz[4 * k + t])
            q = add(q, mul(basis, qz[4 * k + t]))
        qk.append(q)
        put("QK%d" % k, q)
    znn = zp[-1]
    zs = [[(c * a + (bb if i == 0 else 0)) % P for i, c in enumerate(znn)] for a, bb in zps_consts(n)]
    quo = add(mul(zs[0], qk[0]), mul(zs[1], qk[1]))
    prod = [int(x) for x in mul(quo, _sub_base(znn, 1))]
    put("QUO", quo), put("ACC", prod if acc is None else acc)
    return np.tile(row, (1 << SC_LOG_ROWS, 1)).astype(np.uint32), prod


# ---------------------------------------------------------------- tables of a view
def opened16_pre(W, NP, lr):
    pre = np.zeros((1 << lr, OPN_PRE), dtype=np.uint32)
    pre[:, :HA.OPN_PRE] = HA.opened16_pre(W, NP, lr)
    for i in range(W + 4):
        whole = i < W // 2 or i >= W                              # loc and quotient rows
        pre[i, OQ_H0], pre[i, OQ_H1] = int(whole), int(whole or (i - W // 2) % 2 == 1)
    return pre


def air16_pre(W, NP, lr):
    a = HA.head_rows(W, NP)[0]
    G = W // 4
    pre = np.zeros((1 << lr, AIR_PRE), dtype=np.uint32)
    for g in range(G):
        pre[g, :10] = [1, int(g == 0), int(g != 0), int(g == G - 1), g + 1, 2 * g + 3, 5 * g + 7, a + 1 + 2 * g, a + 1 + 2 * g + 1, a + 1 + W // 2 + 2 * g + 1]
    return pre


def scalars16_pre(W, NP):
    a = HA.head_rows(W, NP)[0]
    pre = np.zeros((1 << SC_LOG_ROWS, SC_PRE), dtype=np.uint32)
    pre[0, :5] = [1] + [a + 1 + W + i for i in range(4)]
    return pre


def key_tables(view):
    """the key's tables by table number: the head machine's with alpha's multiplicity, zeta's second receiver and OPENED16's half-row multiplicities; two schedules"""
    R, Q, F, b, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"], len(view["pubs"])
    lr = log_rows(R, F, b, Q, W, NP)
    a = HA.head_rows(W, NP)[0]
    kt = HA.key_tables(view)
    kt[HA.P2TH] = kt[HA.P2TH].copy()
    kt[HA.P2TH][a - 1, PH_AM], kt[HA.P2TH][a, HA.PH_ZM] = 1, ZETA_RECEIVERS
    kt[HA.OPENED16] = opened16_pre(W, NP, lr[HA.OPENED16])
    return kt + [air16_pre(W, NP, lr[AIR16]), scalars16_pre(W, NP)]


def public_values(view):
    return HA.public_values(view)


def tables(view, p24l=None, honest=True, p24r=None, scalars_acc=None):
    """by table number: (main traces, preprocessed traces).  scalars_acc: "air": SCALARS16's ACC column takes AIR16's accumulator (default: QUO (zeta^N - 1); an inner
    proof that holds makes them equal)"""
    R, Q, F, b, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"], len(view["pubs"])
    lr, n = log_rows(R, F, b, Q, W, NP), 4 * R + F
    h = HA.head_of(view)
    main, _ = HA.tables(view, p24l, honest, p24r)
    amain, acco = air16_main(view["opened"], h["alpha"], h["zeta"], W, n, lr[AIR16])
    smain, _ = scalars16_main(view["opened"], h["alpha"], h["zeta"], W, n, acco if scalars_acc == "air" else None)
    return main + [amain, smain], key_tables(view)


def identity_holds(view):
    R, F, W = len(view["roots"]), view["F"], view["W"]
    h = HA.head_of(view)
    return air16_main(view["opened"], h["alpha"], h["zeta"], W, 4 * R + F)[1] == scalars16_main(view["opened"], h["alpha"], h["zeta"], W, 4 * R + F)[1]


def machine(view, p24l=None, honest=True, p24r=None, scalars_acc=None):
    """-> (main traces, preprocessed traces, programs, interaction tables, public values) in machine order"""
    R, Q, F, b, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"], len(view["pubs"])
    assert shape_ok(R, F, b, Q, view["pow_bits"], W, NP)
    main, pre = tables(view, p24l, honest, p24r, scalars_acc)
    progs, tabs = programs(R, F, b, view["pow_bits"], W, NP), interactions(R, F + b, 4 * R + F)
    o = order(R, F, b, Q, W, NP)
    return [main[i] for i in o], [pre[i] for i in o], [progs[i] for i in o], [tabs[i] for i in o], public_values(view)


# ---------------------------------------------------------------- views
def oracle_proof(oracle, R, F, b, Q, W, NP, seed=1, pow_bits=4):
    """an inner proof made by the oracle's shard prover over the synthetic AIR (so the identity holds) -> (proof bytes, log_n, public values, parameter tuple)"""
    log_n = 4 * R + F
    pubs = [(seed * 7 + 3 * i + 1) % P for i in range(NP)]
    shape = (b, Q, pow_bits, 0, 4, F, 24)
    proof = oracle.prove_shard(oracle.gen_trace(seed, 0, log_n, W), pubs, oracle.default_params(*shape))
    return np.frombuffer(np.asarray(proof).tobytes(), dtype=np.uint8), log_n, pubs, shape


def oracle_view(oracle, R, F, b, Q, W, NP, seed=1, pow_bits=4):
    """that proof as the head machine's view (tests/pyverify.py reads it, as it reads the committed ones)"""
    proof, log_n, pubs, shape = oracle_proof(oracle, R, F, b, Q, W, NP, seed, pow_bits)
    return HA.golden_view("made", {"made": dict(shape=list(shape), log_n=log_n, width=W, public=pubs)}, lambda _: proof)
