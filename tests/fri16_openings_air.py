"""The fold-by-16 OPENINGS machine, written a second time -- the first is zktls_amd/csrc/fri16_chip.hip (the machine and its key) and fri16_rows.cuh (the kernel
that fills ROWSUM16 and QUERY16).  It is the indices machine of tests/fri16_transcript_air.py with the reduced openings computed in-circuit: the value every
fold chain starts from is no longer listed in the key, it is derived from the trace row and the quotient row the inner proof opens for the query.

Statement (40 public values: the 8 capacity words of the indices machine, then fa, zeta, zeta g_N, YL, YN, YQ, OFFN = fa^W, OFFQ = fa^(2W), four words each; the
key commits the layer roots, the final coefficients and, by query number, the opened trace row (W words) and quotient row (8 words) -- no reduced opening, no
index, no challenge):
    everything the indices machine states, and: the value at which query q enters layer 0 is
        (AT_q - YL) / (x - zeta) + OFFN (AT_q - YN) / (x - zeta g) + OFFQ (AQ_q - YQ) / (x - zeta),
    AT_q = sum_j fa^j t_{q,j}, AQ_q = sum_j fa^j u_{q,j} over the rows listed for query number q, x = g w_{2^H}^bitrev_H(index_q) at the index DRAWN for q.
The eight constants are PUBLIC in this step (as beta was public in the first fold-16 machine before the transcript came in): nothing here ties them to the
inner proof's transcript, its opened values or its AIR.  STILL OUTSIDE: the Merkle paths of the trace and quotient rows (ROWS is the table a width-24 chip
variant on the same bus replaces), the transcript before the commit phase, lookups (logup_pairs = 0 only), the AIR identity at zeta.

Tables by number: 0 FOLD16C (FOLD16B plus the column XQ = X sum_j O_j w_16^bitrev(j, 4) -- the query's point without the coset shift -- and three unused cells
that keep the width a multiple of four; the send on a chain's first row is (IDX, XQ, OWN[4])); 1 FINAL, 2 P24L, 4 COEFFS, 5 ROOTS, 6 P2T, 7 SAMPLES: the indices
machine's word for word but the public-value count in the header; 3 QUERY16 where QUERIES stood: preprocessed (q, ACT, 0 ...), main the columns of
recursion_air.query_cols(), every constant tied to its public value on every row; 8 ROWSUM16: recursion_air's ROWSUM rows (RS_MAIN), preprocessed
(TAG = 2 q + tree, ACT, NOTFIRST, LAST0, LAST1, QN, K0 = 2 block, K1 = K0 + 1), FA tied to the public values on every row; 9 ROWS: preprocessed
(TAG, K, w0..w3, 1, 0), one row per 4-word group of every opened row, in the tuple form in which P24L's sponge rows receive theirs."""
import functools

import numpy as np

import fri16_air as A
import fri16_paths_air as PA
import fri16_transcript_air as TA
import fri_air as FA
import oracle_lib as O
import pyref
import pyverify
import recursion_air as RA
from recursion_air import RS_ACCIN, RS_FA, RS_MAIN, RS_T, RS_V, ev, eb, eadd, esub, emul, egate, ec, pv, padd, pneg, pscale

P = O.P
V = O.air_var
FOLD16C, FINAL, P24L, QUERY16, COEFFS, ROOTS, P2T, SAMPLES, ROWSUM16, ROWS = range(10)
NAMES = ["FOLD16C", "FINAL", "P24L", "QUERY16", "COEFFS", "ROOTS", "P2T", "SAMPLES", "ROWSUM16", "ROWS"]
BUS_ROW, BUS_AT16, BUS_AQ16 = 81, 82, 83
N_PUBLIC = 40
CONSTS = ("FA", "ZETA", "ZNX", "YL", "YN", "YQ", "OFFN", "OFFQ")                 # the order of the public values behind the capacity
PUB = {name: 8 + 4 * i for i, name in enumerate(CONSTS)}
Q16_PRE, QP_QN, QP_ACT = 8, 0, 1
Q_MAIN = RA.Q_MAIN
RS16_PRE, RP_TAG, RP_ACT, RP_NOTFIRST, RP_LAST0, RP_LAST1, RP_QN, RP_K0, RP_K1 = 8, 0, 1, 2, 3, 4, 5, 6, 7
ROWS_PRE = 8
QROW = 8                                                                         # words of a quotient row
assert Q16_PRE == RA.Q_PRE
HONEST_SHAPES = [(1, 0, 1, 4, 8), (2, 2, 2, 11, 24), (3, 8, 2, 50, 128)]         # (R, F, log_blowup, queries, trace width)


def shape_ok(R, F, b, Q, pow_bits, W):
    return TA.shape_ok(R, F, b, Q, pow_bits) and 8 <= W <= 1024 and W % 8 == 0


def xq_col(lf):
    return A.width_of(lf)


def fold16c_width(lf):
    return A.width_of(lf) + 4


def log_rows(R, F, b, Q, W):
    """ROWSUM16 and ROWS have at least 2^6 rows: a keyed machine takes at most 8 tables of one height, and the other eight can all have 2^5 rows"""
    return TA.log_rows(R, F, b, Q) + [A.lg(Q * (W // 8 + 1), 6), A.lg(Q * (W + 8) // 4, 6)]


def order(R, F, b, Q, W):
    lr = log_rows(R, F, b, Q, W)
    return sorted(range(10), key=lambda i: (-lr[i], i))


def main_widths(lf):
    return [fold16c_width(lf), A.FIN_MAIN, PA.WIDTH_L, Q_MAIN, A.TAB_MAIN, TA.ROOTS_MAIN, TA.T_WIDTH, FA.S_MAIN, RS_MAIN, A.TAB_MAIN]


PRE_WIDTHS = [0, A.FIN_PRE, 0, Q16_PRE, A.C_PRE, PA.ROOTS_PRE, TA.PT_PRE, FA.S_PRE, RS16_PRE, ROWS_PRE]


# ---------------------------------------------------------------- programs
def w16_own(j):
    """w_16^bitrev(j, 4): what the own position j contributes to the query's point"""
    return pow(pyref.two_adic_generator(4), pyref.bitrev(j, 4), P)


def xq_constraint(lf):
    XQ = xq_col(lf)
    return (O.SEL_ALL, [(1, [V(XQ)])] + [((P - w16_own(j)) % P, [V(A.X), V(A.OF + j)]) for j in range(16)])


def fold16c_program(R, lf):
    """FOLD16B's constraints, then XQ = X sum_j O_j w_16^bitrev(j, 4)"""
    cons = TA.constraints_of(TA.fold16b_program(R, lf))
    return O.air_program(fold16c_width(lf), N_PUBLIC, cons + [xq_constraint(lf)])


def pub4(name):
    return [[(1, [V(PUB[name] + c, public=True)])] for c in range(4)]


def query16_constraints():
    """-> [(name, selector, polynomial)]"""
    m = RA.query_cols()
    out = []

    def ext(name, sel, e):
        for c in range(4):
            out.append((name, sel, e[c]))
    for name in RA.QUERY_CONSTS:
        ext("%s = its public value" % name, O.SEL_ALL, esub(ev(m[name]), pub4(name)))
    x = eb(pscale(pv(m["XQ"]), RA.GEN))
    act = pv(QP_ACT)
    ext("I1 (x - zeta) = 1", O.SEL_ALL, egate(act, esub(emul(esub(x, ev(m["ZETA"])), ev(m["I1"])), ec(1))))
    ext("I2 (x - zeta g) = 1", O.SEL_ALL, egate(act, esub(emul(esub(x, ev(m["ZNX"])), ev(m["I2"])), ec(1))))
    ext("P1", O.SEL_ALL, esub(ev(m["P1"]), emul(esub(ev(m["AT"]), ev(m["YL"])), ev(m["I1"]))))
    ext("P2", O.SEL_ALL, esub(ev(m["P2"]), emul(esub(ev(m["AT"]), ev(m["YN"])), ev(m["I2"]))))
    ext("P2O", O.SEL_ALL, esub(ev(m["P2O"]), emul(ev(m["OFFN"]), ev(m["P2"]))))
    ext("P3", O.SEL_ALL, esub(ev(m["P3"]), emul(esub(ev(m["AQ"]), ev(m["YQ"])), ev(m["I1"]))))
    ext("P3O", O.SEL_ALL, esub(ev(m["P3O"]), emul(ev(m["OFFQ"]), ev(m["P3"]))))
    ext("RO = P1 + P2O + P3O", O.SEL_ALL, esub(ev(m["RO"]), eadd(ev(m["P1"]), ev(m["P2O"]), ev(m["P3O"]))))
    return out


def rowsum16_constraints():
    M0 = RS16_PRE
    out = []

    def ext(name, sel, e):
        for c in range(4):
            out.append((name, sel, e[c]))
    fa = ev(M0 + RS_FA)
    ext("FA = its public value", O.SEL_ALL, esub(fa, pub4("FA")))
    prev = ev(M0 + RS_ACCIN)
    for s in range(7, -1, -1):
        cur = ev(M0 + RS_T + 4 * s)
        ext("Horner", O.SEL_ALL, esub(cur, eadd(emul(prev, fa), eb(pv(M0 + RS_V + s)))))
        prev = cur
    ext("ACCIN follows", O.SEL_TRANSITION, egate(pv(RP_NOTFIRST, True), esub(ev(M0 + RS_ACCIN, True), ev(M0 + RS_T))))
    ext("ACCIN = 0 on a first block", O.SEL_ALL, egate(padd(pv(RP_ACT), pneg(pv(RP_NOTFIRST))), ev(M0 + RS_ACCIN)))
    return out


def _program(width, cons):
    c = RA.Cons()
    for _, sel, poly in cons:
        c.add(sel, poly)
    return O.air_program(width, N_PUBLIC, c.c)


def query16_program():
    return _program(Q16_PRE + Q_MAIN, query16_constraints())


def rowsum16_program():
    return _program(RS16_PRE + RS_MAIN, rowsum16_constraints())


def constraint_names(table, pow_bits=0):
    if table == QUERY16:
        return [n for n, _, _ in query16_constraints()]
    if table == ROWSUM16:
        return [n for n, _, _ in rowsum16_constraints()]
    if table == P2T:
        return TA.p2t_constraint_names()
    if table == SAMPLES:
        return TA.samples_constraint_names(pow_bits)
    return None


def programs(R, F, b, pow_bits):
    """by table number"""
    lf = F + b
    ti = [TA.with_public(p, N_PUBLIC) for p in TA.programs(R, F, b, pow_bits)]
    return [fold16c_program(R, lf), ti[TA.FINAL], ti[TA.P24L], query16_program(), ti[TA.COEFFS], ti[TA.ROOTS], ti[TA.P2T], ti[TA.SAMPLES], rowsum16_program(),
            TA.with_public(TA.table_program(ROWS_PRE), N_PUBLIC)]


def interactions(R, lf):
    """by table number"""
    ti = TA.interactions(R)
    S, Rv = O.SEND, O.RECEIVE
    XQ = xq_col(lf)
    fold = [(s, m, bus, cols) if bus != A.BUS_Q16 else (s, m, bus, [A.IDX, XQ, A.OWN, A.OWN + 1, A.OWN + 2, A.OWN + 3]) for s, m, bus, cols in TA._entries(ti[TA.FOLD16B])]
    m = RA.query_cols()
    e4 = lambda c: [c, c + 1, c + 2, c + 3]
    query = [(Rv, QP_ACT, FA.BUS_I, [QP_QN, m["IDX"]]), (Rv, QP_ACT, A.BUS_Q16, [m["IDX"], m["XQ"]] + e4(m["RO"])),
             (Rv, QP_ACT, BUS_AT16, [QP_QN] + e4(m["AT"])), (Rv, QP_ACT, BUS_AQ16, [QP_QN] + e4(m["AQ"]))]
    M0 = RS16_PRE
    rowsum = [(S, RP_ACT, BUS_ROW, [RP_TAG, RP_K0] + e4(M0 + RS_V)), (S, RP_ACT, BUS_ROW, [RP_TAG, RP_K1] + e4(M0 + RS_V + 4)),
              (S, RP_LAST0, BUS_AT16, [RP_QN] + e4(M0 + RS_T)), (S, RP_LAST1, BUS_AQ16, [RP_QN] + e4(M0 + RS_T))]
    rows = [(Rv, 6, BUS_ROW, [0, 1, 2, 3, 4, 5])]
    return [O.interaction_table(fold), ti[TA.FINAL], ti[TA.P24L], O.interaction_table(query), ti[TA.COEFFS], ti[TA.ROOTS], ti[TA.P2T], ti[TA.SAMPLES],
            O.interaction_table(rowsum), O.interaction_table(rows)]


# ---------------------------------------------------------------- the reduced opening
def consts_of(fa, zeta, loc, nxt, qz, W, log_n):
    """the eight constants of a proof from its batching challenge, zeta and its opened values (extension elements) -> {name: [4]}"""
    def batch(vals):
        acc = [0, 0, 0, 0]
        for v in reversed(vals):
            acc = A.e_add(pyref.ext_mul(acc, fa), v)
        return acc
    g = pyref.two_adic_generator(log_n)
    return dict(FA=list(fa), ZETA=list(zeta), ZNX=[c * g % P for c in zeta], YL=batch(loc), YN=batch(nxt), YQ=batch(qz), OFFN=pyref.ext_pow(fa, W),
                OFFQ=pyref.ext_pow(fa, 2 * W))


def rowsum_rows(Q, W):
    """(q, block) in trace order: a query's trace blocks from the last to the first, then its quotient block (block number W / 8)"""
    WB = W // 8
    return [(q, b) for q in range(Q) for b in list(range(WB - 1, -1, -1)) + [WB]]


def point(index, H):
    """XQ: the query's point without the coset shift"""
    return pow(pyref.two_adic_generator(H), pyref.bitrev(index, H), P)


def query_values(index, H, at, aq, c):
    """-> {column name: value} of one QUERY16 row; x = g XQ must differ from zeta and zeta g"""
    xq = point(index, H)
    x = [RA.GEN * xq % P, 0, 0, 0]
    i1, i2 = pyref.ext_inv(RA.e_sub(x, c["ZETA"])), pyref.ext_inv(RA.e_sub(x, c["ZNX"]))
    p1 = pyref.ext_mul(RA.e_sub(at, c["YL"]), i1)
    p2 = pyref.ext_mul(RA.e_sub(at, c["YN"]), i2)
    p2o = pyref.ext_mul(c["OFFN"], p2)
    p3 = pyref.ext_mul(RA.e_sub(aq, c["YQ"]), i1)
    p3o = pyref.ext_mul(c["OFFQ"], p3)
    ro = RA.e_add(RA.e_add(p1, p2o), p3o)
    return dict(IDX=index, XQ=xq, RO=ro, AT=at, AQ=aq, I1=i1, I2=i2, P1=p1, P2=p2, P2O=p2o, P3=p3, P3O=p3o)


def opening_traces(H, W, trows, qrows, consts, indices, lr_rowsum=None, lr_query=None):
    """what zkhip_fri16_openings_gen_traces makes from raw rows: -> (ROWSUM16 main, QUERY16 main, reduced openings [Q][4])"""
    Q, WB = len(indices), W // 8
    lr_rowsum = A.lg(Q * (WB + 1), 6) if lr_rowsum is None else lr_rowsum
    lr_query = A.lg(Q) if lr_query is None else lr_query
    fa = [int(x) for x in consts["FA"]]
    t = np.zeros((1 << lr_rowsum, RS_MAIN), dtype=np.uint64)
    t[:, RS_FA:RS_FA + 4] = fa
    at, aq, acc = {}, {}, [0, 0, 0, 0]
    for r, (q, b) in enumerate(rowsum_rows(Q, W)):
        vals = [int(x) for x in (qrows[q] if b == WB else trows[q][8 * b:8 * b + 8])]
        if b in (WB - 1, WB):
            acc = [0, 0, 0, 0]
        t[r, RS_V:RS_V + 8], t[r, RS_ACCIN:RS_ACCIN + 4] = vals, acc
        steps = RA._horner8(acc, vals, fa)
        for s in range(8):
            t[r, RS_T + 4 * s:RS_T + 4 * s + 4] = steps[s]
        acc = steps[0]
        if b == 0:
            at[q] = acc
        if b == WB:
            aq[q] = acc
    m = RA.query_cols()
    qm = np.zeros((1 << lr_query, Q_MAIN), dtype=np.uint64)
    for name in RA.QUERY_CONSTS:
        qm[:, m[name] - Q16_PRE:m[name] - Q16_PRE + 4] = [int(x) for x in consts[name]]
    ros = []
    for q, index in enumerate(indices):
        vals = query_values(int(index), H, at[q], aq[q], consts)
        for name, val in vals.items():
            c0 = m[name] - Q16_PRE
            if name in ("IDX", "XQ"):
                qm[q, c0] = val
            else:
                qm[q, c0:c0 + 4] = val
        ros.append(vals["RO"])
    return t.astype(np.uint32), qm.astype(np.uint32), ros


def reduced_openings(view):
    """the reduced openings of a view recomputed from its rows, its constants and its indices alone"""
    return opening_traces(view["H"], view["W"], view["trows"], view["qrows"], view["consts"], [q[0] for q in view["queries"]])[2]


# ---------------------------------------------------------------- tables of a view
def rowsum16_pre(Q, W, lr):
    WB = W // 8
    t = np.zeros((1 << lr, RS16_PRE), dtype=np.uint32)
    for r, (q, b) in enumerate(rowsum_rows(Q, W)):
        tree, blk = (1, 0) if b == WB else (0, b)
        t[r] = [2 * q + tree, 1, 0 if b in (WB - 1, WB) else 1, int(b == 0), int(b == WB), q, 2 * blk, 2 * blk + 1]
    return t


def rows_pre(view, lr):
    Q, W = len(view["queries"]), view["W"]
    t = np.zeros((1 << lr, ROWS_PRE), dtype=np.uint32)
    r = 0
    for q in range(Q):
        for tree, row in ((0, view["trows"][q]), (1, view["qrows"][q])):
            for k in range(len(row) // 4):
                t[r, 0], t[r, 1], t[r, 2:6], t[r, 6] = 2 * q + tree, k, row[4 * k:4 * k + 4], 1
                r += 1
    assert r == Q * (W + QROW) // 4
    return t


def key_tables(view):
    """the key's tables by table number (None: no preprocessed columns): the rows go in, no reduced opening, no index and no challenge"""
    R, Q, F, b, W = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"]
    lr = log_rows(R, F, b, Q, W)
    ti = TA.key_tables(view)
    tq = np.zeros((1 << lr[QUERY16], Q16_PRE), dtype=np.uint32)
    for q in range(Q):
        tq[q, QP_QN], tq[q, QP_ACT] = q, 1
    return [None, ti[TA.FINAL], None, tq, ti[TA.COEFFS], ti[TA.ROOTS], ti[TA.P2T], ti[TA.SAMPLES], rowsum16_pre(Q, W, lr[ROWSUM16]), rows_pre(view, lr[ROWS])]


def public_values(view):
    return [int(c) for c in view["capacity"]] + [int(x) for name in CONSTS for x in view["consts"][name]]


def tables(view, p24l=None, honest=True):
    """by table number: (main traces, preprocessed traces).  honest: the view's reduced openings are the ones its rows give (a forger's view keeps its own in
    the fold chains while ROWSUM16 and QUERY16 hold what the rows give)"""
    R, Q, F, b, H, W = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["H"], view["W"]
    lf = F + b
    lr = log_rows(R, F, b, Q, W)
    mi, _ = TA.tables(view, p24l, honest)
    indices = [q[0] for q in view["queries"]]
    rs, qm, ros = opening_traces(H, W, view["trows"], view["qrows"], view["consts"], indices, lr[ROWSUM16], lr[QUERY16])
    if honest:
        assert ros == [[int(c) for c in q[1]] for q in view["queries"]], "the view's reduced openings are not the ones its rows give"
    fold = np.zeros((mi[TA.FOLD16B].shape[0], fold16c_width(lf)), dtype=np.uint32)
    fold[:, :A.width_of(lf)] = mi[TA.FOLD16B]
    for r in range(Q * R):
        own = int(np.argmax(fold[r, A.OF:A.OF + 16]))
        fold[r, xq_col(lf)] = int(fold[r, A.X]) * w16_own(own) % P
    for q, index in enumerate(indices):
        assert int(fold[q * R, xq_col(lf)]) == point(index, H)
    main = [fold, mi[TA.FINAL], mi[TA.P24L], qm, mi[TA.COEFFS], mi[TA.ROOTS], mi[TA.P2T], mi[TA.SAMPLES], rs, np.zeros((1 << lr[ROWS], A.TAB_MAIN), dtype=np.uint32)]
    return main, key_tables(view)


def machine(view, p24l=None, honest=True):
    """-> (main traces, preprocessed traces, programs, interaction tables, public values) in machine order"""
    R, Q, F, b, W = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"]
    assert shape_ok(R, F, b, Q, view["pow_bits"], W)
    main, pre = tables(view, p24l, honest)
    progs, tabs = programs(R, F, b, view["pow_bits"]), interactions(R, F + b)
    o = order(R, F, b, Q, W)
    return [main[i] for i in o], [pre[i] for i in o], [progs[i] for i in o], [tabs[i] for i in o], public_values(view)


# ---------------------------------------------------------------- views
def golden_view(name, GOLDEN, load):
    """the indices view of a committed fold-16 proof (no lookups) plus "W", "trows" [Q][W], "qrows" [Q][8] and "consts": read from pyverify's own view"""
    g = GOLDEN[name]
    s = g["shape"]
    assert s[3] == 0, "lookups are not taken"
    base = TA.golden_view(name, GOLDEN, load)
    return dict(base, **parse_openings(load(name).tobytes(), g["log_n"], g["width"], g["public"], s))


def parse_openings(proof_bytes, log_n, width, public, s):
    """-> {"W", "trows", "qrows", "consts"} of a fold-16 proof with the parameter tuple s (tests/pyverify.py reads the proof)"""
    pv_ = {}
    pyverify.verify(proof_bytes, log_n, width, public, log_blowup=s[0], num_queries=s[1], pow_bits=s[2], logup_pairs=s[3], log_fold=4, log_final=s[5], hash_width=s[6],
                    code_width=s[7] if len(s) > 7 else 0, view=pv_)
    consts = consts_of(pv_["fa"], pv_["zeta"], pv_["loc"], pv_["nxt"], pv_["qz"], width, log_n)
    return dict(W=width, trows=[[int(x) for x in o["trow"]] for o in pv_["openings"]], qrows=[[int(x) for x in o["qrow"]] for o in pv_["openings"]], consts=consts)


def solve_quotient_row(index, H, trow, consts, target, rng):
    """a quotient row under which the query's reduced opening is `target`: four words free, the other four from the 4 x 4 system in 1, fa, fa^2, fa^3.
    -> the row, or None when that system is singular"""
    fa = consts["FA"]
    at = [0, 0, 0, 0]
    for v in reversed(trow):
        at = RA.e_add(pyref.ext_mul(at, fa), [int(v), 0, 0, 0])
    xq = point(index, H)
    x = [RA.GEN * xq % P, 0, 0, 0]
    d1, d2 = RA.e_sub(x, consts["ZETA"]), RA.e_sub(x, consts["ZNX"])
    i1, i2 = pyref.ext_inv(d1), pyref.ext_inv(d2)
    rest = RA.e_sub(RA.e_sub(target, pyref.ext_mul(RA.e_sub(at, consts["YL"]), i1)), pyref.ext_mul(consts["OFFN"], pyref.ext_mul(RA.e_sub(at, consts["YN"]), i2)))
    aq = RA.e_add(pyref.ext_mul(pyref.ext_mul(rest, pyref.ext_inv(consts["OFFQ"])), d1), consts["YQ"])         # the AQ that gives the target
    free = [int(v) for v in rng.integers(0, P, 4)]
    fp = [[1, 0, 0, 0]]
    for _ in range(7):
        fp.append(pyref.ext_mul(fp[-1], fa))
    rhs = list(aq)
    for j in range(4):
        rhs = RA.e_sub(rhs, [c * free[j] % P for c in fp[4 + j]])
    # sum_{j < 4} u_j fa^j = rhs, coefficient by coefficient: a 4 x 4 system over the base field
    M = [[fp[j][c] for j in range(4)] + [rhs[c]] for c in range(4)]
    for col in range(4):
        piv = next((r for r in range(col, 4) if M[r][col]), None)
        if piv is None:
            return None
        M[col], M[piv] = M[piv], M[col]
        inv = pow(M[col][col], P - 2, P)
        M[col] = [v * inv % P for v in M[col]]
        for r in range(4):
            if r != col and M[r][col]:
                f = M[r][col]
                M[r] = [(v - f * w) % P for v, w in zip(M[r], M[col])]
    return [M[j][4] for j in range(4)] + free


@functools.lru_cache(maxsize=None)
def honest_view(R, F, b, Q, W, seed=1, pow_bits=TA.POW_BITS):
    """an honest instance: the indices machine's honest view (its reduced openings lie on a low-degree polynomial), trace rows and constants drawn, every
    query's quotient row solved for the value its chain starts from"""
    base = TA.honest_view(R, F, b, Q, seed, pow_bits)
    H = base["H"]
    rng = np.random.default_rng([seed, R, F, b, Q, W, 16])
    rnd = lambda n: [int(x) for x in rng.integers(0, P, n)]
    while True:
        fa = rnd(4)
        consts = dict(FA=fa, ZETA=rnd(4), YL=rnd(4), YN=rnd(4), YQ=rnd(4), OFFN=pyref.ext_pow(fa, W), OFFQ=pyref.ext_pow(fa, 2 * W))
        consts["ZNX"] = [c * pyref.two_adic_generator(H - b) % P for c in consts["ZETA"]]
        trows = [rnd(W) for _ in range(Q)]
        qrows = [solve_quotient_row(index, H, trows[q], consts, value, rng) for q, (index, value, _) in enumerate(base["queries"])]
        if all(r is not None for r in qrows):
            break
    view = dict(base, W=W, trows=trows, qrows=qrows, consts=consts)
    assert reduced_openings(view) == [list(q[1]) for q in base["queries"]]
    return view


def view_arrays(view):
    """fri16_transcript_air.view_arrays plus trace rows [Q][W], quotient rows [Q][8] and the constants [8][4]"""
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    return TA.view_arrays(view) + (u(view["trows"]), u(view["qrows"]), u([view["consts"][n] for n in CONSTS]))
