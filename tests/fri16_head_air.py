"""The fold-by-16 HEAD machine, written a second time -- the first is zktls_amd/csrc/fri16_chip.hip (the machine, its key and the head of the chain) and
fri16_rows.cuh (fri16_opened_rows_kernel, OPENED16's trace).  It is the row-paths machine of tests/fri16_rowpaths_air.py with the head of the transcript inside.
Written from docs/PROTOCOL.md section 6 and the duplex rules of the challenger: a full block of 8 observed words permutes; a sample with pending inputs permutes
with the remaining rate words kept; a sample right after a full block costs no permutation; words come out from out[7] down.

Statement (the public values are the NP public values of the inner proof and nothing else; the key commits the layer roots, the final coefficients, the trace root,
the quotient root and the header constants -- no opened word, no constant, no challenge):
    everything the row-paths machine states, and: the sponge chain starts from the all-zero state, absorbs (log_n, W, log_blowup, Q, inner_pow_bits, NP, 0, 4, F, 24),
    the trace root listed in ROOTS and the public values, draws alpha, absorbs the quotient root listed in ROOTS, draws zeta, absorbs the 2 W + 8 opened extension
    values (values at zeta, at zeta g, quotient values), draws fa, and the commit phase continues from that very state; the constants of the reduced opening are fa,
    zeta, zeta g_N, YL = sum fa^j loc_j, YN = sum fa^j nxt_j, YQ = sum fa^j quot_j, OFFN = fa^W, OFFQ = OFFN^2.
alpha is drawn and used by NOTHING in this step: the AIR identity at zeta is the step that consumes it.  STILL OUTSIDE: that identity, lookups, version-7 and
version-8 inner proofs, roots leaving the key, the wiring into the shard verifier.

Tables by number: 0 FOLD16C, 1 FINAL, 2 P24L, 4 COEFFS, 7 SAMPLES, 9 P24R: the row-paths machine's programs and interaction tables word for word but the
public-value count (SAMPLES' key table starts at row HD + R + C).  With A = ceil((18 + NP) / 8) and HD = A + 1 + W + 4:
6 P2TH   P2T's columns and chain constraints, row 0's capacity ZERO; 64 preprocessed columns: P2T's twenty, HF[8] HV[8] (header word flags and values), PUBI[6]
         (row i holds public values), RK[8] RM[8] (key 8 tree + word and multiplicity of the receive of a root word), OPN (the row's eight rate words are received
         from OPENED16 under its row number), ZM, FM (multiplicities of the sends of (out[7], out[6], out[5], out[4]) as zeta and as fa), three unused
5 ROOTS  20 preprocessed columns: the row-paths machine's twelve with HM at 11 (1 on the two trees' rows) and the keys HK[8] = 8 tree + j; eight more sends
10 OPENED16  preprocessed ACT NOTFIRST ROW ENDL ENDN ENDQ FIRST 0; main V[8] FA[4] FA2[4] PW[4] T[4] PT[4] Y[4] PWN[4]
3 QUERY16H  every constant c' = c, received on the first row (preprocessed column 6), ZNX = g_N ZETA, OFFQ = OFFN OFFN, then QUERY16's eight products
8 ROWSUM16H 12 preprocessed columns (FIRST at 8), FA' = FA, fa received on the first row"""
import copy
import functools

import numpy as np

import fri16_air as A
import fri16_openings_air as OA
import fri16_paths_air as PA
import fri16_rowpaths_air as RPA
import fri16_transcript_air as TA
import fri_air as FA
import oracle_lib as O
import poseidon2_air as P2
import pyref
import pyverify
import recursion_air as RA
from recursion_air import RS_ACCIN, RS_FA, RS_MAIN, RS_T, RS_V, ev, eb, eadd, esub, emul, egate, ec, escale, pv, padd, pneg

P = O.P
V = O.air_var
FOLD16C, FINAL, P24L, QUERY16H, COEFFS, ROOTS, P2TH, SAMPLES, ROWSUM16H, P24R, OPENED16 = range(11)
NAMES = ["FOLD16C", "FINAL", "P24L", "QUERY16H", "COEFFS", "ROOTS", "P2TH", "SAMPLES", "ROWSUM16H", "P24R", "OPENED16"]
UNCHANGED = [FOLD16C, FINAL, P24L, COEFFS, SAMPLES, P24R]
BUS_HR, BUS_OV0, BUS_OV1, BUS_ZETA, BUS_FA, BUS_YL, BUS_YN, BUS_YQ, BUS_OFFN = range(85, 94)
MAX_NP, STREAM = 30, 18                                                         # the public values start at stream word 18, behind the header and the trace root
PTH_PRE, PH_HF, PH_HV, PH_PUBI, PH_RK, PH_RM, PH_OPN, PH_ZM, PH_FM = 64, 20, 28, 36, 42, 50, 58, 59, 60
ROOTS_PRE, RT_HM, RT_HK = 20, 11, 12
QP_FIRST, RS16H_PRE, RP_FIRST = 6, 12, 8
OPN_PRE, OQ_ACT, OQ_NOTFIRST, OQ_ROW, OQ_ENDL, OQ_ENDN, OQ_ENDQ, OQ_FIRST = 8, 0, 1, 2, 3, 4, 5, 6
OP_V, OP_FA, OP_FA2, OP_PW, OP_T, OP_PT, OP_Y, OP_PWN, OP_MAIN = 0, 8, 12, 16, 20, 24, 28, 32, 36
MAX_SAME_HEIGHT = 8
FA_RECEIVERS = 2                                                                # ROWSUM16H and OPENED16 (QUERY16H keeps no column for fa)


def head_rows(W, NP):
    """-> (A: sponge rows up to alpha, HD: rows in front of the commit phase's)"""
    a = (STREAM + NP + 7) // 8
    return a, a + 1 + W + 4


def header(R, F, b, Q, pow_bits, W, NP):
    """the ten words a version-3 proof's transcript starts with: log_n, width, log_blowup, queries, pow_bits, public values, lookup pairs, log_fold, log_final, hash width"""
    return [4 * R + F, W, b, Q, pow_bits, NP, 0, 4, F, 24]


def log_rows(R, F, b, Q, W, NP):
    lr = RPA.log_rows(R, F, b, Q, W)
    _, _, NT = TA.chain_rows(R, F, Q)
    lr[P2TH] = A.lg(head_rows(W, NP)[1] + NT)
    return lr + [A.lg(W + 4, 6)]


def shape_ok(R, F, b, Q, pow_bits, W, NP):
    """the openings machine's shapes with 1 .. 30 public values, but those at which nine tables would have one height"""
    if not OA.shape_ok(R, F, b, Q, pow_bits, W) or not 1 <= NP <= MAX_NP:
        return False
    lr = log_rows(R, F, b, Q, W, NP)
    return max(lr.count(h) for h in lr) <= MAX_SAME_HEIGHT


def order(R, F, b, Q, W, NP):
    lr = log_rows(R, F, b, Q, W, NP)
    return sorted(range(11), key=lambda i: (-lr[i], i))


def main_widths(lf):
    return RPA.main_widths(lf) + [OP_MAIN]


PRE_WIDTHS = [0, A.FIN_PRE, 0, OA.Q16_PRE, A.C_PRE, ROOTS_PRE, PTH_PRE, FA.S_PRE, RS16H_PRE, 0, OPN_PRE]


# ---------------------------------------------------------------- programs
def p2th_constraints(W, NP):
    """-> [(name, selector, terms)] on the combined row [schedule | permutation columns]"""
    M0, ALL, FIRST, TRANS = PTH_PRE, O.SEL_ALL, O.SEL_FIRST, O.SEL_TRANSITION
    IN, OUT, D, BIT = M0 + P2.IN, M0 + P2.OUTE(7), M0 + P2.D, M0 + P2.BIT
    cons = [("permutation", sel, [(c, [v + M0 for v in vs]) for c, vs in terms]) for sel, terms in P2.permutation_constraints()]
    for j in range(8):
        cons.append(("D = IN", ALL, [(1, [V(D + j)]), (P - 1, [V(IN + j)])]))
    cons.append(("BIT = 0", ALL, [(1, [V(BIT)])]))
    for j in range(8):
        cons.append(("row 0: the capacity is zero", FIRST, [(1, [V(IN + 8 + j)])]))
    for j in range(8):
        cons.append(("SPG: the capacity follows", TRANS, [(1, [V(TA.PT_SPG, True), V(IN + 8 + j, True)]), (P - 1, [V(TA.PT_SPG, True), V(OUT + 8 + j)])]))
    for j in range(8):
        cons.append(("K: kept rate words follow", TRANS, [(1, [V(TA.PT_K + j, True), V(IN + j, True)]), (P - 1, [V(TA.PT_K + j, True), V(OUT + j)])]))
    for j in range(8):
        cons.append(("header pin", ALL, [(1, [V(PH_HF + j), V(IN + j)]), (P - 1, [V(PH_HF + j), V(PH_HV + j)])]))
    for i in range(head_rows(W, NP)[0]):
        for j in range(8):
            k = 8 * i + j - STREAM
            if 0 <= k < NP:
                cons.append(("public pin", ALL, [(1, [V(PH_PUBI + i), V(IN + j)]), (P - 1, [V(PH_PUBI + i), V(k, public=True)])]))
    return cons


def _ext(out, name, sel, e):
    for c in range(4):
        out.append((name, sel, e[c]))


def query16h_constraints(log_n):
    m = RA.query_cols()
    out = []
    for name in RA.QUERY_CONSTS:
        _ext(out, "%s' = %s" % (name, name), O.SEL_TRANSITION, esub(ev(m[name], True), ev(m[name])))
    _ext(out, "ZNX = g ZETA", O.SEL_ALL, esub(ev(m["ZNX"]), escale(ev(m["ZETA"]), pyref.two_adic_generator(log_n))))
    _ext(out, "OFFQ = OFFN OFFN", O.SEL_ALL, esub(ev(m["OFFQ"]), emul(ev(m["OFFN"]), ev(m["OFFN"]))))
    return out + OA.query16_constraints()[4 * len(RA.QUERY_CONSTS):]             # then QUERY16's eight products


def rowsum16h_constraints():
    M0 = RS16H_PRE
    out = []
    fa = ev(M0 + RS_FA)
    _ext(out, "FA' = FA", O.SEL_TRANSITION, esub(ev(M0 + RS_FA, True), fa))
    prev = ev(M0 + RS_ACCIN)
    for s in range(7, -1, -1):
        cur = ev(M0 + RS_T + 4 * s)
        _ext(out, "Horner", O.SEL_ALL, esub(cur, eadd(emul(prev, fa), eb(pv(M0 + RS_V + s)))))
        prev = cur
    _ext(out, "ACCIN follows", O.SEL_TRANSITION, egate(pv(OA.RP_NOTFIRST, True), esub(ev(M0 + RS_ACCIN, True), ev(M0 + RS_T))))
    _ext(out, "ACCIN = 0 on a first block", O.SEL_ALL, egate(padd(pv(OA.RP_ACT), pneg(pv(OA.RP_NOTFIRST))), ev(M0 + RS_ACCIN)))
    return out


def opened16_constraints():
    M0 = OPN_PRE
    out = []
    fa, fa2, pw, t, pt, y, pwn = (ev(M0 + c) for c in (OP_FA, OP_FA2, OP_PW, OP_T, OP_PT, OP_Y, OP_PWN))
    ALL, TRANS = O.SEL_ALL, O.SEL_TRANSITION
    _ext(out, "FA2 = FA FA", ALL, esub(fa2, emul(fa, fa)))
    _ext(out, "T = V0 + FA V1", ALL, esub(t, eadd(ev(M0 + OP_V), emul(fa, ev(M0 + OP_V + 4)))))
    _ext(out, "PT = PW T", ALL, esub(pt, emul(pw, t)))
    _ext(out, "PWN = PW FA2", ALL, esub(pwn, emul(pw, fa2)))
    first = padd(pv(OQ_ACT), pneg(pv(OQ_NOTFIRST)))
    _ext(out, "PW = 1 on a segment's first row", ALL, egate(first, esub(pw, ec(1))))
    _ext(out, "Y = PT on a segment's first row", ALL, egate(first, esub(y, pt)))
    _ext(out, "PW' = PWN", TRANS, egate(pv(OQ_NOTFIRST, True), esub(ev(M0 + OP_PW, True), pwn)))
    _ext(out, "Y' = Y + PT'", TRANS, egate(pv(OQ_NOTFIRST, True), esub(ev(M0 + OP_Y, True), eadd(y, ev(M0 + OP_PT, True)))))
    _ext(out, "FA' = FA", TRANS, esub(ev(M0 + OP_FA, True), fa))
    return out


def _program(width, cons, n_public):
    c = RA.Cons()
    for _, sel, poly in cons:
        c.add(sel, poly)
    return O.air_program(width, n_public, c.c)


def roots_program(n_public):
    RM = ROOTS_PRE
    return O.air_program(RM + TA.ROOTS_MAIN, n_public, [(O.SEL_FIRST, [(1, [V(RM + TA.ROOTS_MAIN - 1)])]), (O.SEL_ALL, [(1, [V(RM + 5)]), (P - 1, [V(RM + 5), V(10)])])])


def constraint_names(table, W=0, NP=0, log_n=0, pow_bits=0):
    if table == P2TH:
        return [n for n, _, _ in p2th_constraints(W, NP)]
    if table == QUERY16H:
        return [n for n, _, _ in query16h_constraints(log_n)]
    if table == ROWSUM16H:
        return [n for n, _, _ in rowsum16h_constraints()]
    if table == OPENED16:
        return [n for n, _, _ in opened16_constraints()]
    return RPA.constraint_names(table, pow_bits)


def programs(R, F, b, pow_bits, W, NP):
    """by table number"""
    rp = [TA.with_public(p, NP) for p in RPA.programs(R, F, b, pow_bits)]
    rp[QUERY16H] = _program(OA.Q16_PRE + OA.Q_MAIN, query16h_constraints(4 * R + F), NP)
    rp[ROOTS] = roots_program(NP)
    rp[P2TH] = O.air_program(PTH_PRE + TA.T_WIDTH, NP, [(sel, terms) for _, sel, terms in p2th_constraints(W, NP)])
    rp[ROWSUM16H] = _program(RS16H_PRE + RS_MAIN, rowsum16h_constraints(), NP)
    return rp + [_program(OPN_PRE + OP_MAIN, opened16_constraints(), NP)]


def interactions(R, lf):
    """by table number"""
    rp = RPA.interactions(R, lf)
    S, Rv = O.SEND, O.RECEIVE
    e4 = lambda c: [c, c + 1, c + 2, c + 3]
    ent = lambda tab: [(int(s), int(m), int(bus), [int(c) for c in cols]) for s, m, bus, cols in TA._entries(tab)]
    m = RA.query_cols()
    query = ent(rp[RPA.QUERY16]) + [(Rv, QP_FIRST, bus, e4(m[name])) for bus, name in ((BUS_ZETA, "ZETA"), (BUS_YL, "YL"), (BUS_YN, "YN"), (BUS_YQ, "YQ"), (BUS_OFFN, "OFFN"))]
    RM, RT = ROOTS_PRE, PA.RT_ROOT
    roots = [(Rv, RM, PA.BUS_RT0, [PA.RT_LN, PA.RT_DEP] + e4(RT)), (Rv, RM, PA.BUS_RT1, [PA.RT_LN, PA.RT_DEP] + e4(RT + 4)),
             (Rv, 10, TA.BUS_TR0, [PA.RT_LN] + e4(RT)), (Rv, 10, TA.BUS_TR1, [PA.RT_LN] + e4(RT + 4)),
             (Rv, 10, TA.BUS_TB, [PA.RT_LN] + e4(RM + 1)), (S, RM + 5, TA.BUS_BF16, [PA.RT_LN] + e4(RM + 1))]
    roots += [(S, RT_HM, BUS_HR, [RT_HK + j, RT + j]) for j in range(8)]
    IN, o = PTH_PRE + P2.IN, PTH_PRE + P2.OUTE(7)
    PT = TA
    p2th = [(Rv, PT.PT_C0, TA.BUS_CT, [PT.PT_KEY0] + e4(IN)), (Rv, PT.PT_C1, TA.BUS_CT, [PT.PT_KEY1] + e4(IN + 4)),
            (S, PT.PT_ROOT, TA.BUS_TR0, [PT.PT_LN] + e4(IN)), (S, PT.PT_ROOT, TA.BUS_TR1, [PT.PT_LN] + e4(IN + 4)),
            (S, PT.PT_ROOT, TA.BUS_TB, [PT.PT_LN, o + 7, o + 6, o + 5, o + 4]),
            (S, PT.PT_SMP, FA.BUS_S0, [PT.PT_ROW, o + 7, o + 6, o + 5, o + 4]), (S, PT.PT_SMP, FA.BUS_S1, [PT.PT_ROW, o + 3, o + 2, o + 1, o])]
    p2th += [(Rv, PH_RM + j, BUS_HR, [PH_RK + j, IN + j]) for j in range(8)]
    p2th += [(Rv, PH_OPN, BUS_OV0, [PT.PT_ROW] + e4(IN)), (Rv, PH_OPN, BUS_OV1, [PT.PT_ROW] + e4(IN + 4)),
             (S, PH_ZM, BUS_ZETA, [o + 7, o + 6, o + 5, o + 4]), (S, PH_FM, BUS_FA, [o + 7, o + 6, o + 5, o + 4])]
    M0 = RS16H_PRE
    rowsum = [(S, OA.RP_ACT, OA.BUS_ROW, [OA.RP_TAG, OA.RP_K0] + e4(M0 + RS_V)), (S, OA.RP_ACT, OA.BUS_ROW, [OA.RP_TAG, OA.RP_K1] + e4(M0 + RS_V + 4)),
              (S, OA.RP_LAST0, OA.BUS_AT16, [OA.RP_QN] + e4(M0 + RS_T)), (S, OA.RP_LAST1, OA.BUS_AQ16, [OA.RP_QN] + e4(M0 + RS_T)),
              (Rv, RP_FIRST, BUS_FA, e4(M0 + RS_FA))]
    M0 = OPN_PRE
    opened = [(S, OQ_ACT, BUS_OV0, [OQ_ROW] + e4(M0 + OP_V)), (S, OQ_ACT, BUS_OV1, [OQ_ROW] + e4(M0 + OP_V + 4)),
              (S, OQ_ENDL, BUS_YL, e4(M0 + OP_Y)), (S, OQ_ENDN, BUS_YN, e4(M0 + OP_Y)), (S, OQ_ENDQ, BUS_YQ, e4(M0 + OP_Y)), (S, OQ_ENDL, BUS_OFFN, e4(M0 + OP_PWN)),
              (Rv, OQ_FIRST, BUS_FA, e4(M0 + OP_FA))]
    out = list(rp)
    out[QUERY16H], out[ROOTS], out[P2TH], out[ROWSUM16H] = (O.interaction_table(t) for t in (query, roots, p2th, rowsum))
    return out + [O.interaction_table(opened)]


# ---------------------------------------------------------------- the head of the chain
class Duplex:
    """the duplex challenger over width-16 Poseidon2, rate 8, remembering the input state of every permutation"""

    def __init__(self):
        self.state, self.pending, self.out, self.rows = [0] * 16, [], [], []

    def permute(self):
        s = self.pending + self.state[len(self.pending):]          # overwrite mode: the rate words behind the pending ones are kept
        self.rows.append(s)
        self.state = [int(x) for x in pyref.poseidon2(s)]
        self.pending, self.out = [], self.state[:8]

    def observe(self, words):
        for w in words:
            self.out = []
            self.pending.append(int(w))
            if len(self.pending) == 8:
                self.permute()

    def sample_ext(self):
        e = []
        for _ in range(4):
            if self.pending or not self.out:
                self.permute()
            e.append(self.out.pop())
        return e


def head_chain(hdr, troot, pubs, qroot, opened):
    """-> {"inputs": [HD][16], "alpha", "zeta", "fa": [4], "capacity": [8] as the commit phase finds it}; opened: [2 W + 8][4] in observation order"""
    d = Duplex()
    d.observe(hdr)
    d.observe(troot)
    d.observe(pubs)
    alpha = d.sample_ext()
    d.observe(qroot)
    zeta = d.sample_ext()
    d.observe([c for e in opened for c in e])
    fa = d.sample_ext()
    assert not d.pending and len(d.rows) == head_rows(len(opened) // 2 - 4, len(pubs))[1]
    return dict(inputs=d.rows, alpha=alpha, zeta=zeta, fa=fa, capacity=d.state[8:])


def head_of(view):
    R, Q, F, b, W = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"]
    return head_chain(header(R, F, b, Q, view["pow_bits"], W, len(view["pubs"])), view["troot"], view["pubs"], view["qroot"], view["opened"])


def derived_consts(view, head=None):
    """the eight constants from the head's challenges and the opened values"""
    h = head or head_of(view)
    W, op = view["W"], [[int(c) for c in e] for e in view["opened"]]
    return OA.consts_of(h["fa"], h["zeta"], op[:W], op[W:2 * W], op[2 * W:], W, view["H"] - view["b"])


_PAD = None


def p2th_main(inputs, lr):
    global _PAD
    if _PAD is None:
        _PAD = P2.row([0] * 16)[0][:TA.T_WIDTH]
    return np.array([P2.row(s)[0][:TA.T_WIDTH] for s in inputs] + [_PAD] * ((1 << lr) - len(inputs)), dtype=np.uint64).astype(np.uint32)


def opened16_main(opened, fa, W, lr=None):
    """OPENED16's main trace -> (trace [2^lr][36], {"YL", "YN", "YQ", "OFFN"} as its segment ends hold them)"""
    lr = A.lg(W + 4, 6) if lr is None else lr
    fa = [int(c) for c in fa]
    fa2 = pyref.ext_mul(fa, fa)
    t = np.zeros((1 << lr, OP_MAIN), dtype=np.uint64)
    t[:, OP_FA:OP_FA + 4], t[:, OP_FA2:OP_FA2 + 4] = fa, fa2
    ends = {}
    for r in range(W + 4):
        if r in (0, W // 2, W):
            pw, y = [1, 0, 0, 0], [0, 0, 0, 0]
        v0, v1 = [int(c) for c in opened[2 * r]], [int(c) for c in opened[2 * r + 1]]
        tt = A.e_add(v0, pyref.ext_mul(fa, v1))
        pt = pyref.ext_mul(pw, tt)
        y = A.e_add(y, pt)
        pwn = pyref.ext_mul(pw, fa2)
        t[r, OP_V:OP_V + 8] = v0 + v1
        for col, val in ((OP_PW, pw), (OP_T, tt), (OP_PT, pt), (OP_Y, y), (OP_PWN, pwn)):
            t[r, col:col + 4] = val
        if r == W // 2 - 1:
            ends["YL"], ends["OFFN"] = list(y), list(pwn)
        if r == W - 1:
            ends["YN"] = list(y)
        if r == W + 3:
            ends["YQ"] = list(y)
        pw = pwn
    return t.astype(np.uint32), ends


def head_traces(R, F, b, Q, pow_bits, W, pubs, troot, qroot, opened, roots, final_poly, witness):
    """what zkhip_fri16_head_gen_traces makes, from the same inputs -> (P2TH main, SAMPLES main, OPENED16 main, the eight constants {name: [4]}, the capacity)"""
    H, NP = 4 * R + F + b, len(pubs)
    C, S, NT = TA.chain_rows(R, F, Q)
    h = head_chain(header(R, F, b, Q, pow_bits, W, NP), troot, pubs, qroot, opened)
    ch = TA.chain(h["capacity"], roots, final_poly, witness, F, Q)
    _, smain, _ = FA.samples_tables(H - 1, Q, ch["words"], A.lg(S), base=head_rows(W, NP)[1] + R + C)
    omain, ends = opened16_main(opened, h["fa"], W)
    g = pyref.two_adic_generator(H - b)
    consts = dict(FA=h["fa"], ZETA=h["zeta"], ZNX=[c * g % P for c in h["zeta"]], YL=ends["YL"], YN=ends["YN"], YQ=ends["YQ"], OFFN=ends["OFFN"],
                  OFFQ=pyref.ext_mul(ends["OFFN"], ends["OFFN"]))
    return p2th_main(h["inputs"] + ch["inputs"], A.lg(len(h["inputs"]) + NT)), smain, omain, consts, h["capacity"]


# ---------------------------------------------------------------- tables of a view
def p2th_pre(R, F, b, Q, pow_bits, W, NP, lr):
    """P2TH's preprocessed schedule: a function of the shape and NP alone"""
    a, HD = head_rows(W, NP)
    C, S, NT = TA.chain_rows(R, F, Q)
    hdr = header(R, F, b, Q, pow_bits, W, NP)
    pre = np.zeros((1 << lr, PTH_PRE), dtype=np.uint32)
    for r in range(HD):
        pre[r, TA.PT_SPG] = int(r > 0)
        if r < a:
            for j in range(8):
                pos = 8 * r + j
                if pos >= STREAM + NP:
                    pre[r, TA.PT_K + j] = 1
                elif pos < 10:
                    pre[r, PH_HF + j], pre[r, PH_HV + j] = 1, hdr[pos]
                elif pos < STREAM:
                    pre[r, PH_RK + j], pre[r, PH_RM + j] = pos - 10, 1
                else:
                    pre[r, PH_PUBI + r] = 1
        elif r == a:
            pre[r, PH_RK:PH_RK + 8], pre[r, PH_RM:PH_RM + 8], pre[r, PH_ZM] = range(8, 16), 1, 1
        else:
            pre[r, PH_OPN], pre[r, TA.PT_ROW] = 1, r
    pre[HD - 1, PH_FM] = FA_RECEIVERS
    old = TA.p2t_pre(R, F, Q)
    pre[HD:HD + NT, :TA.PT_PRE] = old[:NT]
    pre[HD:HD + NT, TA.PT_SPG] = 1
    for r in range(NT):
        if old[r, TA.PT_SMP]:
            pre[HD + r, TA.PT_ROW] = HD + r
    return pre


def opened16_pre(W, NP, lr):
    a = head_rows(W, NP)[0]
    pre = np.zeros((1 << lr, OPN_PRE), dtype=np.uint32)
    for i in range(W + 4):
        first = 0 if i < W // 2 else (W // 2 if i < W else W)
        pre[i, :7] = [1, int(i != first), a + 1 + i, int(i == W // 2 - 1), int(i == W - 1), int(i == W + 3), int(i == 0)]
    return pre


def key_tables(view):
    """the key's tables by table number (None: no preprocessed columns): roots, final coefficients, header constants and schedules -- no opened word, no constant"""
    R, Q, F, b, H, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["H"], view["W"], len(view["pubs"])
    C, S, NT = TA.chain_rows(R, F, Q)
    lr = log_rows(R, F, b, Q, W, NP)
    rk = RPA.key_tables(view)
    tq = rk[RPA.QUERY16].copy()
    tq[0, QP_FIRST] = 1
    tr = np.zeros((1 << lr[ROOTS], ROOTS_PRE), dtype=np.uint32)
    tr[:, :PA.ROOTS_PRE] = rk[RPA.ROOTS]
    for tree in range(2):
        tr[R + tree, RT_HM], tr[R + tree, RT_HK:RT_HK + 8] = 1, range(8 * tree, 8 * tree + 8)
    ts = FA.samples_tables(H - 1, Q, [[0] * 8] * S, lr[SAMPLES], base=head_rows(W, NP)[1] + R + C)[0]
    trs = np.zeros((1 << lr[ROWSUM16H], RS16H_PRE), dtype=np.uint32)
    trs[:, :OA.RS16_PRE] = rk[RPA.ROWSUM16]
    trs[0, RP_FIRST] = 1
    return [None, rk[RPA.FINAL], None, tq, rk[RPA.COEFFS], tr, p2th_pre(R, F, b, Q, view["pow_bits"], W, NP, lr[P2TH]), ts, trs, None, opened16_pre(W, NP, lr[OPENED16])]


def public_values(view):
    return [int(x) for x in view["pubs"]]


def tables(view, p24l=None, honest=True, p24r=None):
    """by table number: (main traces, preprocessed traces).  honest: the view's constants and capacity are the ones the head gives"""
    R, Q, F, b, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"], len(view["pubs"])
    lr = log_rows(R, F, b, Q, W, NP)
    h = head_of(view)
    if honest:
        assert [int(c) for c in view["capacity"]] == h["capacity"], "the view's capacity is not the one the head of the transcript leaves"
        got = derived_consts(view, h)
        for name in OA.CONSTS:
            assert [int(c) for c in view["consts"][name]] == got[name], "the view's %s is not the derived one" % name
    rm, _ = RPA.tables(view, p24l, honest, p24r)
    ch = TA.chain(view["capacity"], view["roots"], view["final_poly"], view["witness"], F, Q)
    omain, _ = opened16_main(view["opened"], h["fa"], W, lr[OPENED16])
    main = list(rm)
    main[P2TH] = p2th_main(h["inputs"] + ch["inputs"], lr[P2TH])
    return main + [omain], key_tables(view)


def machine(view, p24l=None, honest=True, p24r=None):
    """-> (main traces, preprocessed traces, programs, interaction tables, public values) in machine order"""
    R, Q, F, b, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"], len(view["pubs"])
    assert shape_ok(R, F, b, Q, view["pow_bits"], W, NP)
    main, pre = tables(view, p24l, honest, p24r)
    progs, tabs = programs(R, F, b, view["pow_bits"], W, NP), interactions(R, F + b)
    o = order(R, F, b, Q, W, NP)
    return [main[i] for i in o], [pre[i] for i in o], [progs[i] for i in o], [tabs[i] for i in o], public_values(view)


# ---------------------------------------------------------------- views
def golden_view(name, GOLDEN, load):
    """the row-paths view of a committed fold-16 proof plus "pubs" (its public values), "opened" [2 W + 8][4] in observation order and "alpha" (pyverify reads it)"""
    g = GOLDEN[name]
    s = g["shape"]
    base = RPA.golden_view(name, GOLDEN, load)
    pv_ = {}
    pyverify.verify(load(name).tobytes(), g["log_n"], g["width"], g["public"], log_blowup=s[0], num_queries=s[1], pow_bits=s[2], logup_pairs=s[3], log_fold=4,
                    log_final=s[5], hash_width=s[6], code_width=s[7] if len(s) > 7 else 0, view=pv_)
    opened = [[int(c) for c in e] for e in pv_["loc"] + pv_["nxt"] + pv_["qz"]]
    return dict(base, pubs=[int(x) for x in g["public"]], opened=opened, alpha=[int(c) for c in pv_["alpha"]])


def _eval_columns(coeffs, xs):
    """polynomials [cols][n] (base field, lowest coefficient first) at the base-field points xs -> [len(xs)][cols]"""
    x = np.array(xs, dtype=np.uint64).reshape(-1, 1)
    acc = np.zeros((len(xs), len(coeffs)), dtype=np.uint64)
    for k in range(len(coeffs[0]) - 1, -1, -1):
        acc = (acc * x + np.array([c[k] for c in coeffs], dtype=np.uint64)) % P
    return acc


def _eval_ext(coeffs, z):
    """a base-field polynomial at the extension point z"""
    acc = [0, 0, 0, 0]
    for c in reversed(coeffs):
        acc = pyref.ext_mul(acc, z)
        acc[0] = (acc[0] + int(c)) % P
    return acc


@functools.lru_cache(maxsize=None)
def honest_view(R, F, b, Q, W, NP, seed=1, pow_bits=TA.POW_BITS):
    """an honest instance from the transcript's first word on: W trace columns and 8 quotient columns, random polynomials of degree < N = 2^(4 R + F), committed
    over the coset g <w_{2^H}> as two width-24 Merkle trees; NP public values drawn; alpha, zeta drawn by the head of the chain; the opened values are the columns
    AT zeta and zeta g_N (so the reduced openings lie on a polynomial of degree < N - 1 -- no AIR holds between the columns, and nothing here asks for one); fa
    drawn; layer 0 is the reduced opening at every point of the domain, folded by 16 with the challenges the chain draws; the final coefficients are read off the
    last layer; a witness ground; the indices drawn"""
    assert F + b <= 6, "the last layer is interpolated in plain Python"
    rng = np.random.default_rng([seed, R, F, b, Q, W, NP, 17])
    H, log_n = 4 * R + F + b, 4 * R + F
    N = 1 << log_n
    rnd = lambda n: [int(x) for x in rng.integers(0, P, n)]
    pubs = rnd(NP)
    tcols, qcols = [rnd(N) for _ in range(W)], [rnd(N) for _ in range(OA.QROW)]
    xq = [OA.point(i, H) for i in range(1 << H)]
    xs = [RA.GEN * x % P for x in xq]
    trows, qrows = _eval_columns(tcols, xs).tolist(), _eval_columns(qcols, xs).tolist()

    def tree(rows):
        levels = [[pyref.sponge24(r) for r in rows]]
        while len(levels[-1]) > 1:
            prev = levels[-1]
            levels.append([pyref.compress24(prev[2 * i], prev[2 * i + 1]) for i in range(len(prev) // 2)])
        return levels
    ttree, qtree = tree(trows), tree(qrows)
    troot, qroot = [int(x) for x in ttree[-1][0]], [int(x) for x in qtree[-1][0]]
    d = Duplex()
    d.observe(header(R, F, b, Q, pow_bits, W, NP))
    d.observe(troot)
    d.observe(pubs)
    alpha = d.sample_ext()
    d.observe(qroot)
    zeta = d.sample_ext()
    znx = [c * pyref.two_adic_generator(log_n) % P for c in zeta]
    loc, nxt, qz = [_eval_ext(c, zeta) for c in tcols], [_eval_ext(c, znx) for c in tcols], [_eval_ext(c, zeta) for c in qcols]
    opened = loc + nxt + qz
    d.observe([c for e in opened for c in e])
    fa = d.sample_ext()
    capacity = d.state[8:]
    consts = OA.consts_of(fa, zeta, loc, nxt, qz, W, log_n)
    # layer 0: the reduced opening at every point; then fold by 16, layer by layer, with the challenges the commit phase draws
    layer = []
    fp = [[1, 0, 0, 0]]
    for _ in range(max(W, OA.QROW) - 1):
        fp.append(pyref.ext_mul(fp[-1], fa))
    fpa = np.array(fp, dtype=np.uint64)
    at_all = (np.array(trows, dtype=np.uint64)[:, :, None] * fpa[None, :W, :] % P).sum(axis=1) % P
    aq_all = (np.array(qrows, dtype=np.uint64)[:, :, None] * fpa[None, :OA.QROW, :] % P).sum(axis=1) % P
    for i in range(1 << H):
        layer.append(OA.query_values(i, H, [int(c) for c in at_all[i]], [int(c) for c in aq_all[i]], consts)["RO"])
    ts = pyverify.Transcript()
    ts.state = [0] * 8 + list(capacity)
    layers, trees, roots, betas = [], [], [], []
    for l in range(R):
        h = H - 4 * l
        rows = [[c for e in layer[16 * r:16 * r + 16] for c in e] for r in range(1 << (h - 4))]
        levels = tree(rows)
        layers.append(layer)
        trees.append(levels)
        roots.append([int(x) for x in levels[-1][0]])
        ts.observe_many(roots[-1])
        beta = [int(x) for x in ts.sample_ext()]
        betas.append(beta)
        layer = [A.fold_row(r, h - 4, beta, layer[16 * r:16 * r + 16])[1][3][0] for r in range(1 << (h - 4))]
    lf = F + b
    pts = [OA.point(i, lf) for i in range(1 << lf)]
    n = 1 << lf
    inv_n = pow(n, P - 2, P)
    coeffs = [[sum(layer[i][c] * pow(pts[i], (n - k) % n, P) for i in range(n)) * inv_n % P for c in range(4)] for k in range(n)]      # the inverse transform over <w_n>
    assert all(c == [0, 0, 0, 0] for c in coeffs[1 << F:]), "the last layer is not of degree < 2^F"
    final_poly = coeffs[:1 << F]
    for c in final_poly:
        ts.observe_many(c)
    witness = 0
    while True:
        t2 = copy.deepcopy(ts)
        t2.observe(witness)
        if t2.sample_bits(pow_bits) == 0:
            break
        witness += 1
    indices = [t2.sample_bits(H) for _ in range(Q)]
    queries, paths = [], []
    for index in indices:
        sibs, pq = [], []
        for l in range(R):
            idx = index >> (4 * l)
            row, own = idx >> 4, idx & 15
            sibs.append([list(layers[l][16 * row + j]) for j in range(16) if j != own])
            pq.append([int(c) for lvl in range(H - 4 * (l + 1)) for c in trees[l][lvl][(row >> lvl) ^ 1]])
        queries.append((index, list(layers[0][index]), sibs))
        paths.append(pq)
    path = lambda levels, i: [[int(x) for x in levels[lvl][(i >> lvl) ^ 1]] for lvl in range(H)]
    return dict(betas=betas, final_poly=final_poly, queries=queries, roots=roots, paths=paths, F=F, b=b, H=H, hash_width=24, capacity=capacity, witness=witness,
                pow_bits=pow_bits, W=W, trows=[trows[i] for i in indices], qrows=[qrows[i] for i in indices], consts=consts,
                tpaths=[path(ttree, i) for i in indices], qpaths=[path(qtree, i) for i in indices], troot=troot, qroot=qroot, pubs=pubs, opened=opened, alpha=alpha)


def view_arrays(view):
    """fri16_rowpaths_air.view_arrays plus the inner public values and the opened values [2 W + 8][4]"""
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    return RPA.view_arrays(view) + (u(view["pubs"]), u(view["opened"]))
