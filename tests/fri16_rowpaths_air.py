"""The fold-by-16 ROW-PATHS machine, written a second time -- the first is zktls_amd/csrc/fri16_chip.hip (the machine and its key), poseidon2_chip.cpp (P24R's
program) and hash.hip (p24chip_row_paths_kernel, P24R's trace).  It is the openings machine of tests/fri16_openings_air.py with a second layer-paths-style variant
of the width-24 Poseidon2 chip, P24R, where the preprocessed ROWS table stood: the opened trace row and quotient row are no longer listed in the key, they are the
leaves of Merkle paths proven here.

Statement (the 40 public values of the openings machine; the key commits the layer roots, the final coefficients, the trace root and the quotient root -- no opened
word, no index, no value):
    everything the openings machine states, and: the W words from which AT_q is summed are the leaf at the index drawn for query q of the width-24 Merkle tree of
    depth H = 4 R + F + log_blowup whose root the key lists as the trace root; the 8 words from which AQ_q is summed are the leaf at that index of the tree whose
    root it lists as the quotient root.
STILL OUTSIDE: the transcript before the commit phase (so the eight constants and where the two roots come from), lookups, the AIR identity at zeta.

Tables by number: 0 FOLD16C, 1 FINAL, 2 P24L, 4 COEFFS, 5 ROOTS, 6 P2T, 7 SAMPLES, 8 ROWSUM16: the openings machine's programs and interaction tables word for word.
ROOTS' key table gains the rows (R, H, trace root, LISTED = 0) and (R + 1, H, quotient root, LISTED = 0).  3 QUERY16: the program unchanged; preprocessed
(q, ACT, TG0 = 2 q, TG1 = 2 q + 1, LN0 = R, LN1 = R + 1, 0, 0); two more sends, (TG0, LN0, IDX) and (TG1, LN1, IDX), multiplicity ACT, on BUS_TAG.
9 P24R, main only, 552 columns: the 540 of the width-24 chip at their positions, then
    TAG LNR KP DEP | IX BL LSP M0 | K0 K1 K2 K3
One path per (query, tree), tag = 2 q + tree ascending, none shared.  A trace path: ceil(W / 16) sponge rows (block BL = 0, 1, ...; SS on the first, SPG on the
others; the last one has LSP = 1 and, when W mod 16 = 8, absorbs two groups only), then H compression rows; a quotient path: one sponge row of two groups, then H
compression rows.  On sponge rows M0 = 1, KP = 2 IX, K_i = 4 BL + i, DEP = 0; on compression rows KP = index >> level, BIT its low bit, DEP = level + 1.  A sponge
row receives (TAG, K_i, IN[4 i .. 4 i + 4]) with multiplicities M0, G1, G2, G3 on ROWSUM16's bus; the SS row receives (TAG, LNR, IX) from QUERY16; the END row
sends (LNR, DEP, digest) in two halves to ROOTS.  Padding rows: the permutation of the zero state, flags and tail zero."""
import functools

import numpy as np

import fri16_air as A
import fri16_openings_air as OA
import fri16_paths_air as PA
import fri16_transcript_air as TA
import oracle_lib as O
import poseidon2_24_air as P24
import pyref
import pyverify

P = O.P
V = O.air_var
FOLD16C, FINAL, P24L, QUERY16, COEFFS, ROOTS, P2T, SAMPLES, ROWSUM16, P24R = range(10)
NAMES = ["FOLD16C", "FINAL", "P24L", "QUERY16", "COEFFS", "ROOTS", "P2T", "SAMPLES", "ROWSUM16", "P24R"]
UNCHANGED = [FOLD16C, FINAL, P24L, COEFFS, ROOTS, P2T, SAMPLES, ROWSUM16]
BUS_ROW, BUS_TAG = OA.BUS_ROW, 84
N_PUBLIC = OA.N_PUBLIC
R_TAG, R_LNR, R_KP, R_DEP, R_IX, R_BL, R_LSP, R_M0, R_K, WIDTH_R = 540, 541, 542, 543, 544, 545, 546, 547, 548, 552
QP_TG0, QP_TG1, QP_LN0, QP_LN1 = 2, 3, 4, 5
QROW = OA.QROW
HONEST_SHAPES = [(1, 0, 1, 4, 8), (1, 0, 1, 4, 16), (2, 2, 2, 11, 24), (2, 0, 1, 3, 40)]     # (R, F, log_blowup, queries, trace width)
MAX_SAME_HEIGHT = 8                                                                # a keyed machine takes at most 8 tables of one height


def sponge_rows(W):
    return (W + 15) // 16


def log_rows(R, F, b, Q, W):
    H = 4 * R + F + b
    return TA.log_rows(R, F, b, Q) + [A.lg(Q * (W // 8 + 1), 6), A.lg(Q * (sponge_rows(W) + 1 + 2 * H), 6)]


def shape_ok(R, F, b, Q, pow_bits, W):
    """the openings machine's shapes, but those at which nine tables would have one height"""
    if not OA.shape_ok(R, F, b, Q, pow_bits, W):
        return False
    lr = log_rows(R, F, b, Q, W)
    return max(lr.count(h) for h in lr) <= MAX_SAME_HEIGHT


def order(R, F, b, Q, W):
    lr = log_rows(R, F, b, Q, W)
    return sorted(range(10), key=lambda i: (-lr[i], i))


def main_widths(lf):
    return OA.main_widths(lf)[:9] + [WIDTH_R]


PRE_WIDTHS = OA.PRE_WIDTHS[:9] + [0]


# ---------------------------------------------------------------- P24R's program
def p24r_constraints():
    """-> [(name, selector, terms)]: the permutation and the flag constraints the stand-alone chip keeps (all but the public root and count), as P24L has them; then
    the sponge chain, the path shape, tag and tree, index, depth, bus keys"""
    T = P24._term
    IN, D, BIT, CH, END, CNT, SPG, SS, G, C = P24.IN, P24.D, P24.BIT, P24.CH, P24.END, P24.CNT, P24.SPG, P24.SS, P24.G, P24.C
    ALL, FIRST, LAST, TRANS = O.SEL_ALL, O.SEL_FIRST, O.SEL_LAST, O.SEL_TRANSITION
    cons = PA.p24l_constraints()
    cons = cons[:[n for n, _, _ in cons].index("Z boolean")]                     # P24L's list up to its leaf-shape block: the chip's own part
    assert cons[-1][0] == "CNT"

    def add(name, sel, terms):
        cons.append((name, sel, [t for t in terms if t[0]]))
    M0, LSP, BL, IX, KP, DEP, TAG, LNR = R_M0, R_LSP, R_BL, R_IX, R_KP, R_DEP, R_TAG, R_LNR
    # the sponge chain
    add("M0 = SS + SPG", ALL, [T(1, [V(M0)]), T(P - 1, [V(SS)]), T(P - 1, [V(SPG)])])
    add("SS SPG = 0", ALL, [T(1, [V(SS), V(SPG)])])
    for k in (1, 2, 3):
        add("G on sponge rows only", ALL, [T(1, [V(G[k])]), T(P - 1, [V(G[k]), V(M0)])])
    add("LSP boolean", ALL, [T(1, [V(LSP), V(LSP)]), T(P - 1, [V(LSP)])])
    add("LSP on sponge rows only", ALL, [T(1, [V(LSP)]), T(P - 1, [V(LSP), V(M0)])])
    add("SS: BL = 0", ALL, [T(1, [V(SS), V(BL)])])
    add("BL' = BL + 1", TRANS, [T(1, [V(SPG, True), V(BL, True)]), T(P - 1, [V(SPG, True), V(BL)]), T(P - 1, [V(SPG, True)])])
    add("SPG' = M0 - LSP", TRANS, [T(1, [V(SPG, True)]), T(P - 1, [V(M0)]), T(1, [V(LSP)])])
    # path shape
    add("path shape: CH' = LSP + CH - END", TRANS, [T(1, [V(CH, True)]), T(P - 1, [V(LSP)]), T(P - 1, [V(CH)]), T(1, [V(END)])])
    add("the trace does not end inside a path", LAST, [T(1, [V(M0)]), T(1, [V(CH)]), T(P - 1, [V(END)])])
    add("END on a compression row", ALL, [T(1, [V(END)]), T(P - 1, [V(END), V(CH)])])
    add("sponge rows: CH = 0", ALL, [T(1, [V(M0), V(CH)])])
    add("sponge rows: BIT = 0", ALL, [T(1, [V(M0), V(BIT)])])
    for name, col in (("TAG", TAG), ("LNR", LNR)):
        add("%s constant along a path" % name, TRANS, [T(1, [V(CH, True), V(col, True)]), T(P - 1, [V(CH, True), V(col)]),
                                                       T(1, [V(SPG, True), V(col, True)]), T(P - 1, [V(SPG, True), V(col)])])
    # index
    add("sponge rows: KP = 2 IX", ALL, [T(1, [V(M0), V(KP)]), T(P - 2, [V(M0), V(IX)])])
    add("KP constant on a leaf", TRANS, [T(1, [V(SPG, True), V(KP, True)]), T(P - 1, [V(SPG, True), V(KP)])])
    add("IX constant on a leaf", TRANS, [T(1, [V(SPG, True), V(IX, True)]), T(P - 1, [V(SPG, True), V(IX)])])
    add("KP = 2 KP' + BIT", TRANS, [T(1, [V(CH, True), V(KP)]), T(P - 2, [V(CH, True), V(KP, True)]), T(P - 1, [V(CH, True), V(BIT)])])
    add("END: KP = BIT", ALL, [T(1, [V(END), V(KP)]), T(P - 1, [V(END), V(BIT)])])
    # depth
    add("sponge rows: DEP = 0", ALL, [T(1, [V(M0), V(DEP)])])
    add("DEP' = DEP + 1", TRANS, [T(1, [V(CH, True), V(DEP, True)]), T(P - 1, [V(CH, True), V(DEP)]), T(P - 1, [V(CH, True)])])
    # bus keys
    for i in range(4):
        add("K", ALL, [T(1, [V(R_K + i)]), T(P - 4, [V(M0), V(BL)]), T(P - i, [V(M0)])])
    return cons


def p24r_program(n_public=N_PUBLIC):
    return O.air_program(WIDTH_R, n_public, [(sel, terms) for _, sel, terms in p24r_constraints()])


def constraint_names(table, pow_bits=0):
    if table == P24R:
        return [n for n, _, _ in p24r_constraints()]
    if table == P24L:
        return PA.constraint_names()
    return OA.constraint_names(table, pow_bits)


def programs(R, F, b, pow_bits):
    """by table number"""
    return OA.programs(R, F, b, pow_bits)[:9] + [p24r_program()]


def interactions(R, lf):
    """by table number"""
    oi = OA.interactions(R, lf)
    S, Rv = O.SEND, O.RECEIVE
    idx = OA.RA.query_cols()["IDX"]
    query = [(int(s), int(m), int(bus), [int(c) for c in cols]) for s, m, bus, cols in TA._entries(oi[OA.QUERY16])]
    query += [(S, OA.QP_ACT, BUS_TAG, [QP_TG0, QP_LN0, idx]), (S, OA.QP_ACT, BUS_TAG, [QP_TG1, QP_LN1, idx])]
    o7 = P24.OUTE(7)
    mult = [R_M0, P24.G[1], P24.G[2], P24.G[3]]
    p24r = [(Rv, mult[i], BUS_ROW, [R_TAG, R_K + i] + [P24.IN + 4 * i + c for c in range(4)]) for i in range(4)]
    p24r.append((Rv, P24.SS, BUS_TAG, [R_TAG, R_LNR, R_IX]))
    p24r.append((S, P24.END, PA.BUS_RT0, [R_LNR, R_DEP] + [o7 + c for c in range(4)]))
    p24r.append((S, P24.END, PA.BUS_RT1, [R_LNR, R_DEP] + [o7 + 4 + c for c in range(4)]))
    return oi[:QUERY16] + [O.interaction_table(query)] + oi[QUERY16 + 1:9] + [O.interaction_table(p24r)]


# ---------------------------------------------------------------- P24R's trace
_PAD = None


def tail(tag=0, lnr=0, kp=0, dep=0, ix=0, bl=0, lsp=0, m0=0):
    return [tag, lnr, kp, dep, ix, bl, lsp, m0] + ([4 * bl + i for i in range(4)] if m0 else [0, 0, 0, 0])


def path_rows(p, tag, lnr, index, leaf, sibs):
    """the ceil(len(leaf) / 16) + len(sibs) rows of path number p -> (rows, end digest)"""
    rows, out = [], [0] * 24
    nb = sponge_rows(len(leaf))
    for k in range(nb):
        blk = leaf[16 * k:16 * k + 16]
        state = [int(x) for x in blk] + (out[len(blk):16] if k else [0] * (16 - len(blk))) + out[16:]
        r, out = P24.row(state, 0, 0, 0, p, 1 if k else 0, 0 if k else 1, len(blk) // 4 - 1)
        rows.append(r + tail(tag, lnr, 2 * index, 0, index, k, int(k == nb - 1), 1))
    digest = out[:8]
    for lvl, sib in enumerate(sibs):
        bit, end = (index >> lvl) & 1, 1 if lvl == len(sibs) - 1 else 0
        sib = [int(x) for x in sib]
        r, out = P24.row((sib + digest if bit else digest + sib) + [0] * 8, bit, 1, end, p + end)
        rows.append(r + tail(tag, lnr, index >> lvl, lvl + 1))
        digest = out[:8]
    return rows, digest


def row_path_traces(R, H, W, trows, qrows, indices, tpaths, qpaths, lr=None):
    """what zkhip_fri16_rowpaths_gen_trace makes from raw rows, siblings and indices -> (trace [2^lr][552], path ends [2 Q][8] in tag order)"""
    global _PAD
    Q = len(indices)
    lr = A.lg(Q * (sponge_rows(W) + 1 + 2 * H), 6) if lr is None else lr
    rows, ends = [], []
    for q in range(Q):
        for tree, (leaf, sibs) in enumerate(((trows[q], tpaths[q]), (qrows[q], qpaths[q]))):
            assert len(sibs) == H and len(leaf) == (QROW if tree else W)
            r, digest = path_rows(2 * q + tree, 2 * q + tree, R + tree, int(indices[q]), [int(x) for x in leaf], sibs)
            rows += r
            ends.append(digest)
    if _PAD is None:
        _PAD = P24.row([0] * 24)[0]
    pad = list(_PAD)
    pad[P24.CNT] = len(ends)
    assert len(rows) <= 1 << lr
    rows += [pad + tail()] * ((1 << lr) - len(rows))
    return np.array(rows, dtype=np.uint64).astype(np.uint32), ends


# ---------------------------------------------------------------- tables of a view
def key_tables(view):
    """the key's tables by table number (None: no preprocessed columns): roots and final coefficients, no opened word"""
    R, Q, F, b, H, W = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["H"], view["W"]
    lr = log_rows(R, F, b, Q, W)
    ti = TA.key_tables(view)
    tq = np.zeros((1 << lr[QUERY16], OA.Q16_PRE), dtype=np.uint32)
    for q in range(Q):
        tq[q, :6] = [q, 1, 2 * q, 2 * q + 1, R, R + 1]
    tr = ti[TA.ROOTS].copy()
    for tree, root in enumerate((view["troot"], view["qroot"])):
        tr[R + tree, PA.RT_LN], tr[R + tree, PA.RT_DEP], tr[R + tree, PA.RT_ROOT:PA.RT_ROOT + 8] = R + tree, H, root
    return [None, ti[TA.FINAL], None, tq, ti[TA.COEFFS], tr, ti[TA.P2T], ti[TA.SAMPLES], OA.rowsum16_pre(Q, W, lr[ROWSUM16]), None]


def public_values(view):
    return OA.public_values(view)


def tables(view, p24l=None, honest=True, p24r=None):
    """by table number: (main traces, preprocessed traces); p24r: a row_path_traces(...) result made earlier"""
    R, Q, F, b, H, W = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["H"], view["W"]
    lr = log_rows(R, F, b, Q, W)
    om, _ = OA.tables(view, p24l, honest)
    indices = [q[0] for q in view["queries"]]
    trace, ends = row_path_traces(R, H, W, view["trows"], view["qrows"], indices, view["tpaths"], view["qpaths"], lr[P24R]) if p24r is None else p24r
    if honest:
        for p, e in enumerate(ends):
            assert e == [int(x) for x in (view["qroot"] if p & 1 else view["troot"])], "query %d: a row's path does not end in its root" % (p // 2)
    rmain = om[OA.ROOTS].copy()
    rmain[R, 0] = rmain[R + 1, 0] = Q
    return om[:ROOTS] + [rmain] + om[ROOTS + 1:P24R] + [trace], key_tables(view)


def machine(view, p24l=None, honest=True, p24r=None):
    """-> (main traces, preprocessed traces, programs, interaction tables, public values) in machine order"""
    R, Q, F, b, W = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"]
    assert shape_ok(R, F, b, Q, view["pow_bits"], W)
    main, pre = tables(view, p24l, honest, p24r)
    progs, tabs = programs(R, F, b, view["pow_bits"]), interactions(R, F + b)
    o = order(R, F, b, Q, W)
    return [main[i] for i in o], [pre[i] for i in o], [progs[i] for i in o], [tabs[i] for i in o], public_values(view)


# ---------------------------------------------------------------- views
def golden_view(name, GOLDEN, load):
    """the openings view of a committed fold-16 proof plus "tpaths" / "qpaths" [Q][H][8] and "troot" / "qroot", as the proof holds them (pyverify reads it)"""
    g = GOLDEN[name]
    s = g["shape"]
    base = OA.golden_view(name, GOLDEN, load)
    return dict(base, **parse_row_paths(load(name).tobytes(), g["log_n"], g["width"], g["public"], s))


def parse_row_paths(proof_bytes, log_n, width, public, s):
    pv_ = {}
    pyverify.verify(proof_bytes, log_n, width, public, log_blowup=s[0], num_queries=s[1], pow_bits=s[2], logup_pairs=s[3], log_fold=4, log_final=s[5], hash_width=s[6],
                    code_width=s[7] if len(s) > 7 else 0, view=pv_)
    ints = lambda path: [[int(x) for x in d] for d in path]
    return dict(tpaths=[ints(o["tpath"]) for o in pv_["openings"]], qpaths=[ints(o["qpath"]) for o in pv_["openings"]],
                troot=[int(x) for x in pv_["trace_root"]], qroot=[int(x) for x in pv_["quot_root"]])


def sparse_tree(leaves, H, seed):
    """a Merkle tree of depth H known only where it is opened: leaves {index: words}; a node with an opened leaf below is the compression of its children, any
    other node a digest drawn from (seed, level, index) -> (root, node(level, index))"""
    touched = {(lvl, i >> lvl) for i in leaves for lvl in range(H + 1)}
    memo = {}

    def node(lvl, i):
        if (lvl, i) not in memo:
            if (lvl, i) not in touched:
                memo[(lvl, i)] = [int(x) for x in np.random.default_rng([seed, lvl, i]).integers(0, P, 8)]
            elif lvl == 0:
                memo[(lvl, i)] = pyref.sponge24(leaves[i])
            else:
                memo[(lvl, i)] = pyref.compress24(node(lvl - 1, 2 * i), node(lvl - 1, 2 * i + 1))
        return memo[(lvl, i)]
    return node(H, 0), node


def with_row_trees(view, seed=1):
    """give an openings view its two trees: queries that draw one index must open one leaf there (the later query's rows are made the earlier one's only when
    the caller has arranged that; otherwise the indices are distinct)"""
    H = view["H"]
    indices = [q[0] for q in view["queries"]]
    out = {}
    for tree, rows in (("t", view["trows"]), ("q", view["qrows"])):
        leaves = {}
        for q, i in enumerate(indices):
            assert leaves.setdefault(i, [int(x) for x in rows[q]]) == [int(x) for x in rows[q]], "two queries open one leaf differently"
        root, node = sparse_tree(leaves, H, [seed, 0 if tree == "t" else 1, 24])
        out[tree + "root"] = root
        out[tree + "paths"] = [[node(lvl, (i >> lvl) ^ 1) for lvl in range(H)] for i in indices]
    return dict(view, **out)


@functools.lru_cache(maxsize=None)
def honest_view(R, F, b, Q, W, seed=1, pow_bits=TA.POW_BITS):
    """an honest instance: the openings machine's honest view with a trace tree and a quotient tree through its opened rows.  Two queries that draw one index
    (their chains then start from one value) are given the same rows"""
    base = OA.honest_view(R, F, b, Q, W, seed, pow_bits)
    trows, qrows, first = [list(r) for r in base["trows"]], [list(r) for r in base["qrows"]], {}
    for q, (index, _, _) in enumerate(base["queries"]):
        f = first.setdefault(index, q)
        trows[q], qrows[q] = trows[f], qrows[f]
    view = dict(base, trows=trows, qrows=qrows)
    assert OA.reduced_openings(view) == [list(q[1]) for q in base["queries"]]
    return with_row_trees(view, seed)


def view_arrays(view):
    """fri16_openings_air.view_arrays plus trace paths [Q][H][8], quotient paths [Q][H][8], the trace root and the quotient root"""
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    return OA.view_arrays(view) + (u(view["tpaths"]), u(view["qpaths"]), u(view["troot"]), u(view["qroot"]))
