"""The fold-by-16 PATHS machine, written a second time -- the first is zktls_amd/csrc/fri16_chip.hip (the machine), poseidon2_chip.cpp (P24L's
program) and hash.hip (P24L's trace kernel).  It is the fold-by-16 FRI machine of tests/fri16_air.py with a layer-paths variant of the
width-24 Poseidon2 chip (tests/poseidon2_24_air.py) where the preprocessed LAYERS table stood, and a preprocessed ROOTS table: the key holds
the layer roots and no layer value.

Statement (public values: beta_0 .. beta_{R-1}; the key commits QUERIES, COEFFS, ROOTS and FINAL's schedule):
    every query listed in QUERIES, taken as entry index & 15 of row index >> 4 of layer 0, opens the layer commitments listed in ROOTS row by
    row -- each of its R rows is the 64-word leaf at its row index of the width-24 Merkle tree whose root ROOTS lists for that layer -- and
    folds through these rows, at the points its index fixes, to the value at its last point of the polynomial whose coefficients are listed
    in COEFFS.
Still outside: the transcript (challenges, query indices), the reduced openings, the trace / quotient openings.

Tables, by number: 0 FOLD16, 1 FINAL, 3 QUERIES, 4 COEFFS exactly as in fri16_air (imported, not rewritten); 2 P24L; 5 ROOTS.
P24L, main only, 552 columns: the 540 of the width-24 chip at their positions, then
    LN KP M DEP | Z0 Z1 Z2 Z3 | K0 K1 K2 K3
One path per DISTINCT (layer, row), ascending: four sponge rows over the row's 64 words (Z_k = 1 on sponge row k; SS = Z0, SPG = Z1 + Z2 + Z3,
G1 = G2 = G3 = 1; KP = 2 row, BIT = 0, DEP = 0; K_i = 16 row + 4 k + i; M = the queries that read the row), then lh_l = H - 4 (l + 1)
compression rows (CH = 1; KP = row >> level, BIT = its low bit, DEP = level + 1; M = Z = K = 0), the last with END = 1.  Sponge row k receives
(LN, K_i, IN[4 i .. 4 i + 4]), i = 0..3, with multiplicity M on FOLD16's bus; the END row sends (LN, DEP, OUT[0..4]) and (LN, DEP, OUT[4..8]) to
ROOTS.  CNT counts END rows as in the stand-alone chip (no public count).  Padding rows: the permutation of the zero state, flags and tail zero.
The leaf is EXACTLY four full sponge rows and then a compression row: pyref.sponge24 over one 16-word block equals pyref.compress24 of its
halves, so a leaf of floating length would let an inner node's two children pass for a leaf one level up.
ROOTS, preprocessed (layer, depth, root[8], 0, 0), 2^5 rows; main column 0: the number of path ends of the layer (the prover's)."""
import numpy as np

import fri16_air as A
import oracle_lib as O
import poseidon2_24_air as P24
import pyref

P = O.P
V = O.air_var
L_LN, L_KP, L_M, L_DEP, L_Z, L_K, WIDTH_L = 540, 541, 542, 543, 544, 548, 552
LEAF_ROWS = 4
BUS_RT0, BUS_RT1 = 74, 75
ROOTS_PRE, RT_LN, RT_DEP, RT_ROOT = 12, 0, 1, 2
FOLD16, FINAL, P24L, QUERIES, COEFFS, ROOTS = range(6)


def depths(R, F, b):
    H = 4 * R + F + b
    return [H - 4 * (l + 1) for l in range(R)]


def log_rows(R, F, b, Q):
    """heights by table number: functions of the shape alone (P24L has room for all-distinct rows)"""
    lr = A.log_rows(R, F, Q)
    return [lr[0], lr[1], A.lg(Q * sum(LEAF_ROWS + d for d in depths(R, F, b))), lr[3], lr[4], A.lg(R)]


def order(R, F, b, Q):
    lr = log_rows(R, F, b, Q)
    return sorted(range(6), key=lambda i: (-lr[i], i))


def main_widths(lf):
    return [A.width_of(lf), A.FIN_MAIN, WIDTH_L, A.TAB_MAIN, A.TAB_MAIN, A.TAB_MAIN]


PRE_WIDTHS = [0, A.FIN_PRE, 0, A.Q_PRE, A.C_PRE, ROOTS_PRE]


# ---------------------------------------------------------------- P24L's program
def p24l_constraints():
    """-> [(name, selector, terms)]: the permutation, the flag constraints the stand-alone chip keeps (all but the public root and count), then
    leaf shape, path shape, index, depth, receives"""
    T = P24._term
    IN, D, BIT, CH, END, CNT, SPG, SS, G, C = P24.IN, P24.D, P24.BIT, P24.CH, P24.END, P24.CNT, P24.SPG, P24.SS, P24.G, P24.C
    o7 = P24.OUTE(7)
    Z0, Z1, Z2, Z3 = L_Z, L_Z + 1, L_Z + 2, L_Z + 3
    ALL, FIRST, LAST, TRANS = O.SEL_ALL, O.SEL_FIRST, O.SEL_LAST, O.SEL_TRANSITION
    cons = [("permutation", sel, terms) for sel, terms in P24.permutation_constraints()]

    def add(name, sel, terms):
        cons.append((name, sel, [t for t in terms if t[0]]))
    for j in range(8):
        add("D", ALL, [T(1, [V(D + j)]), T(P - 1, [V(IN + j)]), T(1, [V(BIT), V(IN + j)]), T(P - 1, [V(BIT), V(IN + 8 + j)])])
    for f in (BIT, CH, END, SPG, SS, G[1], G[2], G[3]):
        add("boolean", ALL, [T(1, [V(f), V(f)]), T(P - 1, [V(f)])])
    for k in (2, 3):
        add("G prefix", ALL, [T(1, [V(G[k])]), T(P - 1, [V(G[k - 1]), V(G[k])])])
    for k in (1, 2, 3):
        add("C", ALL, [T(1, [V(C[k])]), T(P - 1, [V(SPG)]), T(1, [V(SPG), V(G[k])])])
    add("first row", FIRST, [T(1, [V(CH)])])
    add("first row", FIRST, [T(1, [V(SPG)])])
    for j in range(8):
        add("capacity zero unless SPG", ALL, [T(1, [V(IN + 16 + j)]), T(P - 1, [V(SPG), V(IN + 16 + j)])])
    for k in (1, 2, 3):
        for j in P24.group_words(k):
            add("SS: groups not absorbed are zero", ALL, [T(1, [V(SS), V(IN + j)]), T(P - 1, [V(SS), V(G[k]), V(IN + j)])])
    for j in range(8):
        add("SPG: capacity follows", TRANS, [T(1, [V(SPG, True), V(IN + 16 + j, True)]), T(P - 1, [V(SPG, True), V(o7 + 16 + j)])])
    for k in (1, 2, 3):
        for j in P24.group_words(k):
            add("C: carried groups", TRANS, [T(1, [V(C[k], True), V(IN + j, True)]), T(P - 1, [V(C[k], True), V(o7 + j)])])
    for j in range(8):
        add("CH: digest follows", TRANS, [T(1, [V(CH, True), V(D + j, True)]), T(P - 1, [V(CH, True), V(o7 + j)])])
    add("CNT", FIRST, [T(1, [V(CNT)]), T(P - 1, [V(END)])])
    add("CNT", TRANS, [T(1, [V(CNT, True)]), T(P - 1, [V(CNT)]), T(P - 1, [V(END, True)])])
    # leaf shape
    for k in range(4):
        add("Z boolean", ALL, [T(1, [V(L_Z + k), V(L_Z + k)]), T(P - 1, [V(L_Z + k)])])
    add("Z0 = SS", ALL, [T(1, [V(Z0)]), T(P - 1, [V(SS)])])
    add("SPG = Z1 + Z2 + Z3", ALL, [T(1, [V(SPG)]), T(P - 1, [V(Z1)]), T(P - 1, [V(Z2)]), T(P - 1, [V(Z3)])])
    add("SS SPG = 0", ALL, [T(1, [V(SS), V(SPG)])])
    for k in (1, 2, 3):
        add("leaf blocks are full: G = SS + SPG", ALL, [T(1, [V(G[k])]), T(P - 1, [V(SS)]), T(P - 1, [V(SPG)])])
    for k in range(3):
        add("leaf rows step: Z' = Z", TRANS, [T(1, [V(L_Z + k + 1, True)]), T(P - 1, [V(L_Z + k)])])
    # path shape
    add("path shape: CH' = Z3 + CH - END", TRANS, [T(1, [V(CH, True)]), T(P - 1, [V(Z3)]), T(P - 1, [V(CH)]), T(1, [V(END)])])
    add("the trace does not end inside a path", LAST, [T(1, [V(Z0)]), T(1, [V(Z1)]), T(1, [V(Z2)]), T(1, [V(Z3)]), T(1, [V(CH)]), T(P - 1, [V(END)])])
    add("END on a compression row", ALL, [T(1, [V(END)]), T(P - 1, [V(END), V(CH)])])
    add("sponge rows: CH = 0", ALL, [T(1, [V(SS), V(CH)]), T(1, [V(SPG), V(CH)])])
    add("sponge rows: BIT = 0", ALL, [T(1, [V(SS), V(BIT)]), T(1, [V(SPG), V(BIT)])])
    add("LN constant along a path", TRANS, [T(1, [V(CH, True), V(L_LN, True)]), T(P - 1, [V(CH, True), V(L_LN)]),
                                             T(1, [V(SPG, True), V(L_LN, True)]), T(P - 1, [V(SPG, True), V(L_LN)])])
    # index
    add("KP constant on a leaf", TRANS, [T(1, [V(SPG, True), V(L_KP, True)]), T(P - 1, [V(SPG, True), V(L_KP)])])
    add("KP = 2 KP' + BIT", TRANS, [T(1, [V(CH, True), V(L_KP)]), T(P - 2, [V(CH, True), V(L_KP, True)]), T(P - 1, [V(CH, True), V(BIT)])])
    add("END: KP = BIT", ALL, [T(1, [V(END), V(L_KP)]), T(P - 1, [V(END), V(BIT)])])
    # depth
    add("sponge rows: DEP = 0", ALL, [T(1, [V(SS), V(L_DEP)]), T(1, [V(SPG), V(L_DEP)])])
    add("DEP' = DEP + 1", TRANS, [T(1, [V(CH, True), V(L_DEP, True)]), T(P - 1, [V(CH, True), V(L_DEP)]), T(P - 1, [V(CH, True)])])
    # receives
    add("M on sponge rows only", ALL, [T(1, [V(L_M)]), T(P - 1, [V(L_M), V(SS)]), T(P - 1, [V(L_M), V(SPG)])])
    for i in range(4):
        add("K", ALL, [T(1, [V(L_K + i)]), T(P - 8, [V(SS), V(L_KP)]), T(P - 8, [V(SPG), V(L_KP)]), T(P - i, [V(Z0)]), T(P - (4 + i), [V(Z1)]),
                       T(P - (8 + i), [V(Z2)]), T(P - (12 + i), [V(Z3)])])
    return cons


def p24l_program(n_public):
    return O.air_program(WIDTH_L, n_public, [(sel, terms) for _, sel, terms in p24l_constraints()])


def constraint_names():
    return [name for name, _, _ in p24l_constraints()]


def programs(R, lf):
    """by table number"""
    a = A.programs(R, lf)
    return [a[A.FOLD16], a[A.FINAL], p24l_program(4 * R), a[A.QUERIES], a[A.COEFFS], A.table_program(R, ROOTS_PRE)]


def interactions(R):
    """by table number"""
    a = A.interactions(R)
    o7 = P24.OUTE(7)
    p24l = [(O.RECEIVE, L_M, A.BUS_L16, [L_LN, L_K + i] + [P24.IN + 4 * i + c for c in range(4)]) for i in range(4)]
    p24l.append((O.SEND, P24.END, BUS_RT0, [L_LN, L_DEP] + [o7 + c for c in range(4)]))
    p24l.append((O.SEND, P24.END, BUS_RT1, [L_LN, L_DEP] + [o7 + 4 + c for c in range(4)]))
    roots = [(O.RECEIVE, ROOTS_PRE, BUS_RT0, [RT_LN, RT_DEP] + [RT_ROOT + c for c in range(4)]),
             (O.RECEIVE, ROOTS_PRE, BUS_RT1, [RT_LN, RT_DEP] + [RT_ROOT + 4 + c for c in range(4)])]
    return [a[A.FOLD16], a[A.FINAL], O.interaction_table(p24l), a[A.QUERIES], a[A.COEFFS], O.interaction_table(roots)]


# ---------------------------------------------------------------- traces and tables
def distinct_paths(view):
    """one path per distinct (layer, row), ascending: [(layer, row, 64 leaf words, readers, siblings [lh][8])]; readers that share a row must
    agree about its entries and its path"""
    seen = {}
    for q, (rows, xf, val) in enumerate(A.chains(view)):
        for l, r in enumerate(rows):
            flat = [int(c) for e in r["entries"] for c in e]
            pth = [int(x) for x in view["paths"][q][l]]
            assert len(pth) == 8 * r["lh"]
            e = seen.setdefault((l, r["row"]), [flat, pth, 0])
            assert e[0] == flat, "query %d layer %d disagrees about a shared row" % (q, l)
            assert e[1] == pth, "query %d layer %d disagrees about the path of a shared row" % (q, l)
            e[2] += 1
    return [(l, row, seen[(l, row)][0], seen[(l, row)][2], [seen[(l, row)][1][8 * i:8 * i + 8] for i in range(len(seen[(l, row)][1]) // 8)])
            for l, row in sorted(seen)]


_PAD = None


def tail(ln=0, kp=0, m=0, dep=0, z=None, key=None):
    t = [ln, kp, m, dep, 0, 0, 0, 0, 0, 0, 0, 0]
    if z is not None:
        t[4 + z] = 1
        t[8:12] = [key + i for i in range(4)]
    return t


def path_rows(p, l, row, leaf, mult, sibs):
    """the 4 + lh rows of path number p -> (rows, end digest)"""
    rows, out = [], [0] * 24
    for k in range(LEAF_ROWS):
        r, out = P24.row(leaf[16 * k:16 * k + 16] + out[16:], 0, 0, 0, p, 1 if k else 0, 0 if k else 1, 3)
        rows.append(r + tail(l, 2 * row, mult, 0, k, 16 * row + 4 * k))
    digest = out[:8]
    for lvl, sib in enumerate(sibs):
        bit, end = (row >> lvl) & 1, 1 if lvl == len(sibs) - 1 else 0
        r, out = P24.row((sib + digest if bit else digest + sib) + [0] * 8, bit, 1, end, p + end)
        rows.append(r + tail(l, row >> lvl, 0, lvl + 1))
        digest = out[:8]
    return rows, digest


def p24l_trace(view, lr=None):
    """-> (trace [2^lr][552], path ends [n][8], path ends per layer [R])"""
    global _PAD
    R, Q = len(view["betas"]), len(view["queries"])
    lr = log_rows(R, view["F"], view["b"], Q)[P24L] if lr is None else lr
    rows, ends, counts = [], [], [0] * R
    for p, (l, row, leaf, mult, sibs) in enumerate(distinct_paths(view)):
        assert len(sibs) == view["H"] - 4 * (l + 1)
        r, digest = path_rows(p, l, row, leaf, mult, sibs)
        rows += r
        ends.append(digest)
        counts[l] += 1
    if _PAD is None:
        _PAD = P24.row([0] * 24)[0]
    pad = list(_PAD)
    pad[P24.CNT] = len(ends)
    assert len(rows) <= 1 << lr
    rows += [pad + tail()] * ((1 << lr) - len(rows))
    return np.array(rows, dtype=np.uint64).astype(np.uint32), ends, counts


def roots_tables(view, counts):
    """-> (preprocessed, main) of ROOTS"""
    R = len(view["betas"])
    pre = np.zeros((1 << A.lg(R), ROOTS_PRE), dtype=np.uint32)
    main = np.zeros((1 << A.lg(R), A.TAB_MAIN), dtype=np.uint32)
    for l in range(R):
        pre[l, RT_LN], pre[l, RT_DEP], pre[l, RT_ROOT:RT_ROOT + 8] = l, view["H"] - 4 * (l + 1), view["roots"][l]
        main[l, 0] = counts[l]
    return pre, main


def key_tables(view):
    """the key's tables by table number (None: no preprocessed columns) -- from the final coefficients, the queries and the roots alone"""
    fpre = A.final_tables(view)[0]
    _, tq, tc = A.key_tables(view)
    return [None, fpre, None, tq, tc, roots_tables(view, [0] * len(view["betas"]))[0]]


def tables(view, p24l=None):
    """by table number: (main traces, preprocessed traces); p24l: a p24l_trace(view) result made earlier"""
    am, ap = A.tables(view)
    trace, ends, counts = p24l_trace(view) if p24l is None else p24l
    for (l, *_), e in zip(distinct_paths(view), ends):
        assert e == [int(x) for x in view["roots"][l]], "a path does not end in its layer's root"
    rpre, rmain = roots_tables(view, counts)
    return ([am[A.FOLD16], am[A.FINAL], trace, am[A.QUERIES], am[A.COEFFS], rmain], [None, ap[A.FINAL], None, ap[A.QUERIES], ap[A.COEFFS], rpre])


def machine(view, p24l=None):
    """-> (main traces, preprocessed traces, programs, interaction tables, public values) in machine order"""
    R, Q, F, b = len(view["betas"]), len(view["queries"]), view["F"], view["b"]
    assert A.shape_ok(R, F, b, Q)
    main, pre = tables(view, p24l)
    progs, tabs = programs(R, F + b), interactions(R)
    o = order(R, F, b, Q)
    return [main[i] for i in o], [pre[i] for i in o], [progs[i] for i in o], [tabs[i] for i in o], [c for bt in view["betas"] for c in bt]


# ---------------------------------------------------------------- views
def with_trees(view, seed=1):
    """give a fri16_air.random_view Merkle trees without materialising a layer: per layer a sparse tree -- the touched leaves hashed with
    pyref's width-24 sponge, every untouched subtree a seeded random digest keyed by (layer, level, node), touched nodes compressed bottom-up --
    so all paths of a layer end in one root.  -> the view with "roots" [R][8], "paths" [query][layer] flat words and "hash_width" 24"""
    R, H = len(view["betas"]), view["H"]
    leaves = {}
    for rows, xf, val in A.chains(view):
        for l, r in enumerate(rows):
            leaves.setdefault(l, {})[r["row"]] = [int(c) for e in r["entries"] for c in e]
    roots, node_of = [], []
    for l in range(R):
        lh = H - 4 * (l + 1)
        touched = {(lvl, row >> lvl) for row in leaves[l] for lvl in range(lh + 1)}
        memo = {}

        def node(lvl, i, l=l, touched=touched, memo=memo):
            if (lvl, i) not in memo:
                if (lvl, i) not in touched:
                    memo[(lvl, i)] = [int(x) for x in np.random.default_rng([seed, l, lvl, i]).integers(0, P, 8)]
                elif lvl == 0:
                    memo[(lvl, i)] = pyref.sponge24(leaves[l][i])
                else:
                    memo[(lvl, i)] = pyref.compress24(node(lvl - 1, 2 * i), node(lvl - 1, 2 * i + 1))
            return memo[(lvl, i)]
        roots.append(node(lh, 0))
        node_of.append(node)
    paths = []
    for index, _, _ in view["queries"]:
        pq = []
        for l in range(R):
            row = index >> (4 * (l + 1))
            pq.append([c for lvl in range(H - 4 * (l + 1)) for c in node_of[l](lvl, (row >> lvl) ^ 1)])
        paths.append(pq)
    return dict(view, roots=roots, paths=paths, hash_width=24, _nodes=node_of)


def random_view(R, F, b, Q, seed=1):
    return with_trees(A.random_view(R, F, b, Q, seed=seed), seed)


def view_arrays(view):
    """fri16_air.view_arrays plus roots [R][8] and paths [Q][sum_l 8 lh_l]"""
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    return A.view_arrays(view) + (u(view["roots"]), u([c for pq in view["paths"] for pl in pq for c in pl]))
