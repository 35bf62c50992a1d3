"""The fold-by-16 FRI machine (FOLD16, FINAL and three preprocessed tables), written a second time -- the first is
zktls_amd/csrc/fri16_chip.hip: constraint programs, interaction tables, traces, the preprocessed tables and a parser of the FRI part of a
fold-16 shard proof, in plain Python on tests/pyref.py's field arithmetic.  The tests require the library's words to be EQUAL to these, and
the oracle's generic keyed-machine prover on these arrays to produce the library's proof bytes.

What the inner verifier does (tests/pyverify.py, the query loop): with H = log_n + log_blowup, R = (log_n - F) / 4 committed layers and
lf = F + log_blowup, layer l is a matrix of 2^lh rows, lh = H - 4 (l + 1), of 16 adjacent extension entries.  A query (idx, val) reads row
idx >> 4, puts val at position idx & 15, takes the other 15 entries from the proof, folds the row four times by 2 with beta, beta^2, beta^4,
beta^8 and goes on with (idx >> 4, folded); after R layers the value must be sum_j c_j xf^j, xf = w_{2^lf}^bitrev(idx, lf).

The points (derived in fold_row below and asserted there against the pair-by-pair fold of pyverify): with row = idx >> 4 and
x0 = w_{2^(lh+4)}^bitrev(row, lh), fold step s (0..3) folds pair t at x0^(2^s) w_{2^(4-s)}^bitrev(t, 3-s): one base-field value per row, the rest
constants.  x0 = prod_i w_{2^(i+5)}^{bit_i(row)}; the next row's x0' = x0^16 w_16^(-bitrev(row & 15, 4)); after the last layer x0^16 = xf.

Statement of the machine (public values: beta_0 .. beta_{R-1}, 4 words each; the key commits LAYERS, QUERIES, COEFFS):
    every query listed in QUERIES, taken as entry index & 15 of row index >> 4 of layer 0, folds through rows listed in LAYERS -- each
    listed row read exactly as often as listed -- at the points its index fixes, to the value at its last point of the polynomial whose
    coefficients are listed in COEFFS.
NOT in the machine: the Merkle paths of the layer rows (LAYERS is the table a width-24 Poseidon2 chip on the same bus replaces), the
transcript (challenges, query indices), the reduced openings.

FOLD16, main, one row per (query, layer); sections start on multiples of 4 columns:
    E[16][4]        the row's entries                                F1[8][4] F2[4][4] F3[2][4] FOLD[4]   the four fold steps
    OWN[4]          sum_j O_j E_j, the query's own entry             BETA B2 B4 B8 [4]   the layer's challenge and its squarings
    X X2 X4 X8 X16  x0 and its squarings                             XI XI2 XI4 XI8      1 / x0 and its squarings
    ROW IDX LN      row index, IDX = 16 ROW + own, layer number      ACTIVE G GX16 GT    G = ACTIVE - L_{R-1}; G X16, G T (a selector counts a degree)
    T B U TL        backward product: T = the factor of the own position's nibble in the FIRST row's x0 (1 at layer 0), B = T B' down the
                    chain, on its last row B = T TL with TL = the factor of the lf bits of ROW left there (U: product of the first two nibble forms)
    O[16]           one-hot own position                             KJ[16]   16 ROW + j ACTIVE, the bus keys of the 16 entries
    L[8]            one-hot layer (columns R .. 7 are zero)          N        the last row's remaining lf bits of ROW as up to three one-hot nibbles
Sends: the 16 entries (LN, KJ_j, E_j) with multiplicity ACTIVE to LAYERS; (IDX, OWN) with multiplicity L_0 to QUERIES; (X16, FOLD) with
multiplicity L_{R-1} to FINAL.  Padding rows are zero.
FINAL, one block of 2^F rows per query (Horner from the top coefficient down).  Preprocessed J (coefficient number, descending in a
block), FIRST, LAST, ACT, NL = ACT - LAST; main C[4], ACC[4], AX[4] = ACC X, X.  X' = X and ACC' = AX + C' under NL, ACC = C under FIRST;
receives (J, C) from COEFFS on every active row and (X, ACC) from FOLD16 on a block's last row.
LAYERS, preprocessed: per distinct (layer, row) ascending LN, KEY[16], M (queries reading it), E[16][4].  QUERIES: distinct
(index, value[4], M).  COEFFS: (j, c_j[4], M = queries).  Each has four unused main columns and one harmless identity."""
import struct

import numpy as np

import oracle_lib as O
import pyverify
from pyref import P, bitrev, ext_inv, ext_mul, two_adic_generator

V = O.air_var
INV2 = (P + 1) // 2
EXT_W = 11
E, F1, F2, F3, FOLD, OWN, BETA, B2, B4, B8 = 0, 64, 96, 112, 120, 124, 128, 132, 136, 140
X, X2, X4, X8, X16, XI, XI2, XI4, XI8, ROW, IDX, LN, ACTIVE, G, GX16, GT, T, B, U, TL = range(144, 164)
OF, KJ, L, N = 164, 180, 196, 204
STEP_IN, STEP_OUT, STEP_BETA, STEP_XI = (E, F1, F2, F3), (F1, F2, F3, FOLD), (BETA, B2, B4, B8), (XI, XI2, XI4, XI8)
BUS_L16, BUS_Q16, BUS_FIN16, BUS_COEF = 70, 71, 72, 73
# FINAL: combined row [preprocessed | main]
FIN_PRE, FIN_MAIN = 8, 16
FJ, FFIRST, FLAST, FACT, FNL = 0, 1, 2, 3, 4
FC, FACC, FAX, FX = 8, 12, 16, 20
LAY_PRE, LAY_LN, LAY_KEY, LAY_M, LAY_E = 84, 0, 1, 17, 20
Q_PRE, C_PRE, TAB_MAIN = 8, 8, 4
FOLD16, FINAL, LAYERS, QUERIES, COEFFS = range(5)
MAX_R, MAX_F, MAX_LF, MAX_Q = 5, 8, 11, 1024


def shape_ok(R, F, b, Q):
    """the shapes the machine takes; 4 R + F + b <= 27: the field has no larger two-adic domain"""
    return 1 <= R <= MAX_R and 0 <= F <= MAX_F and 1 <= b <= 3 and F + b <= MAX_LF and 1 <= Q <= MAX_Q and 4 * R + F + b <= 27


def nibbles(lf):
    """the lf bits left of ROW on a chain's last row, as nibbles: -> [bits per nibble], lowest first"""
    return [min(4, lf - 4 * k) for k in range((lf + 3) // 4)]


def width_of(lf):
    return (N + sum(1 << nb for nb in nibbles(lf)) + 3) & ~3


def bit_root(i):
    """what bit i of a layer-0 row index contributes to x0: w_{2^(i+5)}"""
    return two_adic_generator(i + 5)


def nibble_factor(first_bit, nbits, j):
    """prod_i bit_root(first_bit + i)^{bit_i(j)}"""
    f = 1
    for i in range(nbits):
        if (j >> i) & 1:
            f = f * bit_root(first_bit + i) % P
    return f


def step_cinv(s, t):
    """1 / w_{2^(4-s)}^bitrev(t, 3-s): the constant part of 1/x of pair t in fold step s"""
    return pow(pow(two_adic_generator(4 - s), bitrev(t, 3 - s), P), P - 2, P)


def own_winv(j):
    """w_16^(-bitrev(j, 4)): x0' = x0^16 times this, j the next row's own position"""
    return pow(pow(two_adic_generator(4), bitrev(j, 4), P), P - 2, P)


def lg(n, lo=5):
    l = lo
    while (1 << l) < n:
        l += 1
    return l


def log_rows(R, F, Q):
    """heights by table number (functions of the shape alone: LAYERS and QUERIES have room for all-distinct rows)"""
    return [lg(Q * R), lg(Q << F), lg(Q * R), lg(Q), lg(1 << F)]


def order(R, F, Q):
    """machine order: tallest first, equal heights by table number"""
    lr = log_rows(R, F, Q)
    return sorted(range(5), key=lambda i: (-lr[i], i))


def _add(cons, sel, terms):
    cons.append((sel, [(c % P, list(vs)) for c, vs in terms if c % P]))


def fold16_program(R, lf):
    cons = []
    END = L + R - 1
    nbs = nibbles(lf)

    def add(sel, terms):
        _add(cons, sel, terms)

    def ext_product(out, a, b):
        """out = a b in F_p[x] / (x^4 - 11), a and b column groups"""
        for c in range(4):
            t = [(1, [V(out + c)])]
            for i in range(4):
                for j in range(4):
                    if (i + j) % 4 == c:
                        t.append((P - (EXT_W if i + j >= 4 else 1), [V(a + i), V(b + j)]))
            add(O.SEL_ALL, t)
    add(O.SEL_ALL, [(1, [V(ACTIVE)])] + [(P - 1, [V(L + l)]) for l in range(R)])
    add(O.SEL_ALL, [(1, [V(LN)])] + [(P - l, [V(L + l)]) for l in range(R)])
    add(O.SEL_ALL, [(1, [V(ACTIVE), V(ACTIVE)]), (P - 1, [V(ACTIVE)])])
    for l in range(8):
        add(O.SEL_ALL, [(1, [V(L + l), V(L + l)]), (P - 1, [V(L + l)])] if l < R else [(1, [V(L + l)])])
    for j in range(16):
        add(O.SEL_ALL, [(1, [V(OF + j), V(OF + j)]), (P - 1, [V(OF + j)])])
    add(O.SEL_ALL, [(1, [V(ACTIVE)])] + [(P - 1, [V(OF + j)]) for j in range(16)])
    for c in range(4):
        add(O.SEL_ALL, [(1, [V(BETA + c)])] + [(P - 1, [V(L + l), V(4 * l + c, public=True)]) for l in range(R)])
    ext_product(B2, BETA, BETA)
    ext_product(B4, B2, B2)
    ext_product(B8, B4, B4)
    add(O.SEL_ALL, [(1, [V(G)]), (P - 1, [V(ACTIVE)]), (1, [V(END)])])
    for hi, lo in ((X2, X), (X4, X2), (X8, X4), (X16, X8), (XI2, XI), (XI4, XI2), (XI8, XI4)):
        add(O.SEL_ALL, [(1, [V(hi)]), (P - 1, [V(lo), V(lo)])])
    add(O.SEL_ALL, [(1, [V(ACTIVE), V(X), V(XI)]), (P - 1, [V(ACTIVE)])])
    add(O.SEL_ALL, [(1, [V(GX16)]), (P - 1, [V(G), V(X16)])])
    add(O.SEL_ALL, [(1, [V(GT)]), (P - 1, [V(G), V(T)])])
    add(O.SEL_ALL, [(1, [V(IDX)]), (P - 16, [V(ROW)])] + [(P - j, [V(OF + j)]) for j in range(16)])
    for j in range(16):
        add(O.SEL_ALL, [(1, [V(KJ + j)]), (P - 16, [V(ROW)]), (P - j, [V(ACTIVE)])])
    for c in range(4):
        add(O.SEL_ALL, [(1, [V(OWN + c)])] + [(P - 1, [V(OF + j), V(E + 4 * j + c)]) for j in range(16)])
    for s in range(4):
        src, dst, beta, xi = STEP_IN[s], STEP_OUT[s], STEP_BETA[s], STEP_XI[s]
        for t in range(8 >> s):
            e0, e1, ci = src + 8 * t, src + 8 * t + 4, step_cinv(s, t)
            for c in range(4):
                terms = [(1, [V(dst + 4 * t + c)]), (P - INV2, [V(e0 + c)]), (P - INV2, [V(e1 + c)])]
                for a in range(4):
                    for d in range(4):
                        if (a + d) % 4 != c:
                            continue
                        w = INV2 * ci % P * (EXT_W if a + d >= 4 else 1) % P
                        terms.append((P - w, [V(beta + a), V(e0 + d), V(xi)]))
                        terms.append((w, [V(beta + a), V(e1 + d), V(xi)]))
                add(O.SEL_ALL, terms)
    # the backward product: T, the last row's nibble forms, B
    add(O.SEL_ALL, [(1, [V(T)]), (P - 1, [V(L)])]
        + [(P - nibble_factor(4 * (l - 1), 4, j), [V(L + l), V(OF + j)]) for l in range(1, R) for j in range(16)])
    forms, col = [], N
    for k, nb in enumerate(nbs):
        flags = [col + j for j in range(1 << nb)]
        col += 1 << nb
        for f in flags:
            add(O.SEL_ALL, [(1, [V(f), V(f)]), (P - 1, [V(f)])])
        add(O.SEL_ALL, [(1, [V(END)])] + [(P - 1, [V(f)]) for f in flags])
        forms.append([(nibble_factor(4 * (R - 1) + 4 * k, nb, j), f) for j, f in enumerate(flags)])
    for c in range(col, width_of(lf)):
        add(O.SEL_ALL, [(1, [V(c)])])
    row_terms, col = [(1, [V(END), V(ROW)])], N
    for k, nb in enumerate(nbs):
        row_terms += [(P - (j << (4 * k)), [V(col + j)]) for j in range(1 << nb)]
        col += 1 << nb
    add(O.SEL_ALL, row_terms)
    if len(forms) == 1:
        add(O.SEL_ALL, [(1, [V(U)])] + [(P - c, [V(f)]) for c, f in forms[0]])
    else:
        add(O.SEL_ALL, [(1, [V(U)])] + [(P - c0 * c1, [V(f0), V(f1)]) for c0, f0 in forms[0] for c1, f1 in forms[1]])
    if len(forms) == 3:
        add(O.SEL_ALL, [(1, [V(TL)])] + [(P - c, [V(U), V(f)]) for c, f in forms[2]])
    else:
        add(O.SEL_ALL, [(1, [V(TL)]), (P - 1, [V(U)])])
    add(O.SEL_ALL, [(1, [V(END), V(B)]), (P - 1, [V(END), V(T), V(TL)])])
    add(O.SEL_ALL, [(1, [V(L), V(X)]), (P - 1, [V(L), V(B)])])
    # the chain
    for l in range(R - 1):
        add(O.SEL_TRANSITION, [(1, [V(L + l + 1, True)]), (P - 1, [V(L + l)])])
    add(O.SEL_TRANSITION, [(1, [V(G), V(ROW)]), (P - 1, [V(G), V(IDX, True)])])
    add(O.SEL_TRANSITION, [(1, [V(G), V(X, True)])] + [(P - own_winv(j), [V(GX16), V(OF + j, True)]) for j in range(16)])
    add(O.SEL_TRANSITION, [(1, [V(G), V(B)]), (P - 1, [V(GT), V(B, True)])])
    for c in range(4):
        add(O.SEL_TRANSITION, [(1, [V(G), V(FOLD + c)]), (P - 1, [V(G), V(OWN + c, True)])])
    add(O.SEL_FIRST, [(1, [V(ACTIVE)]), (P - 1, [V(L)])])
    add(O.SEL_LAST, [(1, [V(G)])])
    return O.air_program(width_of(lf), 4 * R, cons)


def final_program(R):
    cons = []
    for c in range(4):
        _add(cons, O.SEL_ALL, [(1, [V(FAX + c)]), (P - 1, [V(FACC + c), V(FX)])])
    for c in range(4):
        _add(cons, O.SEL_ALL, [(1, [V(FFIRST), V(FACC + c)]), (P - 1, [V(FFIRST), V(FC + c)])])
    _add(cons, O.SEL_TRANSITION, [(1, [V(FNL), V(FX, True)]), (P - 1, [V(FNL), V(FX)])])
    for c in range(4):
        _add(cons, O.SEL_TRANSITION, [(1, [V(FNL), V(FACC + c, True)]), (P - 1, [V(FNL), V(FAX + c)]), (P - 1, [V(FNL), V(FC + c, True)])])
    return O.air_program(FIN_PRE + FIN_MAIN, 4 * R, cons)


def table_program(R, pre_width):
    return O.air_program(pre_width + TAB_MAIN, 4 * R, [(O.SEL_FIRST, [(1, [V(pre_width + TAB_MAIN - 1)])])])


def programs(R, lf):
    """by table number"""
    return [fold16_program(R, lf), final_program(R), table_program(R, LAY_PRE), table_program(R, Q_PRE), table_program(R, C_PRE)]


def interactions(R):
    """by table number"""
    fold = [(O.SEND, ACTIVE, BUS_L16, [LN, KJ + j] + [E + 4 * j + c for c in range(4)]) for j in range(16)]
    fold.append((O.SEND, L, BUS_Q16, [IDX, OWN, OWN + 1, OWN + 2, OWN + 3]))
    fold.append((O.SEND, L + R - 1, BUS_FIN16, [X16, FOLD, FOLD + 1, FOLD + 2, FOLD + 3]))
    fin = [(O.RECEIVE, FACT, BUS_COEF, [FJ, FC, FC + 1, FC + 2, FC + 3]), (O.RECEIVE, FLAST, BUS_FIN16, [FX, FACC, FACC + 1, FACC + 2, FACC + 3])]
    lay = [(O.RECEIVE, LAY_M, BUS_L16, [LAY_LN, LAY_KEY + j] + [LAY_E + 4 * j + c for c in range(4)]) for j in range(16)]
    return [O.interaction_table(t) for t in (fold, fin, lay, [(O.RECEIVE, 5, BUS_Q16, [0, 1, 2, 3, 4])], [(O.SEND, 5, BUS_COEF, [0, 1, 2, 3, 4])])]


# ---------------------------------------------------------------- arithmetic of a row
def e_add(a, b):
    return [(x + y) % P for x, y in zip(a, b)]


def e_sub(a, b):
    return [(x - y) % P for x, y in zip(a, b)]


def e_scale(a, k):
    return [x * k % P for x in a]


def fold_row(row, lh, beta, entries, check=False):
    """-> (x0, [F1, F2, F3, [fold]] stage outputs): the four fold steps of one row of 16 entries at the points described above.
    check: assert every pair against the pair-by-pair fold of pyverify (point w_{2^(lh+4-s)}^bitrev(row 2^(3-s) + t, lh+3-s))"""
    x0 = pow(two_adic_generator(lh + 4), bitrev(row, lh), P)
    xi = pow(x0, P - 2, P)
    stages, cur, bs = [], [list(e) for e in entries], list(beta)
    for s in range(4):
        nxt = []
        for t in range(8 >> s):
            inv = xi * step_cinv(s, t) % P
            if check:
                x = pow(two_adic_generator(lh + 4 - s), bitrev(row * (8 >> s) + t, lh + 3 - s), P)
                assert x * inv % P == 1, "fold point"
            e0, e1 = cur[2 * t], cur[2 * t + 1]
            nxt.append(e_add(e_scale(e_add(e0, e1), INV2), ext_mul(bs, e_scale(e_sub(e0, e1), INV2 * inv % P))))
        stages.append(nxt)
        cur, bs, xi = nxt, ext_mul(bs, bs), xi * xi % P
    return x0, stages


def horner(coeffs, x):
    v = [0, 0, 0, 0]
    for c in reversed(coeffs):
        v = e_add(e_scale(v, x), c)
    return v


def chains(view, check=False):
    """walk every query: -> per query the list of per-layer dicts (row, own, entries, x0, stages, idx) and the chain's end (xf, folded)"""
    R, F, b, H = len(view["betas"]), view["F"], view["b"], view["H"]
    lf = F + b
    assert H == 4 * R + lf and len(view["final_poly"]) == 1 << F
    out = []
    for index, value, sibs in view["queries"]:
        assert 0 <= index < (1 << H)
        idx, val, rows = index, list(value), []
        for l in range(R):
            lh = H - 4 * (l + 1)
            row, own = idx >> 4, idx & 15
            entries = [list(e) for e in sibs[l]]
            entries.insert(own, list(val))
            x0, stages = fold_row(row, lh, view["betas"][l], entries, check)
            rows.append(dict(row=row, own=own, idx=idx, entries=entries, x0=x0, stages=stages, lh=lh))
            val, idx = stages[3][0], row
        xf = pow(two_adic_generator(lf), bitrev(idx, lf), P)
        assert pow(rows[-1]["x0"], 16, P) == xf
        out.append((rows, xf, val))
    return out


def consistent(view):
    """every chain ends in the final polynomial at its last point, and queries that meet agree about the row"""
    seen = {}
    for rows, xf, val in chains(view):
        if val != horner(view["final_poly"], xf):
            return False
        for l, r in enumerate(rows):
            if seen.setdefault((l, r["row"]), r["entries"]) != r["entries"]:
                return False
    return True


# ---------------------------------------------------------------- traces and tables
def fold16_trace(view, lr=None):
    R, Q = len(view["betas"]), len(view["queries"])
    lf = view["F"] + view["b"]
    nbs = nibbles(lf)
    lr = lg(Q * R) if lr is None else lr
    t = np.zeros((1 << lr, width_of(lf)), dtype=np.uint64)
    for q, (rows, xf, val) in enumerate(chains(view)):
        tcol = []
        for l, r in enumerate(rows):
            w = t[q * R + l]
            for j in range(16):
                w[E + 4 * j:E + 4 * j + 4] = r["entries"][j]
                w[KJ + j] = 16 * r["row"] + j
            for s, base in enumerate(STEP_OUT):
                for k, e in enumerate(r["stages"][s]):
                    w[base + 4 * k:base + 4 * k + 4] = e
            w[OWN:OWN + 4] = r["entries"][r["own"]]
            bs = list(view["betas"][l])
            for col in STEP_BETA:
                w[col:col + 4] = bs
                bs = ext_mul(bs, bs)
            x, xi = r["x0"], pow(r["x0"], P - 2, P)
            for col in (X, X2, X4, X8, X16):
                w[col], x = x, x * x % P
            for col in (XI, XI2, XI4, XI8):
                w[col], xi = xi, xi * xi % P
            w[ROW], w[IDX], w[LN], w[ACTIVE], w[OF + r["own"]], w[L + l] = r["row"], r["idx"], l, 1, 1, 1
            tcol.append(1 if l == 0 else nibble_factor(4 * (l - 1), 4, r["own"]))
            w[T] = tcol[-1]
            if l + 1 < R:
                w[G], w[GX16], w[GT] = 1, w[X16], tcol[-1]
        # the last row: the lf bits of its ROW, their forms, and B up the chain
        w, rest, col, forms = t[q * R + R - 1], rows[-1]["row"], N, []
        for k, nb in enumerate(nbs):
            j = (rest >> (4 * k)) & ((1 << nb) - 1)
            w[col + j] = 1
            col += 1 << nb
            forms.append(nibble_factor(4 * (R - 1) + 4 * k, nb, j))
        w[U] = forms[0] * (forms[1] if len(forms) > 1 else 1) % P
        w[TL] = w[U] * (forms[2] if len(forms) > 2 else 1) % P
        acc = int(w[TL])
        for l in reversed(range(R)):
            acc = acc * tcol[l] % P
            t[q * R + l, B] = acc
        assert acc == rows[0]["x0"], "the backward product is the first row's x0"
    return t.astype(np.uint32)


def final_tables(view, lr=None):
    """-> (preprocessed, main) of FINAL"""
    Q, F = len(view["queries"]), view["F"]
    n = 1 << F
    lr = lg(Q << F) if lr is None else lr
    pre = np.zeros((1 << lr, FIN_PRE), dtype=np.uint32)
    main = np.zeros((1 << lr, FIN_MAIN), dtype=np.uint64)
    for q, (rows, xf, val) in enumerate(chains(view)):
        acc = [0, 0, 0, 0]
        for i in range(n):
            j, r = n - 1 - i, q * n + i
            pre[r, FJ], pre[r, FFIRST], pre[r, FLAST], pre[r, FACT], pre[r, FNL] = j, int(i == 0), int(i == n - 1), 1, int(i != n - 1)
            c = view["final_poly"][j]
            acc = e_add(e_scale(acc, xf), c)
            m = main[r]
            m[FC - FIN_PRE:FC - FIN_PRE + 4], m[FACC - FIN_PRE:FACC - FIN_PRE + 4] = c, acc
            m[FAX - FIN_PRE:FAX - FIN_PRE + 4], m[FX - FIN_PRE] = e_scale(acc, xf), xf
    return pre, main.astype(np.uint32)


def key_tables(view):
    """-> (LAYERS, QUERIES, COEFFS) preprocessed"""
    R, Q, F = len(view["betas"]), len(view["queries"]), view["F"]
    lay, qs = {}, {}
    for (index, value, _), (rows, xf, val) in zip(view["queries"], chains(view)):
        k = (index, tuple(value))
        qs[k] = qs.get(k, 0) + 1
        for l, r in enumerate(rows):
            e = lay.setdefault((l, r["row"]), [r["entries"], 0])
            assert e[0] == r["entries"], "two queries disagree about a layer row"
            e[1] += 1
    tl = np.zeros((1 << lg(Q * R), LAY_PRE), dtype=np.uint32)
    for i, (l, row) in enumerate(sorted(lay)):
        tl[i, LAY_LN], tl[i, LAY_KEY:LAY_KEY + 16], tl[i, LAY_M] = l, [16 * row + j for j in range(16)], lay[(l, row)][1]
        tl[i, LAY_E:LAY_E + 64] = [c for e in lay[(l, row)][0] for c in e]
    tq = np.zeros((1 << lg(Q), Q_PRE), dtype=np.uint32)
    for i, (index, value) in enumerate(sorted(qs)):
        tq[i, 0], tq[i, 1:5], tq[i, 5] = index, value, qs[(index, value)]
    tc = np.zeros((1 << lg(1 << F), C_PRE), dtype=np.uint32)
    for j, c in enumerate(view["final_poly"]):
        tc[j, 0], tc[j, 1:5], tc[j, 5] = j, c, Q
    return tl, tq, tc


def tables(view):
    """by table number: (main traces, preprocessed traces)"""
    fpre, fmain = final_tables(view)
    tl, tq, tc = key_tables(view)
    z = lambda t: np.zeros((t.shape[0], TAB_MAIN), dtype=np.uint32)
    return [fold16_trace(view), fmain, z(tl), z(tq), z(tc)], [None, fpre, tl, tq, tc]


def machine(view):
    """-> (main traces, preprocessed traces, programs, interaction tables, public values) in machine order"""
    R, Q, F = len(view["betas"]), len(view["queries"]), view["F"]
    assert shape_ok(R, F, view["b"], Q)
    main, pre = tables(view)
    progs, tabs = programs(R, F + view["b"]), interactions(R)
    o = order(R, F, Q)
    return [main[i] for i in o], [pre[i] for i in o], [progs[i] for i in o], [tabs[i] for i in o], [c for bt in view["betas"] for c in bt]


def bus_balance(main, pre, tabs):
    """the buses in plain integers: -> {(bus, tuple): net multiplicity} of what does not cancel (empty: balanced)"""
    net = {}
    for m, p, tab in zip(main, pre, tabs):
        rows = np.asarray(m, dtype=np.int64) if p is None else np.concatenate([np.asarray(p, dtype=np.int64), np.asarray(m, dtype=np.int64)], axis=1)
        tab = [int(x) for x in tab]
        pos = 3
        for _ in range(tab[1]):
            sign, mult, bus, nv = tab[pos:pos + 4]
            cols = tab[pos + 4:pos + 4 + nv]
            pos += 4 + nv
            for r in rows[rows[:, mult] != 0]:
                k = (bus, tuple(int(r[c]) for c in cols))
                net[k] = net.get(k, 0) + (-int(r[mult]) if sign else int(r[mult]))
    return {k: v for k, v in net.items() if v}


# ---------------------------------------------------------------- views
def parse_view(proof_bytes, log_n, width, public_values, log_blowup, num_queries, pow_bits, logup_pairs=0, log_final=0, hash_width=0, code_width=0):
    """the FRI part of a fold-16 shard proof without the library: pyverify gives the challenges, the layer roots and per query the index and
    the reduced opening; the siblings, the paths and the final coefficients are read by position (the queries are the tail of the proof,
    the final polynomial and the proof-of-work witness sit right before the first one)"""
    v = {}
    pyverify.verify(proof_bytes, log_n, width, public_values, log_blowup=log_blowup, num_queries=num_queries, pow_bits=pow_bits, logup_pairs=logup_pairs,
                    log_fold=4, log_final=log_final, hash_width=hash_width, code_width=code_width, view=v)
    w = list(struct.unpack("<%dI" % (len(proof_bytes) // 4), bytes(proof_bytes)))
    F, b = log_final, log_blowup
    H, R = log_n + b, (log_n - log_final) // 4
    wp = 4 * (logup_pairs + 1) if logup_pairs else 0
    lhs = [H - 4 * (l + 1) for l in range(R)]
    commitments = width + (8 * H if code_width else 0) + 8 * H + ((wp + 8 * H) if logup_pairs else 0) + 8 + 8 * H
    per_query = commitments + sum(60 + 8 * lh for lh in lhs)
    q0 = len(w) - num_queries * per_query
    fp = w[q0 - 1 - 4 * (1 << F):q0 - 1]
    queries, paths = [], []
    for q in range(num_queries):
        pos = q0 + q * per_query + commitments
        sibs, pth = [], []
        for lh in lhs:
            sibs.append([w[pos + 4 * k:pos + 4 * k + 4] for k in range(15)])
            pth.append(w[pos + 60:pos + 60 + 8 * lh])
            pos += 60 + 8 * lh
        index, value = v["queries"][q][0], v["queries"][q][1]
        queries.append((index, list(value), sibs))
        paths.append(pth)
    return dict(betas=v["betas"], final_poly=[fp[4 * j:4 * j + 4] for j in range(1 << F)], queries=queries, roots=v["roots"], paths=paths, F=F, b=b, H=H)


def random_view(R, F, b, n_queries, seed=1):
    """a consistent view that belongs to no proof, built sparsely (no layer is materialised): random final coefficients; per query, from the
    last layer back to layer 0, a row is either one already made (the own entry is what it holds) or 15 random siblings plus the own entry
    solved for -- a row's fold is affine in one entry, so two evaluations of the fold give it.  Queries 1 and 2 are neighbours of query 0
    (the same row at layer 0; the same rows from layer 1 on), so multiplicities above 1 occur."""
    rng = np.random.default_rng(seed)
    lf = F + b
    H = 4 * R + lf
    rnd = lambda: [int(x) for x in rng.integers(0, P, 4)]
    betas = [rnd() for _ in range(R)]
    final_poly = [rnd() for _ in range(1 << F)]
    made = {}
    indices = [int(rng.integers(0, 1 << H)) for _ in range(n_queries)]
    if n_queries > 1:
        indices[1] = indices[0] ^ 1
    if n_queries > 2 and R > 1:
        indices[2] = indices[0] ^ (1 << 5)
    queries = []
    for index in indices:
        target = None
        for l in reversed(range(R)):
            idx = index >> (4 * l)
            row, own, lh = idx >> 4, idx & 15, H - 4 * (l + 1)
            if l == R - 1:
                target = horner(final_poly, pow(two_adic_generator(lf), bitrev(row, lf), P))
            if (l, row) not in made:
                entries = [rnd() for _ in range(16)]
                entries[own] = [0, 0, 0, 0]
                f0 = fold_row(row, lh, betas[l], entries)[1][3][0]
                entries[own] = [1, 0, 0, 0]
                f1 = fold_row(row, lh, betas[l], entries)[1][3][0]
                entries[own] = ext_mul(e_sub(target, f0), ext_inv(e_sub(f1, f0)))
                made[(l, row)] = entries
            target = made[(l, row)][own]
        sibs = []
        for l in range(R):
            idx = index >> (4 * l)
            e = made[(l, idx >> 4)]
            sibs.append([list(e[j]) for j in range(16) if j != (idx & 15)])
        queries.append((index, list(target), sibs))
    return dict(betas=betas, final_poly=final_poly, queries=queries, F=F, b=b, H=H)


def view_arrays(view):
    """the flat canonical arrays the library's entries take: betas [R][4], final_poly [2^F][4], indices [Q], values [Q][4], siblings [Q][R][15][4]"""
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    return (u(view["betas"]), u(view["final_poly"]), u([q[0] for q in view["queries"]]), u([q[1] for q in view["queries"]]),
            u([q[2] for q in view["queries"]]))
