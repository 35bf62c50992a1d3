"""The width-24 Poseidon2 permutation as a constraint program, with Merkle-path chaining and leaf hashing (test-side restatement; the
product's generator is the width-24 part of csrc/poseidon2_chip.cpp, its trace generator csrc/hash.hip).  It is the width-16 chip
(tests/poseidon2_air.py) for RISC Zero-shape commitments: rate 16, overwrite-mode sponge from the zero state, digest = state[0..8],
parent = permute(l || r || 0^8)[0..8] (tests/pyref.py: poseidon2_24, sponge24, compress24).

One row = one permutation out = pyref.poseidon2_24(in).  540 columns, every constraint of degree <= 3 including its selector:
  IN 24 | S0 24 (after the initial external layer) | X3E[r] 24, OUTE[r] 24 for external rounds 0..3 (cubes of input + constant, state after
  the round) | S0P[r], X3P[r], SBP[r] for the 21 internal rounds (element 0 before the S-box, its cube, its seventh power; the other 23
  elements stay linear forms) | column 303 unused | SP 24 (after the internal rounds) | X3E[r], OUTE[r] for external rounds 4..7 |
  D 8 = IN[j] (1 - BIT) + IN[8 + j] BIT | BIT CH END CNT | SPG SS | G1 G2 G3 | C1 C2 C3
  BIT: right child; CH: the row continues the previous row's digest (D = previous OUTE[7][0..8]); END: the row's digest is the public root;
  CNT: running count of END rows, the last row's is the public count.
  SS: the first sponge row of a leaf; SPG: a later one (capacity = the previous row's OUTE[7][16..24]).
  Gk: rate words 4k .. 4k + 4 are absorbed by this sponge row (words 0..4 always are); prefix-ordered.  Ck = SPG (1 - Gk): those words
  carry over from the previous output.  On an SS row a group that is not absorbed is zero.
  The capacity IN[16..24] is zero on every row that is not SPG (compression rows absorb l || r || 0^8).
Public values: root[8], count.
"""
import numpy as np

import oracle_lib as O
import pyref

P = O.P
V = O.air_var
PARAMS24 = pyref.PARAMS24
T, RP = 24, 21

IN, S0, SPARE, SP, D = 0, 24, 303, 304, 520
BIT, CH, END, CNT, SPG, SS = 528, 529, 530, 531, 532, 533
G = {1: 534, 2: 535, 3: 536}
C = {1: 537, 2: 538, 3: 539}
WIDTH = 540
N_PUBLIC = 9


def X3E(r):
    return 48 + 48 * r if r < 4 else 328 + 48 * (r - 4)


def OUTE(r):
    return X3E(r) + 24


def S0P(r):
    return 240 + 3 * r


def X3P(r):
    return 241 + 3 * r


def SBP(r):
    return 242 + 3 * r


def ext_input(r):
    return S0 if r == 0 else (SP if r == 4 else OUTE(r - 1))


# the matrices exactly as pyref.poseidon2_24 writes them
M4 = PARAMS24["m4"]
ME = [[(2 if i // 4 == j // 4 else 1) * M4[i % 4][j % 4] % P for j in range(T)] for i in range(T)]
DIAG = PARAMS24["internal_diag"]
MI = [[(1 + (DIAG[i] if i == j else 0)) % P for j in range(T)] for i in range(T)]
RC_E, RC_I = PARAMS24["external_rc"], PARAMS24["internal_rc"]


def _mv(M, v):
    return [sum(M[i][j] * v[j] for j in range(T)) % P for i in range(T)]


def _term(coeff, vs):
    return (coeff % P, list(vs))


def _cube_def(x3, c, k):
    t = [_term(1, [V(x3)]), _term(P - 1, [V(c)] * 3), _term(P - 3 * k, [V(c)] * 2), _term(P - 3 * k * k, [V(c)]), _term(P - pow(k, 3, P), [])]
    return [x for x in t if x[0]]


def _linear_def(col, form):
    return [_term(1, [V(col)])] + [_term(P - form[c], [V(c)]) for c in sorted(form) if form[c] % P]


def _drop_zero(terms):
    return [t for t in terms if t[0]]


def permutation_constraints():
    cons = []
    for i in range(T):
        cons.append((O.SEL_ALL, _linear_def(S0 + i, {IN + j: ME[i][j] for j in range(T)})))

    def external_round(r):
        c0 = ext_input(r)
        for i in range(T):
            cons.append((O.SEL_ALL, _cube_def(X3E(r) + i, c0 + i, RC_E[r][i])))
        for i in range(T):
            t = [_term(1, [V(OUTE(r) + i)])]
            for j in range(T):
                x3, c = V(X3E(r) + j), V(c0 + j)
                t.append(_term(P - ME[i][j], [x3, x3, c]))
                t.append(_term(P - ME[i][j] * RC_E[r][j] % P, [x3, x3]))
            cons.append((O.SEL_ALL, _drop_zero(t)))
    for r in range(4):
        external_round(r)
    lin = [{OUTE(3) + i: 1} for i in range(T)]
    for r in range(RP):
        k = RC_I[r]
        cons.append((O.SEL_ALL, _linear_def(S0P(r), lin[0])))
        cons.append((O.SEL_ALL, _cube_def(X3P(r), S0P(r), k)))
        cons.append((O.SEL_ALL, _drop_zero([_term(1, [V(SBP(r))]), _term(P - 1, [V(X3P(r)), V(X3P(r)), V(S0P(r))]), _term(P - k, [V(X3P(r)), V(X3P(r))])])))
        lin[0] = {SBP(r): 1}
        total = {}
        for f in lin:
            for c, v in f.items():
                total[c] = (total.get(c, 0) + v) % P
        lin = [{c: (DIAG[i] * lin[i].get(c, 0) + total.get(c, 0)) % P for c in set(lin[i]) | set(total)} for i in range(T)]
    for i in range(T):
        cons.append((O.SEL_ALL, _linear_def(SP + i, lin[i])))
    for r in range(4, 8):
        external_round(r)
    return cons


def group_words(k):
    return range(4 * k, 4 * k + 4)


def program():
    cons = permutation_constraints()
    o7 = OUTE(7)
    for j in range(8):
        cons.append((O.SEL_ALL, [_term(1, [V(D + j)]), _term(P - 1, [V(IN + j)]), _term(1, [V(BIT), V(IN + j)]), _term(P - 1, [V(BIT), V(IN + 8 + j)])]))
    for b in (BIT, CH, END, SPG, SS, G[1], G[2], G[3]):
        cons.append((O.SEL_ALL, [_term(1, [V(b), V(b)]), _term(P - 1, [V(b)])]))
    for k in (2, 3):                                            # G_k (1 - G_{k-1}) = 0
        cons.append((O.SEL_ALL, [_term(1, [V(G[k])]), _term(P - 1, [V(G[k - 1]), V(G[k])])]))
    for k in (1, 2, 3):                                         # C_k = SPG (1 - G_k)
        cons.append((O.SEL_ALL, [_term(1, [V(C[k])]), _term(P - 1, [V(SPG)]), _term(1, [V(SPG), V(G[k])])]))
    cons.append((O.SEL_FIRST, [_term(1, [V(CH)])]))
    cons.append((O.SEL_FIRST, [_term(1, [V(SPG)])]))
    for j in range(8):                                          # the capacity is zero unless the row continues a sponge
        cons.append((O.SEL_ALL, [_term(1, [V(IN + 16 + j)]), _term(P - 1, [V(SPG), V(IN + 16 + j)])]))
    for k in (1, 2, 3):                                         # a leaf's first row: groups it does not absorb are zero
        for j in group_words(k):
            cons.append((O.SEL_ALL, [_term(1, [V(SS), V(IN + j)]), _term(P - 1, [V(SS), V(G[k]), V(IN + j)])]))
    for j in range(8):
        cons.append((O.SEL_TRANSITION, [_term(1, [V(SPG, True), V(IN + 16 + j, True)]), _term(P - 1, [V(SPG, True), V(o7 + 16 + j)])]))
    for k in (1, 2, 3):
        for j in group_words(k):
            cons.append((O.SEL_TRANSITION, [_term(1, [V(C[k], True), V(IN + j, True)]), _term(P - 1, [V(C[k], True), V(o7 + j)])]))
    for j in range(8):
        cons.append((O.SEL_TRANSITION, [_term(1, [V(CH, True), V(D + j, True)]), _term(P - 1, [V(CH, True), V(o7 + j)])]))
    for j in range(8):
        cons.append((O.SEL_ALL, [_term(1, [V(END), V(o7 + j)]), _term(P - 1, [V(END), V(j, public=True)])]))
    cons.append((O.SEL_FIRST, [_term(1, [V(CNT)]), _term(P - 1, [V(END)])]))
    cons.append((O.SEL_TRANSITION, [_term(1, [V(CNT, True)]), _term(P - 1, [V(CNT)]), _term(P - 1, [V(END, True)])]))
    cons.append((O.SEL_LAST, [_term(1, [V(CNT)]), _term(P - 1, [V(8, public=True)])]))
    return O.air_program(WIDTH, N_PUBLIC, cons)


def row(state_in, bit=0, ch=0, end=0, cnt=0, spg=0, ss=0, groups=0):
    """one trace row: every intermediate of poseidon2_24(state_in) -> (row, output state); groups = rate-word groups 4..8, 8..12, 12..16
    absorbed by a sponge row (0..3)"""
    t = [0] * WIDTH
    s = [x % P for x in state_in]
    t[IN:IN + T] = s
    s = _mv(ME, s)
    t[S0:S0 + T] = s

    def external_round(r, s):
        y = [(s[i] + RC_E[r][i]) % P for i in range(T)]
        x3 = [pow(v, 3, P) for v in y]
        t[X3E(r):X3E(r) + T] = x3
        s = _mv(ME, [x3[i] * x3[i] % P * y[i] % P for i in range(T)])
        t[OUTE(r):OUTE(r) + T] = s
        return s
    for r in range(4):
        s = external_round(r, s)
    for r in range(RP):
        t[S0P(r)] = s[0]
        y = (s[0] + RC_I[r]) % P
        t[X3P(r)] = pow(y, 3, P)
        s[0] = t[SBP(r)] = pow(y, 7, P)
        s = _mv(MI, s)
    t[SP:SP + T] = s
    for r in range(4, 8):
        s = external_round(r, s)
    for j in range(8):
        t[D + j] = state_in[8 + j] % P if bit else state_in[j] % P
    t[BIT], t[CH], t[END], t[CNT], t[SPG], t[SS] = bit, ch, end, cnt % P, spg, ss
    for k in (1, 2, 3):
        t[G[k]] = 1 if groups >= k else 0
        t[C[k]] = 1 if spg and groups < k else 0
    return t, s


def merkle_trace(leaves, siblings, indices, log_n=None, row_width=0):
    """paths p: leaf digest leaves[p] (8 values) -- or, with row_width > 0, the opened ROW leaves[p] (row_width values, a multiple of 4),
    hashed by ceil(row_width / 16) sponge rows first --, siblings[p][level] (8 values each), indices[p] (bit `level`: right child)
    -> (trace [2^log_n][WIDTH], roots [n_paths][8]); rows after the paths are permutations of the zero state with no flags"""
    n_paths, depth = len(leaves), len(siblings[0])
    rows, roots, cnt = [], [], 0
    for p in range(n_paths):
        vals = [int(v) % P for v in leaves[p]]
        if row_width:
            assert len(vals) == row_width and row_width % 4 == 0
            out = [0] * T
            for k in range(0, row_width, 16):
                blk = vals[k:k + 16]
                state = blk + out[len(blk):]
                r, out = row(state, 0, 0, 0, cnt, 1 if k else 0, 0 if k else 1, len(blk) // 4 - 1)
                rows.append(r)
            digest = out[:8]
        else:
            digest = vals
        for lvl in range(depth):
            bit = (int(indices[p]) >> lvl) & 1
            sib = [int(v) % P for v in siblings[p][lvl]]
            end = 1 if lvl == depth - 1 else 0
            cnt += end
            r, out = row((sib + digest if bit else digest + sib) + [0] * 8, bit, 1 if (lvl or row_width) else 0, end, cnt)
            rows.append(r)
            digest = out[:8]
        roots.append(digest)
    need = max(len(rows), 32)
    if log_n is None:
        log_n = max(5, (need - 1).bit_length())
    pad, _ = row([0] * T, 0, 0, 0, cnt)
    assert len(rows) <= 1 << log_n
    rows += [pad] * ((1 << log_n) - len(rows))
    return np.array(rows, dtype=np.uint64).astype(np.uint32), roots


def tree(rows_or_digests, row_width=0):
    """every level of the RISC Zero-shape tree over the given leaves (rows hashed with pyref.sponge24 when row_width > 0)"""
    level = [pyref.sponge24(r) for r in rows_or_digests] if row_width else [list(d) for d in rows_or_digests]
    levels = [level]
    while len(level) > 1:
        level = [pyref.compress24(level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
        levels.append(level)
    return levels


def tree_paths(depth, n_paths, row_width=0, seed=1):
    """a random tree of 2^depth leaves (rows of row_width values, or digests) and n_paths openings -> (leaves, siblings, indices, root)"""
    rng = np.random.default_rng(seed)
    leaves_all = [[int(v) for v in rng.integers(0, P, row_width or 8)] for _ in range(1 << depth)]
    levels = tree(leaves_all, row_width)
    idx = [int(v) for v in rng.integers(0, 1 << depth, n_paths)]
    sibs = [[levels[l][(i >> l) ^ 1] for l in range(depth)] for i in idx]
    return [leaves_all[i] for i in idx], sibs, idx, levels[-1][0]


def sparse_tree_paths(depth, n_paths, row_width, seed):
    """n_paths openings of one random tree of 2^depth leaves whose opened leaves are rows of row_width values (digests when 0); the other
    leaves are random digests -> (leaves, siblings, indices, root)"""
    rng = np.random.default_rng(seed)
    idx = [int(v) for v in rng.choice(1 << depth, size=n_paths, replace=(n_paths > (1 << depth)))]
    digests = [[int(v) for v in rng.integers(0, P, 8)] for _ in range(1 << depth)]
    opened = {}
    for i in idx:
        if i not in opened:
            opened[i] = [int(v) for v in rng.integers(0, P, row_width)] if row_width else digests[i]
            if row_width:
                digests[i] = pyref.sponge24(opened[i])
    levels = tree(digests)
    sibs = [[levels[l][(i >> l) ^ 1] for l in range(depth)] for i in idx]
    return [opened[i] for i in idx], sibs, idx, levels[-1][0]


def check_constraints(prog, trace, public_values):
    """evaluate every constraint of `prog` on every row of `trace` (canonical words); -> list of (constraint index, row) that fail.
    Selectors as the prover applies them: FIRST on row 0, LAST on the last row, TRANSITION on rows 0 .. n-2 with `next` = row + 1."""
    prog = [int(x) for x in prog]
    n = len(trace)
    pub = [int(v) % P for v in public_values]
    cons, p = [], 6
    for _ in range(prog[3]):
        sel, nt = prog[p], prog[p + 1]
        p += 2
        terms = []
        for _ in range(nt):
            coeff, d = prog[p], prog[p + 1]
            terms.append((coeff, prog[p + 2:p + 2 + d]))
            p += 2 + d
        cons.append((sel, terms))
    loc = np.asarray(trace, dtype=np.uint64) % P
    nxt = np.roll(loc, -1, axis=0)
    rows = np.arange(n)
    bad = []
    for ci, (sel, terms) in enumerate(cons):
        acc = np.zeros(n, dtype=np.uint64)
        for coeff, vs in terms:
            m = np.full(n, coeff, dtype=np.uint64)
            for v in vs:
                kind, idx = v >> 30, v & 0xFFFF
                m = m * (loc[:, idx] if kind == 0 else nxt[:, idx] if kind == 1 else np.uint64(pub[idx])) % P
            acc = (acc + m) % P
        if sel == O.SEL_FIRST:
            acc[1:] = 0
        elif sel == O.SEL_LAST:
            acc[:-1] = 0
        elif sel == O.SEL_TRANSITION:
            acc[-1] = 0
        bad += [(ci, int(r)) for r in rows[acc != 0]]
    return bad
