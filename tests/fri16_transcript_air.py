"""The fold-by-16 INDICES machine, written a second time -- the first is zktls_amd/csrc/fri16_chip.hip (the machine and its key), fri_chip.hip (the SAMPLES
chip) and hash.hip (the transcript kernel).  It is the paths machine of tests/fri16_paths_air.py with the Fiat-Shamir transcript inside, from the commit
phase on: no challenge and no query index is an input.

Statement (public values: the 8 capacity words of the duplex challenger as the commit phase finds it; the key commits the layer roots, the final
coefficients and (query number, reduced opening)):
    a sponge chain starts from this capacity; it absorbs root_0 .. root_{R-1} and draws beta_l after each; it then absorbs the listed final coefficients
    and a proof-of-work witness; the first word it hands out has its low pow_bits bits zero; the low H bits of the following words are the indices of
    queries 0 .. Q-1; every query, at the index drawn for it, opens the listed layer commitments row by row and folds under the drawn challenges to the
    value of the listed polynomial at its last point.

The duplex rules (tests/pyverify.py Transcript; the chain is written out row by row in chain() below and compared with that class where views are made):
pending inputs are zero when the commit phase starts; a root is one full rate block and beta_l = (out[7], out[6], out[5], out[4]); for F >= 1 the
4 2^F coefficient words are 2^(F-1) full blocks and the witness then overwrites rate word 0 only, words 1..7 keep the previous output; for F = 0 one block
takes the coefficient in words 0..3 and the witness in word 4; words are handed out from out[7] down; a permutation with no input follows whenever the
eight are used up; the proof-of-work word is always drawn.

Tables by number: 0 FOLD16B (FOLD16 of fri16_air without the constraints that name a public value, plus one receive of (LN, BETA)); 1 FINAL and 2 P24L as in
the paths machine (imported); 3 QUERIES: preprocessed (q, value[4], 1, 0, 0), main (index, 0, 0, 0); 4 COEFFS: preprocessed (j, c_j[4], Q, 1, 0); 5 ROOTS:
preprocessed (layer, depth, root[8], LISTED = 1, 0), main (path ends, beta[4], fold rows, 0, 0), with the constraint fold rows (1 - LISTED) = 0: the send of
(layer, beta) to FOLD16B has a main multiplicity, and a padding row (all preprocessed cells zero: layer 0, nothing received from the transcript) must not send; 6 P2T: main the 352 permutation columns IN .. BIT of the width-16
chip (tests/poseidon2_air.py), preprocessed the schedule
    SPG | K0..K7 | ROOT LN | C0 KEY0 C1 KEY1 | SMP ROW | 0 0 0
(SPG: the capacity half follows the previous row's output; K_j: rate word j does; ROOT: a root row of layer LN; C0 / C1: the row's first / second four rate
words are coefficient KEY0 / KEY1; SMP: the row hands its eight words out, ROW its number); 7 SAMPLES: the chip of tests/fri_air.py with H index bits and
first row number R + C.  All programs carry 8 public values in their header."""
import copy
import functools

import numpy as np

import fri16_air as A
import fri16_paths_air as PA
import fri_air as FA
import oracle_lib as O
import poseidon2_air as P2
import pyref
import pyverify

P = O.P
V = O.air_var
FOLD16B, FINAL, P24L, QUERIES, COEFFS, ROOTS, P2T, SAMPLES = range(8)
BUS_TR0, BUS_TR1, BUS_TB, BUS_BF16, BUS_CT = 76, 77, 78, 79, 80
N_PUBLIC, ROOTS_MAIN, T_WIDTH = 8, 8, 352
PT_PRE, PT_SPG, PT_K, PT_ROOT, PT_LN, PT_C0, PT_KEY0, PT_C1, PT_KEY1, PT_SMP, PT_ROW = 20, 0, 1, 9, 10, 11, 12, 13, 14, 15, 16
HONEST_SHAPES = [(1, 0, 1, 4), (1, 1, 1, 7), (1, 1, 1, 8), (2, 2, 2, 11)]          # (R, F, log_blowup, queries): H <= 12
POW_BITS = 4


def chain_rows(R, F, Q):
    """-> (coefficient rows C, rows that hand words out S, rows of the chain NT)"""
    C = (1 << (F - 1)) if F >= 1 else 0
    S = FA.sample_rows(Q)
    return C, S, R + C + S


def shape_ok(R, F, b, Q, pow_bits):
    return A.shape_ok(R, F, b, Q) and 0 <= pow_bits <= 30


def log_rows(R, F, b, Q):
    C, S, NT = chain_rows(R, F, Q)
    return PA.log_rows(R, F, b, Q) + [A.lg(NT), A.lg(S)]


def order(R, F, b, Q):
    lr = log_rows(R, F, b, Q)
    return sorted(range(8), key=lambda i: (-lr[i], i))


def main_widths(lf):
    return [A.width_of(lf), A.FIN_MAIN, PA.WIDTH_L, A.TAB_MAIN, A.TAB_MAIN, ROOTS_MAIN, T_WIDTH, FA.S_MAIN]


PRE_WIDTHS = [0, A.FIN_PRE, 0, A.Q_PRE, A.C_PRE, PA.ROOTS_PRE, PT_PRE, FA.S_PRE]


# ---------------------------------------------------------------- programs
def constraints_of(prog):
    """a constraint program's words -> [(selector, [(coefficient, [variables])])]"""
    prog = [int(x) for x in prog]
    out, p = [], 6
    for _ in range(prog[3]):
        sel, nt = prog[p], prog[p + 1]
        p += 2
        terms = []
        for _ in range(nt):
            d = prog[p + 1]
            terms.append((prog[p], prog[p + 2:p + 2 + d]))
            p += 2 + d
        out.append((sel, terms))
    return out


def with_public(prog, n_public):
    """the same program in a machine with n_public public values (the count is word 4 of the header)"""
    out = np.array(prog, dtype=np.uint32)
    out[4] = n_public
    return out


def fold16b_program(R, lf):
    """FOLD16 without the constraints that tie BETA to public values: exactly those that name a public value"""
    cons = constraints_of(A.fold16_program(R, lf))
    kept = [(sel, terms) for sel, terms in cons if not any(v >> 30 == 2 for _, vs in terms for v in vs)]
    assert len(cons) - len(kept) == 4
    return O.air_program(A.width_of(lf), N_PUBLIC, kept)


def p2t_constraints():
    """-> [(name, selector, terms)] on the combined row [schedule | permutation columns]"""
    M0, ALL, FIRST, TRANS = PT_PRE, O.SEL_ALL, O.SEL_FIRST, O.SEL_TRANSITION
    IN, OUT, D, BIT = M0 + P2.IN, M0 + P2.OUTE(7), M0 + P2.D, M0 + P2.BIT
    cons = [("permutation", sel, [(c, [v + M0 for v in vs]) for c, vs in terms]) for sel, terms in P2.permutation_constraints()]
    for j in range(8):
        cons.append(("D = IN", ALL, [(1, [V(D + j)]), (P - 1, [V(IN + j)])]))
    cons.append(("BIT = 0", ALL, [(1, [V(BIT)])]))
    for j in range(8):
        cons.append(("row 0: the capacity is public", FIRST, [(1, [V(IN + 8 + j)]), (P - 1, [V(j, public=True)])]))
    for j in range(8):
        cons.append(("SPG: the capacity follows", TRANS, [(1, [V(PT_SPG, True), V(IN + 8 + j, True)]), (P - 1, [V(PT_SPG, True), V(OUT + 8 + j)])]))
    for j in range(8):
        cons.append(("K: kept rate words follow", TRANS, [(1, [V(PT_K + j, True), V(IN + j, True)]), (P - 1, [V(PT_K + j, True), V(OUT + j)])]))
    return cons


def samples_constraint_names(pow_bits):
    """the SAMPLES program's constraints by what they say, in program order"""
    names = []
    for j in range(8):
        names += ["bit"] * 31 + ["word = sum of bits", "H1", "H2", "HH", "canonical", "index = low bits"]
    return names + (["proof of work"] if pow_bits else [])


def p2t_program():
    return O.air_program(PT_PRE + T_WIDTH, N_PUBLIC, [(sel, terms) for _, sel, terms in p2t_constraints()])


def p2t_constraint_names():
    return [name for name, _, _ in p2t_constraints()]


def table_program(pre_width, main_width=A.TAB_MAIN):
    return O.air_program(pre_width + main_width, N_PUBLIC, [(O.SEL_FIRST, [(1, [V(pre_width + main_width - 1)])])])


def roots_program():
    """the harmless identity of a key table, then: a row that is not listed sends no challenge to FOLD16B"""
    RM = PA.ROOTS_PRE
    return O.air_program(RM + ROOTS_MAIN, N_PUBLIC, [(O.SEL_FIRST, [(1, [V(RM + ROOTS_MAIN - 1)])]),
                                                     (O.SEL_ALL, [(1, [V(RM + 5)]), (P - 1, [V(RM + 5), V(10)])])])


def programs(R, F, b, pow_bits):
    """by table number"""
    lf, H = F + b, 4 * R + F + b
    return [fold16b_program(R, lf), with_public(A.final_program(R), N_PUBLIC), PA.p24l_program(N_PUBLIC), table_program(A.Q_PRE), table_program(A.C_PRE),
            roots_program(), p2t_program(), FA.samples_program(H - 1, None, pow_bits, N_PUBLIC)]


def interactions(R):
    """by table number"""
    pa = PA.interactions(R)
    S, Rv = O.SEND, O.RECEIVE
    fold = [(int(s), int(m), int(bus), [int(c) for c in cols]) for s, m, bus, cols in _entries(A.interactions(R)[A.FOLD16])]
    fold.append((Rv, A.ACTIVE, BUS_BF16, [A.LN, A.BETA, A.BETA + 1, A.BETA + 2, A.BETA + 3]))
    queries = [(Rv, 5, A.BUS_Q16, [A.Q_PRE, 1, 2, 3, 4]), (Rv, 5, FA.BUS_I, [0, A.Q_PRE])]
    coeffs = [(S, 5, A.BUS_COEF, [0, 1, 2, 3, 4]), (S, 6, BUS_CT, [0, 1, 2, 3, 4])]
    RM, RT = PA.ROOTS_PRE, PA.RT_ROOT
    roots = [(Rv, RM, PA.BUS_RT0, [PA.RT_LN, PA.RT_DEP] + [RT + c for c in range(4)]), (Rv, RM, PA.BUS_RT1, [PA.RT_LN, PA.RT_DEP] + [RT + 4 + c for c in range(4)]),
             (Rv, 10, BUS_TR0, [PA.RT_LN] + [RT + c for c in range(4)]), (Rv, 10, BUS_TR1, [PA.RT_LN] + [RT + 4 + c for c in range(4)]),
             (Rv, 10, BUS_TB, [PA.RT_LN] + [RM + 1 + c for c in range(4)]), (S, RM + 5, BUS_BF16, [PA.RT_LN] + [RM + 1 + c for c in range(4)])]
    IN, o = PT_PRE + P2.IN, PT_PRE + P2.OUTE(7)
    p2t = [(Rv, PT_C0, BUS_CT, [PT_KEY0] + [IN + c for c in range(4)]), (Rv, PT_C1, BUS_CT, [PT_KEY1] + [IN + 4 + c for c in range(4)]),
           (S, PT_ROOT, BUS_TR0, [PT_LN] + [IN + c for c in range(4)]), (S, PT_ROOT, BUS_TR1, [PT_LN] + [IN + 4 + c for c in range(4)]),
           (S, PT_ROOT, BUS_TB, [PT_LN, o + 7, o + 6, o + 5, o + 4]),
           (S, PT_SMP, FA.BUS_S0, [PT_ROW, o + 7, o + 6, o + 5, o + 4]), (S, PT_SMP, FA.BUS_S1, [PT_ROW, o + 3, o + 2, o + 1, o])]
    M0 = FA.S_PRE
    samples = [(Rv, FA.S_ROW, FA.BUS_S0, [FA.S_C] + [M0 + FA.S_W + j for j in range(4)]), (Rv, FA.S_ROW, FA.BUS_S1, [FA.S_C] + [M0 + FA.S_W + j for j in range(4, 8)])] \
        + [(S, FA.S_ACT + j, FA.BUS_I, [FA.S_KQ + j, M0 + FA.S_IDX + j]) for j in range(8)]
    return [O.interaction_table(fold), pa[PA.FINAL], pa[PA.P24L]] + [O.interaction_table(t) for t in (queries, coeffs, roots, p2t, samples)]


def _entries(tab):
    tab = [int(x) for x in tab]
    pos = 3
    for _ in range(tab[1]):
        sign, mult, bus, nv = tab[pos:pos + 4]
        yield sign, mult, bus, tab[pos + 4:pos + 4 + nv]
        pos += 4 + nv


# ---------------------------------------------------------------- the chain
def chain(capacity, roots, final_poly, witness, F, Q):
    """the duplex challenger from the commit phase on, one permutation per row -> {"inputs": [NT][16], "outputs": [NT][16], "betas": [R][4],
    "words": [S][8] in the order they are handed out, "indices_of": H -> the Q indices}"""
    R = len(roots)
    C, S, NT = chain_rows(R, F, Q)
    flat = [int(c) for cf in final_poly for c in cf]
    assert len(flat) == 4 << F and len(capacity) == 8
    ins, outs, betas, words = [], [], [], []
    st = [0] * 8 + [int(c) for c in capacity]

    def step(rate_prefix):
        s = [int(x) for x in rate_prefix] + st[len(rate_prefix):]
        ins.append(s)
        out = pyref.poseidon2(s)
        outs.append(list(out))
        return list(out)
    for l in range(R):
        st = step(roots[l])
        betas.append([st[7], st[6], st[5], st[4]])
    for i in range(C):
        st = step(flat[8 * i:8 * i + 8])
    st = step(flat + [witness] if F == 0 else [witness])
    words.append(st[7::-1])
    for _ in range(S - 1):
        st = step([])
        words.append(st[7::-1])
    assert len(ins) == NT
    return dict(inputs=ins, outputs=outs, betas=betas, words=words)


def drawn_indices(ch, H, Q):
    flat = [w for row in ch["words"] for w in row]
    return [flat[1 + q] & ((1 << H) - 1) for q in range(Q)]


_PAD = None


def p2t_pre(R, F, Q, lr=None):
    """P2T's preprocessed schedule: a function of the shape alone"""
    C, S, NT = chain_rows(R, F, Q)
    lr = A.lg(NT) if lr is None else lr
    pre = np.zeros((1 << lr, PT_PRE), dtype=np.uint32)
    for r in range(NT):
        pre[r, PT_SPG] = int(r > 0)
        kept_from = 8
        if r < R:
            pre[r, PT_ROOT], pre[r, PT_LN] = 1, r
        elif r < R + C:
            i = r - R
            pre[r, PT_C0], pre[r, PT_KEY0], pre[r, PT_C1], pre[r, PT_KEY1] = 1, 2 * i, 1, 2 * i + 1
        elif r == R + C:
            if F == 0:
                pre[r, PT_C0], kept_from = 1, 5
            else:
                kept_from = 1
        else:
            kept_from = 0
        pre[r, PT_K + kept_from:PT_K + 8] = 1
        if r >= R + C:
            pre[r, PT_SMP], pre[r, PT_ROW] = 1, r
    return pre


def p2t_main(ch, lr=None):
    """P2T's main trace: one permutation per chain row, then permutations of the zero state"""
    global _PAD
    NT = len(ch["inputs"])
    lr = A.lg(NT) if lr is None else lr
    if _PAD is None:
        _PAD = P2.row([0] * 16)[0][:T_WIDTH]
    return np.array([P2.row(s)[0][:T_WIDTH] for s in ch["inputs"]] + [_PAD] * ((1 << lr) - NT), dtype=np.uint64).astype(np.uint32)


def transcript_traces(R, F, b, Q, capacity, roots, final_poly, witness):
    """what zkhip_fri16_indices_gen_traces makes, from the same inputs: -> (P2T main, SAMPLES main, betas, indices); no layer data"""
    H = 4 * R + F + b
    C, S, NT = chain_rows(R, F, Q)
    ch = chain(capacity, roots, final_poly, witness, F, Q)
    _, smain, idx = FA.samples_tables(H - 1, Q, ch["words"], A.lg(S), base=R + C)
    assert idx == drawn_indices(ch, H, Q)
    return p2t_main(ch), smain, ch["betas"], idx


# ---------------------------------------------------------------- tables of a view
def key_tables(view):
    """the key's tables by table number (None: no preprocessed columns) -- no index and no challenge goes in"""
    R, Q, F, b, H = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["H"]
    C, S, NT = chain_rows(R, F, Q)
    lr = log_rows(R, F, b, Q)
    n = 1 << F
    fpre = np.zeros((1 << lr[FINAL], A.FIN_PRE), dtype=np.uint32)
    for r in range(Q * n):
        i = r % n
        fpre[r, A.FJ], fpre[r, A.FFIRST], fpre[r, A.FLAST], fpre[r, A.FACT], fpre[r, A.FNL] = n - 1 - i, int(i == 0), int(i == n - 1), 1, int(i != n - 1)
    tq = np.zeros((1 << lr[QUERIES], A.Q_PRE), dtype=np.uint32)
    for q, (_, value, _) in enumerate(view["queries"]):
        tq[q, 0], tq[q, 1:5], tq[q, 5] = q, value, 1
    tc = np.zeros((1 << lr[COEFFS], A.C_PRE), dtype=np.uint32)
    for j, c in enumerate(view["final_poly"]):
        tc[j, 0], tc[j, 1:5], tc[j, 5], tc[j, 6] = j, c, Q, 1
    tr = np.zeros((1 << lr[ROOTS], PA.ROOTS_PRE), dtype=np.uint32)
    for l in range(R):
        tr[l, PA.RT_LN], tr[l, PA.RT_DEP], tr[l, PA.RT_ROOT:PA.RT_ROOT + 8], tr[l, 10] = l, H - 4 * (l + 1), view["roots"][l], 1
    tp = p2t_pre(R, F, Q, lr[P2T])
    ts = FA.samples_tables(H - 1, Q, [[0] * 8] * S, lr[SAMPLES], base=R + C)[0]
    return [None, fpre, None, tq, tc, tr, tp, ts]


def tables(view, p24l=None, honest=True):
    """by table number: (main traces, preprocessed traces); the view's betas and indices must be the drawn ones (honest=False: a forger's view, whose QUERIES
    and ROOTS main columns and FOLD16B rows then hold the VIEW's indices and challenges while P2T and SAMPLES hold what the chain draws)"""
    R, Q, F, b, H = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["H"]
    C, S, NT = chain_rows(R, F, Q)
    lr = log_rows(R, F, b, Q)
    ch = chain(view["capacity"], view["roots"], view["final_poly"], view["witness"], F, Q)
    if honest:
        assert ch["betas"] == [[int(c) for c in bt] for bt in view["betas"]], "the view's challenges are not the drawn ones"
        assert drawn_indices(ch, H, Q) == [q[0] for q in view["queries"]], "the view's indices are not the drawn ones"
        assert ch["words"][0][0] & ((1 << view["pow_bits"]) - 1) == 0, "the witness fails the proof of work"
    pm, pp = PA.tables(view, p24l)
    pre = key_tables(view)
    qmain = np.zeros((1 << lr[QUERIES], A.TAB_MAIN), dtype=np.uint32)
    qmain[:Q, 0] = [q[0] for q in view["queries"]]
    rmain = np.zeros((1 << lr[ROOTS], ROOTS_MAIN), dtype=np.uint32)
    for l in range(R):
        rmain[l, 0], rmain[l, 1:5], rmain[l, 5] = pm[PA.ROOTS][l, 0], view["betas"][l], Q
    _, smain, _ = FA.samples_tables(H - 1, Q, ch["words"], lr[SAMPLES], base=R + C)
    main = [pm[PA.FOLD16], pm[PA.FINAL], pm[PA.P24L], qmain, np.zeros((1 << lr[COEFFS], A.TAB_MAIN), dtype=np.uint32), rmain, p2t_main(ch, lr[P2T]), smain]
    assert (pre[FINAL] == pp[PA.FINAL]).all()
    return main, pre


def machine(view, p24l=None, honest=True):
    """-> (main traces, preprocessed traces, programs, interaction tables, public values) in machine order"""
    R, Q, F, b = len(view["roots"]), len(view["queries"]), view["F"], view["b"]
    assert shape_ok(R, F, b, Q, view["pow_bits"])
    main, pre = tables(view, p24l, honest)
    progs, tabs = programs(R, F, b, view["pow_bits"]), interactions(R)
    o = order(R, F, b, Q)
    return [main[i] for i in o], [pre[i] for i in o], [progs[i] for i in o], [tabs[i] for i in o], [int(c) for c in view["capacity"]]


# ---------------------------------------------------------------- views
class _Recorder(pyverify.Transcript):
    """pyverify's transcript, remembering what it is given and in what state: ("many", words, capacity half of the state, inputs pending) per
    observe_many, ("one", word) per observe called on its own"""
    log = []

    def observe_many(self, vs):
        _Recorder.log.append(("many", [int(v) for v in vs], [int(x) for x in self.state[8:]], len(self.pending)))
        self._inside = True
        try:
            super().observe_many(vs)
        finally:
            self._inside = False

    def observe(self, v):
        if not getattr(self, "_inside", False):
            _Recorder.log.append(("one", int(v)))
        super().observe(v)


def golden_view(name, GOLDEN, load):
    """the paths view of a committed fold-16 proof plus "capacity", "witness" and "pow_bits": pyverify runs with the recording transcript in place of its own
    for the duration of this call"""
    g = GOLDEN[name]
    s = g["shape"]
    kept = pyverify.Transcript
    _Recorder.log = []
    pyverify.Transcript = _Recorder
    try:
        v = A.parse_view(load(name).tobytes(), g["log_n"], g["width"], g["public"], s[0], s[1], s[2], logup_pairs=s[3], log_final=s[5], hash_width=s[6],
                         code_width=s[7] if len(s) > 7 else 0)
    finally:
        pyverify.Transcript = kept
    log = _Recorder.log
    at = [i for i, e in enumerate(log) if e[0] == "many" and e[1] == [int(c) for c in v["roots"][0]]]
    assert at, "the first layer root is observed"
    _, _, capacity, pending = log[at[-1]]
    assert pending == 0
    witness = [e[1] for e in log if e[0] == "one"][-1]
    return dict(v, capacity=capacity, witness=witness, pow_bits=s[2], hash_width=s[6])


def _evaluate(coeffs, h):
    """a polynomial with extension coefficients [n][4] at the 2^h points w_{2^h}^bitrev(i, h), i ascending -> [2^h][4]"""
    w = pyref.two_adic_generator(h)
    x = np.array([pow(w, pyref.bitrev(i, h), P) for i in range(1 << h)], dtype=np.uint64).reshape(-1, 1)
    acc = np.zeros((1 << h, 4), dtype=np.uint64)
    for c in reversed(coeffs):
        acc = (acc * x + np.array(c, dtype=np.uint64)) % P
    return [[int(v) for v in row] for row in acc]


@functools.lru_cache(maxsize=None)
def honest_view(R, F, b, Q, seed=1, pow_bits=POW_BITS):
    """an honest fold-16 FRI instance from the commit phase on: a random polynomial of degree < 2^(4 R + F) on the domain of 2^H points, every layer committed
    as a width-24 Merkle tree over its rows of 16 entries, beta_l drawn from the transcript after root_l, the coefficients folded (c'_j = c_2j + beta c_2j+1,
    four times per layer with beta, beta^2, beta^4, beta^8), the final coefficients, a witness ground here, the indices drawn.  The transcript is pyverify's,
    started from a random capacity"""
    rng = np.random.default_rng([seed, R, F, b, Q])
    H = 4 * R + F + b
    rnd = lambda n: [int(x) for x in rng.integers(0, P, n)]
    capacity = rnd(8)
    ts = pyverify.Transcript()
    ts.state = [0] * 8 + list(capacity)
    coeffs = [rnd(4) for _ in range(1 << (4 * R + F))]
    layers, trees, roots, betas = [], [], [], []
    for l in range(R):
        h = H - 4 * l
        ev = _evaluate(coeffs, h)
        rows = [[c for e in ev[16 * r:16 * r + 16] for c in e] for r in range(1 << (h - 4))]
        levels = [[pyref.sponge24(r) for r in rows]]
        while len(levels[-1]) > 1:
            prev = levels[-1]
            levels.append([pyref.compress24(prev[2 * i], prev[2 * i + 1]) for i in range(len(prev) // 2)])
        layers.append(ev)
        trees.append(levels)
        roots.append([int(x) for x in levels[-1][0]])
        ts.observe_many(roots[-1])
        beta = ts.sample_ext()
        betas.append([int(x) for x in beta])
        bs = list(beta)
        for _ in range(4):
            coeffs = [A.e_add(coeffs[2 * j], pyref.ext_mul(bs, coeffs[2 * j + 1])) for j in range(len(coeffs) // 2)]
            bs = pyref.ext_mul(bs, bs)
    final_poly = [[int(x) for x in c] for c in coeffs]
    assert len(final_poly) == 1 << F
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
    view = dict(betas=betas, final_poly=final_poly, queries=queries, roots=roots, paths=paths, F=F, b=b, H=H, hash_width=24, capacity=capacity, witness=witness,
                pow_bits=pow_bits)
    ch = chain(capacity, roots, final_poly, witness, F, Q)                      # the chain written out row by row draws what pyverify's transcript drew
    assert ch["betas"] == betas and drawn_indices(ch, H, Q) == indices
    return view


def view_arrays(view):
    """fri16_paths_air.view_arrays plus the capacity [8]"""
    return PA.view_arrays(view) + (np.ascontiguousarray(np.array(view["capacity"], dtype=np.uint32)),)
