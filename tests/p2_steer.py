"""Steering: canonical Poseidon2 inputs that put chosen words at a chosen place INSIDE the permutation.

The suite's edge states sit at the input, and the first S-box turns every one of them into pseudo-random words, so no exact boundary inside
the rounds (an S-box input of 0 or +-1 in round 5, a row sum of exactly 0, a digit word of 0x00 bytes in all 16 lanes, an output word of
P - 1) is ever asked.  Poseidon2 is a permutation: pick the state wanted at a probe point, run the steps before it backwards (inverse M_E,
inverse M_I, x -> x^(1/7)), and the result is a canonical input that arrives there.  CPU only, pure Python integers, built from pyref.

The permutation is written here the way the device runs it (poseidon2.cuh): the constants of the round that follows ride forward through
the external layer, so the probes name values the device really holds.

  ("L0",)      input of the first external layer
  ("F", r)     S-box inputs of full round r, round constant included                                        r = 0..7
  ("U", r)     S-box outputs of full round r plus the constant the device folds in: M_E^-1 rc_next, (int_rc[0], 0, ...) after round 3,
               zero after round 7 -- the value whose lazy form the matrix-core path turns into digits
  ("P", r)     the state entering partial round r, int_rc[r] already in word 0                            r = 0..12 (0..20 at width 24)
  ("OUT",)     the permutation's output

target_words / forward_probe speak MONTGOMERY WORDS (x R mod P, R = 2^32), what the device holds; states in and out are canonical."""
import pyref

P = pyref.P
R = 2**32 % P
RINV = pow(R, -1, P)
INV7 = pow(7, -1, P - 1)
H_LO, H_HI = (P - 1) // 2, (P + 1) // 2


def inv_matrix(m):
    n = len(m)
    a = [[int(m[i][j]) % P for j in range(n)] + [int(i == j) for j in range(n)] for i in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if a[r][c])
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], P - 2, P)
        a[c] = [x * inv % P for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


def matvec(M, v):
    return [sum(a * b for a, b in zip(row, v)) % P for row in M]


def _me24():
    m4 = pyref.PARAMS24["m4"]
    return [[(2 if i // 4 == j // 4 else 1) * m4[i % 4][j % 4] for j in range(24)] for i in range(24)]


ME = {16: pyref.ME, 24: _me24()}
ME_INV = {w: inv_matrix(m) for w, m in ME.items()}
N_PARTIAL = {16: 13, 24: 21}


def params(width, diag=None, rc_i=None):
    """(external constants, internal constants, internal diagonal) of a width; at width 16 the last two may be given"""
    prm = pyref.PARAMS if width == 16 else pyref.PARAMS24
    assert width == 16 or (diag is None and rc_i is None)
    return prm["external_rc"], list(rc_i or prm["internal_rc"]), [x % P for x in (diag or prm["internal_diag"])]


def folds(width, rc_e, rc_i):
    """fold[r] = M_E^-1 of the constant vector that FOLLOWS full round r (canonical)"""
    out = []
    for r in range(8):
        v = [0] * width
        if r == 3:
            v[0] = rc_i[0]
        elif r < 7:
            v = rc_e[r + 1]
        out.append(matvec(ME_INV[width], v))
    return out


class _Steps:
    """the permutation as a list of (forward, backward, probe reached) steps"""

    def __init__(self, width, diag=None, rc_i=None):
        rc_e, rc_i, d = params(width, diag, rc_i)
        w, me, mei = width, ME[width], ME_INV[width]
        fold = folds(w, rc_e, rc_i)
        # M_I = J + diag(d):  y = d x + sum(x)  =>  x = (y - t) / d,  t = sum(x) = sum(y / d) / (1 + sum(1 / d))
        dinv = [pow(x, P - 2, P) for x in d]
        assert all(d) and (1 + sum(dinv)) % P
        tinv = pow(1 + sum(dinv), P - 2, P)

        def mi(s):
            t = sum(s)
            return [(d[i] * s[i] + t) % P for i in range(w)]

        def mi_inv(y):
            t = sum(a * b for a, b in zip(y, dinv)) * tinv % P
            return [(y[i] - t) * dinv[i] % P for i in range(w)]

        add = lambda c: (lambda s: [(a + b) % P for a, b in zip(s, c)])
        sub = lambda c: (lambda s: [(a - b) % P for a, b in zip(s, c)])
        sb = lambda s: [pow(x, 7, P) for x in s]
        sb_inv = lambda s: [pow(x, INV7, P) for x in s]
        sb0 = lambda s: [pow(s[0], 7, P)] + s[1:]
        sb0_inv = lambda s: [pow(s[0], INV7, P)] + s[1:]
        lin = lambda s: matvec(me, s)
        lin_inv = lambda s: matvec(mei, s)
        e0 = lambda c: [c] + [0] * (w - 1)

        st = [(None, None, ("L0",)), (lin, lin_inv, None)]
        for r in range(4):
            if r == 0:
                st.append((add(rc_e[0]), sub(rc_e[0]), ("F", 0)))
            else:
                st[-1] = (lin, lin_inv, ("F", r))
            st += [(sb, sb_inv, None), (add(fold[r]), sub(fold[r]), ("U", r)), (lin, lin_inv, None)]
        st[-1] = (lin, lin_inv, ("P", 0))
        for r in range(N_PARTIAL[w]):
            st += [(sb0, sb0_inv, None), (mi, mi_inv, None)]
            if r + 1 < N_PARTIAL[w]:
                st.append((add(e0(rc_i[r + 1])), sub(e0(rc_i[r + 1])), ("P", r + 1)))
        for r in range(4, 8):
            if r == 4:
                st.append((add(rc_e[4]), sub(rc_e[4]), ("F", 4)))
            else:
                st[-1] = (lin, lin_inv, ("F", r))
            st += [(sb, sb_inv, None), (add(fold[r]), sub(fold[r]), ("U", r)), (lin, lin_inv, None)]
        st[-1] = (lin, lin_inv, ("OUT",))
        self.steps = st
        self.at = {p: i for i, (_, _, p) in enumerate(st) if p is not None}


_CACHE = {}


def _steps(width, diag, rc_i):
    key = (width, tuple(diag) if diag else None, tuple(rc_i) if rc_i else None)
    if key not in _CACHE:
        _CACHE[key] = _Steps(width, diag, rc_i)
    return _CACHE[key]


def probes(width):
    return list(_steps(width, None, None).at)


def forward_probe(width, probe, state, diag=None, rc_i=None):
    """the Montgomery words the device holds at `probe` when it permutes the canonical `state`"""
    k = _steps(width, diag, rc_i)
    s = [int(x) % P for x in state]
    for f, _, _ in k.steps[1:k.at[tuple(probe)] + 1]:
        s = f(s)
    return [x * R % P for x in s]


def steer(width, probe, target_words, diag=None, rc_i=None):
    """the canonical input state whose permutation holds the Montgomery words `target_words` at `probe`"""
    k = _steps(width, diag, rc_i)
    words = [int(x) % P for x in target_words]
    assert len(words) == width
    s = [x * RINV % P for x in words]
    for _, b, _ in reversed(k.steps[1:k.at[tuple(probe)] + 1]):
        s = b(s)
    assert forward_probe(width, probe, s, diag, rc_i) == words
    return s


def permute(width, state, diag=None, rc_i=None):
    """the whole permutation through the steps above (canonical in and out): pyref.poseidon2 / poseidon2_24 for the built-in parameters"""
    return [x * RINV % P for x in forward_probe(width, ("OUT",), state, diag, rc_i)]


# ---- the catalogue
def edge_words():
    from field_edges import EDGE_WORDS
    return sorted({int(x) for x in EDGE_WORDS} | {H_LO, H_HI})


# balanced base-256 digits (planes 0..2) of the matrix-core path's digit words: the extremes, and the bytes next to the sign change
DIGITS = (-128, 127, 0, -1)
TOP_DIGITS = (1, -1, 2, -2, 3, -3, 8, -8, 32, -32, 64, -64, 100, -100, 119, -119)
ALT_DIGITS = ((-128, -128, -128, 0), (127, 127, 127, 0), (-128, 127, -128, 0), (127, -128, 127, -1))
# the row-sum scales: dsmred(2^sh S) = tau  <=>  S = tau 2^(32 - sh) (Montgomery words).  27: one round at a time (width 16), 26: width 24,
# 24: a pair's first round, 0: a pair's second round (its row sum is not scaled)
SUM_TARGETS = (0, 1, P - 1, H_LO, H_HI)
SUM_PASSIVE = (0, P - 1, H_LO)


def _sum_scales(width, r):
    if width == 24:
        return (26,)
    return (27,) if r == 0 else (27, 24) if r % 2 else (27, 0)


def word_patterns(width, k):
    """labelled target states (Montgomery words) from the edge words; k rotates the one-hot lane so every lane meets every word"""
    ws = edge_words()
    lanes = (0, 1, 15) + ((23,) if width == 24 else ())
    out = []
    for n, w in enumerate(ws):
        out.append(("eq:%d" % w, [w] * width))
        if w:
            out.append(("alt:%d" % w, [w if i % 2 == 0 else P - w for i in range(width)]))
            lane = lanes[(n + k) % len(lanes)]
            out.append(("hot%d:%d" % (lane, w), [w if i == lane else 0 for i in range(width)]))
        out.append(("lane0:%d" % w, [w] + [ws[(n + 1) % len(ws)]] * (width - 1)))
    return out


def digit_word(d):
    """the Montgomery word whose lazy value n + P has the balanced digits d (plane 0 first)"""
    return sum(x * 256**i for i, x in enumerate(d)) % P


def digit_patterns():
    out = []
    for a in DIGITS:
        for b in DIGITS:
            for c in DIGITS:
                out.append(("dig:%d,%d,%d,0" % (a, b, c), [digit_word((a, b, c, 0))] * 16))
    for d in ALT_DIGITS:
        n = sum(x * 256**i for i, x in enumerate(d))
        out.append(("digalt:%d,%d,%d,%d" % d, [(n if i % 2 == 0 else -1 - n) % P for i in range(16)]))
    for t in TOP_DIGITS:
        out.append(("digtop:%d" % t, [digit_word((0, 0, 0, t))] * 16))
    return out


def catalogue(width, diag=None):
    """deterministic list of (label, probe, canonical input state): about 2 300 states at width 16 and 600 at width 24"""
    out = []
    k = _steps(width, diag, None)

    def put(label, probe, words):
        out.append(("%s/%s" % ("".join(str(x) for x in probe), label), probe, steer(width, probe, words, diag)))

    word_probes = [p for p in k.at if p[0] != "U"]
    keep, keep_words = ("eq:0", "eq:1", "eq:%d" % (P - 1)), ("0", "1", str(P - 1))
    for n, probe in enumerate(word_probes):
        pats = word_patterns(width, n)
        if width == 24:                                                # a quarter of width 16's budget: every sixth pattern, rotating with the probe
            # (after a signed external layer every pattern of the words 0, 1 and P - 1: which signed representative arrives depends on the lane)
            pats = [x for i, x in enumerate(pats) if probe[0] in ("L0", "OUT") or i % 6 == n % 6 or x[0] in keep
                    or ((probe[0] == "F" or probe == ("P", 0)) and x[0].split(":")[1] in keep_words)]
        for label, words in pats:
            put(label, probe, words)
    for r in range(N_PARTIAL[width]):
        done = set()
        for e in (SUM_PASSIVE if width == 16 else SUM_PASSIVE[1:2]):
            for tau in SUM_TARGETS + (None,):
                for sh in _sum_scales(width, r):
                    for S in ([tau * 2**(32 - sh) % P] if tau is not None else [1, P - 1]):
                        if (e, S) in done:
                            continue
                        done.add((e, S))
                        # row sum (Montgomery words) u + (width - 1) e = S with u the S-box OUTPUT of word 0: its input is the seventh root
                        u = (S - (width - 1) * e) * RINV % P
                        v0 = pow(u, INV7, P) * R % P
                        put("sum:%d,e=%d" % (S, e), ("P", r), [v0] + [e] * (width - 1))
    if width == 16:
        # the first layer's digit words: the lazy value is input word + u0 (u0 = the word of M_E^-1 ext_rc[0]), no reduction in between
        u0 = [x * R % P for x in matvec(ME_INV[16], params(16)[0][0])]
        for label, words in digit_patterns():
            lazy = [x + P if x < P // 2 else x for x in words]           # n + P as an integer, n the signed digit value
            put(label, ("L0",), [(a - b) % P for a, b in zip(lazy, u0)])
        for r in range(8):
            for label, words in digit_patterns():
                put(label, ("U", r), words)
    return out
