"""An exact Python-integer model of the paired partial rounds of the width-16 Poseidon2 permutation (poseidon2.cuh,
p2_internal_rounds_dev): elements 1..15 are updated once per two partial rounds, the second round's row sum comes from the old elements
through exact small multipliers.  Same dsmred / v_mad_i64_i32 semantics as the device, every 64-bit accumulator and 32-bit result asserted in
range on the way, the constants recomputed here from the parameter file (not read from derive_tables()).

  round t   : u = sbox(v0);  T = 2^24 (u + sum_{i>=1} v_i);  sum_t = T / R;  v0' = (u D_0 + sum_t K24 + rc) / R
  round t+1 : u' = sbox(v0');  A = sum_{i>=1} d_i v_i + sum_t C15 + u';  sum1 = A / R;  T2 = sum1 K1;  v0'' = (u' D_0 + T2 + rc') / R
              v_i'' = (v_i D2_i + sum_t E_i + T2) / R        (i >= 1)
with R = 2^32, K24 = R^2 / 2^24, C15 = 15 R / 2^24 = 3840, K1 = R^2, D2_i = d_i^2 R, E_i = d_i R^2 / 2^24 (all mod P, centred).  The first of
the 13 rounds runs in the one-round form (row sum scaled by 2^27), then six pairs."""
import numpy as np

import pyref

P = pyref.P
R = 2**32 % P
MU = pow(P, -1, 2**32)
H = (P - 1) // 2                        # the largest magnitude of a centred constant
SH_ONE, SH_PAIR = 27, 24                # row-sum scales: the one-round form's, a pair's first round's
I32 = 2**31 - 1


def cen(x):
    x %= P
    return x - P if x > P // 2 else x


def dsmred(t):
    """babybear.cuh dsmred: t / 2^32 mod P for a signed 64-bit t, the device's exact integer steps"""
    assert -2**63 <= t < 2**63
    m = (t & 0xFFFFFFFF) * MU & 0xFFFFFFFF
    m = m - 2**32 if m >= 2**31 else m
    y = t - m * P
    assert -2**63 <= y < 2**63 and y % 2**32 == 0
    r = y >> 32
    assert -2**31 <= r < 2**31
    return r


def mad(a, k, c):
    """v_mad_i64_i32: a, k int32, c and the result int64"""
    assert -2**31 <= a < 2**31 and -2**31 <= k < 2**31
    d = a * k + c
    assert -2**63 <= d < 2**63
    return d


def sbox(t):
    x2 = dsmred(mad(t, t, 0))
    x4 = dsmred(mad(x2, x2, 0))
    x6 = dsmred(mad(x4, x2, 0))
    return dsmred(mad(x6, t, 0))


def pair_budget_ok(sum_d, sh_pair=SH_PAIR):
    """The interval pass: magnitudes only, every centred constant taken at its largest (P - 1) / 2, so the answer depends on the diagonal
    through sum_{i>=1} d_i alone.  red(x) bounds |dsmred(X)| for |X| <= x; sh_pair is the row-sum scale of a pair's first round."""
    def red(x):
        if x > 2**63 - 1 - 2**31 * P:
            raise OverflowError
        r = x // 2**32 + P // 2 + 1
        if r > I32:
            raise OverflowError
        return r

    def sbox_b(t):
        x2 = red(t * t)
        x4 = red(x2 * x2)
        x6 = red(x4 * x2)
        return red(x6 * t)

    try:
        b0 = bv = P - 1
        u = sbox_b(b0)                                                  # the leading round, one-round form
        s = red((u + 15 * bv) << SH_ONE)
        b0, bv = red(u * H + s * H + H), red(bv * H + s * H)
        if max(b0, bv) > P - 1:
            return False
        for _ in range(6):
            u = sbox_b(b0)
            st = red((u + 15 * bv) << sh_pair)
            v0 = red(u * H + st * H + H)
            u2 = sbox_b(v0)
            s1 = red(sum_d * bv + st * 15 * 2**(32 - sh_pair) + u2)
            t2 = s1 * H
            b0, bv = red(u2 * H + t2 + H), red(bv * H + st * H + t2)
            if max(b0, bv, v0) > P - 1:
                return False
        return True
    except OverflowError:
        return False


class Consts:
    def __init__(self, diag, rc_i):
        self.d = [x % P for x in diag]
        self.D = [cen(x * R) for x in self.d]
        self.rc_fold = [cen(rc_i[r + 1] * R * R) for r in range(12)] + [0]
        self.K27 = cen(2**(64 - SH_ONE))
        self.K24 = cen(2**(64 - SH_PAIR))
        self.K1 = cen(R * R)
        self.C15 = cen(15 * 2**(32 - SH_PAIR))
        self.D2 = [cen(x * x * R) for x in self.d]
        self.E = [cen(x * 2**(64 - SH_PAIR)) for x in self.d]
        self.pair = all(1 <= x <= 2**15 for x in self.d[1:]) and pair_budget_ok(sum(self.d[1:]))


def round_one(v, r, k):
    u = sbox(v[0])
    T = 0
    for x in [u] + v[1:]:
        T = mad(x, 1 << SH_ONE, T)
    s = dsmred(T)
    T2 = mad(s, k.K27, 0)
    return [dsmred(mad(u, k.D[0], T2 + k.rc_fold[r]))] + [dsmred(mad(v[i], k.D[i], T2)) for i in range(1, 16)]


def round_pair(v, r, k, track=None):
    A = 0
    for i in range(1, 16):
        A = mad(v[i], k.d[i], A)                                       # the exact multipliers d_i 2^s, s = 0
    u = sbox(v[0])
    T = 0
    for x in [u] + v[1:]:
        T = mad(x, 1 << SH_PAIR, T)
    st = dsmred(T)
    v0 = dsmred(mad(u, k.D[0], mad(st, k.K24, 0) + k.rc_fold[r]))
    A = mad(st, k.C15, A)
    u2 = sbox(v0)
    A = mad(u2, 1, A)
    s1 = dsmred(A)
    T2 = mad(s1, k.K1, 0)
    out = [dsmred(mad(u2, k.D[0], T2 + k.rc_fold[r + 1]))] + [dsmred(mad(v[i], k.D2[i], mad(st, k.E[i], T2))) for i in range(1, 16)]
    if track is not None:
        track["st"] = max(track.get("st", 0), abs(st))
        track["s1"] = max(track.get("s1", 0), abs(s1))
        track["v"] = max(track.get("v", 0), max(abs(x) for x in out), abs(v0))
    return out


def internal_rounds(v, k, track=None):
    """v: signed Montgomery-form words in (-P, P), int_rc[0] already in v[0]; returns canonical Montgomery-form words"""
    assert all(abs(x) < P for x in v)
    v = round_one(v, 0, k)
    if k.pair:
        for r in range(1, 13, 2):
            v = round_pair(v, r, k, track)
    else:
        for r in range(1, 13):
            v = round_one(v, r, k)
    assert all(abs(x) < P for x in v)
    return [x % P for x in v]


def reference(state, diag, rc_i):
    """pyref.poseidon2 with the internal layer's diagonal and constants given"""
    rc_e = pyref.PARAMS["external_rc"]
    s = pyref._matvec(pyref.ME, [x % P for x in state])
    for r in range(4):
        s = pyref._matvec(pyref.ME, [pow((s[i] + rc_e[r][i]) % P, 7, P) for i in range(16)])
    for r in range(13):
        s[0] = pow((s[0] + rc_i[r]) % P, 7, P)
        t = sum(s) % P
        s = [(diag[i] * s[i] + t) % P for i in range(16)]
    for r in range(4, 8):
        s = pyref._matvec(pyref.ME, [pow((s[i] + rc_e[r][i]) % P, 7, P) for i in range(16)])
    return s


def permutation(state, k, rc_i, rng=None, track=None):
    """the whole permutation, its 13 partial rounds through the device model (signed Montgomery-form words, either representative)"""
    rc_e = pyref.PARAMS["external_rc"]
    s = pyref._matvec(pyref.ME, [x % P for x in state])
    for r in range(4):
        s = pyref._matvec(pyref.ME, [pow((s[i] + rc_e[r][i]) % P, 7, P) for i in range(16)])
    s[0] = (s[0] + rc_i[0]) % P
    w = [x * R % P for x in s]
    w = [x - P if x and (rng.integers(2) if rng is not None else x > P // 2) else x for x in w]
    w = internal_rounds(w, k, track)
    rinv = pow(R, -1, P)
    s = [x * rinv % P for x in w]
    for r in range(4, 8):
        s = pyref._matvec(pyref.ME, [pow((s[i] + rc_e[r][i]) % P, 7, P) for i in range(16)])
    return s


BUILTIN = Consts(pyref.PARAMS["internal_diag"], pyref.PARAMS["internal_rc"])


def _edge_states():
    st = [[0] * 16, [P - 1] * 16, [1] * 16, [0, P - 1] * 8, [P - 1, 0] * 8]
    st += [[P - 1 if j == i else 0 for j in range(16)] for i in range(16)]
    st += [[1 if j == i else 0 for j in range(16)] for i in (0, 1, 15)]
    return st


def test_builtin_diagonal_qualifies():
    d = BUILTIN.d
    assert d[0] == P - 2 and d[1:] == [1 << k for k in range(14)] + [1 << 15]
    assert BUILTIN.pair
    assert BUILTIN.C15 == 3840 and BUILTIN.K24 == cen(2**40) and BUILTIN.E[1] == BUILTIN.K24


def test_paired_permutation_matches_pyref():
    rng = np.random.default_rng(23)
    states = _edge_states() + [[int(x) for x in rng.integers(0, P, 16)] for _ in range(40)]
    track = {}
    for st in states:
        exp = pyref.poseidon2(st)
        assert permutation(st, BUILTIN, pyref.PARAMS["internal_rc"], None, track) == exp
        assert permutation(st, BUILTIN, pyref.PARAMS["internal_rc"], rng, track) == exp
    assert track["v"] < P and track["st"] <= P // 2 + P // 16 + 1 and track["s1"] <= P // 2 + 2**16


def test_paired_rounds_on_extreme_words():
    # the partial rounds alone on the largest signed words of either sign, against the field arithmetic
    k = BUILTIN
    rc = pyref.PARAMS["internal_rc"]
    rinv = pow(R, -1, P)
    for v in ([P - 1] * 16, [-(P - 1)] * 16, [P - 1, -(P - 1)] * 8, [-(P - 1)] + [P - 1] * 15, [P - 1] + [-(P - 1)] * 15):
        s = [x * rinv % P for x in v]
        for r in range(13):
            s[0] = pow(s[0] if r == 0 else (s[0] + rc[r]) % P, 7, P)
            t = sum(s) % P
            s = [(k.d[i] * s[i] + t) % P for i in range(16)]
        assert [x * rinv % P for x in internal_rounds(list(v), k)] == s


def test_interval_budget():
    sum_d = sum(BUILTIN.d[1:])
    assert sum_d == 2**14 - 1 + 2**15
    assert pair_budget_ok(sum_d)
    assert pair_budget_ok(15 * 2**15)                                   # the largest sum the flag's per-entry limit admits
    # the budget is real: with the one-round form's 2^27 row-sum scale (|sum_t| up to P instead of P/2 + P/16) a pair's three products
    # leave the range the next product assumes
    assert not pair_budget_ok(sum_d, sh_pair=SH_ONE)
    assert not pair_budget_ok(2**40)                                     # and a row-sum accumulator that is too large


def test_full_size_diagonal_takes_the_one_round_form():
    rng = np.random.default_rng(5)
    diag = list(pyref.PARAMS["internal_diag"])
    diag[7] = 0x3C4F1E2B % P
    k = Consts(diag, pyref.PARAMS["internal_rc"])
    assert not k.pair
    for st in _edge_states()[:5] + [[int(x) for x in rng.integers(0, P, 16)] for _ in range(8)]:
        assert permutation(st, k, pyref.PARAMS["internal_rc"], rng) == reference(st, diag, pyref.PARAMS["internal_rc"])
    # a small non-power-of-two diagonal still qualifies, and the pairs compute it
    diag = [P - 2, 1, 3, 5, 7, 9, 11, 13, 17, 19, 23, 29, 31, 37, 41, 32768]
    k = Consts(diag, pyref.PARAMS["internal_rc"])
    assert k.pair
    for st in _edge_states()[:5] + [[int(x) for x in rng.integers(0, P, 16)] for _ in range(8)]:
        assert permutation(st, k, pyref.PARAMS["internal_rc"], rng) == reference(st, diag, pyref.PARAMS["internal_rc"])
    assert reference([3] * 16, pyref.PARAMS["internal_diag"], pyref.PARAMS["internal_rc"]) == pyref.poseidon2([3] * 16)
