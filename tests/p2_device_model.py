"""The device's integer steps of every Poseidon2 permutation form (poseidon2.cuh, hash.hip / poseidon2_coop.cuh), exactly, in Python integers.

One model per form, all on MONTGOMERY WORDS as the device holds them (canonical states are converted at the door):
  permute_valu    p2_permute_dev: + ext_rcm, p2_sbox_fold_dev (signed products, the fold constant biased by P 2^31, dmred_lazy, dred),
                  p2_external_linear_signed_dev (dadd / ddbl on canonical words, then + t - P), the partial rounds paired or one at a time
  permute_mx      p2_permute_mx_dev: the same S-box with the fold constant carrying MX_BIAS 2^32 as well, the real dmred_lazy (which of u,
                  u + P comes out is computed, not guessed), the digit contraction mx_layer, the same partial rounds
  permute_coop    coop_permute: p2_sbox_rc_dev, dadd / ddbl / dmul on canonical words, one state over 16 lanes
  permute24       p24_permute_dev end to end, 21 partial rounds at the 2^26 row-sum scale
Every 64-bit accumulator and 32-bit result is asserted in range where it is made, and with a `log` list every intermediate is appended as
(round, lane, name, value); round is the probe of p2_steer ("L0", ("F", r), ("P", r), "OUT").  The constants are recomputed here from the
parameter JSON files (not read from derive_tables()).

The interval passes (magnitudes only, every centred constant at its largest) are pair_budget_ok for the paired partial rounds of width 16
and round_budget_ok for a partial round on its own: width 24 holds at the 2^26 scale and fails at 2^27."""
import numpy as np

import p2_steer
import pyref

P = pyref.P
R = 2**32 % P
RINV = pow(R, -1, P)
MU = pow(P, -1, 2**32)                  # MONTY_MU_POS
MU_NEG = 2**32 - MU                     # MONTY_MU_NEG
M32 = 2**32 - 1
H = (P - 1) // 2                        # the largest magnitude of a centred constant
SH_ONE, SH_PAIR, SH_24 = 27, 24, 26     # row-sum scales: the one-round form's, a pair's first round's, width 24's
I32 = 2**31 - 1
MX_BIAS = 0x80808080 - P
C24 = pow(2, 56, P) if pow(2, 56, P) <= P // 2 else pow(2, 56, P) - P     # centred(2^56 mod P)
ME = np.array(pyref.ME, dtype=np.int64)


def cen(x):
    x %= P
    return x - P if x > P // 2 else x


def i32(x):
    """the low 32 bits read as int32"""
    x &= M32
    return x - 2**32 if x >= 2**31 else x


# ---- babybear.cuh
def dsmred(t):
    """dsmred: t / 2^32 mod P for a signed 64-bit t, the device's exact integer steps"""
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


def dsmont(a, b):
    return dsmred(mad(a, b, 0))


def dmred_lazy(x):
    """dmred_lazy: x / 2^32 mod P for an unsigned 64-bit x, result in [0, 2P) when x < 2^32 P"""
    assert 0 <= x < 2**64
    m = (x & M32) * MU_NEG & M32
    y = x + m * P
    assert y < 2**64 and y % 2**32 == 0
    return y >> 32


def dred(x):
    """[0, 2P) -> [0, P): v_subrev_co + v_cndmask"""
    assert 0 <= x < 2 * P
    return x - P if x >= P else x


def dadd(a, b):
    assert 0 <= a < P and 0 <= b < P
    return dred(a + b)


def ddbl(a):
    return dadd(a, a)


def dmul(a, b):
    assert 0 <= a < P and 0 <= b < P
    return dred(dmred_lazy(a * b))


def dcanon(x):
    """[-P, P) -> [0, P): v_add + v_min_u32 (-P, which the signed external layer can hand over, wraps to 0 like any negative word)"""
    assert -P <= x < P
    u = x & M32
    v = (u + P) & M32
    r = v if v < u else u
    assert r < P
    return r


def sbox(t, log=None, at=None):
    """p2_sbox_signed: t^7 in four signed Montgomery products"""
    x2 = dsmred(mad(t, t, 0))
    x4 = dsmred(mad(x2, x2, 0))
    x6 = dsmred(mad(x4, x2, 0))
    x7 = dsmred(mad(x6, t, 0))
    if log is not None:
        log += [at + ("t", t), at + ("x2", x2), at + ("x4", x4), at + ("x6", x6), at + ("x7", x7)]
    return x7


# ---- the interval passes
def _red(x):
    """a bound of |dsmred(X)| for |X| <= x; raises where the reduction's 64-bit sum or its 32-bit result could overflow"""
    if x > 2**63 - 1 - 2**31 * P:
        raise OverflowError
    r = x // 2**32 + P // 2 + 1
    if r > I32:
        raise OverflowError
    return r


def _sbox_b(t):
    x2 = _red(t * t)
    x4 = _red(x2 * x2)
    x6 = _red(x4 * x2)
    return _red(x6 * t)


def pair_budget_ok(sum_d, sh_pair=SH_PAIR, bounds=None):
    """The interval pass: magnitudes only, every centred constant taken at its largest (P - 1) / 2, so the answer depends on the diagonal
    through sum_{i>=1} d_i alone.  sh_pair is the row-sum scale of a pair's first round.  bounds (a dict) receives the largest |st|, |s1| and
    state word |v| the pass derives."""
    red, sbox_b = _red, _sbox_b
    try:
        b0 = bv = P                                                     # the signed external layer hands over words in [-P, P)
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
            if bounds is not None:
                bounds["st"] = max(bounds.get("st", 0), st)
                bounds["s1"] = max(bounds.get("s1", 0), s1)
                bounds["v"] = max(bounds.get("v", 0), b0, bv, v0)
        return True
    except OverflowError:
        return False


def round_budget_ok(n, sh, rounds, bounds=None):
    """The same pass for partial rounds run one at a time on n words with the row sum scaled by 2^sh (p2_internal_round_dev: n = 16, sh = 27;
    p24_internal_rounds_dev: n = 24, sh = 26): T = 2^sh (u + sum v_i), sum = T / R, T2 = sum K, v_i <- (v_i D_i + T2 [+ rc]) / R.
    bounds receives the largest |sum| and |v| derived."""
    try:
        b0 = bv = P
        for _ in range(rounds):
            u = _sbox_b(b0)
            s = _red((u + (n - 1) * bv) << sh)
            b0, bv = _red(u * H + s * H + H), _red(bv * H + s * H)
            if max(b0, bv) > P - 1:
                return False
            if bounds is not None:
                bounds["sum"] = max(bounds.get("sum", 0), s)
                bounds["v"] = max(bounds.get("v", 0), b0, bv)
        return True
    except OverflowError:
        return False


# ---- the partial rounds of width 16
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


def round_one(v, r, k, log=None, track=None):
    u = sbox(v[0], log, (("P", r), 0))
    T = 0
    for x in [u] + v[1:]:
        T = mad(x, 1 << SH_ONE, T)
    s = dsmred(T)
    T2 = mad(s, k.K27, 0)
    out = [dsmred(mad(u, k.D[0], T2 + k.rc_fold[r]))] + [dsmred(mad(v[i], k.D[i], T2)) for i in range(1, 16)]
    if log is not None:
        log.append((("P", r), 0, "sum", s))
        log += [(("P", r), i, "v", x) for i, x in enumerate(out)]
    if track is not None:
        track["sum"] = max(track.get("sum", 0), abs(s))
        track["v1"] = max(track.get("v1", 0), max(abs(x) for x in out))
    return out


def round_pair(v, r, k, track=None, log=None):
    A = 0
    for i in range(1, 16):
        A = mad(v[i], k.d[i], A)                                       # the exact multipliers d_i 2^s, s = 0
    u = sbox(v[0], log, (("P", r), 0))
    T = 0
    for x in [u] + v[1:]:
        T = mad(x, 1 << SH_PAIR, T)
    st = dsmred(T)
    v0 = dsmred(mad(u, k.D[0], mad(st, k.K24, 0) + k.rc_fold[r]))
    A = mad(st, k.C15, A)
    u2 = sbox(v0, log, (("P", r + 1), 0))
    A = mad(u2, 1, A)
    s1 = dsmred(A)
    T2 = mad(s1, k.K1, 0)
    out = [dsmred(mad(u2, k.D[0], T2 + k.rc_fold[r + 1]))] + [dsmred(mad(v[i], k.D2[i], mad(st, k.E[i], T2))) for i in range(1, 16)]
    if track is not None:
        track["st"] = max(track.get("st", 0), abs(st))
        track["s1"] = max(track.get("s1", 0), abs(s1))
        track["v"] = max(track.get("v", 0), max(abs(x) for x in out), abs(v0))
    if log is not None:
        log += [(("P", r), 0, "sum", st), (("P", r + 1), 0, "sum", s1)]
        log += [(("P", r + 1), i, "v", x) for i, x in enumerate(out)]
    return out


def internal_rounds(v, k, track=None, log=None, pair=None):
    """v: signed Montgomery-form words in (-P, P), int_rc[0] already in v[0]; returns canonical Montgomery-form words.  pair = False runs one
    round at a time whatever the constants' flag says (the device's pk16.pair cleared)"""
    assert all(-P <= x < P for x in v)                                  # -P comes out of the signed external layer on zero words
    v = round_one(v, 0, k, log)
    if k.pair and pair is not False:
        for r in range(1, 13, 2):
            v = round_pair(v, r, k, track, log)
    else:
        for r in range(1, 13):
            v = round_one(v, r, k, log, track)
    assert all(abs(x) < P for x in v)
    return [dcanon(x) for x in v]


# ---- the matrix-core external layer
def mx_layer(u, stats=None):
    """u: 16 ints in [0, 2P) (the S-box's lazy outputs, or the input word + the word of M_E^-1 rc_0).  Returns w = M_E (u - P) mod P as
    signed words.  stats receives the largest |Y| of all planes ("Y"), of each plane ("Y0".."Y3"), |w| and the top digit ("d3")."""
    u = np.asarray(u, dtype=np.int64)
    assert ((u >= 0) & (u < 2 * P)).all()
    y = u + MX_BIAS                                                       # step 1: what dmred_lazy returns with the biased fold constant
    assert ((y >= 0) & (y < 2**32)).all()
    b = (y[:, None] >> (8 * np.arange(4))) & 255                        # bytes of y; xor 0x80 and read as int8
    d = (b ^ 0x80).astype(np.int8).astype(np.int64)
    assert (d @ (256 ** np.arange(4)) == u - P).all()
    assert d.min() >= -128 and d.max() <= 127 and np.abs(d[:, 3]).max() <= 120
    Y = ME @ d                                                            # step 2: [element i][plane k], exact in i32
    assert np.abs(Y).max() <= 35 * 128 < 2**13
    L = Y[:, 0] + (Y[:, 1] << 8) + (Y[:, 2] << 16)                       # step 3
    assert np.abs(L).max() < 2**28.2
    T = [(int(L[i]) << 32) + int(Y[i, 3]) * C24 for i in range(16)]
    assert max(abs(t) for t in T) < 2**60.2
    w = [dsmred(t) for t in T]
    assert max(abs(x) for x in w) < 2**28.2 + P / 2 < P
    assert all((w[i] - sum(int(ME[i, j]) * int(u[j]) for j in range(16))) % P == 0 for i in range(16))
    if stats is not None:
        ay = np.abs(Y).max(axis=0)
        stats["Y"] = max(stats.get("Y", 0), int(ay.max()))
        for p in range(4):
            stats["Y%d" % p] = max(stats.get("Y%d" % p, 0), int(ay[p]))
        stats["d3"] = max(stats.get("d3", 0), int(np.abs(d[:, 3]).max()))
        stats["w"] = max(stats.get("w", 0), max(abs(x) for x in w))
    return w


# ---- the full rounds
def _m4(x0, x1, x2, x3):
    t01, t23 = dadd(x0, x1), dadd(x2, x3)
    t0123 = dadd(t01, t23)
    t01123, t01233 = dadd(t0123, x1), dadd(t0123, x3)
    return dadd(t01123, t01), dadd(t01123, ddbl(x2)), dadd(t01233, t23), dadd(t01233, ddbl(x0))


def _m4_hl(x0, x1, x2, x3):
    t0, t1 = dadd(x0, x1), dadd(x2, x3)
    t2, t3 = dadd(ddbl(x1), t1), dadd(ddbl(x3), t0)
    t4, t5 = dadd(ddbl(ddbl(t1)), t3), dadd(ddbl(ddbl(t0)), t2)
    return dadd(t3, t5), t5, dadd(t2, t4), t4


def _blocks(s, w):
    m4 = _m4 if w == 16 else _m4_hl
    s = [x for b in range(0, w, 4) for x in m4(*s[b:b + 4])]
    if w == 16:
        t = [dadd(dadd(s[k], s[4 + k]), dadd(s[8 + k], s[12 + k])) for k in range(4)]
    else:
        t = [dadd(dadd(dadd(s[k], s[4 + k]), dadd(s[8 + k], s[12 + k])), dadd(s[16 + k], s[20 + k])) for k in range(4)]
    return s, t


def external_linear(s, w):
    """p2_external_linear_dev / p24_external_linear_dev: canonical in and out"""
    s, t = _blocks(s, w)
    return [dadd(s[i], t[i & 3]) for i in range(w)]


def external_linear_signed(s, w):
    """p2_external_linear_signed_dev / p24_...: canonical in, s_i + (t - P) out as signed words in [-P, P - 2]: -P itself where a word
    and its column sum are both 0"""
    s, t = _blocks(s, w)
    out = [i32(s[i] + ((t[i & 3] - P) & M32)) for i in range(w)]
    assert all(-P <= x <= P - 2 for x in out)
    return out


class FullConsts:
    """the full rounds' constants of a width as the table builder derives them (make_p2_consts, make_p2_ext_fold, make_p2_mx_consts)"""

    def __init__(self, width, rc_i0=None):
        rc_e, rc_i, _ = p2_steer.params(width)
        self.w = width
        self.ext_rc = [[c * R % P for c in row] for row in rc_e]
        self.ext_rcm = [[(c - P) & M32 for c in row] for row in self.ext_rc]              # rc - P mod 2^32
        pre = p2_steer.folds(width, rc_e, [rc_i[0] if rc_i0 is None else rc_i0])
        self.fold = [[cen(u * R * R) + (P << 31) for u in row] for row in pre]
        self.fold_mx = [[c + (MX_BIAS << 32) for c in row] for row in self.fold]
        self.u0 = [u * R % P for u in p2_steer.matvec(p2_steer.ME_INV[width], rc_e[0])]  # in0 - MX_BIAS
        assert all(abs(c - (P << 31)) <= P // 2 for row in self.fold for c in row)


def sbox_fold(t, fold, log, at):
    """p2_sbox_fold_dev / p2_sbox_mx_dev up to the lazy value: dmred_lazy(x6 t + fold), fold biased by P 2^31 (and MX_BIAS 2^32)"""
    assert -P <= t <= P
    x2 = dsmont(t, t)
    x4 = dsmont(x2, x2)
    x6 = dsmont(x4, x2)
    x = mad(x6, t, fold)
    assert x > 0
    y = dmred_lazy(x)
    assert y < 2**32
    if log is not None:
        log += [at + ("t", t), at + ("x2", x2), at + ("x4", x4), at + ("x6", x6)]
    return y


def _full_valu(s, r, k, log):
    """one full round of the all-VALU form: signed S-box inputs in, the next round's signed S-box inputs (or the partial rounds' state) out"""
    u = [sbox_fold(s[i], k.fold[r][i], log, (("F", r), i)) for i in range(k.w)]
    assert all(x < 2 * P for x in u)
    if log is not None:
        log += [(("F", r), i, "u", x) for i, x in enumerate(u)]
    return external_linear_signed([dred(x) for x in u], k.w)


def _full_mx(s, r, k, log, stats):
    y = [sbox_fold(s[i], k.fold_mx[r][i], log, (("F", r), i)) for i in range(16)]
    u = [x - MX_BIAS for x in y]
    assert all(0 <= x < 2 * P for x in u)
    if log is not None:
        log += [(("F", r), i, "u", x) for i, x in enumerate(u)]
    st = {}
    w = mx_layer(u, st)
    if log is not None:
        log += [(("F", r), p, "Y", st["Y%d" % p]) for p in range(4)] + [(("F", r), 0, "d3", st["d3"])]
    if stats is not None:
        for key, val in st.items():
            stats[key] = max(stats.get(key, 0), val)
    return w


def _log_out(out, log):
    if log is not None:
        log += [("OUT", i, "out", x) for i, x in enumerate(out)]
    return [x * RINV % P for x in out]


FULL16 = FullConsts(16)
FULL24 = FullConsts(24)
BUILTIN = Consts(pyref.PARAMS["internal_diag"], pyref.PARAMS["internal_rc"])


def _full16_for(k):
    """the full rounds' constants that go with a set of partial-round constants: fold[3] carries int_rc[0]"""
    return FULL16 if k is BUILTIN else k.full


def consts_for(diag, rc_i):
    """the constants of a loaded width-16 parameter set (the external ones stay the built-in)"""
    k = Consts(diag, rc_i)
    k.full = FullConsts(16, rc_i[0])
    k.int_rc = [c * R % P for c in rc_i]
    k.diag_m = [x * R % P for x in k.d]
    return k


BUILTIN.int_rc = [c * R % P for c in pyref.PARAMS["internal_rc"]]
BUILTIN.diag_m = [x * R % P for x in BUILTIN.d]


def permute_valu(state, k=BUILTIN, pair=None, log=None, track=None):
    """p2_permute_dev on a canonical state; pair = None takes the flag of the constants, False clears it (one round at a time)"""
    f = _full16_for(k)
    s = external_linear([int(x) % P * R % P for x in state], 16)
    s = [i32(s[i] + f.ext_rcm[0][i]) for i in range(16)]
    for r in range(4):
        s = _full_valu(s, r, f, log)
    s = internal_rounds(s, k, track, log, pair)
    s = [i32(s[i] + f.ext_rcm[4][i]) for i in range(16)]
    for r in range(4, 8):
        s = _full_valu(s, r, f, log)
    return _log_out([dcanon(x) for x in s], log)


def permute_mx(state, k=BUILTIN, pair=None, log=None, track=None, stats=None):
    """p2_permute_mx_dev on a canonical state"""
    f = _full16_for(k)
    x = [int(v) % P * R % P for v in state]
    st = {}
    w = mx_layer([x[i] + f.u0[i] for i in range(16)], st)               # canonical word + in0 - MX_BIAS < 2P
    if log is not None:
        log += [("L0", p, "Y", st["Y%d" % p]) for p in range(4)] + [("L0", 0, "d3", st["d3"])]
    if stats is not None:
        for key, val in st.items():
            stats[key] = max(stats.get(key, 0), val)
    for r in range(4):
        w = _full_mx(w, r, f, log, stats)
    s = internal_rounds(w, k, track, log, pair)
    w = [i32(s[i] + f.ext_rcm[4][i]) for i in range(16)]
    for r in range(4, 8):
        w = _full_mx(w, r, f, log, stats)
    return _log_out([dcanon(x) for x in w], log)


# ---- coop_permute: one state over the 16 lanes of a DPP row, canonical words throughout
def sbox_rc(x, rcm, log, at):
    """p2_sbox_rc_dev: (x + rc)^7 for canonical x, rcm = rc - P mod 2^32; the last product carries + P, then dred"""
    assert 0 <= x < P
    t = i32(x + rcm)
    assert -P < t < P
    x2 = dsmont(t, t)
    x4 = dsmont(x2, x2)
    x6 = dsmont(x4, x2)
    u = (dsmont(x6, t) + P) & M32
    if log is not None:
        log += [at + ("t", t), at + ("x2", x2), at + ("x4", x4), at + ("x6", x6), at + ("u", u)]
    return dred(u)


def _coop_linear(x):
    rot = lambda v, n: v[n:] + v[:n]
    quad = lambda v, n: [v[4 * (i // 4) + (i + n) % 4] for i in range(16)]
    r1, r2, r3 = quad(x, 1), quad(x, 2), quad(x, 3)
    y = [dadd(dadd(dadd(dadd(x[i], r1[i]), dadd(r2[i], r3[i])), x[i]), ddbl(r1[i])) for i in range(16)]
    # row_ror:n gives lane i the value of lane (i - n) mod 16
    t = [dadd(y[i], y[(i - 4) % 16]) for i in range(16)]
    t = [dadd(t[i], t[(i - 8) % 16]) for i in range(16)]
    return [dadd(y[i], t[i]) for i in range(16)]


def permute_coop(state, k=BUILTIN, log=None):
    f = _full16_for(k)
    int_rcm = [(c - P) & M32 for c in k.int_rc]
    x = _coop_linear([int(v) % P * R % P for v in state])
    for r in range(8):
        if r == 4:
            for p in range(13):
                x = [sbox_rc(x[0], int_rcm[p], log, (("P", p), 0))] + x[1:]
                t = x
                for n in (8, 4, 2, 1):
                    t = [dadd(t[i], t[(i - n) % 16]) for i in range(16)]
                if log is not None:
                    log.append((("P", p), 0, "sum", t[0]))
                x = [dadd(dmul(x[i], k.diag_m[i]), t[i]) for i in range(16)]
        x = _coop_linear([sbox_rc(x[i], f.ext_rcm[r][i], log, (("F", r), i)) for i in range(16)])
    return _log_out(x, log)


# ---- width 24
class Consts24:
    def __init__(self):
        _, rc_i, d = p2_steer.params(24)
        self.D = [cen(x * R) for x in d]
        self.rc_fold = [cen(rc_i[r + 1] * R * R) for r in range(20)] + [0]
        self.K = cen(2**(64 - SH_24))                                  # to_monty(64) = 2^38
        self.ok = round_budget_ok(24, SH_24, 21)


BUILTIN24 = Consts24()


def internal_rounds24(v, k=BUILTIN24, track=None, log=None):
    """p24_internal_rounds_dev: signed words in (int_rc[0] already in v[0]), canonical words out"""
    assert all(-P <= x < P for x in v)
    for r in range(21):
        u = sbox(v[0], log, (("P", r), 0))
        T = 0
        for x in [u] + v[1:]:
            T = mad(x, 1 << SH_24, T)
        s = dsmred(T)
        T2 = mad(s, k.K, 0)
        v = [dsmred(mad(u, k.D[0], T2 + k.rc_fold[r]))] + [dsmred(mad(v[i], k.D[i], T2)) for i in range(1, 24)]
        assert all(abs(x) < P for x in v)
        if log is not None:
            log.append((("P", r), 0, "sum", s))
            log += [(("P", r), i, "v", x) for i, x in enumerate(v)]
        if track is not None:
            track["sum"] = max(track.get("sum", 0), abs(s))
            track["v"] = max(track.get("v", 0), max(abs(x) for x in v))
    return [dcanon(x) for x in v]


def permute24(state, log=None, track=None):
    """p24_permute_dev on a canonical state"""
    f = FULL24
    s = external_linear([int(x) % P * R % P for x in state], 24)
    s = [i32(s[i] + f.ext_rcm[0][i]) for i in range(24)]
    for r in range(4):
        s = _full_valu(s, r, f, log)
    s = internal_rounds24(s, BUILTIN24, track, log)
    s = [i32(s[i] + f.ext_rcm[4][i]) for i in range(24)]
    for r in range(4, 8):
        s = _full_valu(s, r, f, log)
    return _log_out([dcanon(x) for x in s], log)
