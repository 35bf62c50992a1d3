"""The sponge forms of the matrix-core permutation (poseidon2.cuh: p2_permute_mx_form ABSORB / ABSORB_RATE / SQUEEZE) in the device's exact
integer steps, on top of p2_device_model.  CPU only.

Between the blocks of an overwrite-mode sponge the capacity words 8..15 travel as the last layer's signed words with the next first layer's
constant already in them: round 7 of a non-final block takes fold7a = M_E^-1 (0 on the rate elements, u0 on the capacity elements) where the
closed form has zero, u0 = M_E^-1 ext_rc[0], and the next first layer adds the digit bias 0x80808080 alone to such a word.  A sponge starts from
cap0 = centred(u0[8..15]), the all-zero capacity in that form.  Words are Montgomery form as the device holds them; rows and digests at the
module's edge are canonical field elements like pyref's."""
import numpy as np

import p2_device_model as dm
import p2_steer

P, R, RINV, M32, MX_BIAS = dm.P, dm.R, dm.RINV, dm.M32, dm.MX_BIAS
DIGIT_BIAS = 0x80808080
# the largest |w| a matrix-core layer hands on (mx_layer's own bound): 2^28.2 + P / 2
W_BOUND = int(2**28.2) + P // 2 + 2


class SpongeConsts:
    """make_p2_mx_consts' fold7a and cap0, beside the closed form's constants"""

    def __init__(self, full=dm.FULL16):
        self.full = full
        u0_plain = [u * RINV % P for u in full.u0]
        v = p2_steer.matvec(p2_steer.ME_INV[16], [0] * 8 + u0_plain[8:])
        self.fold7a = [dm.cen(x * R * R) + (P << 31) + (MX_BIAS << 32) for x in v]
        self.cap0 = [dm.cen(x) for x in full.u0[8:]]
        assert all(abs(c - (P << 31) - (MX_BIAS << 32)) <= P // 2 for c in self.fold7a)
        # pushed through the layer, fold7a's preimage gives nothing on the rate elements and u0 on the capacity elements
        assert p2_steer.matvec(p2_steer.ME[16], v) == [0] * 8 + u0_plain[8:]


SPONGE = SpongeConsts()


def first_layer_digits(word, const):
    """The first layer's digit word of one element: (word + const) mod 2^32 xor 0x80808080, bytes read as int8.  Asserts the device's add does
    not wrap and returns (digits plane 0 first, the integer they spell)."""
    y = word + const
    assert 0 <= y < 2**32, "the biased word leaves 32 bits"
    d = [((y >> (8 * k) & 255) ^ 0x80) - (256 if (y >> (8 * k) & 255) ^ 0x80 >= 128 else 0) for k in range(4)]
    return d, sum(x * 256**k for k, x in enumerate(d))


def first_layer_interval(lo, hi, const, meaning):
    """Interval pass of one first-layer element over the input words lo..hi (integers as the register holds them, signed or canonical) with the
    32-bit constant `const`.  meaning(word) = the field element (Montgomery word mod P) the digits must spell.  Asserts: no 32-bit wrap, every
    plane within [-128, 127], the top plane within [-120, 120], the digits spell the meaning, and returns the bound on |Y| (a row of M_E sums to 35)."""
    top = []
    for w in (lo, hi):
        d, n = first_layer_digits(w, const)
        assert all(-128 <= x <= 127 for x in d)
        assert (n - meaning(w)) % P == 0, "the digits spell another field element"
        top.append(d[3])
    # the integer spelled is word + const - 0x80808080, monotone in the word, and so is its top balanced digit
    assert -120 <= top[0] <= top[1] <= 120, "top digit plane out of [-120, 120]"
    y_bound = 35 * 128
    assert y_bound <= 4480
    return y_bound


def _stats(stats, st):
    if stats is not None:
        for key, val in st.items():
            stats[key] = max(stats.get(key, 0), val)


def permute_form(form, rate, cap, signed_cap=True, k=dm.BUILTIN, stats=None, log=None):
    """p2_permute_mx_form<form> on Montgomery words: rate = 8 canonical words, cap = 8 capacity words, signed with the first layer's constant
    in them (signed_cap, the sponge forms) or canonical (the CLOSED form).  Returns (rate out or None, capacity out or None): rate canonical;
    capacity signed with the next constant in it for ABSORB / ABSORB_RATE, canonical for CLOSED."""
    assert form in ("CLOSED", "ABSORB", "ABSORB_RATE", "SQUEEZE") and signed_cap == (form != "CLOSED")
    f = dm._full16_for(k)
    assert all(0 <= x < P for x in rate)
    if signed_cap:
        assert all(abs(x) < W_BOUND for x in cap)
        for x in cap:                                   # the device's add of the digit bias alone: no wrap, the digits spell the word
            d, n = first_layer_digits(x, DIGIT_BIAS)
            assert n == x and abs(d[3]) <= 120
        u = [rate[i] + f.u0[i] for i in range(8)] + [x + P for x in cap]
    else:
        assert all(0 <= x < P for x in cap)
        u = [(list(rate) + list(cap))[i] + f.u0[i] for i in range(16)]
    st = {}
    w = dm.mx_layer(u, st)
    _stats(stats, st)
    for r in range(4):
        w = dm._full_mx(w, r, f, log, stats)
    s = dm.internal_rounds(w, k, None, log, None)
    w = [dm.i32(s[i] + f.ext_rcm[4][i]) for i in range(16)]
    for r in range(4, 7):
        w = dm._full_mx(w, r, f, log, stats)
    fold7 = f.fold_mx[7] if form in ("CLOSED", "SQUEEZE") else (SPONGE.fold7a if k is dm.BUILTIN else SpongeConsts(f).fold7a)
    y = [dm.sbox_fold(w[i], fold7[i], log, (("F", 7), i)) for i in range(16)]
    u7 = [x - MX_BIAS for x in y]
    assert all(0 <= x < 2 * P for x in u7)
    st = {}
    w = dm.mx_layer(u7, st)                                            # rows are independent: a block of the layer is a slice of this
    _stats(stats, st)
    if form == "CLOSED":
        out = [dm.dcanon(x) for x in w]
        return out[:8], out[8:]
    if form == "SQUEEZE":
        return [dm.dcanon(x) for x in w[:8]], None
    if form == "ABSORB":
        return None, w[8:]
    return [dm.dcanon(x) for x in w[:8]], w[8:]


def signed_cap(cap_canonical, full=dm.FULL16):
    """canonical capacity words (Montgomery form) in the sponge forms' signed form: centred(c + u0)"""
    return [dm.cen(c + full.u0[8 + i]) for i, c in enumerate(cap_canonical)]


def sponge_forms(row, cap=None, stats=None):
    """hash_rows_sponge_body on one row of canonical field elements (a multiple of 4 of them), optionally from a given canonical capacity
    (field elements): the digest, 8 canonical field elements"""
    assert len(row) % 4 == 0 and len(row) > 0
    x = [int(v) % P * R % P for v in row]
    c = list(SPONGE.cap0) if cap is None else signed_cap([int(v) % P * R % P for v in cap])
    rate = [0] * 8
    nb, half = len(x) // 8, len(x) % 8
    q = 0
    while q + 1 < nb:
        _, c = permute_form("ABSORB", x[8 * q:8 * q + 8], c, stats=stats)
        q += 1
    if half and nb:
        rate, c = permute_form("ABSORB_RATE", x[8 * q:8 * q + 8], c, stats=stats)
        q += 1
    rate = x[8 * q:8 * q + (4 if half else 8)] + (rate[4:] if half else [])
    out, _ = permute_form("SQUEEZE", rate, c, stats=stats)
    return [v * RINV % P for v in out]


def sponge_closed(row, cap=None):
    """the same sponge with the closed matrix-core permutation per block (p2_device_model.permute_mx), canonical field elements"""
    s = [0] * 8 + ([0] * 8 if cap is None else [int(v) % P for v in cap])
    for q in range(0, len(row), 8):
        blk = [int(v) % P for v in row[q:q + 8]]
        s[:len(blk)] = blk
        s = dm.permute_mx(s)
    return s[:8]


def steered_rows(n_blocks=2):
    """Rows of n_blocks blocks with an initial capacity, as (label, capacity, row) of canonical field elements, whose SECOND block's first layer
    meets chosen digit words in all eight capacity lanes: every (a, b, c, 0) with a, b, c in -128 / 127 / 0 / -1, and the alternating and top-digit
    patterns of p2_steer.  The first block is run backwards from an output whose capacity words are the targets minus u0 (the device adds u0 in
    round 7 of the first block), as p2_steer.steer does; what comes back is a full 16-word input, so the row starts from a non-zero capacity."""
    out = []
    rng = np.random.default_rng(0x53504F4E)
    u0 = dm.FULL16.u0
    for label, words in p2_steer.digit_patterns():
        target = [int(rng.integers(0, P)) for _ in range(8)] + [(words[8 + i] - u0[8 + i]) % P for i in range(8)]
        s0 = p2_steer.steer(16, ("OUT",), target)
        rest = [int(v) for v in rng.integers(0, P, 8 * (n_blocks - 1))]
        out.append((label, s0[8:], s0[:8] + rest))
    return out
