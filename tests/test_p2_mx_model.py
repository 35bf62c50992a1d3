"""A numpy model of the matrix-core external layer of the width-16 Poseidon2 permutation (poseidon2.cuh, p2_permute_mx_dev), steps 1-3:
S-box output as balanced base-256 digits, the int8 contraction with M_E, and the recombination to one signed word per element.  The model
runs the whole permutation with it and must give pyref.poseidon2's words; every bound the device arithmetic relies on is asserted on the
way.  The layer is linear, so the model works on canonical words: the Montgomery factor of the device state commutes with it."""
import numpy as np

import pyref
from p2_device_model import dsmred, mx_layer  # noqa: F401

P = pyref.P
MX_BIAS = 0x80808080 - P
C24 = pow(2, 56, P) if pow(2, 56, P) <= P // 2 else pow(2, 56, P) - P     # centred(2^56 mod P)
MU = pow(P, -1, 2**32)
ME = np.array(pyref.ME, dtype=np.int64)


def _inv_mod_matrix(m):
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


ME_INV = _inv_mod_matrix(pyref.ME)


def _pre(v):
    return [sum(ME_INV[i][j] * v[j] for j in range(16)) % P for i in range(16)]


def _lazy(v, rng):
    """a value in [0, P) as the device's lazy reduction may leave it: v or v + P"""
    return v + P if rng is not None and rng.integers(2) else v


def poseidon2_mx(state, rng=None, stats=None):
    rc_e, rc_i = pyref.PARAMS["external_rc"], pyref.PARAMS["internal_rc"]
    folds = [_pre(rc_e[r + 1]) for r in range(3)] + [_pre([rc_i[0]] + [0] * 15)] + [_pre(rc_e[r + 1]) for r in range(4, 7)] + [[0] * 16]
    s = [x % P for x in state]
    w = mx_layer([s[i] + _pre(rc_e[0])[i] for i in range(16)], stats)   # first layer: canonical + M_E^-1 rc_0 < 2P
    for r in range(4):
        w = mx_layer([_lazy((pow(w[i] % P, 7, P) + folds[r][i]) % P, rng) for i in range(16)], stats)
    s = [x % P for x in w]                                                # int_rc[0] is in s[0] already
    for r in range(13):
        s[0] = pow(s[0], 7, P)
        s = [(sum(pyref.MI[i][j] * s[j] for j in range(16))) % P for i in range(16)]
        if r < 12:
            s[0] = (s[0] + rc_i[r + 1]) % P
    w = [(s[i] + rc_e[4][i]) % P for i in range(16)]
    w = mx_layer([_lazy((pow(w[i], 7, P) + folds[4][i]) % P, rng) for i in range(16)], stats)
    for r in range(5, 8):
        w = mx_layer([_lazy((pow(w[i] % P, 7, P) + folds[r][i]) % P, rng) for i in range(16)], stats)
    return [x % P for x in w]


def test_mx_layer_extremes():
    stats = {}
    for u in ([0] * 16, [2 * P - 1] * 16, [P - 1] * 16, [P] * 16, [0, 2 * P - 1] * 8, [2 * P - 1, 0] * 8,
              [P - 1 if i % 4 == 0 else 2 * P - 1 for i in range(16)]):
        mx_layer(u, stats)
    # the worst digits: every u - P with all four digits at -128 or 127 where the range allows
    lo = [-128 - 128 * 256 - 128 * 65536 - 119 * 2**24 + P] * 16
    hi = [127 + 127 * 256 + 127 * 65536 + 119 * 2**24 + P] * 16
    for u in (lo, hi, [lo[0], hi[0]] * 8):
        assert all(0 <= x < 2 * P for x in u)
        mx_layer(u, stats)
    assert stats["Y"] <= 35 * 128


def test_mx_layer_random():
    rng = np.random.default_rng(7)
    for _ in range(300):
        mx_layer([int(x) for x in rng.integers(0, 2 * P, 16)])


def test_fold_bias_bounds():
    # the S-box's last product sum x6 t + fold, fold = c + P 2^31 + MX_BIAS 2^32 with |c| <= P/2, |x6|, |t| < P: positive, and the unsigned
    # Montgomery reduction's 64-bit sum (x + m P, m < 2^32) stays below 2^64, so the result is u + MX_BIAS with u in [0, 2P)
    for prod in (-(P - 1) ** 2, (P - 1) ** 2):
        for c in (-(P // 2), P // 2):
            x = prod + c + (P << 31) + (MX_BIAS << 32)
            assert 0 < x < 2**63
            assert x + (2**32 - 1) * P < 2**64
            assert (x + (2**32 - 1) * P) >> 32 < 2 * P + MX_BIAS <= 2**32


def test_permutation_matches_pyref():
    rng = np.random.default_rng(11)
    states = [[0] * 16, [P - 1] * 16, [1] * 16, [0, P - 1] * 8, [P - 1] + [0] * 15, list(range(16))]
    states += [[int(x) for x in rng.integers(0, P, 16)] for _ in range(24)]
    stats = {}
    for st in states:
        assert poseidon2_mx(st, rng, stats) == pyref.poseidon2(st)
        assert poseidon2_mx(st, None, stats) == pyref.poseidon2(st)
    assert stats["w"] < P
