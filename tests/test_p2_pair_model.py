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

from p2_device_model import (H, I32, MU, P, R, SH_ONE, SH_PAIR, Consts, cen, dsmred, internal_rounds, mad, pair_budget_ok, round_one,  # noqa: F401
                             round_pair, sbox)


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
