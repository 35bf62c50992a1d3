"""The leaf sponge's permutation forms (ABSORB / ABSORB_RATE / SQUEEZE, poseidon2.cuh p2_permute_mx_form) in the device's exact integer steps
(p2_sponge_model): every accumulator in range, the signed capacity words' first layer by intervals, and chains of blocks against the closed
matrix-core form applied block by block and against the specification's sponge.  CPU only."""
import numpy as np
import pytest

import p2_device_model as dm
import p2_sponge_model as sm
import p2_steer
import pyref

P, R, RINV = dm.P, dm.R, dm.RINV


def _spec_sponge(row):
    s = [0] * 16
    for q in range(0, len(row), 8):
        blk = [int(v) % P for v in row[q:q + 8]]
        s[:len(blk)] = blk
        s = [int(v) for v in pyref.poseidon2(s)]
    return s[:8]


def test_constants():
    k = sm.SPONGE
    u0 = dm.FULL16.u0
    assert all(abs(c) <= P // 2 and (c - u0[8 + i]) % P == 0 for i, c in enumerate(k.cap0))
    # the all-zero capacity in the signed form is cap0, and a first layer on it spells u0 itself
    assert sm.signed_cap([0] * 8) == k.cap0
    for c in k.cap0:
        d, n = sm.first_layer_digits(c, sm.DIGIT_BIAS)
        assert n == c and abs(d[3]) <= 120


def test_signed_first_layer_intervals():
    """a signed capacity word w in (-P, P), |w| up to the bound a layer can emit, takes the digit bias alone"""
    B = sm.W_BOUND
    assert B >= 2**28.2 + P / 2
    mean = lambda w: w % P                                            # the word already means s + u0
    assert sm.first_layer_interval(-B, B, sm.DIGIT_BIAS, mean) <= 4480
    for w in (0, 1, -1, P - 1, -(P - 1)):                             # the edge words, exactly (P - 1 is past what a layer emits, and still in range)
        d, n = sm.first_layer_digits(w, sm.DIGIT_BIAS)
        assert n == w and all(-128 <= x <= 127 for x in d) and abs(d[3]) <= 120
        assert 35 * max(abs(x) for x in d) <= 4480


def test_signed_first_layer_fails_with_the_canonical_constant():
    """the same pass with in0 = u0 + MX_BIAS, the canonical words' constant, on a signed word: every capacity element fails it (the value leaves the
    digit range or the digits spell w + u0 - P, another element); and adding u0 to the signed word in the first layer, without the - P, leaves the
    range for the built-in constants too"""
    B = sm.W_BOUND
    mean = lambda w: w % P
    for i in range(8, 16):
        in0 = dm.FULL16.u0[i] + dm.MX_BIAS
        with pytest.raises(AssertionError):
            sm.first_layer_interval(-B, B, in0, mean)
    assert any(B + u + sm.DIGIT_BIAS >= 2**32 for u in dm.FULL16.u0[8:])
    with pytest.raises(AssertionError):
        for i in range(8, 16):
            sm.first_layer_interval(-B, B, dm.FULL16.u0[i] + sm.DIGIT_BIAS, lambda w, i=i: (w + dm.FULL16.u0[i]) % P)


def _rows(n_blocks, seed):
    rng = np.random.default_rng(seed)
    rows = [[int(v) for v in rng.integers(0, P, 8 * n_blocks)] for _ in range(3)]
    edges = p2_steer.edge_words()
    for n, w in enumerate(edges):                                      # an edge word in the rate words of every block, and rotating through them
        rows.append([w * RINV % P] * (8 * n_blocks))                   # (the DEVICE word is the edge word: rows are field elements, words x R)
        rows.append([edges[(n + i) % len(edges)] * RINV % P for i in range(8 * n_blocks)])
    return rows


@pytest.mark.parametrize("n_blocks", [2, 3])
def test_chains_equal_the_closed_form(n_blocks):
    stats = {}
    for row in _rows(n_blocks, 0x5350 + n_blocks):
        got = sm.sponge_forms(row, stats=stats)
        assert got == sm.sponge_closed(row)
        assert got == _spec_sponge(row)
    assert stats["Y"] <= 4480 and stats["d3"] <= 120 and stats["w"] < 2**28.2 + P / 2


def test_chain_of_32_blocks():
    """the headline's 256-wide row: 31 ABSORB and one SQUEEZE; random words, and the edge words rotating through all 256 positions"""
    rng = np.random.default_rng(0x53503332)
    edges = p2_steer.edge_words()
    rows = [[int(v) for v in rng.integers(0, P, 256)], [edges[i % len(edges)] * RINV % P for i in range(256)], [0] * 256, [(P - 1) * RINV % P] * 256]
    stats = {}
    for row in rows:
        got = sm.sponge_forms(row, stats=stats)
        assert got == sm.sponge_closed(row) == _spec_sponge(row)
    assert stats["Y"] <= 4480 and stats["d3"] <= 120


@pytest.mark.parametrize("width", [4, 8, 12, 16, 20, 24, 260])
def test_widths_with_a_half_block(width):
    """SQUEEZE alone (4, 8), ABSORB_RATE before a half block (12, 20, 260: the half block keeps s[4..7]), plain chains (16, 24)"""
    rng = np.random.default_rng(width)
    for row in ([int(v) for v in rng.integers(0, P, width)], [0] * width, [(P - 1) * RINV % P] * width):
        assert sm.sponge_forms(row) == sm.sponge_closed(row) == _spec_sponge(row)


def test_steered_second_block_capacity():
    """every capacity lane of the SECOND block's first layer meets the digit words -128 / 127 / 0 / -1 (all 64 triples), and the alternating and
    top-digit patterns: the first block run backwards from them"""
    exact = 0
    for label, cap, row in sm.steered_rows(2):
        x = [v * R % P for v in row]
        _, c = sm.permute_form("ABSORB", x[:8], sm.signed_cap([v * R % P for v in cap]))
        words = dict(p2_steer.digit_patterns())[label]
        assert [v % P for v in c] == list(words[8:])                   # the field elements arrive
        if label.startswith("dig:"):
            # ... and as these very integers: |n| < 2^24 and |n +- P| is past what a layer emits, so the digits are the pattern's
            a, b, cc, _ = (int(t) for t in label[4:].split(","))
            for v in c:
                d, n = sm.first_layer_digits(v, sm.DIGIT_BIAS)
                assert d == [a, b, cc, 0] and n == v
            exact += 1
        assert sm.sponge_forms(row, cap) == sm.sponge_closed(row, cap)
    assert exact == 64
