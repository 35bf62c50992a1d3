"""The references of test_gpu_reduced_edges.py, held on the CPU: orc_reduced_opening (oracle/stark.c, which orc_prove_shard calls -- the
committed golden proofs pin it inside a proof) against a pure-Python restatement on every switch combination; the case table's literal
forms against the mirror of csrc/stark.hip rowdot_form; the one-candidate-at-a-time proof-of-work search against the oracle's challenger.
All arithmetic is exact: every comparison is word for word."""
import numpy as np
import pytest

import reduced_edges as RE
from oracle_lib import P


@pytest.mark.parametrize("fill", RE.FILLS)
@pytest.mark.parametrize("case", RE.SMALL_CASES, ids=[c[0] for c in RE.SMALL_CASES])
def test_oracle_reduced_opening_matches_the_python_restatement(oracle, case, fill):
    d = RE.build(case, fill, seed=7)
    before = {k: None if d[k] is None else d[k].copy() for k in ("tbuf", "pbuf", "qbuf", "weights", "dinv", "scalars", "out0")}
    got = RE.oracle_expected(oracle, d)
    assert got.dtype == np.uint32 and got.shape == (d["rows"], 4) and (got < P).all()
    assert (got == RE.python_expected(d)).all(), case[0]
    for k, v in before.items():
        assert v is None or (d[k] == v).all(), k


def test_the_padding_columns_do_not_enter(oracle):
    """the padded layout reads only its block: other words in the padding, same result"""
    case = ("pad", 3, 12, 1, 8, 16, 0, 0, 0)
    d = RE.build(case, "uniform")
    exp = RE.oracle_expected(oracle, d)
    d["tbuf"][:, :4] ^= 1
    d["tbuf"][:, 16:] ^= 1
    d["pbuf"][:, 8:] ^= 1
    d["qbuf"][:, 16:] ^= 1
    assert (RE.oracle_expected(oracle, d) == exp).all()
    d["tbuf"][5, 4] ^= 1                                            # ... and a word of the block does
    assert (RE.oracle_expected(oracle, d) != exp).any()


def test_case_table_forms_are_the_mirror_of_rowdot_form():
    assert [RE.lanes_for(w) for w in (4, 8, 12, 16, 20, 32, 36, 64, 68, 1024)] == [1, 2, 4, 4, 8, 8, 16, 16, 16, 16]
    seen = set()
    for name, log_rows, width, padded, p_width, q_width, acc, form_t, form_p in RE.CASES:
        rows = 1 << log_rows
        assert form_t == RE.rowdot_form(width, rows), name
        assert form_p == (RE.rowdot_form(p_width, rows) if p_width else -1), name
        assert width % 4 == 0 and p_width in (0, 8, 260) and q_width in (0, 8, 16)
        seen |= {("t", form_t), ("p", form_p), ("pw", p_width, padded), ("q", q_width, acc), ("regs-beside-generic", form_t > 0 and p_width == 260)}
    assert len({c[0] for c in RE.CASES}) == len(RE.CASES)
    # every kernel, and every switch value in both layouts / both output modes
    assert {("t", f) for f in range(5)} <= seen and {("p", -1), ("p", 0), ("p", 1)} <= seen and ("regs-beside-generic", True) in seen
    assert {("pw", pw, pad) for pw in (0, 8, 260) for pad in (0, 1)} <= seen and {("q", q, a) for q in (0, 8, 16) for a in (0, 1)} <= seen
    # the thresholds: (256 / L) * 16 rows takes the register form, half of it does not, nk = 5 never does
    for width, thr in ((4, 4096), (8, 2048), (12, 1024), (32, 512), (64, 256)):
        assert RE.rowdot_form(width, thr) == 1 and RE.rowdot_form(width, thr // 2) == 0 and RE.rowdot_form(width, 2 * thr) == 1
    assert [RE.rowdot_form(w, 256) for w in (64, 68, 128, 132, 192, 196, 256, 260)] == [1, 2, 2, 3, 3, 4, 4, 0]
    assert RE.rowdot_form(260, 1 << 20) == 0 and RE.rowdot_form(1024, 64) == 0


@pytest.mark.parametrize("pending", range(8))
def test_grind_reference_agrees_with_the_oracle_challenger(oracle, pending):
    _, state, slot = RE.grind_state(oracle, [100 + pending] * 8, pending)
    assert slot == pending
    for bits in (0, 1, 4, 8):
        w = RE.grind_reference(oracle, state, slot, bits, 0, 1 << 14)
        assert w != 0xFFFFFFFF and RE.is_witness(oracle, state, slot, bits, w)
        assert not any(RE.is_witness(oracle, state, slot, bits, v) for v in range(w))           # no smaller candidate passes
        assert RE.grind_state(oracle, [100 + pending] * 8, pending)[0].grind(bits) == w         # (grind moves its challenger on: a fresh one per search)
    assert RE.grind_reference(oracle, state, slot, 0, 5, 10) == 5                               # bits 0: the first candidate
    w4 = RE.grind_reference(oracle, state, slot, 4, 0, 1 << 14)
    assert RE.grind_reference(oracle, state, slot, 4, 0, 1 << 14, result=w4 + 1) == w4          # a larger prefill is lowered
    if w4:
        assert RE.grind_reference(oracle, state, slot, 4, 0, 1 << 14, result=w4 - 1) == w4 - 1  # a prefill below every hit is kept
    assert not RE.is_witness(oracle, state, slot, 0, P)                                         # candidates >= P are never witnesses


def test_the_late_witness_literal(oracle):
    """the committed state's smallest 10-bit witness lies past the first two 256-candidate windows"""
    ch, state, slot = RE.grind_state(oracle, RE.LATE_SEED, RE.LATE_PENDING)
    assert RE.LATE_WITNESS >= 512
    assert RE.grind_reference(oracle, state, slot, RE.LATE_BITS, 0, RE.LATE_WITNESS + 1) == RE.LATE_WITNESS
    assert ch.grind(RE.LATE_BITS) == RE.LATE_WITNESS
