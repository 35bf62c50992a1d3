"""The case tables of stream_rows.py against its mirrors of the dispatch, and the mirrors against the source's constants (no GPU)."""
import os
import re

import reduced_edges as RE
import stream_rows as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_source_constants_match_the_mirror():
    text = open(os.path.join(ROOT, "zktls_amd", "csrc", "stark.hip")).read()
    assert int(re.search(r"constexpr int SLICE_COLS = (\d+);", text).group(1)) == SR.SLICE_COLS
    assert int(re.search(r"constexpr uint64_t STREAM_MIN_ROWS = (\d+);", text).group(1)) == SR.STREAM_MIN_ROWS


def test_rowdot_case_literals():
    seen = set()
    for case, stream_t, stream_p in SR.ROWDOT_CASES:
        _, log_rows, width, _, p_width, _, _, form_t, form_p = case
        rows = 1 << log_rows
        assert RE.rowdot_form(width, rows) == form_t, case[0]
        assert (RE.rowdot_form(p_width, rows) if p_width else -1) == form_p, case[0]
        assert SR.rowdot_stream_form(width, rows) == stream_t, case[0]
        assert (SR.rowdot_stream_form(p_width, rows) if p_width else False) == stream_p, case[0]
        assert not stream_t or form_t in (1, 2, 3, 4)                      # the new form sits inside the register forms
        seen.add((stream_t, width // SR.SLICE_COLS if stream_t else 0))
    assert {(True, 1), (True, 3), (True, 8), (False, 0)} <= seen           # one slice, an odd count, the headline's eight, and the 16-lane forms
    assert any(s and (1 << c[1]) == SR.STREAM_MIN_ROWS for c, s, _ in SR.ROWDOT_CASES)
    assert any(not s and c[2] % SR.SLICE_COLS == 0 and (1 << c[1]) < SR.STREAM_MIN_ROWS for c, s, _ in SR.ROWDOT_CASES)
    assert any(not s and c[2] % SR.SLICE_COLS != 0 and (1 << c[1]) >= SR.STREAM_MIN_ROWS for c, s, _ in SR.ROWDOT_CASES)


def test_quotient_case_literals():
    assert all(SR.quotient_stream_form(ln, w) for ln, w in SR.QUOTIENT_CASES)
    assert not any(SR.quotient_stream_form(ln, w) for ln, w in SR.QUOTIENT_FALLBACK)
    assert min(2 << ln for ln, _ in SR.QUOTIENT_CASES) == SR.STREAM_MIN_ROWS
    assert SR.quotient_stream_form(20, 256) and SR.rowdot_stream_form(256, 2 << 20)      # the headline shard takes both
