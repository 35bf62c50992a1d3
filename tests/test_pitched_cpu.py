"""tests/pitched.py without a GPU: the layout embed() builds, that check_out() fires, and the case tables of test_gpu_pitched.py held
against the restated launcher predicates -- a case that silently stops reaching its form shows up here, in review."""
import numpy as np
import pytest

import pitched as PT
from oracle_lib import P, from_monty, to_monty


@pytest.mark.parametrize("rows,width,ld,lead,margin_rows", [(8, 5, 5, 0, 1), (8, 5, 7, 3, 1), (33, 16, 20, 1, 2), (4, 3, 3000, 2, 3), (1, 1 << 12, 1 << 12, 2, 1)])
def test_embed_layout_round_trip(rows, width, ld, lead, margin_rows):
    m = np.random.default_rng(rows).integers(0, P, size=(rows, width), dtype=np.uint32)
    image, off = PT.embed_image(m, ld, lead, margin_rows)
    mg = PT.margin_words(ld, margin_rows)
    assert mg % 4 == 0 and mg >= ld and mg >= margin_rows * ld and 4 * mg >= 4096
    assert off == mg + lead and off % 4 == lead % 4              # the view lies `lead % 4` words off 16-byte alignment
    assert image.size == 2 * mg + lead + rows * ld
    body = image[off:off + rows * ld].reshape(rows, ld)
    assert (from_monty(body[:, :width]) == m).all() and (body[:, :width] == to_monty(m)).all()
    assert (body[:, width:] == PT.POISON).all()                  # padding columns
    assert (image[:off] == PT.POISON).all()                      # margin and lead
    assert (image[off + rows * ld:] == PT.POISON).all() and image.size - (off + rows * ld) == mg
    # a row before the first and a row after the last are still inside the allocation
    assert off - ld >= 0 and off + (rows + 1) * ld <= image.size
    # an output image: nothing but the sentinel
    out, ooff = PT.embed_image(np.zeros((rows, 0), dtype=np.uint32), ld, lead, margin_rows, fill=PT.SENTINEL)
    assert ooff == off and out.size == image.size and (out == PT.SENTINEL).all()


def _good_output(rows=6, width=4, ld=7, lead=1):
    want = np.random.default_rng(3).integers(0, P, size=(rows, width), dtype=np.uint32)
    words, off = PT.embed_image(want, ld, lead, fill=PT.SENTINEL)
    return words, off, rows, width, ld, want


def test_check_out_accepts_the_expected_words():
    words, off, rows, width, ld, want = _good_output()
    PT.check_out(words, off, rows, width, ld, want)
    PT.check_out(*_good_output(5, 8, 8, 0))                      # dense rows


def test_check_out_fires_on_a_wrong_or_non_canonical_data_word():
    words, off, rows, width, ld, want = _good_output()
    w = words.copy()
    w[off + 2 * ld + 1] = to_monty([(int(want[2, 1]) + 1) % P])[0]
    with pytest.raises(AssertionError, match="data words differ, first at \\(row 2, column 1\\)"):
        PT.check_out(w, off, rows, width, ld, want)
    w = words.copy()
    w[off + 3 * ld] = P + 5                                      # a word no kernel may leave: download() would reduce it and hide it
    with pytest.raises(AssertionError, match="non-canonical"):
        PT.check_out(w, off, rows, width, ld, want)
    w = words.copy()
    w[off] = PT.SENTINEL                                         # a data word never written
    with pytest.raises(AssertionError, match="non-canonical"):
        PT.check_out(w, off, rows, width, ld, want)


def test_check_out_fires_on_a_touched_padding_word():
    words, off, rows, width, ld, want = _good_output()
    w = words.copy()
    w[off + 4 * ld + width] = 0                                  # the first padding word of row 4: a vector store across the row's end
    with pytest.raises(AssertionError, match="padding of row 4, column 4"):
        PT.check_out(w, off, rows, width, ld, want)
    w = words.copy()
    w[off + (rows - 1) * ld + ld - 1] = 5                        # the last padding word of the last row
    with pytest.raises(AssertionError, match="padding of row 5, column 6"):
        PT.check_out(w, off, rows, width, ld, want)


def test_check_out_fires_on_a_touched_lead_or_margin_word():
    words, off, rows, width, ld, want = _good_output()
    for idx, what in ((off - 1, "1 words before"), (0, "%d words before" % off), (off + rows * ld, "0 words after"), (words.size - 1, "words after")):
        w = words.copy()
        w[idx] = 1
        with pytest.raises(AssertionError, match=what):
            PT.check_out(w, off, rows, width, ld, want)


# ------------------------------------------------------------------ the case tables of test_gpu_pitched.py reach the forms they name
def _cases(table):
    return [p.values for p in table]


def test_gpu_cases_reach_the_forms_they_name():
    import test_gpu_pitched as G
    seen = set()

    def note(entry, form):
        seen.add((entry, form))

    for (c,) in _cases(G.DFT_CASES):
        args = (c.log_n, c.width, c.in_ld, c.out_ld, c.in_off, c.out_off)
        assert PT.dft_forms(*args, inverse=False) == c.fwd, c
        assert PT.dft_forms(*args, inverse=True) == c.inv, c
        for f in (c.fwd + "+" + c.inv).split("+"):
            note("dft", f)
    for ld, form in _cases(G.BIG_DFT_CASES):
        assert PT.combine_form(4, 4, ld, 0, 0) == form           # natural order: dense workspace -> the caller's rows
        assert PT.combine_form(4, ld, ld, 0, 0) == form          # bit-reversed order: in place on the caller's rows
        note("dft21", form)
    for (c,) in _cases(G.LDE_CASES):
        assert PT.lde_forms(c.log_n, c.width, c.in_ld, c.out_ld, c.in_off, 0) == c.form, c
        off = PT.lde_forms(c.log_n, c.width, c.in_ld, c.out_ld, c.in_off, 0, fusion=False)
        assert "fused" not in off and "lde_small" not in off     # the other run of every case: the tile passes alone
        note("lde", c.form)
    for (c,) in _cases(G.HASH_CASES):
        assert PT.hash_rows_form(c.height, G.hash_case_descs(c)) == c.form, c
        note("hash_rows", c.form)
    for (c,) in _cases(G.MERKLE_CASES):
        assert PT.merkle_commit_form(c.log_h, [(c.width, c.ld, 0)]) == c.form, c
        note("merkle_commit", c.form)
    lh0, w0, ld0 = G.MIXED_TALL
    assert PT.hash_rows_form(1 << lh0, [(w0, ld0, 0)]) == "vec"
    for ld, form in _cases(G.MIXED_CASES):
        assert PT.inject_form(1 << G.MIXED_SHORT[0], [(G.MIXED_SHORT[1], ld, 0)]) == form
        note("mixed", form)
    for (log_n, width), form in G.QUOTIENT_SHAPES.items():
        assert PT.quotient_form(log_n, width) == form
        note("quotient", form.split("<")[0])
    assert set(G.QUOTIENT_VARIANTS) == {"ld+4", "ld+1", "off1", "slice"} and G.SLICE_EXTRA == 8
    for (c,) in _cases(G.OPEN_CASES):
        assert PT.open_form(c.width, c.ld, c.off) == c.form, c
        note("open", c.form)
    assert PT.gen_trace_store(G.GEN_SHAPE[2], G.GEN_SHAPE[3]) == "store4" and PT.gen_trace_store(8, 0) == "store16"
    for off, form in _cases(G.COLMAJOR_CASES):
        assert PT.colmajor_form(G.COLMAJOR_LOG, off, off) == form
        note("colmajor", form)
    # both sides of every predicate of the issue's table occur
    for want in (("dft", "pair"), ("dft", "single"), ("dft", "small_eval"), ("dft21", "combine<4>"), ("dft21", "combine<1>"),
                 ("lde", "lde_small"), ("lde", "I1 pair, fused, F2 pair"), ("lde", "I1 single, fused, F2 pair"), ("lde", "I1 pair, I2, F1 single, F2 single"),
                 ("hash_rows", "hash_rows16"), ("hash_rows", "vec"), ("hash_rows", "mvec"), ("hash_rows", "generic"),
                 ("merkle_commit", "hash_sub16"), ("merkle_commit", "vec"), ("mixed", "compress_inject_mvec"), ("mixed", "level+generic+inject"),
                 ("quotient", "quotient_kernel"), ("quotient", "stream"), ("open", "quads"), ("open", "generic"),
                 ("colmajor", "native"), ("colmajor", "adapter")):
        assert want in seen, want


def test_the_restated_predicates_on_their_own_edges():
    """the sides the issue's table names, spelled out once each (so that a slip in the restatement is not hidden behind the case tables)"""
    assert PT.ntt_pass_form(32, 32, 32, 0, 0) == "pair" and PT.ntt_pass_form(30, 32, 32, 0, 0) == "single"
    assert PT.ntt_pass_form(32, 32, 32, 2, 2) == "pair" and PT.ntt_pass_form(32, 32, 32, 0, 3) == "single" and PT.ntt_pass_form(32, 34, 35, 0, 0) == "single"
    assert PT.combine_form(4, 4, 8, 0, 0) == "combine<4>" and PT.combine_form(4, 4, 8, 0, 2) == "combine<1>" and PT.combine_form(6, 8, 8, 0, 0) == "combine<1>"
    assert PT.lde_form(20, 64, 64, 96, 0, 0) == "I1 pair, fused, F2 pair" and "fused" not in PT.lde_form(20, 64, 64, 96, 0, 0, log_blowup=0)
    assert PT.lde_form(13, 128, 128, 128, 0, 0) == "lde_small" and PT.lde_form(14, 128, 128, 128, 0, 0) != "lde_small" and PT.lde_form(12, 96, 96, 96, 0, 0) != "lde_small"
    assert PT.hash_rows_form(16384, [(16, 16, 0)]) == "hash_rows16" and PT.hash_rows_form(16385, [(16, 16, 0)]) == "vec"
    assert PT.hash_rows_form(16385, [(16, 16, 0), (8, 8, 0)]) == "mvec" and PT.hash_rows_form(16385, [(16, 16, 0), (8, 8, 2)]) == "generic"
    assert PT.merkle_commit_form(9, [(8, 8, 0)]) == "hash_rows16" and PT.merkle_commit_form(10, [(8, 8, 0)]) == "hash_sub16" and PT.merkle_commit_form(14, [(8, 8, 0)]) == "hash_sub16"
    assert PT.inject_form(16384, [(4, 8, 0)]) == "level+hash_rows16+inject"
    assert PT.quotient_form(9, 32) == "quotient_kernel<1>" and PT.quotient_form(9, 64) == "quotient_kernel<1>" and PT.quotient_form(9, 68) == "quotient_kernel<2>" and PT.quotient_form(10, 32) == "stream" and PT.quotient_form(10, 36) == "quotient_kernel<1>"
    assert PT.quotient_form(12, 260) == "quotient_kernel<8>" and PT.quotient_form(9, 1024) == "quotient_kernel<16>" and PT.quotient_form(10, 1024) == "stream"
    assert PT.open_form(64, 64, 0) == "quads" and PT.open_form(60, 60, 0) == "generic" and PT.open_form(64, 64, 4) == "quads"
    assert PT.colmajor_form(19, 0, 0) == "adapter" and PT.colmajor_form(20, 2, 0) == "native" and PT.colmajor_form(20, 2, 1) == "adapter"
