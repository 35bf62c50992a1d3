"""Pitched rows, column slices and unaligned bases for the kernel entries of include/zkhip.h, shared by test_pitched_cpu.py and
test_gpu_pitched.py.

The entries take a row pitch (ld >= width) and a bare device pointer per matrix; below them nearly every launcher picks its kernel by
pitch and pointer alignment.  embed() builds the inputs that reach either side of those choices: ONE allocation

    [ margin | lead words | rows at pitch ld | margin ]

whose data words are to_monty(m) and whose every other word -- padding columns, lead, margins -- is POISON, a word that is no field
element.  A kernel that indexes padding as data, or steps with a stride that assumes ld == width, then computes a wrong result; one
that is off by a row still lands inside the allocation (margins: at least one pitch and at least 4 KiB).  Outputs with a pitch go
into buffers prefilled with SENTINEL (out_buffer) and check_out() requires the data words canonical and equal to the expectation and
every other word still the sentinel.

`off` everywhere: how many words the first data word lies off a 16-byte aligned address (device allocations are aligned far beyond
that, and the margin is a multiple of four words, so off = lead % 4).

The second half restates, in plain Python, the predicates by which the launchers choose (file:function named at each); the case
tables of test_gpu_pitched.py carry the form every case is meant to reach and test_pitched_cpu.py holds them to these functions.
"""
import numpy as np

from field_edges import assert_canonical_words
from oracle_lib import P, from_monty, to_monty

POISON = 0xFFFFFFFF                  # inputs: every word that is not data (no canonical element, no Montgomery word)
SENTINEL = 0xA5A5A5A5                # outputs: prefill (>= P, so a kernel cannot have written it as a field element)
assert POISON >= P and SENTINEL >= P


def margin_words(ld, margin_rows=1):
    """at least margin_rows pitches, at least one pitch, at least 4 KiB; a multiple of four words (keeps off = lead % 4)"""
    return (max(int(margin_rows) * ld, ld, 1024) + 3) & ~3


def embed_image(m, ld, lead=0, margin_rows=1, fill=POISON, raw=False):
    """the words of embed()'s allocation and the index of the first data word; raw: m holds device words already"""
    m = np.asarray(m, dtype=np.uint32)
    rows, width = m.shape
    assert ld >= width and lead >= 0
    mg = margin_words(ld, margin_rows)
    image = np.full(2 * mg + lead + rows * ld, fill, dtype=np.uint32)
    image[mg + lead:mg + lead + rows * ld].reshape(rows, ld)[:, :width] = m if raw else to_monty(m)
    return image, mg + lead


def embed(ctx, m, ld, lead=0, margin_rows=1):
    """m: the dense canonical matrix -> (buffer, view at the first data word); buffer.image = the uploaded words, buffer.view_off = the
    view's word offset (column c of the matrix as a slice: DeviceView(buffer, buffer.view_off + c), pitch ld)"""
    from zktls_amd.device import DeviceView
    image, off = embed_image(m, ld, lead, margin_rows)
    buf = ctx.from_raw(image)
    buf.image, buf.view_off = image, off
    return buf, DeviceView(buf, off)


def assert_unchanged(buf):
    """the input allocation word for word, poison included"""
    now = buf.download_monty()
    bad = np.flatnonzero(now != buf.image)
    assert bad.size == 0, "input changed at words %s (view at %d)" % (bad[:8].tolist(), buf.view_off)


def out_buffer(ctx, rows, ld, lead=0, margin_rows=1):
    """an output allocation of embed()'s layout, every word SENTINEL -> (buffer, view); buffer.view_off as above"""
    from zktls_amd.device import DeviceView
    image, off = embed_image(np.zeros((rows, 0), dtype=np.uint32), ld, lead, margin_rows, fill=SENTINEL)
    buf = ctx.from_raw(image)
    buf.view_off = off
    return buf, DeviceView(buf, off)


def check_out(buf, view_off, rows, width, ld, want):
    """buf: a device buffer (or its raw words as an array) prefilled with SENTINEL; the rows x width words from view_off on at pitch ld
    are canonical Montgomery words of `want` (canonical values), every other word of the buffer still holds the sentinel"""
    words = np.array(buf.download_monty() if hasattr(buf, "download_monty") else buf, dtype=np.uint32)
    want = np.asarray(want, dtype=np.uint32).reshape(rows, width)
    assert view_off + (rows - 1) * ld + width <= words.size
    span = words[view_off:view_off + rows * ld] if view_off + rows * ld <= words.size else None
    assert span is not None, "the last row's padding lies outside the buffer"
    data = span.reshape(rows, ld)[:, :width]
    assert_canonical_words(data)
    bad = np.argwhere(from_monty(data) != want)
    assert bad.size == 0, "%d data words differ, first at (row %d, column %d)" % (len(bad), bad[0][0], bad[0][1])
    rest = words.copy()
    rest[view_off:view_off + rows * ld].reshape(rows, ld)[:, :width] = SENTINEL
    touched = np.flatnonzero(rest != SENTINEL)
    if touched.size:
        i = int(touched[0])
        inside = view_off <= i < view_off + rows * ld
        where = "padding of row %d, column %d" % ((i - view_off) // ld, (i - view_off) % ld) if inside else \
                ("the lead / margin %d words before the data" % (view_off - i) if i < view_off else "the margin %d words after the last row" % (i - view_off - rows * ld))
        raise AssertionError("%d words outside the data were written, first in %s" % (touched.size, where))


# ---------------------------------------------------------------------------------------------- the launchers' predicates, restated
COOP_MAX_NODES = 16384               # kernels.h (coop_max_nodes() outside a lock-step batch): the 16-lane hash kernels' limit
COOP_TOP_NODES = 512                 # kernels.h: the levels one workgroup finishes
STREAM_MIN_ROWS = 2048               # stark.hip


def ntt_pass_form(ncols, in_ld, out_ld, in_off, out_off):
    """ntt.hip launch_ntt_pass `pair_ok`: two columns per lane (8-byte loads and stores) or one"""
    pair = ncols >= 32 and ncols % 2 == 0 and in_ld % 2 == 0 and out_ld % 2 == 0 and in_off % 2 == 0 and out_off % 2 == 0
    return "pair" if pair else "single"


def dft_forms(log_n, width, in_ld, out_ld, in_off, out_off, inverse):
    """context.cpp zkhip_dft -> run_forward_natural / run_inverse: the form of every tile pass ("+"-joined), or the small kernel.
    Two-pass sizes (log_n >= 11) go through a dense, aligned workspace: forward in -> tmp -> out; inverse in -> out, out -> tmp (then a 2-D copy)"""
    if log_n < 5:
        return "small_eval"
    if log_n <= 10:
        return ntt_pass_form(width, in_ld, out_ld, in_off, out_off)
    if log_n > 20:
        return "big"
    if inverse:
        return ntt_pass_form(width, in_ld, out_ld, in_off, out_off) + "+" + ntt_pass_form(width, out_ld, width, out_off, 0)
    return ntt_pass_form(width, in_ld, width, in_off, 0) + "+" + ntt_pass_form(width, width, out_ld, 0, out_off)


def combine_form(ncols, in_ld, out_ld, in_off, out_off):
    """ntt.hip launch_ntt_combine `vec`: four columns per lane (16-byte loads and stores) or one"""
    vec = ncols % 4 == 0 and in_ld % 4 == 0 and out_ld % 4 == 0 and in_off % 4 == 0 and out_off % 4 == 0
    return "combine<4>" if vec else "combine<1>"


def lde_form(log_n, width, in_ld, out_ld, in_off, out_off, fusion=True, log_blowup=1):
    """context.cpp op_coset_lde for 5 <= log_n <= 20 and width <= 32 or a multiple of 32 (other widths split into two such calls):
    lde_small (one launch, b32 accesses), or the tile passes I1 [I2 | fused middle] F1 F2 with the form of I1 (reads the caller's
    trace) and of F1 / F2 (write the caller's LDE); the coefficient workspace is dense and aligned"""
    if 11 <= log_n <= 13 and width >= 128 and fusion:
        return "lde_small"
    if log_n <= 10:
        return "single-pass:" + ntt_pass_form(width, in_ld, width, in_off, 0) + "," + ntt_pass_form(width, width, out_ld, 0, out_off)
    cosets = 1 << log_blowup
    fused = fusion and log_n == 20 and width % 32 == 0 and out_ld % 2 == 0 and cosets % 2 == 0      # context.cpp lde_fused_shape (coef_ld = width)
    i1 = ntt_pass_form(width, in_ld, width, in_off, 0)
    f2 = ntt_pass_form(width, out_ld, out_ld, out_off, out_off)
    if fused:
        return "I1 %s, fused, F2 %s" % (i1, f2)
    return "I1 %s, I2, F1 %s, F2 %s" % (i1, ntt_pass_form(width, width, out_ld, 0, out_off), f2)


def lde_forms(log_n, width, in_ld, out_ld, in_off, out_off, fusion=True, log_blowup=1):
    """op_coset_lde's split of a width above 32 that is no multiple of 32: the whole 32-column tiles, then the rest as a matrix of its
    own whose bases lie `w32` columns on"""
    if width > 32 and width % 32 and not (11 <= log_n <= 13 and width >= 128 and fusion):
        w32 = width & ~31
        return lde_form(log_n, w32, in_ld, out_ld, in_off, out_off, fusion, log_blowup) + " | " + \
               lde_form(log_n, width - w32, in_ld, out_ld, in_off + w32, out_off + w32, fusion, log_blowup)
    return lde_form(log_n, width, in_ld, out_ld, in_off, out_off, fusion, log_blowup)


def _mats_vec(mats):
    """hash.hip leaf_mats_vec; mats: (width, ld, off)"""
    return len(mats) >= 1 and all(w > 0 and w % 4 == 0 and ld % 4 == 0 and off % 4 == 0 for w, ld, off in mats)


def hash_rows_form(height, mats, bound=COOP_MAX_NODES):
    """hash.hip launch_hash_rows; bound: coop_max_nodes(), lower inside a lock-step batch (lockstep_forms.coop_bound)"""
    if height <= bound:
        return "hash_rows16"
    if len(mats) == 1 and mats[0][0] % 4 == 0 and mats[0][1] % 4 == 0 and mats[0][2] % 4 == 0:
        return "vec"
    return "mvec" if _mats_vec(mats) else "generic"


def merkle_commit_form(log_h, mats, bound=COOP_MAX_NODES):
    """context.cpp op_merkle_commit: medium trees hash their leaves inside the subtree launch"""
    count = 1 << log_h
    if COOP_TOP_NODES < count <= bound:
        return "hash_sub16"
    return hash_rows_form(count, mats, bound)


def inject_form(height, mats, bound=COOP_MAX_NODES):
    """hash.hip compress_inject_ok (context.cpp op_merkle_commit_mixed): one launch per injection level, or level + hash_rows + inject"""
    return "compress_inject_mvec" if height > bound and _mats_vec(mats) else "level+" + hash_rows_form(height, mats, bound) + "+inject"


def quotient_form(log_n, width):
    """stark.hip launch_quotient: neither form looks at pitch or alignment -- both read rows with 16-byte loads wherever they start"""
    if width % 32 == 0 and (2 << log_n) >= STREAM_MIN_ROWS:
        return "stream"
    G = width // 4
    lanes = 1
    while lanes < G and lanes < 16:
        lanes *= 2
    ng = (G + lanes - 1) // lanes
    return "quotient_kernel<%d>" % (ng if ng <= 4 else (8 if ng <= 8 else 16))


def open_form(width, ld, off):
    """stark.hip open_uses_quads"""
    return "quads" if width >= 64 and width % 4 == 0 and ld % 4 == 0 and off % 4 == 0 else "generic"


def gen_trace_store(ld, off):
    """util.hip gen_trace_kernel: one 16-byte store per column group, or four words"""
    return "store16" if ld % 4 == 0 and off % 4 == 0 else "store4"


def colmajor_form(log_size, in_off, out_off):
    """context.cpp zkhip_batch_interpolate_colmajor / zkhip_batch_expand_colmajor"""
    return "native" if log_size == 20 and in_off % 2 == 0 and out_off % 2 == 0 else "adapter"
