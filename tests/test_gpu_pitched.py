"""The kernel entries of include/zkhip.h on pitched rows, column slices of wider matrices and bases off 16-byte alignment, against the
oracle on the DENSE matrix (exact field arithmetic: equality, no tolerance).

The header states one pitch rule (ld >= width) and no alignment rule for these entries, and below them nearly every launcher picks
its kernel by pitch and alignment.  Every case: the reference once per shape on the dense matrix (module cache, shared by the pitch
variants), the entry on pitched.embed()ed inputs (data words in one allocation whose padding, lead and margins are poison), equality,
the input allocation unchanged word for word, and for outputs that have a pitch pitched.check_out() (canonical data words, every
other word of a sentinel-filled allocation untouched).  W = width, off = words the base lies off a 16-byte aligned address.

Which kernel each case is meant to reach -- pitched.py restates the launchers' predicates, test_pitched_cpu.py holds the `form`
column of every table below to them:

  entry / launcher            predicate side                                   kernel                       cases (ids)
  --------------------------  -----------------------------------------------  ---------------------------  ------------------------------
  dft: launch_ntt_pass        pair_ok: W >= 32, W / in_ld / out_ld even,       ntt_pass_kernel<4,.,2,BF>    2^12 x 32 ld 36/32, 32/36, off 2;
                              both bases 8-byte aligned                        (two columns per lane)       2^10 x 32 ld 36/36
                              otherwise                                        ntt_pass_kernel<4,.,1> /     ld 33, off 1 on either side,
                                                                               <3,.,1> (W <= 8)             40/40 off 3/1; 2^10 ld 33/35;
                                                                                                            2^5 x 8 ld 9 off 1
                              log_n < 5                                        small_eval_kernel            2^3 x 8 ld 11/9 off 1
  dft 2^21: ntt_combine       vec: W, in_ld, out_ld % 4, bases 16-byte aligned ntt_combine_kernel<1,4>      2^21 x 4 ld 8
                              otherwise                                        ntt_combine_kernel<1,1>      2^21 x 4 ld 6
  coset_lde: lde_small        2^11..2^13 rows, W >= 128 (32-bit accesses)      lde_small_kernel             2^11 x 128 in 132, 129, off 1,
                                                                                                            out 129
             tile passes      I1 / F1 / F2 by pair_ok as above                 ntt_pass_kernel pair/single  2^12 x 32, 2^12 x 40 (32 + 8)
             fused middle     2^20 rows, W % 32 == 0, out_ld even              lde_fused_kernel             2^20 x 32 in 36; in 33 off 1
                                                                                                            (I1 single); out 34
                              out_ld odd                                       I2 + F1 (single)             2^20 x 32 out 33
  hash_rows                   height <= 16384                                  hash_rows16_kernel           1024 x 40 ld 41, off 3, both 
                              vec: one matrix, W / ld % 4, base aligned        hash_rows_vec_kernel         2^15 x 16 ld 20; off 4;
                                                                                                            (16384 + 37) x 16 ld 20
                              every matrix so                                  hash_rows_mvec_kernel        slices [0:8] + [8:20] of ld 24
                              otherwise                                        hash_rows_generic_kernel     ld 18; off 1; slices [1:9] +
                                                                                                            [9:21]; widths 6 + 10; 2^15 x 5
  merkle_commit               512 < rows <= 16384                              hash_sub16_kernel            2^12 x 8 ld 9
                              above                                            hash_rows_vec_kernel + ..    2^15 x 16 ld 20
  merkle_commit_mixed         compress_inject_ok: rows > 16384, every matrix   compress_inject_mvec_kernel  2^16 x 8 ld 12 + 2^15 x 4 ld 8
                              vec; otherwise                                   compress_level + hash_rows   .. + 2^15 x 4 ld 6
                                                                               (generic) + inject
  merkle_commit_p24_colmajor  (none: word loads)                               hash_cols24_kernel           7 x 2^5, 24 x 2^12 off 1
  quotient_values             W % 32 == 0 and 2N >= 2048                       quotient_stream_kernel       2^10 x 32
                              otherwise                                        quotient_kernel<1>           2^10 x 16 (4 lanes a row), 2^9 x 32 (8)
                              (no side looks at pitch or base: 16-byte loads from rows that start anywhere -- ld W + 4, W + 1, off 1, slice)
  open_at                     open_uses_quads: W >= 64, W / ld % 4, aligned    open_partial4_kernel<2>      2^10 x 64 ld 68; 2^12 x 64 ld 68
                              otherwise                                        open_partial_kernel<2>       ld 66; off 1; 2^10 x 20 ld 21
  gen_trace                   ld % 4 and base aligned: 16-byte store, else 4   gen_trace_kernel             2^8 x 8 ld 9 off 1
  batch_*_colmajor            2^20 and both bases 8-byte aligned               ntt_colpass_kernel           off 2
                              otherwise                                        transpose + tile passes      off 1
  prove_shard, commit         the trace enters through coset_lde alone         (as above)                   ld W + 4, W + 1, off 1

quotient_values_air on pitched rows: tests/test_gpu_air_forms.py (its ld= / ptr_off= rows).
The kernels reached were read once from `rocprofv3 --kernel-trace --stats -- python -m pytest -m gpu tests/test_gpu_pitched.py`: every
kernel named above occurs, with the call counts the cases add up to (hash_rows_vec 6, generic 6, mvec 1, compress_inject_mvec 1 and
inject 1, ntt_combine<1,4> 2 and <1,1> 2, lde_fused 3, lde_small 4, quotient_stream 4, open_partial4<2> 2, ntt_colpass 12, transpose 4).
The file's 79 cases take about 7 s on an MI355X, the oracle included.
"""
import collections

import numpy as np
import pytest

import pitched as PT
from field_edges import assert_canonical, bitrev_perm
from zktls_amd._lib import Params
from zktls_amd.device import DeviceView

pytestmark = pytest.mark.gpu

P = 2013265921
SEED = 0x5A4B544C53

_CACHE = {}


def cached(key, make):
    """references are computed once per shape and shared by the pitch variants; nobody writes to them"""
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _free(*bufs):
    for b in bufs:
        b.free()


# ------------------------------------------------------------------ DFT
Dft = collections.namedtuple("Dft", "log_n width in_ld out_ld in_off out_off fwd inv")
DFT_CASES = [pytest.param(c, id="n%d-W%d-ld%d/%d-off%d/%d" % c[:6]) for c in (
    Dft(12, 32, 36, 32, 0, 0, "pair+pair", "pair+pair"),
    Dft(12, 32, 32, 36, 0, 0, "pair+pair", "pair+pair"),
    Dft(12, 32, 33, 32, 0, 0, "single+pair", "single+pair"),
    Dft(12, 32, 32, 33, 0, 0, "pair+single", "single+single"),
    Dft(12, 32, 32, 32, 2, 0, "pair+pair", "pair+pair"),          # still 8-byte aligned
    Dft(12, 32, 32, 32, 1, 0, "single+pair", "single+pair"),
    Dft(12, 32, 32, 32, 0, 1, "pair+single", "single+single"),
    Dft(12, 32, 40, 40, 3, 1, "single+single", "single+single"),
    Dft(10, 32, 36, 36, 0, 0, "pair", "pair"),
    Dft(10, 32, 33, 35, 1, 3, "single", "single"),
    Dft(5, 8, 9, 9, 1, 1, "single", "single"),
    Dft(3, 8, 11, 9, 1, 0, "small_eval", "small_eval"),
)]


def _dft_refs(oracle, log_n, width):
    def make():
        m = oracle.fill_uniform(SEED + 900 + log_n, log_n, width)
        return m, oracle.ntt(m), oracle.ntt(m, inverse=True)
    return cached(("dft", log_n, width), make)


@pytest.mark.parametrize("c", DFT_CASES)
def test_dft_on_pitched_rows(ctx, oracle, c):
    m, fwd, inv = _dft_refs(oracle, c.log_n, c.width)
    rows = 1 << c.log_n
    src, sv = PT.embed(ctx, m, c.in_ld, c.in_off)
    for inverse, bitrev, want in ((False, False, fwd), (False, True, fwd[bitrev_perm(c.log_n)]), (True, False, inv)):
        out, ov = PT.out_buffer(ctx, rows, c.out_ld, c.out_off)
        ctx.dft(sv, c.log_n, c.width, inverse=inverse, bitrev_out=bitrev, out=ov, in_ld=c.in_ld, out_ld=c.out_ld)
        PT.check_out(out, out.view_off, rows, c.width, c.out_ld, want)
        out.free()
    PT.assert_unchanged(src)
    src.free()


BIG_DFT_CASES = [pytest.param(8, "combine<4>", id="ld8"), pytest.param(6, "combine<1>", id="ld6")]


@pytest.mark.parametrize("ld,form", BIG_DFT_CASES)
def test_dft_2pow21_combine_pass_on_pitched_rows(ctx, oracle, ld, form):
    """2^21 rows: two 2^20-row class transforms (pitch 2 ld) and the radix-2 combine pass, which writes the caller's rows at pitch ld
    -- from the dense workspace (natural order) or in place (bit-reversed order)"""
    log_n, width = 21, 4
    m, fwd = cached(("dft21",), lambda: (lambda x: (x, oracle.ntt(x)))(oracle.fill_uniform(SEED + 921, log_n, width)))
    rows = 1 << log_n
    src, sv = PT.embed(ctx, m, ld)
    for bitrev in (False, True):
        out, ov = PT.out_buffer(ctx, rows, ld)
        ctx.dft(sv, log_n, width, bitrev_out=bitrev, out=ov, in_ld=ld, out_ld=ld)
        PT.check_out(out, out.view_off, rows, width, ld, fwd[bitrev_perm(log_n)] if bitrev else fwd)
        out.free()
    PT.assert_unchanged(src)
    src.free()


# ------------------------------------------------------------------ coset LDE (blowup 1; fusion on and off must agree)
Lde = collections.namedtuple("Lde", "log_n width in_ld out_ld in_off form")
_P32 = "I1 pair, I2, F1 pair, F2 pair"
_S8 = "I1 single, I2, F1 single, F2 single"
LDE_CASES = [pytest.param(c, id="n%d-W%d-in%d-out%d-off%d" % c[:5]) for c in (
    Lde(11, 128, 132, 128, 0, "lde_small"), Lde(11, 128, 129, 128, 0, "lde_small"), Lde(11, 128, 128, 128, 1, "lde_small"),
    Lde(11, 128, 128, 129, 0, "lde_small"),
    Lde(12, 32, 36, 32, 0, _P32), Lde(12, 32, 33, 32, 0, "I1 single, I2, F1 pair, F2 pair"),
    Lde(12, 32, 32, 32, 1, "I1 single, I2, F1 pair, F2 pair"), Lde(12, 32, 32, 32, 2, _P32),
    Lde(12, 32, 32, 33, 0, "I1 pair, I2, F1 single, F2 single"),
    Lde(12, 40, 44, 40, 0, _P32 + " | " + _S8), Lde(12, 40, 41, 40, 0, "I1 single, I2, F1 pair, F2 pair | " + _S8),
    Lde(20, 32, 36, 32, 0, "I1 pair, fused, F2 pair"), Lde(20, 32, 33, 32, 1, "I1 single, fused, F2 pair"),
    Lde(20, 32, 32, 34, 0, "I1 pair, fused, F2 pair"),                      # an even padded pitch keeps the fused launch
    Lde(20, 32, 32, 33, 0, "I1 pair, I2, F1 single, F2 single"),            # an odd one takes the four-pass sequence
)]


def _lde_refs(oracle, log_n, width):
    def make():
        m = oracle.fill_uniform(SEED + 700 + 7 * log_n + width, log_n, width)
        return m, oracle.coset_lde(m, 1, 31)
    return cached(("lde", log_n, width), make)


@pytest.mark.parametrize("c", LDE_CASES)
def test_coset_lde_on_pitched_rows(ctx, oracle, c):
    m, want = _lde_refs(oracle, c.log_n, c.width)
    rows = 2 << c.log_n
    src, sv = PT.embed(ctx, m, c.in_ld, c.in_off)
    try:
        for fused in (True, False):
            ctx.set_lde_fusion(fused)
            out, ov = PT.out_buffer(ctx, rows, c.out_ld)
            ctx.coset_lde(sv, c.log_n, c.width, 1, out=ov, in_ld=c.in_ld, out_ld=c.out_ld)
            PT.check_out(out, out.view_off, rows, c.width, c.out_ld, want)
            out.free()
    finally:
        ctx.set_lde_fusion(True)
    PT.assert_unchanged(src)
    src.free()


# ------------------------------------------------------------------ hashing
# a matrix: (width, ld, off) embedded on its own; ("slice", first column, width) = columns of the one 24-column buffer of the case
Hash = collections.namedtuple("Hash", "height mats form")
_TALL = 1 << 15
HASH_CASES = [pytest.param(c, id=i) for i, c in (
    ("2^15x16-ld20", Hash(_TALL, [(16, 20, 0)], "vec")),
    ("2^15x16-ld18", Hash(_TALL, [(16, 18, 0)], "generic")),
    ("2^15x16-off1", Hash(_TALL, [(16, 16, 1)], "generic")),
    ("2^15x16-off4", Hash(_TALL, [(16, 16, 4)], "vec")),               # four words on: 16-byte aligned again
    ("slices-0:8+8:20", Hash(_TALL, [("slice", 0, 8), ("slice", 8, 12)], "mvec")),
    ("slices-1:9+9:21", Hash(_TALL, [("slice", 1, 8), ("slice", 9, 12)], "generic")),
    ("slices-0:6+6:16", Hash(_TALL, [("slice", 0, 6), ("slice", 6, 10)], "generic")),
    ("2^15x5-ld7", Hash(_TALL, [(5, 7, 0)], "generic")),
    ("1024x40-ld41", Hash(1024, [(40, 41, 0)], "hash_rows16")),
    ("1024x40-off3", Hash(1024, [(40, 40, 3)], "hash_rows16")),
    ("1024x40-ld41-off3", Hash(1024, [(40, 41, 3)], "hash_rows16")),
    ("16421x16-ld20", Hash(16384 + 37, [(16, 20, 0)], "vec")),          # a tail workgroup on pitched rows
)]
SLICE_LD = 24


def hash_case_descs(c):
    """(width, ld, off) per matrix as the launcher sees them"""
    return [(m[2], SLICE_LD, m[1]) if m[0] == "slice" else m for m in c.mats]


def _hash_inputs(ctx, height, mats, seed):
    """-> (dense matrices, wrapper tuples (view, width, ld), the embedded buffers)"""
    rng = np.random.default_rng(seed)
    dense, args, bufs = [], [], []
    wide = None
    for m in mats:
        if m[0] == "slice":
            if wide is None:
                wide = rng.integers(0, P, size=(height, SLICE_LD), dtype=np.uint32)
                wbuf, _ = PT.embed(ctx, wide, SLICE_LD)
                bufs.append(wbuf)
            _, c0, w = m
            dense.append(np.ascontiguousarray(wide[:, c0:c0 + w]))
            args.append((DeviceView(wbuf, wbuf.view_off + c0), w, SLICE_LD))
        else:
            w, ld, off = m
            d = rng.integers(0, P, size=(height, w), dtype=np.uint32)
            b, v = PT.embed(ctx, d, ld, off)
            dense.append(d)
            args.append((v, w, ld))
            bufs.append(b)
    return dense, args, bufs


@pytest.mark.parametrize("c", HASH_CASES)
def test_hash_rows_on_pitched_rows_and_column_slices(ctx, oracle, c):
    dense, args, bufs = _hash_inputs(ctx, c.height, c.mats, c.height)
    d = ctx.hash_rows(args, c.height)
    got = d.download().reshape(-1, 8)
    assert (got == oracle.hash_rows(dense)).all()
    assert_canonical(d)
    for b in bufs:
        PT.assert_unchanged(b)
    _free(d, *bufs)


Commit = collections.namedtuple("Commit", "log_h width ld form")
MERKLE_CASES = [pytest.param(Commit(12, 8, 9, "hash_sub16"), id="2^12x8-ld9"), pytest.param(Commit(15, 16, 20, "vec"), id="2^15x16-ld20")]


@pytest.mark.parametrize("c", MERKLE_CASES)
def test_merkle_commit_on_pitched_rows(ctx, oracle, c):
    m = np.random.default_rng(c.log_h).integers(0, P, size=(1 << c.log_h, c.width), dtype=np.uint32)
    b, v = PT.embed(ctx, m, c.ld)
    t = ctx.merkle_commit([(v, c.width, c.ld)], c.log_h)
    assert (t.download().reshape(-1, 8) == oracle.merkle_tree([m])).all()
    PT.assert_unchanged(b)
    _free(t, b)


MIXED_CASES = [pytest.param(8, "compress_inject_mvec", id="inject-ld8"), pytest.param(6, "level+generic+inject", id="inject-ld6")]
MIXED_TALL = (16, 8, 12)                        # log height, width, pitch of the leaves' matrix (hash_rows_vec_kernel)
MIXED_SHORT = (15, 4)


@pytest.mark.parametrize("ld,form", MIXED_CASES)
def test_merkle_commit_mixed_injection_on_pitched_rows(ctx, oracle, ld, form):
    (lh0, w0, ld0), (lh1, w1) = MIXED_TALL, MIXED_SHORT
    mats, want = cached(("mixed",), lambda: (lambda ms: (ms, oracle.merkle_tree_mixed(list(ms))))(
        tuple(np.random.default_rng(60 + lh).integers(0, P, size=(1 << lh, w), dtype=np.uint32) for lh, w in ((lh0, w0), (lh1, w1)))))
    b0, v0 = PT.embed(ctx, mats[0], ld0)
    b1, v1 = PT.embed(ctx, mats[1], ld)
    t = ctx.merkle_commit_mixed([(v0, w0, lh0, ld0), (v1, w1, lh1, ld)])
    assert (t.download().reshape(-1, 8) == want).all()
    PT.assert_unchanged(b0)
    PT.assert_unchanged(b1)
    _free(t, b0, b1)


@pytest.mark.parametrize("cols,log_rows", [(7, 5), (24, 12)])
def test_merkle_commit_p24_colmajor_from_an_unaligned_base(ctx, oracle, cols, log_rows):
    mat = np.random.default_rng(cols).integers(0, P, size=(cols, 1 << log_rows), dtype=np.uint32)      # [cols][rows], dense
    b, v = PT.embed(ctx, mat, 1 << log_rows, lead=1)
    t = ctx.merkle_commit_p24_colmajor(v, cols, log_rows)
    assert (t.download().reshape(-1, 8) == oracle.merkle_tree_p24_colmajor(mat)).all()
    PT.assert_unchanged(b)
    _free(t, b)


# ------------------------------------------------------------------ quotient
QUOTIENT_SHAPES = {(10, 16): "quotient_kernel<1>", (9, 32): "quotient_kernel<1>", (10, 32): "stream"}
QUOTIENT_VARIANTS = ("ld+4", "ld+1", "off1", "slice")
SLICE_EXTRA, SLICE_COL = 8, 4                   # the LDE as columns [4, 4 + W) of a matrix 8 columns wider


def _quotient_refs(oracle, log_n, width):
    def make():
        lde = oracle.coset_lde(oracle.gen_trace(SEED, 2, log_n, width), 1, 31)
        alpha = np.random.default_rng(log_n + width).integers(0, P, 4, dtype=np.uint32)
        return lde, alpha, oracle.quotient_values(lde, log_n, alpha)
    return cached(("quotient", log_n, width), make)


@pytest.mark.parametrize("variant", QUOTIENT_VARIANTS)
@pytest.mark.parametrize("log_n,width", sorted(QUOTIENT_SHAPES))
def test_quotient_values_on_pitched_rows(ctx, oracle, log_n, width, variant):
    lde, alpha, want = _quotient_refs(oracle, log_n, width)
    if variant == "slice":
        wide = np.random.default_rng(5).integers(0, P, size=(lde.shape[0], width + SLICE_EXTRA), dtype=np.uint32)
        wide[:, SLICE_COL:SLICE_COL + width] = lde
        ld = width + SLICE_EXTRA
        b, _ = PT.embed(ctx, wide, ld)
        v = DeviceView(b, b.view_off + SLICE_COL)
    else:
        ld, lead = {"ld+4": (width + 4, 0), "ld+1": (width + 1, 0), "off1": (width, 1)}[variant]
        b, v = PT.embed(ctx, lde, ld, lead)
    out, ov = PT.out_buffer(ctx, lde.shape[0], 4)
    ctx.quotient_values(v, log_n, width, alpha, out=ov, ld=ld)
    PT.check_out(out, out.view_off, lde.shape[0], 4, 4, want)
    assert want.any()
    PT.assert_unchanged(b)
    _free(out, b)


# ------------------------------------------------------------------ openings
Open = collections.namedtuple("Open", "log_n width ld off form")
OPEN_CASES = [pytest.param(c, id="n%d-W%d-ld%d-off%d" % c[:4]) for c in (
    Open(10, 64, 68, 0, "quads"), Open(10, 64, 66, 0, "generic"), Open(10, 64, 64, 1, "generic"),
    Open(10, 20, 21, 0, "generic"),
    Open(12, 64, 68, 0, "quads"),                                           # four row chunks of the quads form
)]


def _open_refs(oracle, log_n, width):
    def make():
        lde = oracle.coset_lde(oracle.fill_uniform(SEED + 500 + log_n, log_n, width), 1, 31)
        z = np.random.default_rng(log_n + width).integers(0, P, (2, 4), dtype=np.uint32)
        return lde, z, np.stack([oracle.open_at(lde, log_n, z[0]), oracle.open_at(lde, log_n, z[1])])
    return cached(("open", log_n, width), make)


@pytest.mark.parametrize("c", OPEN_CASES)
def test_open_at_on_pitched_rows(ctx, oracle, c):
    lde, z, want = _open_refs(oracle, c.log_n, c.width)
    b, v = PT.embed(ctx, lde, c.ld, c.off)
    got = ctx.open_at(v, c.log_n, 1, c.width, z, ld=c.ld)
    assert (got == want).all()
    PT.assert_unchanged(b)
    b.free()


# ------------------------------------------------------------------ whole entries
PROVE_SHAPES = [(9, 12, 20, 10, 1), (6, 8, 10, 8, 3)]              # (log_n, W, queries, pow bits, public values) of test_gpu_stark.py
TRACE_VARIANTS = ("ld+4", "ld+1", "off1")


def _trace_layout(width, variant):
    return {"ld+4": (width + 4, 0), "ld+1": (width + 1, 0), "off1": (width, 1)}[variant]


@pytest.mark.parametrize("variant", TRACE_VARIANTS)
@pytest.mark.parametrize("log_n,width,q,pw,npub", PROVE_SHAPES)
def test_prove_shard_from_a_pitched_trace(ctx, oracle, log_n, width, q, pw, npub, variant):
    pub = [7, 8, 9][:npub]

    def make():
        t = oracle.gen_trace(SEED, 3, log_n, width)
        return t, oracle.prove_shard(t, pub, oracle.default_params(1, q, pw)).tobytes()
    trace, want = cached(("prove", log_n, width), make)
    ld, lead = _trace_layout(width, variant)
    b, v = PT.embed(ctx, trace, ld, lead)
    proof = ctx.prove_shard(v, log_n, width, pub, Params(1, q, pw), ld=ld)
    assert proof.tobytes() == want
    PT.assert_unchanged(b)
    b.free()


@pytest.mark.parametrize("ld", [20, 17])
@pytest.mark.parametrize("hw", [16, 24])
def test_commit_from_a_pitched_trace(ctx, oracle, hw, ld):
    log_n, width, log_blowup = 10, 16, 2

    def make():
        m = oracle.fill_uniform(SEED + 30, log_n, width)
        return m, oracle.coset_lde(m, log_blowup, 31)
    m, exp = cached(("commit",), make)
    otree = cached(("commit-tree", hw), lambda: oracle.merkle_tree_hw(exp, hw))
    b, v = PT.embed(ctx, m, ld)
    lde, tree, root = ctx.commit(v, log_n, width, log_blowup, hw, ld=ld)
    assert (lde.download().reshape(-1, width) == exp).all()
    assert_canonical(lde)
    assert (tree.download().reshape(-1, 8) == otree).all()
    assert root.tolist() == otree[-1].tolist()
    PT.assert_unchanged(b)
    _free(lde, tree, b)


GEN_SHAPE = (8, 8, 9, 1)                         # log_n, W, ld, off: gen_trace stores word by word (pitched.gen_trace_store)


@pytest.mark.parametrize("which", ["fill_uniform", "gen_trace", "gen_trace_logup"])
def test_generators_write_pitched_outputs(ctx, oracle, which):
    log_n, width, ld, off = GEN_SHAPE
    out, ov = PT.out_buffer(ctx, 1 << log_n, ld, off)
    if which == "fill_uniform":
        ctx.fill_uniform(SEED, log_n, width, out=ov, ld=ld)
        want = oracle.fill_uniform(SEED, log_n, width)
    elif which == "gen_trace":
        ctx.gen_trace(SEED, 3, log_n, width, out=ov, ld=ld)
        want = oracle.gen_trace(SEED, 3, log_n, width)
    else:
        ctx.gen_trace_logup(SEED, 3, log_n, width, 1, out=ov, ld=ld)
        want = oracle.gen_trace_logup(SEED, 3, log_n, width, 1)
    PT.check_out(out, out.view_off, 1 << log_n, width, ld, want)
    out.free()


# ------------------------------------------------------------------ column-major HAL
COLMAJOR_CASES = [pytest.param(2, "native", id="off2"), pytest.param(1, "adapter", id="off1")]
COLMAJOR_LOG = 20


def _colmajor_refs(ctx):
    """one polynomial of 2^20 on aligned buffers: (evaluations, coefficients, expansion at blowup 1), raw device words"""
    def make():
        n = 1 << COLMAJOR_LOG
        ev = np.random.default_rng(20).integers(0, P, n, dtype=np.uint32)
        d = ctx.from_raw(ev)
        c = ctx.batch_interpolate_colmajor(d, 1, COLMAJOR_LOG)
        e = ctx.batch_expand_colmajor(c, 1, COLMAJOR_LOG, 1, 31)
        r = (ev, c.download_monty(), e.download_monty())
        _free(d, c, e)
        return r
    return cached(("colmajor",), make)


@pytest.mark.parametrize("off,form", COLMAJOR_CASES)
def test_colmajor_transforms_from_unaligned_bases(ctx, off, form):
    """both bases `off` words on: 2 keeps the native column passes (8-byte accesses), 1 takes the transposing adapter; either way the
    result on aligned buffers (itself held to the oracle by test_gpu_parity.py)"""
    n = 1 << COLMAJOR_LOG
    ev, coef, exp = _colmajor_refs(ctx)
    src, sv = PT.embed(ctx, PT.from_monty(ev).reshape(1, n), n, off)
    out, ov = PT.out_buffer(ctx, 1, n, off)
    ctx.batch_interpolate_colmajor(sv, 1, COLMAJOR_LOG, out=ov)
    PT.check_out(out, out.view_off, 1, n, n, PT.from_monty(coef))
    PT.assert_unchanged(src)
    _free(src, out)
    src, sv = PT.embed(ctx, PT.from_monty(coef).reshape(1, n), n, off)
    out, ov = PT.out_buffer(ctx, 1, 2 * n, off)
    ctx.batch_expand_colmajor(sv, 1, COLMAJOR_LOG, 1, 31, out=ov)
    PT.check_out(out, out.view_off, 1, 2 * n, 2 * n, PT.from_monty(exp))
    PT.assert_unchanged(src)
    _free(src, out)
