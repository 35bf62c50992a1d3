"""Every live form of the constraint-program quotient kernel (csrc/stark.hip launch_quotient_air) at its boundaries, on edge Montgomery
words, against the oracle (oracle/air.c, pinned against Python integers on the same kind of input by test_air_forms_cpu.py).

Stage level (zkhip_quotient_values_air): a case is a free program with a chosen number of distinct monomials per factor count
(tests/air_forms.py class_program: edge-word coefficients, all selectors, next-row and repeated variables, merging records), an LDE
of edge words (field_edges.edge_matrix) and edge alphas.  Every case requires download() equal to the oracle, canonical raw output
words, the 64 words after the output untouched, and the input LDE unchanged word for word.  (The entry hands the kernel's chunks
through its gather and conversion kernels, which reduce: the canonical check sees THEIR words.  A non-canonical word of a quotient
kernel is seen by the whole proofs below, whose chunks go on into the transforms.)  Whole proofs in lock-step
(zkhip_prove_shards_air_multi) reach the batched twin of every form but the wide one, which the host refuses inside a batch.

Which kernel each shape reaches -- air_forms.form() restates the launcher, test_air_forms_cpu.py holds every id below to it.
M = distinct monomials rounded up to even, W = width, n = log_n; every public entry refuses n < 5 and widths that are no multiple of
four (proof_common.h check_shape), so the launcher's branches for n <= 4 -- the interpreter at n <= 2, terms<64> (n = 3 only) and a
chain of two groups (n = 4) -- and for W % 4 != 0 are not live: test_shapes_below_the_entries_limits_are_refused.

  kernel                       chosen when (first match)                       shapes in this file (n 5, M 100 unless said)
  ---------------------------  ----------------------------------------------  -----------------------------------------------------
  quotient_air_wide_kernel<16> M >= 2048, W <= 624, n >= 6, 16-byte aligned    W 48 M 2048 (n 6, n 8, four chunks, 300 public values);
                               rows, not in a lock-step batch                  W 248 / 252 (64 KiB of tile), W 624; saturated
  quotient_air_kernel          rows not 16-byte aligned, or M <= 512 and       W 8 (two and four chunks); W 16 M 512; W 64 ld 66 M 600;
  (row-per-lane interpreter)   W <= 16                                         W 64 pointer + 4 bytes; W 48 M 2048 pointer + 4 bytes;
                                                                               saturated
  quotient_air_chain_kernel    M <= 512: <64,4> W <= 128, <64,8> W <= 256,     the two ends of every range: 20 128 | 132 256 | 260 384
    <64,4> <64,8> <64,12>      <64,12> W <= 384, <128,8> W <= 512,             | 388 512 | 516 768 | 772 1024; W 132 at n 6 7 8 9
    <128,8> <128,12> <128,16>  <128,12> W <= 768, <128,16> W <= 1024           (chains of 8, 16, 32, two chains a coset); W 20 388
                                                                               1024 with four chunks at n 6; W 20 M 512; W 132 with
                                                                               one public value; saturated W 64
  quotient_air_terms_kernel    512 < M <= 8192 (and not wide)                  M 514 at W 16 and W 20; M 2046 W 48 n 7; M 2048 W 48
    <128>                                                                      (two and four chunks); M 2048 and 8192 at W 628 n 6;
                                                                               64 public values; saturated W 48 M 600
  quotient_air_terms_kernel    M > 8192 (and not wide)                         M 8194 W 628 n 6; M 9000 W 48; M 8200 W 1024 four
    <256>                                                                      chunks; M 9000 W 48 four chunks with 65 public values
  ..._batch twins              the same inside a lock-step batch               whole proofs: W 8, 64, 132, 388, 48 (M 2118: terms<128>
                                                                               in the batch, wide<16> outside), 1024

Pitched rows: chain<64,4>, chain<128,8>, terms<128>, terms<256> and wide<16> each once with ld = W + 4 (the form stays) and once with
ld = W + 2 (rows off 16-byte boundaries: the same program must reach the interpreter).

A reviewer can confirm one row with `rocprofv3 --kernel-trace --stats -- python -m pytest -m gpu <file>::<test>[<id>]` on a stage-level
case (whole-proof cases are not run under the profiler: profiles/r04_segv.md).
"""
import collections
import ctypes as C

import numpy as np
import pytest

import air_forms as AF
from field_edges import P, assert_canonical_words, edge_canonical, edge_ext, edge_matrix
from zktls_amd._lib import Params, ZkHipError, check, from_monty, to_monty, u32p

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF                                   # no field element: an output word that still holds it was not written
TAIL = 64

Case = collections.namedtuple("Case", "form width log_n counts lqd n_public ld ptr_off M pairs seed saturated")


def _case(form, width, log_n, counts=None, M=100, lqd=1, n_public=0, ld=None, ptr_off=0, pairs=None, saturated=None, tag=""):
    if counts is None and saturated is None:
        counts = AF.counts_for(M, lqd)
    if counts is not None:
        M = sum(counts) + sum(counts) % 2
    else:
        M = sum(saturated) + sum(saturated) % 2
    name = "%s:W%d-n%d-M%d" % (form, width, log_n, M) + ("-lqd2" if lqd == 2 else "") + ("-pub%d" % n_public if n_public else "") + \
           ("-ld%d" % ld if ld else "") + ("-off%d" % ptr_off if ptr_off else "") + ("-saturated" if saturated else "") + tag
    seed = 7 * width + 31 * log_n + M + n_public
    return pytest.param(Case(form, width, log_n, counts, lqd, n_public, ld or width, ptr_off, M, pairs, seed, saturated), id=name)


# The wide form's class-count vectors (counts of distinct monomials with 1 .. 5 factors) and the record pairs p_n they give; a class
# of p pairs is dealt in runs of per = 4 ceil(p / 64) pairs to wavefronts 0, 1, ..; a wavefront walks its run in trips of 4, 2 and 1:
#   A [1, 13, 2034]            p = 1 (one record, padded), 7 (13 records, padded: 4 | 2 + 1), 1017 (per 64; the last run 57 = 14 x 4 + 1)
#   B [4, 128, 1916]           p = 2 (one trip of 2), 64 (one trip of 4 on every wavefront), 958 (per 60; the last run 58 = 14 x 4 + 2)
#   C [0, 6, 130, 1000, 912]   p = 0 (empty), 3 (2 + 1), 65 (per 8: eight full runs, then 1, then idle wavefronts), 500, 456 (per 32:
#                              the fifteenth run 8, the sixteenth wavefront idle)
WIDE_A, PAIRS_A = [1, 13, 2034, 0, 0], [1, 7, 1017, 0, 0]
WIDE_B, PAIRS_B = [4, 128, 1916, 0, 0], [2, 64, 958, 0, 0]
WIDE_C, PAIRS_C = [0, 6, 130, 1000, 912], [0, 3, 65, 500, 456]

STAGE_CASES = [
    # ---- the row-per-lane interpreter
    _case("interpreter", 8, 5), _case("interpreter", 8, 5, lqd=2),
    _case("interpreter", 16, 5, M=512),                                      # the `small` edge; its neighbour M 514 is below
    _case("interpreter", 64, 6, M=600, ld=66),                               # rows that start off 16-byte boundaries
    _case("interpreter", 64, 5, ptr_off=1),                                  # the LDE pointer one word on
    _case("interpreter", 48, 6, counts=WIDE_A, ptr_off=1),                   # the host's own wide predicate refuses the pointer
    _case("interpreter", 16, 5, saturated=(32, 168)),
    # ---- the chained form: both ends of every (lanes, prefetch loads) range; W 20, 260, 772 have W / 4 no power of two (at W 20
    # lanes 40 .. 63 hold repeat slots)
    _case("chain<64,4>", 20, 5), _case("chain<64,4>", 128, 5),
    _case("chain<64,8>", 132, 5), _case("chain<64,8>", 256, 5),
    _case("chain<64,12>", 260, 5), _case("chain<64,12>", 384, 5),
    _case("chain<128,8>", 388, 5), _case("chain<128,8>", 512, 5),
    _case("chain<128,12>", 516, 5), _case("chain<128,12>", 768, 5),
    _case("chain<128,16>", 772, 5), _case("chain<128,16>", 1024, 5),
    _case("chain<64,8>", 132, 6), _case("chain<64,8>", 132, 7), _case("chain<64,8>", 132, 8), _case("chain<64,8>", 132, 9),
    _case("chain<64,4>", 20, 6, lqd=2), _case("chain<128,8>", 388, 6, lqd=2), _case("chain<128,16>", 1024, 6, lqd=2),
    _case("chain<64,4>", 20, 5, M=512),
    _case("chain<64,8>", 132, 5, n_public=1),
    _case("chain<64,4>", 64, 5, saturated=(60, 140)),
    # ---- one group per workgroup, two wavefronts
    _case("terms<128>", 16, 5, M=514), _case("terms<128>", 20, 5, M=514),
    _case("terms<128>", 48, 7, M=2046),
    _case("terms<128>", 48, 5, M=2048), _case("terms<128>", 48, 5, M=2048, lqd=2),
    _case("terms<128>", 628, 6, M=2048), _case("terms<128>", 628, 6, M=8192),
    _case("terms<128>", 48, 5, M=2048, n_public=64),
    _case("terms<128>", 48, 5, saturated=(96, 504)),
    # ---- four wavefronts
    _case("terms<256>", 628, 6, M=8194),
    _case("terms<256>", 48, 5, M=9000),
    _case("terms<256>", 1024, 5, M=8200, lqd=2),
    _case("terms<256>", 48, 5, M=9000, lqd=2, n_public=65),                 # (degree 5: a term of five public values and nothing else)
    # ---- the wide form.  W 252 is the first tile above 64 KiB (65 (W + 4) 4 bytes): it raises the dynamic-LDS limit and runs before W 624
    _case("wide<16>", 48, 6, counts=WIDE_A, pairs=PAIRS_A),                  # the lowest shape that takes it
    _case("wide<16>", 248, 6, M=2048), _case("wide<16>", 252, 6, M=2048),
    _case("wide<16>", 624, 6, M=2048),
    _case("wide<16>", 48, 8, counts=WIDE_A, pairs=PAIRS_A),                  # four tiles a coset: the last tile's 65th row wraps
    _case("wide<16>", 48, 6, counts=WIDE_C, lqd=2, pairs=PAIRS_C),
    _case("wide<16>", 48, 6, counts=WIDE_B, n_public=300, pairs=PAIRS_B),
    _case("wide<16>", 48, 6, saturated=(96, 1952)),
    # ---- pitched rows under every term-parallel form and the wide form: ld = W + 4 keeps 16-byte aligned rows and the form (the
    # padding holds the sentinel: a row step of W, or a read past the row's end, changes the result); ld = W + 2 must fall back to the
    # interpreter (stark.hip launch_quotient_air `fits`, prover.cpp run_quotient_air `wide`)
    _case("chain<64,4>", 20, 5, ld=24), _case("interpreter", 20, 5, ld=22),
    _case("chain<128,8>", 388, 5, ld=392), _case("interpreter", 388, 5, ld=390),
    _case("terms<128>", 48, 5, M=2048, ld=52), _case("interpreter", 48, 5, M=2048, ld=50),
    _case("terms<256>", 48, 5, M=9000, ld=52), _case("interpreter", 48, 5, M=9000, ld=50),
    _case("wide<16>", 48, 6, counts=WIDE_A, ld=52), _case("interpreter", 48, 6, counts=WIDE_A, ld=50),
]


def build_program(case):
    if case.saturated:
        return AF.saturated_program(case.width, *case.saturated), []
    return AF.class_program(case.width, case.counts, case.seed, case.n_public, max_degree=3 if case.lqd == 1 else 5)


def _quotient_words(ctx, prog, lde_ptr, ld, log_n, width, pub, alpha, lqd):
    """zkhip_quotient_values_air into a buffer 64 words longer than the output, pre-filled: the raw words of the whole buffer"""
    nout = 4 << (log_n + lqd)
    out = ctx.alloc(nout + TAIL)
    out.upload_monty(np.full(nout + TAIL, SENTINEL, dtype=np.uint32))
    prog = np.ascontiguousarray(prog, dtype=np.uint32)
    pv = np.ascontiguousarray(np.array(pub, dtype=np.uint32))
    a = to_monty(np.asarray(alpha, dtype=np.uint32))
    check(ctx.lib.zkhip_quotient_values_air(ctx.handle, prog.ctypes.data_as(u32p), prog.size, C.c_void_p(lde_ptr), ld, log_n, width,
                                            pv.ctypes.data_as(u32p), pv.size, a.ctypes.data_as(u32p), C.c_void_p(out.ptr)))
    words = out.download_monty()
    out.free()
    return words[:nout].reshape(-1, 4), words[nout:]


@pytest.mark.parametrize("case", STAGE_CASES)
def test_quotient_form_on_edge_words(ctx, oracle, case):
    prog, pub = build_program(case)
    lqd, W = case.lqd, case.width
    rows = 1 << (case.log_n + lqd)
    if case.saturated:
        lde = np.full((rows, W), edge_canonical([P - 1])[0], dtype=np.uint32)
    else:
        lde = edge_matrix(rows, W, seed=case.seed)
    # the device image: `ptr_off` words, then rows of `ld` words whose padding holds the sentinel
    image = np.full(case.ptr_off + rows * case.ld, SENTINEL, dtype=np.uint32)
    image[case.ptr_off:].reshape(rows, case.ld)[:, :W] = to_monty(lde)
    d = ctx.from_raw(image)
    for alpha in edge_ext(np.random.default_rng(case.seed), 1):              # the fixed edge elements ([1, 0, 0, 0] among them) and one draw
        got, tail = _quotient_words(ctx, prog, d.ptr + 4 * case.ptr_off, case.ld, case.log_n, W, pub, alpha, lqd)
        exp = oracle.quotient_values_air(prog, lde, case.log_n, pub, alpha)
        bad = np.flatnonzero((from_monty(got) != exp).any(axis=1))
        assert bad.size == 0, "alpha %s: %d rows differ, first %d: got %s, oracle %s" % (alpha.tolist(), bad.size, bad[0], from_monty(got)[bad[0]].tolist(), exp[bad[0]].tolist())
        assert_canonical_words(got)
        assert (tail == SENTINEL).all()
        assert exp.any()                                                    # (a quotient of zeros would compare nothing)
    assert (d.download_monty() == image).all()                              # input preserved, word for word
    d.free()


def test_shapes_below_the_entries_limits_are_refused(ctx):
    """the launcher has branches for traces of fewer than 32 rows and for widths that are no multiple of four; no entry lets them
    through, so terms<64> (log_n 3), a chain of two groups (log_n 4) and the interpreter's log_n <= 2 / W % 4 branches carry no case"""
    from zktls_amd.device import air_synthetic
    for width, log_n in ((64, 2), (132, 3), (1024, 3), (132, 4), (20, 4)):
        assert not AF.enterable(width, log_n)
        prog, pub = AF.class_program(width, AF.counts_for(100), seed=1)
        lde = ctx.alloc(width << (log_n + 1))
        with pytest.raises(ZkHipError):
            ctx.quotient_values_air(prog, lde, log_n, width, pub, [1, 2, 3, 4])
        with pytest.raises(ZkHipError):
            ctx.prove_shard_air(air_synthetic(width, 0), lde, log_n, width, [], Params(1, 6, 4))
        lde.free()
    assert not AF.enterable(6, 6)
    prog, pub = AF.class_program(6, [4, 8, 12], seed=1)
    lde = ctx.alloc(6 << 7)
    with pytest.raises(ZkHipError):
        ctx.quotient_values_air(prog, lde, 6, 6, pub, [1, 2, 3, 4])
    lde.free()


# ------------------------------------------------------------------ the batched twins: whole proofs in lock-step
Twin = collections.namedtuple("Twin", "form log_n base derived terms_per seed wide_outside")
TWIN_CASES = [pytest.param(t, id=t.form) for t in (
    Twin("interpreter", 5, 4, 4, 3, 1, False),                              # W 8
    Twin("chain<64,4>", 6, 16, 48, 2, 2, False),                            # W 64
    Twin("chain<64,8>", 5, 20, 112, 2, 3, False),                           # W 132
    Twin("chain<128,8>", 5, 260, 128, 2, 4, False),                         # W 388
    Twin("terms<128>", 6, 16, 32, 65, 5, True),                             # W 48, M 2118: wide<16> outside a batch
    Twin("terms<256>", 5, 112, 912, 8, 6, False),                           # W 1024, M 8214
)]


@pytest.fixture()
def lockstep():
    from zktls_amd.device import set_lockstep
    yield set_lockstep
    set_lockstep(16, 6)                                       # the library's defaults


@pytest.mark.parametrize("tw", TWIN_CASES)
def test_lockstep_twin_proves_the_same_bytes(ctx, oracle, lockstep, tw):
    """four traces of one program in which every record has a non-zero weight (air_forms.derived_program_and_trace), proven one
    context per worker and in one lock-step batch of four: the same bytes, the first job's equal to the oracle's, launches merged.
    The M 2118 program runs terms<128> in the batch and wide<16> through the single-shard entry: the same bytes again."""
    from zktls_amd.device import lockstep_stats, prove_shards_air_multi
    width = tw.base + tw.derived
    made = [AF.derived_program_and_trace(tw.log_n, tw.base, tw.derived, tw.terms_per, tw.seed, trace_seed=100 * tw.seed + j) for j in range(4)]
    prog = made[0][0]
    assert AF.form(width, AF.monomial_count(prog), tw.log_n, lockstep=True) == tw.form
    traces = [ctx.from_numpy(t) for _, t, _ in made]
    pubs = [pub for _, _, pub in made]
    prm, oprm = Params(1, 6, 4), oracle.default_params(1, 6, 4)
    lockstep(0)
    ref = prove_shards_air_multi(prog, traces, tw.log_n, width, pubs, prm, devices=[0])
    lockstep(4, 2)
    s0 = lockstep_stats()
    got = prove_shards_air_multi(prog, traces, tw.log_n, width, pubs, prm, devices=[0])
    s1 = lockstep_stats()
    assert all(a.size > 0 and a.tobytes() == b.tobytes() for a, b in zip(ref, got))
    assert 0 < s1[0] - s0[0] < s1[1] - s0[1], (s0, s1)         # something merged
    assert got[0].tobytes() == oracle.prove_shard_air(prog, made[0][1], pubs[0], oprm).tobytes()
    if tw.wide_outside:
        assert AF.form(width, AF.monomial_count(prog), tw.log_n) == "wide<16>"
        assert ctx.prove_shard_air(prog, traces[1], tw.log_n, width, pubs[1], prm).tobytes() == got[1].tobytes()
    for t in traces:
        t.free()
