"""The fold-by-16 ROW-PATHS machine on the GPU (zktls_amd/csrc/fri16_chip.hip, p24chip_row_paths_kernel in hash.hip): the device's P24R table against the Python
restatement (tests/fri16_rowpaths_air.py) word for word from raw rows, random siblings and given indices -- at the widths on both sides of the partial-block cases
and on edge words --, the device key against the host key and the oracle's setup, proof bytes against the oracle's generic keyed-machine prover on the
restatement's arrays, what the prover refuses before proving, and one full-size measurement beside the openings machine."""
import time

import numpy as np
import pytest

import fri16_openings_air as OA
import fri16_rowpaths_air as RPA
from field_edges import edge_canonical
from test_fri16_chip_cpu import GOLDEN, load, shape_of
from test_gpu_fri16_chip import SEED
from test_gpu_fri16_transcript import gpu_segment_view
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import (fri16_openings_key_host, fri16_rowpaths_key_host, fri16_view_openings, fri16_view_row_paths, fri16_view_shard, fri16_view_transcript,
                              verify_fri16_openings, verify_fri16_rowpaths)

pytestmark = pytest.mark.gpu
P = 2013265921
RAW = (2, 0, 1)                                               # R, F, log_blowup of the raw-row tests: H = 9
WIDTHS = [8, 16, 24, 40, 128]                                 # a lone half block, a lone full block, full + half, two full + half, eight full
QUERIES = [1, 3, 33]                                          # 33: 66 paths and the padding waves behind them in one grid


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


def compare_with_the_restatement(ctx, Q, W, trows, qrows, indices, tpaths, qpaths):
    """the whole table and every path's END (no root is involved: the siblings are arbitrary)"""
    R, F, b = RAW
    H = 4 * R + F + b
    trace, ends = RPA.row_path_traces(R, H, W, trows, qrows, indices, tpaths, qpaths)
    g_trace, g_ends = ctx.fri16_rowpaths_gen_trace(R, F, b, Q, 0, W, trows, qrows, indices, tpaths, qpaths)
    assert g_trace.shape == trace.shape == (1 << RPA.log_rows(R, F, b, Q, W)[RPA.P24R], 552)
    assert (g_trace == trace).all(), np.argwhere(g_trace != trace)[:8]
    assert g_ends.tolist() == ends


# ------------------------------------------------------------------ (1) the device's P24R = the restatement's
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("Q", QUERIES)
def test_gen_trace_equals_the_python_restatement(ctx, Q, W):
    H = 4 * RAW[0] + RAW[1] + RAW[2]
    rng = np.random.default_rng([23, Q, W])
    rnd = lambda n: [int(x) for x in rng.integers(0, P, n)]
    trows, qrows = [rnd(W) for _ in range(Q)], [rnd(8) for _ in range(Q)]
    tpaths, qpaths = [[rnd(8) for _ in range(H)] for _ in range(Q)], [[rnd(8) for _ in range(H)] for _ in range(Q)]
    indices = [int(x) for x in rng.integers(0, 1 << H, Q)]
    if Q > 2:
        indices[2] = indices[0]                               # two queries at one index: a path each
    compare_with_the_restatement(ctx, Q, W, trows, qrows, indices, tpaths, qpaths)


@pytest.mark.parametrize("Q,W", [(3, 24), (4, 8), (2, 40)])
def test_gen_trace_on_edge_words_and_the_all_left_and_all_right_paths(ctx, Q, W):
    """rows and siblings drawn from the words 0, 1, P - 1, (P - 1) / 2, (P + 1) / 2 -- as canonical values and as the canonical values whose Montgomery words
    they are --, indices 0 and 2^H - 1 among them"""
    H = 4 * RAW[0] + RAW[1] + RAW[2]
    words = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]
    pool = words + [int(x) for x in edge_canonical(words)]
    rng = np.random.default_rng([29, Q, W])
    rnd = lambda n: [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    trows, qrows = [rnd(W) for _ in range(Q)], [rnd(8) for _ in range(Q)]
    tpaths, qpaths = [[rnd(8) for _ in range(H)] for _ in range(Q)], [[rnd(8) for _ in range(H)] for _ in range(Q)]
    trows[0], qrows[0], tpaths[0] = [P - 1] * W, [0] * 8, [[0] * 8 for _ in range(H)]
    trows[1], qrows[1], qpaths[1] = [0] * W, [P - 1] * 8, [[P - 1] * 8 for _ in range(H)]
    indices = [0, (1 << H) - 1, 1, 1 << (H - 1)][:Q]
    compare_with_the_restatement(ctx, Q, W, trows, qrows, indices, tpaths, qpaths)


def test_gen_trace_refuses_bad_arguments(ctx):
    R, F, b = RAW
    H, Q, W = 4 * R + F + b, 3, 16
    rng = np.random.default_rng(31)
    rnd = lambda n: [int(x) for x in rng.integers(0, P, n)]
    trows, qrows, indices = [rnd(W) for _ in range(Q)], [rnd(8) for _ in range(Q)], [5, 77, 300]
    tpaths, qpaths = [[rnd(8) for _ in range(H)] for _ in range(Q)], [[rnd(8) for _ in range(H)] for _ in range(Q)]
    with pytest.raises(ZkHipError, match="canonical"):
        ctx.fri16_rowpaths_gen_trace(R, F, b, Q, 0, W, [[P] + trows[0][1:]] + trows[1:], qrows, indices, tpaths, qpaths)
    bad = [[list(d) for d in p] for p in qpaths]
    bad[2][4][1] = P
    with pytest.raises(ZkHipError, match="query 2, quotient tree: path words must be canonical"):
        ctx.fri16_rowpaths_gen_trace(R, F, b, Q, 0, W, trows, qrows, indices, tpaths, bad)
    with pytest.raises(ZkHipError, match="more bits"):
        ctx.fri16_rowpaths_gen_trace(R, F, b, Q, 0, W, trows, qrows, [1 << H, 0, 1], tpaths, qpaths)


# ------------------------------------------------------------------ (2) device key = host key = oracle setup; proof bytes = the oracle's
def prove_and_compare(ctx, O, v, outer):
    R, F, b, Q = shape(v)
    pb, W = v["pow_bits"], v["W"]
    main, pre, progs, tabs, pub = RPA.machine(v)
    lns, ws, pws = shape_of(main, pre)
    prm, oprm = Params(*outer), O.default_params(*outer)
    key = ctx.fri16_rowpaths_key(v, prm)
    try:
        assert key.root.tolist() == fri16_rowpaths_key_host(v, prm).tolist() == O.machine_setup(pre, lns, oprm).tolist()
        proof = ctx.prove_fri16_rowpaths(key, v, prm)
        assert proof.tobytes() == O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm).tobytes()
        assert verify_fri16_rowpaths(proof, pub, R, F, b, Q, pb, W, key.root, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tabs, pub, oprm) == 0
        bad = list(pub)
        bad[21] = (bad[21] + 1) % P
        assert verify_fri16_rowpaths(proof, bad, R, F, b, Q, pb, W, key.root, prm)[0] != 0
    finally:
        key.close()
    return proof


@pytest.mark.parametrize("outer", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_the_golden_view_equal_the_oracles(ctx, oracle, outer):
    prove_and_compare(ctx, oracle, RPA.golden_view("v3_r0_9x8", GOLDEN, load), outer)


def test_proof_bytes_of_a_synthetic_view_equal_the_oracles(ctx, oracle):
    """W = 40: two full blocks and a half one"""
    prove_and_compare(ctx, oracle, RPA.honest_view(2, 0, 1, 3, 40), (1, 10, 2))


def test_proof_bytes_of_a_gpu_segment_proofs_view(ctx, oracle):
    """2^10 x 16, 12 queries, R = 2, four final coefficients, made on the GPU"""
    log_n, width, sp, public = 10, 16, segment_params(12, 0, 2), [7]
    v = gpu_segment_view(ctx, oracle, log_n, width, sp, public)
    t = oracle.gen_trace(SEED, 3, log_n, width)
    cols = ctx.from_numpy(np.ascontiguousarray(t.T))
    proof = ctx.prove_segment(cols, log_n, width, public, sp)
    cols.free()
    v = dict(v, **fri16_view_openings(proof, log_n, width, public, sp), **fri16_view_row_paths(proof, log_n, width, public, sp))
    assert shape(v) == (2, 2, 2, 12) and v["hash_width"] == 24 and v["W"] == 16 and v["H"] == 12
    prove_and_compare(ctx, oracle, v, (1, 12, 4))


# ------------------------------------------------------------------ (3) refused before anything is proven
def test_prover_refusals_each_by_its_message(ctx):
    v = RPA.honest_view(2, 0, 1, 3, 40)
    R, F, b, Q = shape(v)
    prm = Params(1, 8, 2)
    key = ctx.fri16_rowpaths_key(v, prm)
    try:
        assert verify_fri16_rowpaths(ctx.prove_fri16_rowpaths(key, v, prm), RPA.public_values(v), R, F, b, Q, v["pow_bits"], v["W"], key.root, prm) == (0, 0)
        moved = lambda paths, q, lvl, j: [[[(c + 1) % P if (qq, l, k) == (q, lvl, j) else c for k, c in enumerate(d)] for l, d in enumerate(p)] for qq, p in enumerate(paths)]
        with pytest.raises(ZkHipError, match="query 1, trace tree: the opened row's path does not end in the root"):
            ctx.prove_fri16_rowpaths(key, dict(v, tpaths=moved(v["tpaths"], 1, 4, 3)), prm)
        with pytest.raises(ZkHipError, match="query 2, quotient tree: the opened row's path does not end in the root"):
            ctx.prove_fri16_rowpaths(key, dict(v, qpaths=moved(v["qpaths"], 2, 0, 7)), prm)
        with pytest.raises(ZkHipError, match="query 0, trace tree: the opened row's path does not end in the root"):      # a root that is not the paths'
            ctx.prove_fri16_rowpaths(key, dict(v, troot=[(v["troot"][0] + 1) % P] + list(v["troot"][1:])), prm)
        with pytest.raises(ZkHipError, match="width-16 hash"):
            ctx.prove_fri16_rowpaths(key, dict(v, hash_width=16), prm)
        bad = [[list(d) for d in p] for p in v["tpaths"]]
        bad[1][8][0] = P
        with pytest.raises(ZkHipError, match="query 1, trace tree: path words must be canonical"):
            ctx.prove_fri16_rowpaths(key, dict(v, tpaths=bad), prm)
        # what the openings machine refuses
        trows = [list(r) for r in v["trows"]]
        trows[2][5] = (trows[2][5] + 1) % P
        with pytest.raises(ZkHipError, match="the reduced opening of query 2 computed from its rows and the constants is not the view's"):
            ctx.prove_fri16_rowpaths(key, dict(v, trows=trows), prm)
        betas = [list(bt) for bt in v["betas"]]
        betas[1][2] = (betas[1][2] + 1) % P
        with pytest.raises(ZkHipError, match="challenges are not the ones the transcript draws"):
            ctx.prove_fri16_rowpaths(key, dict(v, betas=betas), prm)
    finally:
        key.close()


# ------------------------------------------------------------------ (4) full size, measured and printed
def test_full_size_segment_measured(ctx):
    """one 2^20 x 128 segment at the RISC Zero parameters (50 queries, R = 3, 256 final coefficients, H = 22), outer (1, 50, 16): after one warm-up call each, host
    clock around calls that end in a synchronise -- the P24R table alone (100 paths, 2 650 rows in 2^12), the whole row-paths proof, and the openings machine's proof
    of the same view in the same process (the difference is what the row paths cost).  Single measurements; printed, not asserted.  Both proofs are verified."""
    log_n, width = 20, 128
    sp = segment_params(50, 0, 8)
    t = ctx.gen_trace(SEED, 0, log_n, width)
    proof = ctx.prove_shard(t, log_n, width, [1, 2, 3], sp)
    t.free()
    v, tv = fri16_view_shard(proof, log_n, width, [1, 2, 3], sp), fri16_view_transcript(proof, log_n, width, [1, 2, 3], sp)
    v = dict(v, capacity=tv["capacity"], witness=tv["witness"], pow_bits=tv["pow_bits"], **fri16_view_openings(proof, log_n, width, [1, 2, 3], sp),
             **fri16_view_row_paths(proof, log_n, width, [1, 2, 3], sp))
    R, F, b, Q = shape(v)
    assert (R, F, b, Q, v["W"], v["H"]) == (3, 8, 2, 50, 128, 22) and v["hash_width"] == 24
    prm = Params(1, 50, 16)
    rkey, okey = ctx.fri16_rowpaths_key(v, prm), ctx.fri16_openings_key(v, prm)
    indices = [q[0] for q in v["queries"]]
    args = (R, F, b, Q, v["pow_bits"], v["W"], v["trows"], v["qrows"], indices, v["tpaths"], v["qpaths"])
    try:
        ctx.prove_fri16_rowpaths(rkey, v, prm)                       # warm-up (allocations, programs)
        ctx.prove_fri16_openings(okey, v, prm)
        ctx.fri16_rowpaths_gen_trace(*args)
        t0 = time.perf_counter()
        trace, ends = ctx.fri16_rowpaths_gen_trace(*args)
        t1 = time.perf_counter()
        rproof = ctx.prove_fri16_rowpaths(rkey, v, prm)
        t2 = time.perf_counter()
        oproof = ctx.prove_fri16_openings(okey, v, prm)
        t3 = time.perf_counter()
        assert trace.shape == (1 << 12, 552) and ends.tolist() == [v["qroot"] if p & 1 else v["troot"] for p in range(2 * Q)]
        assert rkey.root.tolist() == fri16_rowpaths_key_host(v, prm).tolist() and okey.root.tolist() == fri16_openings_key_host(v, prm).tolist()
        assert verify_fri16_rowpaths(rproof, RPA.public_values(v), R, F, b, Q, v["pow_bits"], v["W"], rkey.root, prm) == (0, 0)
        assert verify_fri16_openings(oproof, OA.public_values(v), R, F, b, Q, v["pow_bits"], v["W"], okey.root, prm) == (0, 0)
    finally:
        rkey.close(); okey.close()
    print("fri16 row-paths machine of a 2^20 x 128 segment: %d paths, %d P24R rows in 2^12; the P24R table (with its download) %.3f ms, whole row-paths proof %.3f ms "
          "(%d bytes); the openings machine's proof of the same view %.3f ms (%d bytes)"
          % (2 * Q, Q * (width // 16 + 1 + 2 * v["H"]), 1e3 * (t1 - t0), 1e3 * (t2 - t1), rproof.size, 1e3 * (t3 - t2), oproof.size))
