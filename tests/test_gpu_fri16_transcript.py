"""The fold-by-16 INDICES machine on the GPU (zktls_amd/csrc/fri16_chip.hip, the transcript kernel in hash.hip): the device's P2T and SAMPLES tables against
the Python restatement (tests/fri16_transcript_air.py) word for word -- also at shapes where no honest FRI instance fits in a test, since the transcript side
needs no layer data --, the SAMPLES rows of edge words, the device key against the host key and the oracle's setup, proof bytes against the oracle's generic
keyed-machine prover on the restatement's arrays, what the prover refuses before proving, and one full-size measurement beside the paths machine."""
import functools
import time

import numpy as np
import pytest

import fri16_air as A
import fri16_transcript_air as TA
import fri_air as FA
from test_fri16_chip_cpu import GOLDEN, load, shape_of
from test_gpu_fri16_chip import SEED
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import fri16_indices_key_host, fri16_paths_key_host, fri16_view_shard, fri16_view_transcript, verify_fri16_indices, verify_fri16_paths

pytestmark = pytest.mark.gpu
P = 2013265921
TRANSCRIPT_ONLY_SHAPES = [(5, 4, 3, 3), (3, 8, 2, 50), (1, 8, 1, 1024)]          # H = 27; the RISC Zero parameters on a 2^20-row segment; 129 SAMPLES rows


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


# ------------------------------------------------------------------ (1) the device's P2T and SAMPLES = the restatement's
@pytest.mark.parametrize("S", TA.HONEST_SHAPES + TRANSCRIPT_ONLY_SHAPES)
def test_gen_traces_equal_the_python_restatement(ctx, S):
    R, F, b, Q = S
    rng = np.random.default_rng([11, R, F, b, Q])
    capacity, roots = [int(x) for x in rng.integers(0, P, 8)], rng.integers(0, P, (R, 8)).tolist()
    final_poly, witness = rng.integers(0, P, (1 << F, 4)).tolist(), int(rng.integers(0, P))
    p2t, smp, betas, idx = TA.transcript_traces(R, F, b, Q, capacity, roots, final_poly, witness)
    g_p2t, g_smp, g_betas, g_idx = ctx.fri16_indices_gen_traces(R, F, b, Q, TA.POW_BITS, capacity, roots, final_poly, witness)
    assert g_p2t.shape == p2t.shape and g_smp.shape == smp.shape
    assert (g_p2t == p2t).all(), np.argwhere(g_p2t != p2t)[:8]
    assert (g_smp == smp).all(), np.argwhere(g_smp != smp)[:8]
    assert g_betas.tolist() == betas and g_idx.tolist() == idx
    if S == (1, 8, 1, 1024):
        C_, S_, NT = TA.chain_rows(R, F, Q)
        assert (C_, S_, NT) == (128, 129, 258) and smp.shape == (256, FA.S_MAIN) and p2t.shape == (512, TA.T_WIDTH)


@pytest.mark.parametrize("H,Q", [(5, 7), (12, 8), (27, 7), (27, 20)])
def test_samples_rows_of_edge_words(ctx, H, Q):
    edge = [0, 1, P - 1, 0x77FFFFFF, (1 << 27) - 1, 1 << 27, (1 << H) - 1, 0x78000000]
    rows = FA.sample_rows(Q)
    rng = np.random.default_rng(H)
    words = [edge] + [[int(x) for x in rng.integers(0, P, 8)] for _ in range(rows - 1)]
    if rows > 1:
        words[1][:4] = [P - 2, (1 << 27) + 1, 0x70000000, 0x0FFFFFFF]
    mine = FA.samples_tables(H - 1, Q, words, A.lg(rows), base=0)[1]
    got = ctx.fri16_samples_gen_trace(H, Q, words)
    assert got.shape == mine.shape and (got == mine).all(), np.argwhere(got != mine)[:8]
    with pytest.raises(ZkHipError, match="canonical"):
        ctx.fri16_samples_gen_trace(H, Q, [[P] + edge[1:]] + words[1:])


# ------------------------------------------------------------------ (2) device key = host key = oracle setup; proof bytes = the oracle's
def prove_and_compare(ctx, O, v, outer):
    R, F, b, Q = shape(v)
    pb = v["pow_bits"]
    main, pre, progs, tabs, pub = TA.machine(v)
    lns, ws, pws = shape_of(main, pre)
    prm, oprm = Params(*outer), O.default_params(*outer)
    key = ctx.fri16_indices_key(v, prm)
    try:
        assert key.root.tolist() == fri16_indices_key_host(v, prm).tolist() == O.machine_setup(pre, lns, oprm).tolist()
        proof = ctx.prove_fri16_indices(key, v, prm)
        assert proof.tobytes() == O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm).tobytes()
        assert verify_fri16_indices(proof, pub, R, F, b, Q, pb, key.root, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tabs, pub, oprm) == 0
        bad = list(pub)
        bad[0] = (bad[0] + 1) % P
        assert verify_fri16_indices(proof, bad, R, F, b, Q, pb, key.root, prm)[0] != 0
    finally:
        key.close()
    return proof


@pytest.mark.parametrize("outer", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_a_golden_view_equal_the_oracles(ctx, oracle, outer):
    prove_and_compare(ctx, oracle, TA.golden_view("v8_groups_r0_lookup_8x16", GOLDEN, load), outer)


def test_proof_bytes_of_an_honest_view_with_proof_of_work_equal_the_oracles(ctx, oracle):
    prove_and_compare(ctx, oracle, TA.honest_view(1, 1, 1, 8), (1, 10, 2))


def gpu_segment_view(ctx, oracle, log_n, width, sp, public, shard=3):
    """a RISC Zero-shape segment proof made on the GPU, its fold-16 view and its transcript view in one dict"""
    t = oracle.gen_trace(SEED, shard, log_n, width)
    cols = ctx.from_numpy(np.ascontiguousarray(t.T))
    proof = ctx.prove_segment(cols, log_n, width, public, sp)
    cols.free()
    v, tv = fri16_view_shard(proof, log_n, width, public, sp), fri16_view_transcript(proof, log_n, width, public, sp)
    assert tv["roots"] == v["roots"] and tv["betas"] == v["betas"] and tv["pending"] == 0
    return dict(v, capacity=tv["capacity"], witness=tv["witness"], pow_bits=tv["pow_bits"])


def test_proof_bytes_of_a_gpu_segment_proofs_view(ctx, oracle):
    """2^10 x 16, 50 queries, R = 2, four final coefficients, made on the GPU"""
    v = gpu_segment_view(ctx, oracle, 10, 16, segment_params(50, 0, 2), [7])
    assert shape(v) == (2, 2, 2, 50) and v["hash_width"] == 24
    prove_and_compare(ctx, oracle, v, (1, 12, 4))


# ------------------------------------------------------------------ (3) refused before anything is proven
def test_prover_refusals_each_by_its_message(ctx):
    v = TA.honest_view(2, 2, 2, 11)
    R, F, b, Q = shape(v)
    prm = Params(1, 8, 2)
    key = ctx.fri16_indices_key(v, prm)
    try:
        assert verify_fri16_indices(ctx.prove_fri16_indices(key, v, prm), v["capacity"], R, F, b, Q, v["pow_bits"], key.root, prm) == (0, 0)
        # a challenge that the chain does not draw
        betas = [list(bt) for bt in v["betas"]]
        betas[1][2] = (betas[1][2] + 1) % P
        with pytest.raises(ZkHipError, match="challenges are not the ones the transcript draws"):
            ctx.prove_fri16_indices(key, dict(v, betas=betas), prm)
        # ... or draws from another capacity
        with pytest.raises(ZkHipError, match="challenges are not the ones the transcript draws"):
            ctx.prove_fri16_indices(key, dict(v, capacity=[(v["capacity"][0] + 1) % P] + list(v["capacity"][1:])), prm)
        # a witness that fails the proof of work
        w = v["witness"]
        while True:
            w += 1
            if TA.chain(v["capacity"], v["roots"], v["final_poly"], w, F, Q)["words"][0][0] & ((1 << v["pow_bits"]) - 1):
                break
        with pytest.raises(ZkHipError, match="witness does not satisfy the proof of work"):
            ctx.prove_fri16_indices(key, dict(v, witness=w), prm)
        # indices that are not the drawn ones: two queries exchanged, each with its own openings (every chain and path holds)
        q, pt = list(v["queries"]), list(v["paths"])
        q[0], q[4], pt[0], pt[4] = q[4], q[0], pt[4], pt[0]
        assert q[0][0] != q[4][0]
        with pytest.raises(ZkHipError, match="query indices are not the ones the transcript draws"):
            ctx.prove_fri16_indices(key, dict(v, queries=q, paths=pt), prm)
        # what the paths machine refuses: a path that does not open, a chain that does not end in the final polynomial
        rows0 = [i >> 4 for i, _, _ in v["queries"]]
        lone = [k for k, r in enumerate(rows0) if rows0.count(r) == 1][0]          # a query that shares its layer-0 row with no other
        paths = [[list(pl) for pl in pq] for pq in v["paths"]]
        paths[lone][0][8 * 2 + 3] = (paths[lone][0][8 * 2 + 3] + 1) % P
        with pytest.raises(ZkHipError, match="query %d layer 0 does not open" % lone):
            ctx.prove_fri16_indices(key, dict(v, paths=paths), prm)
        q = list(v["queries"])
        sibs = [[list(e) for e in row] for row in q[4][2]]
        sibs[1][6][2] = (sibs[1][6][2] + 1) % P
        with pytest.raises(ZkHipError, match="does not end in the final polynomial"):
            ctx.prove_fri16_indices(key, dict(v, queries=q[:4] + [(q[4][0], q[4][1], sibs)] + q[5:]), prm)
        # width-16-hash inner proofs, and grinding bits out of range
        with pytest.raises(ZkHipError, match="width-16 hash"):
            ctx.prove_fri16_indices(key, dict(v, hash_width=16), prm)
        with pytest.raises(ZkHipError, match="inner_pow_bits"):
            ctx.prove_fri16_indices(key, dict(v, pow_bits=31), prm)
    finally:
        key.close()


# ------------------------------------------------------------------ (4) full size, measured and printed
def test_full_size_segment_measured(ctx):
    """one 2^20 x 128 segment at the RISC Zero parameters (50 queries, R = 3, 256 final coefficients), outer (1, 50, 16): after one warm-up call each, host
    clock around calls that end in a synchronise -- the transcript tables alone, the whole indices-machine proof, and the paths machine's proof of the same
    view in the same process (the difference is what the transcript costs).  Single measurements; printed, not asserted.  Both proofs are verified."""
    log_n, width = 20, 128
    sp = segment_params(50, 0, 8)
    t = ctx.gen_trace(SEED, 0, log_n, width)
    proof = ctx.prove_shard(t, log_n, width, [1, 2, 3], sp)
    t.free()
    v, tv = fri16_view_shard(proof, log_n, width, [1, 2, 3], sp), fri16_view_transcript(proof, log_n, width, [1, 2, 3], sp)
    v = dict(v, capacity=tv["capacity"], witness=tv["witness"], pow_bits=tv["pow_bits"])
    R, F, b, Q = shape(v)
    assert (R, F, b, Q) == (3, 8, 2, 50) and v["hash_width"] == 24 and tv["roots"] == v["roots"] and tv["betas"] == v["betas"]
    prm = Params(1, 50, 16)
    ikey, pkey = ctx.fri16_indices_key(v, prm), ctx.fri16_paths_key(v, prm)
    args = (R, F, b, Q, v["pow_bits"], v["capacity"], v["roots"], v["final_poly"], v["witness"])
    try:
        ctx.prove_fri16_indices(ikey, v, prm)                        # warm-up (allocations, programs)
        ctx.prove_fri16_paths(pkey, v, prm)
        ctx.fri16_indices_gen_traces(*args)
        t0 = time.perf_counter()
        _, _, betas, idx = ctx.fri16_indices_gen_traces(*args)
        t1 = time.perf_counter()
        iproof = ctx.prove_fri16_indices(ikey, v, prm)
        t2 = time.perf_counter()
        pproof = ctx.prove_fri16_paths(pkey, v, prm)
        t3 = time.perf_counter()
        assert betas.tolist() == v["betas"] and idx.tolist() == [q[0] for q in v["queries"]]
        assert ikey.root.tolist() == fri16_indices_key_host(v, prm).tolist() and pkey.root.tolist() == fri16_paths_key_host(v, prm).tolist()
        assert verify_fri16_indices(iproof, v["capacity"], R, F, b, Q, v["pow_bits"], ikey.root, prm) == (0, 0)
        assert verify_fri16_paths(pproof, [c for bt in v["betas"] for c in bt], R, F, b, Q, pkey.root, prm) == (0, 0)
    finally:
        ikey.close(); pkey.close()
    C_, S_, NT = TA.chain_rows(R, F, Q)
    print("fri16 indices machine of a 2^20 x 128 segment: %d chain rows, %d SAMPLES rows; transcript tables (with two downloads) %.3f ms, whole indices proof "
          "%.3f ms (%d bytes); the paths machine's proof of the same view %.3f ms (%d bytes)"
          % (NT, S_, 1e3 * (t1 - t0), 1e3 * (t2 - t1), iproof.size, 1e3 * (t3 - t2), pproof.size))
