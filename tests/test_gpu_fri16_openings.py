"""The fold-by-16 OPENINGS machine on the GPU (zktls_amd/csrc/fri16_chip.hip, the ROWSUM16 / QUERY16 kernel in fri16_rows.cuh): the device's two tables against the
Python restatement (tests/fri16_openings_air.py) word for word from raw rows -- at the widths where the kernel's lane packing changes (two-row segments across
a wave, a wave filled exactly, the carry between rounds of 64 blocks) and on edge words --, the device key against the host key and the oracle's setup, proof
bytes against the oracle's generic keyed-machine prover on the restatement's arrays, what the prover refuses before proving, and one full-size measurement
beside the indices machine."""
import time

import numpy as np
import pytest

import fri16_openings_air as OA
import fri16_transcript_air as TA
import pyref
from field_edges import edge_canonical
from test_fri16_chip_cpu import GOLDEN, load, shape_of
from test_gpu_fri16_chip import SEED
from test_gpu_fri16_transcript import gpu_segment_view
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import (fri16_indices_key_host, fri16_openings_key_host, fri16_view_openings, fri16_view_shard, fri16_view_transcript, verify_fri16_indices,
                              verify_fri16_openings)

pytestmark = pytest.mark.gpu
P = 2013265921
RAW = (2, 0, 1)                                               # R, F, log_blowup of the raw-row tests: H = 9
WIDTHS = [8, 16, 24, 128, 496, 504, 512, 520]                 # blocks + 1 per query: 2, 3, 4, 17, 63, 64 (a wave filled exactly), 65 (the carry), 66
QUERIES = [1, 3, 33, 65]                                      # W = 8, Q = 33: two-row segments across a wave


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


def consts_from(rnd, W, H, b):
    fa, zeta = rnd(4), rnd(4)
    return dict(FA=fa, ZETA=zeta, ZNX=[c * pyref.two_adic_generator(H - b) % P for c in zeta], YL=rnd(4), YN=rnd(4), YQ=rnd(4), OFFN=pyref.ext_pow(fa, W),
                OFFQ=pyref.ext_pow(fa, 2 * W))


def compare_with_the_restatement(ctx, Q, W, trows, qrows, consts, indices):
    R, F, b = RAW
    H = 4 * R + F + b
    rs, qm, ros = OA.opening_traces(H, W, trows, qrows, consts, indices)
    g_rs, g_qm, g_ros = ctx.fri16_openings_gen_traces(R, F, b, Q, 0, W, trows, qrows, [consts[n] for n in OA.CONSTS], indices)
    assert g_rs.shape == rs.shape and g_qm.shape == qm.shape
    assert (g_rs == rs).all(), np.argwhere(g_rs != rs)[:8]
    assert (g_qm == qm).all(), np.argwhere(g_qm != qm)[:8]
    assert g_ros.tolist() == ros


# ------------------------------------------------------------------ (1) the device's ROWSUM16 and QUERY16 = the restatement's
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("Q", QUERIES)
def test_gen_traces_equal_the_python_restatement(ctx, Q, W):
    H = 4 * RAW[0] + RAW[1] + RAW[2]
    rng = np.random.default_rng([13, Q, W])
    rnd = lambda n: [int(x) for x in rng.integers(0, P, n)]
    trows, qrows = [rnd(W) for _ in range(Q)], [rnd(8) for _ in range(Q)]
    indices = [int(x) for x in rng.integers(0, 1 << H, Q)]
    compare_with_the_restatement(ctx, Q, W, trows, qrows, consts_from(rnd, W, H, RAW[2]), indices)


@pytest.mark.parametrize("Q,W", [(3, 24), (33, 8), (2, 512)])
def test_gen_traces_on_edge_words_and_the_first_and_last_index(ctx, Q, W):
    """rows and constants drawn from the words 0, 1, P - 1, (P - 1) / 2, (P + 1) / 2 -- as canonical values and as the canonical values whose Montgomery words
    they are --, indices 0 and 2^H - 1 among them"""
    H = 4 * RAW[0] + RAW[1] + RAW[2]
    words = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]
    pool = words + [int(x) for x in edge_canonical(words)]
    rng = np.random.default_rng([17, Q, W])
    rnd = lambda n: [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    trows, qrows = [rnd(W) for _ in range(Q)], [rnd(8) for _ in range(Q)]
    trows[0], qrows[0] = [P - 1] * W, [0] * 8
    if Q > 1:
        trows[1], qrows[1] = [0] * W, [P - 1] * 8
    consts = dict(FA=[P - 1, (P + 1) // 2, 1, (P - 1) // 2], ZETA=[(P - 1) // 2, 1, 0, P - 1], YL=rnd(4), YN=rnd(4), YQ=rnd(4))
    consts["ZNX"] = [c * pyref.two_adic_generator(H - RAW[2]) % P for c in consts["ZETA"]]
    consts["OFFN"], consts["OFFQ"] = pyref.ext_pow(consts["FA"], W), pyref.ext_pow(consts["FA"], 2 * W)
    indices = [0, (1 << H) - 1, 1][:Q] + [int(x) for x in rng.integers(0, 1 << H, max(Q - 3, 0))]
    compare_with_the_restatement(ctx, Q, W, trows, qrows, consts, indices)
    # FA = 0 and FA = 1: every sum is its row's first word / the plain sum of the words
    for fa in ([0, 0, 0, 0], [1, 0, 0, 0]):
        c2 = dict(consts, FA=fa, OFFN=pyref.ext_pow(fa, W), OFFQ=pyref.ext_pow(fa, 2 * W))
        compare_with_the_restatement(ctx, Q, W, trows, qrows, c2, indices)


def test_gen_traces_refuses_a_point_without_an_inverse_and_bad_arguments(ctx):
    R, F, b = RAW
    H, Q, W = 4 * R + F + b, 3, 16
    rng = np.random.default_rng(19)
    rnd = lambda n: [int(x) for x in rng.integers(0, P, n)]
    trows, qrows, indices = [rnd(W) for _ in range(Q)], [rnd(8) for _ in range(Q)], [5, 77, 300]
    consts = consts_from(rnd, W, H, b)
    x1 = 31 * OA.point(indices[1], H) % P
    at_zeta = dict(consts, ZETA=[x1, 0, 0, 0], ZNX=[x1 * pyref.two_adic_generator(H - b) % P, 0, 0, 0])
    with pytest.raises(ZkHipError, match="the point of query 1 is zeta or zeta g"):
        ctx.fri16_openings_gen_traces(R, F, b, Q, 0, W, trows, qrows, [at_zeta[n] for n in OA.CONSTS], indices)
    x2 = 31 * OA.point(indices[2], H) % P
    at_znx = dict(consts, ZNX=[x2, 0, 0, 0])
    with pytest.raises(ZkHipError, match="the point of query 2 is zeta or zeta g"):
        ctx.fri16_openings_gen_traces(R, F, b, Q, 0, W, trows, qrows, [at_znx[n] for n in OA.CONSTS], indices)
    with pytest.raises(ZkHipError, match="canonical"):
        ctx.fri16_openings_gen_traces(R, F, b, Q, 0, W, [[P] + trows[0][1:]] + trows[1:], qrows, [consts[n] for n in OA.CONSTS], indices)
    with pytest.raises(ZkHipError, match="more bits"):
        ctx.fri16_openings_gen_traces(R, F, b, Q, 0, W, trows, qrows, [consts[n] for n in OA.CONSTS], [1 << H, 0, 1])


# ------------------------------------------------------------------ (2) device key = host key = oracle setup; proof bytes = the oracle's
def prove_and_compare(ctx, O, v, outer):
    R, F, b, Q = shape(v)
    pb, W = v["pow_bits"], v["W"]
    main, pre, progs, tabs, pub = OA.machine(v)
    lns, ws, pws = shape_of(main, pre)
    prm, oprm = Params(*outer), O.default_params(*outer)
    key = ctx.fri16_openings_key(v, prm)
    try:
        assert key.root.tolist() == fri16_openings_key_host(v, prm).tolist() == O.machine_setup(pre, lns, oprm).tolist()
        proof = ctx.prove_fri16_openings(key, v, prm)
        assert proof.tobytes() == O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm).tobytes()
        assert verify_fri16_openings(proof, pub, R, F, b, Q, pb, W, key.root, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tabs, pub, oprm) == 0
        bad = list(pub)
        bad[21] = (bad[21] + 1) % P
        assert verify_fri16_openings(proof, bad, R, F, b, Q, pb, W, key.root, prm)[0] != 0
    finally:
        key.close()
    return proof


@pytest.mark.parametrize("outer", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_the_golden_view_equal_the_oracles(ctx, oracle, outer):
    prove_and_compare(ctx, oracle, OA.golden_view("v3_r0_9x8", GOLDEN, load), outer)


def test_proof_bytes_of_a_synthetic_view_equal_the_oracles(ctx, oracle):
    prove_and_compare(ctx, oracle, OA.honest_view(2, 2, 2, 11, 24), (1, 10, 2))


def openings_view(ctx, oracle, log_n, width, sp, public):
    v = gpu_segment_view(ctx, oracle, log_n, width, sp, public)
    t = oracle.gen_trace(SEED, 3, log_n, width)
    cols = ctx.from_numpy(np.ascontiguousarray(t.T))
    proof = ctx.prove_segment(cols, log_n, width, public, sp)
    cols.free()
    return dict(v, **fri16_view_openings(proof, log_n, width, public, sp))


def test_proof_bytes_of_a_gpu_segment_proofs_view(ctx, oracle):
    """2^10 x 16, 50 queries, R = 2, four final coefficients, made on the GPU"""
    v = openings_view(ctx, oracle, 10, 16, segment_params(50, 0, 2), [7])
    assert shape(v) == (2, 2, 2, 50) and v["hash_width"] == 24 and v["W"] == 16
    assert OA.reduced_openings(v) == [[int(c) for c in q[1]] for q in v["queries"]]
    prove_and_compare(ctx, oracle, v, (1, 12, 4))


# ------------------------------------------------------------------ (3) refused before anything is proven
def test_prover_refusals_each_by_its_message(ctx):
    v = OA.honest_view(2, 2, 2, 11, 24)
    R, F, b, Q = shape(v)
    prm = Params(1, 8, 2)
    key = ctx.fri16_openings_key(v, prm)
    try:
        assert verify_fri16_openings(ctx.prove_fri16_openings(key, v, prm), OA.public_values(v), R, F, b, Q, v["pow_bits"], v["W"], key.root, prm) == (0, 0)
        # a reduced opening that the rows do not give: one row word changed (the key would differ too; the prover refuses first)
        trows = [list(r) for r in v["trows"]]
        trows[6][5] = (trows[6][5] + 1) % P
        with pytest.raises(ZkHipError, match="the reduced opening of query 6 computed from its rows and the constants is not the view's"):
            ctx.prove_fri16_openings(key, dict(v, trows=trows), prm)
        qrows = [list(r) for r in v["qrows"]]
        qrows[3][7] = (qrows[3][7] + 1) % P
        qrows[9][0] = (qrows[9][0] + 1) % P
        with pytest.raises(ZkHipError, match="the reduced opening of query 3 computed"):
            ctx.prove_fri16_openings(key, dict(v, qrows=qrows), prm)
        # ... or another constant
        yl = [(v["consts"]["YL"][0] + 1) % P] + list(v["consts"]["YL"][1:])
        with pytest.raises(ZkHipError, match="the reduced opening of query 0 computed"):
            ctx.prove_fri16_openings(key, dict(v, consts=dict(v["consts"], YL=yl)), prm)
        # constants that do not match each other
        for name in ("ZNX", "OFFN", "OFFQ"):
            moved = [(v["consts"][name][0] + 1) % P] + list(v["consts"][name][1:])
            with pytest.raises(ZkHipError, match="the constants do not match each other"):
                ctx.prove_fri16_openings(key, dict(v, consts=dict(v["consts"], **{name: moved})), prm)
        # a query point equal to zeta
        x4 = 31 * OA.point(v["queries"][4][0], v["H"]) % P
        zeta = [x4, 0, 0, 0]
        at_zeta = dict(v["consts"], ZETA=zeta, ZNX=[c * pyref.two_adic_generator(v["H"] - b) % P for c in zeta])
        with pytest.raises(ZkHipError, match="the point of query 4 is zeta or zeta g"):
            ctx.prove_fri16_openings(key, dict(v, consts=at_zeta), prm)
        # what the indices machine refuses
        betas = [list(bt) for bt in v["betas"]]
        betas[1][2] = (betas[1][2] + 1) % P
        with pytest.raises(ZkHipError, match="challenges are not the ones the transcript draws"):
            ctx.prove_fri16_openings(key, dict(v, betas=betas), prm)
        q, pt = list(v["queries"]), list(v["paths"])
        q[0], q[4], pt[0], pt[4] = q[4], q[0], pt[4], pt[0]
        with pytest.raises(ZkHipError, match="query indices are not the ones the transcript draws"):
            ctx.prove_fri16_openings(key, dict(v, queries=q, paths=pt), prm)
        rows0 = [i >> 4 for i, _, _ in v["queries"]]
        lone = [k for k, r in enumerate(rows0) if rows0.count(r) == 1][0]
        paths = [[list(pl) for pl in pq] for pq in v["paths"]]
        paths[lone][0][8 * 2 + 3] = (paths[lone][0][8 * 2 + 3] + 1) % P
        with pytest.raises(ZkHipError, match="query %d layer 0 does not open" % lone):
            ctx.prove_fri16_openings(key, dict(v, paths=paths), prm)
        with pytest.raises(ZkHipError, match="width-16 hash"):
            ctx.prove_fri16_openings(key, dict(v, hash_width=16), prm)
        with pytest.raises(ZkHipError, match="trace width"):
            ctx.prove_fri16_openings(key, dict(v, W=20, trows=[r[:20] for r in v["trows"]]), prm)
    finally:
        key.close()


# ------------------------------------------------------------------ (4) full size, measured and printed
def test_full_size_segment_measured(ctx):
    """one 2^20 x 128 segment at the RISC Zero parameters (50 queries, R = 3, 256 final coefficients), outer (1, 50, 16): after one warm-up call each, host
    clock around calls that end in a synchronise -- the ROWSUM16 / QUERY16 tables alone, the whole openings-machine proof, and the indices machine's proof of
    the same view in the same process (the difference is what the openings cost).  Single measurements; printed, not asserted.  Both proofs are verified."""
    log_n, width = 20, 128
    sp = segment_params(50, 0, 8)
    t = ctx.gen_trace(SEED, 0, log_n, width)
    proof = ctx.prove_shard(t, log_n, width, [1, 2, 3], sp)
    t.free()
    v, tv = fri16_view_shard(proof, log_n, width, [1, 2, 3], sp), fri16_view_transcript(proof, log_n, width, [1, 2, 3], sp)
    v = dict(v, capacity=tv["capacity"], witness=tv["witness"], pow_bits=tv["pow_bits"], **fri16_view_openings(proof, log_n, width, [1, 2, 3], sp))
    R, F, b, Q = shape(v)
    assert (R, F, b, Q, v["W"]) == (3, 8, 2, 50, 128) and v["hash_width"] == 24
    prm = Params(1, 50, 16)
    okey, ikey = ctx.fri16_openings_key(v, prm), ctx.fri16_indices_key(v, prm)
    indices = [q[0] for q in v["queries"]]
    args = (R, F, b, Q, v["pow_bits"], v["W"], v["trows"], v["qrows"], [v["consts"][n] for n in OA.CONSTS], indices)
    try:
        ctx.prove_fri16_openings(okey, v, prm)                       # warm-up (allocations, programs)
        ctx.prove_fri16_indices(ikey, v, prm)
        ctx.fri16_openings_gen_traces(*args)
        t0 = time.perf_counter()
        _, _, ros = ctx.fri16_openings_gen_traces(*args)
        t1 = time.perf_counter()
        oproof = ctx.prove_fri16_openings(okey, v, prm)
        t2 = time.perf_counter()
        iproof = ctx.prove_fri16_indices(ikey, v, prm)
        t3 = time.perf_counter()
        assert ros.tolist() == [[int(c) for c in q[1]] for q in v["queries"]]
        assert okey.root.tolist() == fri16_openings_key_host(v, prm).tolist() and ikey.root.tolist() == fri16_indices_key_host(v, prm).tolist()
        assert verify_fri16_openings(oproof, OA.public_values(v), R, F, b, Q, v["pow_bits"], v["W"], okey.root, prm) == (0, 0)
        assert verify_fri16_indices(iproof, v["capacity"], R, F, b, Q, v["pow_bits"], ikey.root, prm) == (0, 0)
    finally:
        okey.close(); ikey.close()
    print("fri16 openings machine of a 2^20 x 128 segment: %d ROWSUM16 rows, %d ROWS rows; ROWSUM16 / QUERY16 tables (with two downloads) %.3f ms, whole openings "
          "proof %.3f ms (%d bytes); the indices machine's proof of the same view %.3f ms (%d bytes)"
          % (Q * (width // 8 + 1), Q * (width + 8) // 4, 1e3 * (t1 - t0), 1e3 * (t2 - t1), oproof.size, 1e3 * (t3 - t2), iproof.size))
