"""The fold-by-16 HEAD machine on the GPU (zktls_amd/csrc/fri16_chip.hip, fri16_opened_rows_kernel in fri16_rows.cuh): the device's P2TH, SAMPLES and OPENED16 tables,
the eight derived constants and the capacity against the Python restatement (tests/fri16_head_air.py) word for word from random inputs -- at the widths on both
sides of every boundary the kernel has (a wave of 64 rows, a round of 256) and on edge words --, the device key against the host key and the oracle's setup, proof
bytes against the oracle's generic keyed-machine prover on the restatement's arrays, what the prover refuses before proving, and one full-size measurement beside
the row-paths machine."""
import time

import numpy as np
import pytest

import fri16_head_air as HA
import fri16_openings_air as OA
import fri16_rowpaths_air as RPA
from field_edges import edge_canonical
from test_fri16_chip_cpu import GOLDEN, load, shape_of
from test_gpu_fri16_chip import SEED
from test_gpu_fri16_transcript import gpu_segment_view
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import (fri16_head_key_host, fri16_rowpaths_key_host, fri16_view_head, fri16_view_openings, fri16_view_row_paths, fri16_view_shard,
                              fri16_view_transcript, verify_fri16_head, verify_fri16_rowpaths)

pytestmark = pytest.mark.gpu
P = 2013265921
RAW = (2, 0, 1)                                               # R, F, log_blowup of the raw tests
Q_RAW, POW_RAW = 3, 4
# the first segment has W / 2 rows: 60, 64, 68 lie inside, fill and straddle a wave; W + 4 rows are active: 252 / 260, 508 / 516, 764 / 772, 1020 / 1028 lie on
# either side of a round of 256 lanes (at 512 the first segment itself straddles a round)
WIDTHS = [8, 16, 120, 128, 136, 248, 256, 504, 512, 760, 768, 1016, 1024]
NPS = [1, 3, 6, 30]                                           # 19, 21 (partial rows), 24 (no partial row), 48 (six full rows) stream words up to alpha


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


def compare_with_the_restatement(ctx, W, pubs, troot, qroot, opened, roots, final_poly, witness):
    R, F, b = RAW
    want = HA.head_traces(R, F, b, Q_RAW, POW_RAW, W, pubs, troot, qroot, opened, roots, final_poly, witness)
    got = ctx.fri16_head_gen_traces(R, F, b, Q_RAW, POW_RAW, W, pubs, troot, qroot, opened, roots, final_poly, witness)
    lr = HA.log_rows(R, F, b, Q_RAW, W, len(pubs))
    assert got[0].shape == want[0].shape == (1 << lr[HA.P2TH], 352) and got[2].shape == want[2].shape == (1 << lr[HA.OPENED16], 36)
    for name, g, w in zip(("P2TH", "SAMPLES", "OPENED16"), got[:3], want[:3]):
        assert (g == w).all(), (name, np.argwhere(g != w)[:8])
    assert got[3].tolist() == [[int(c) for c in want[3][n]] for n in OA.CONSTS]
    assert got[4].tolist() == [int(c) for c in want[4]]
    return want


def random_inputs(rng, W, NP, pool=None):
    rnd = (lambda n: [int(x) for x in rng.integers(0, P, n)]) if pool is None else (lambda n: [pool[int(i)] for i in rng.integers(0, len(pool), n)])
    return rnd(NP), rnd(8), rnd(8), [rnd(4) for _ in range(2 * W + 8)], [rnd(8) for _ in range(RAW[0])], [rnd(4)], rnd(1)[0]


# ------------------------------------------------------------------ (1) the device's tables, constants and capacity = the restatement's
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("NP", NPS)
def test_gen_traces_equal_the_python_restatement(ctx, NP, W):
    compare_with_the_restatement(ctx, W, *random_inputs(np.random.default_rng([37, NP, W]), W, NP))


@pytest.mark.parametrize("W,NP", [(8, 3), (136, 6), (256, 1)])
def test_gen_traces_on_edge_words(ctx, W, NP):
    """every input drawn from the words 0, 1, P - 1, (P - 1) / 2, (P + 1) / 2 -- as canonical values and as the canonical values whose Montgomery words they are;
    fa is steered by nothing: whatever the chain draws"""
    words = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]
    pool = words + [int(x) for x in edge_canonical(words)]
    compare_with_the_restatement(ctx, W, *random_inputs(np.random.default_rng([41, NP, W]), W, NP, pool))


def test_gen_traces_on_all_zero_opened_values(ctx):
    pubs, troot, qroot, _, roots, final_poly, witness = random_inputs(np.random.default_rng(43), 16, 3)
    want = compare_with_the_restatement(ctx, 16, pubs, troot, qroot, [[0] * 4] * 40, roots, final_poly, witness)
    assert want[3]["YL"] == want[3]["YN"] == want[3]["YQ"] == [0, 0, 0, 0] and want[3]["OFFN"] != [0, 0, 0, 0]
    want = compare_with_the_restatement(ctx, 16, pubs, troot, qroot, [[P - 1] * 4] * 40, roots, final_poly, witness)
    assert want[3]["YL"] != [0, 0, 0, 0]


def test_gen_traces_refuses_bad_arguments(ctx):
    R, F, b = RAW
    pubs, troot, qroot, opened, roots, final_poly, witness = random_inputs(np.random.default_rng(47), 16, 3)
    with pytest.raises(ZkHipError, match="the opened values must be canonical"):
        ctx.fri16_head_gen_traces(R, F, b, Q_RAW, POW_RAW, 16, pubs, troot, qroot, [[P, 0, 0, 0]] + opened[1:], roots, final_poly, witness)
    with pytest.raises(ZkHipError, match="the inner public values must be canonical"):
        ctx.fri16_head_gen_traces(R, F, b, Q_RAW, POW_RAW, 16, [P] + pubs[1:], troot, qroot, opened, roots, final_poly, witness)
    with pytest.raises(ZkHipError, match="1 .. 30 inner public values"):
        ctx.fri16_head_gen_traces(R, F, b, Q_RAW, POW_RAW, 16, list(range(31)), troot, qroot, opened, roots, final_poly, witness)


# ------------------------------------------------------------------ (2) device key = host key = oracle setup; proof bytes = the oracle's
def prove_and_compare(ctx, O, v, outer):
    R, F, b, Q = shape(v)
    pb, W = v["pow_bits"], v["W"]
    main, pre, progs, tabs, pub = HA.machine(v)
    lns, ws, pws = shape_of(main, pre)
    prm, oprm = Params(*outer), O.default_params(*outer)
    key = ctx.fri16_head_key(v, prm)
    try:
        assert key.root.tolist() == fri16_head_key_host(v, prm).tolist() == O.machine_setup(pre, lns, oprm).tolist()
        proof = ctx.prove_fri16_head(key, v, prm)
        assert proof.tobytes() == O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm).tobytes()
        assert pub == [int(x) for x in v["pubs"]]
        assert verify_fri16_head(proof, pub, R, F, b, Q, pb, W, key.root, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tabs, pub, oprm) == 0
        for k in range(len(pub)):                                # one inner public value changed
            bad = list(pub)
            bad[k] = (bad[k] + 1) % P
            assert verify_fri16_head(proof, bad, R, F, b, Q, pb, W, key.root, prm)[0] != 0
    finally:
        key.close()
    return proof


@pytest.mark.parametrize("outer", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_the_golden_view_equal_the_oracles(ctx, oracle, outer):
    prove_and_compare(ctx, oracle, HA.golden_view("v3_r0_9x8", GOLDEN, load), outer)


def test_proof_bytes_of_a_synthetic_view_equal_the_oracles(ctx, oracle):
    """W = 40, NP = 7: 25 stream words, a partial row of one word"""
    prove_and_compare(ctx, oracle, HA.honest_view(1, 1, 1, 3, 40, 7), (1, 10, 2))


def head_view_of_a_gpu_proof(ctx, oracle, log_n, width, sp, public, seed_index=3):
    v = gpu_segment_view(ctx, oracle, log_n, width, sp, public)
    t = oracle.gen_trace(SEED, seed_index, log_n, width)
    cols = ctx.from_numpy(np.ascontiguousarray(t.T))
    proof = ctx.prove_segment(cols, log_n, width, public, sp)
    cols.free()
    return dict(v, **fri16_view_openings(proof, log_n, width, public, sp), **fri16_view_row_paths(proof, log_n, width, public, sp),
                **fri16_view_head(proof, log_n, width, public, sp))


def test_proof_bytes_of_a_gpu_segment_proofs_view(ctx, oracle):
    """2^10 x 16, 12 queries, R = 2, four final coefficients, one public value, made on the GPU"""
    v = head_view_of_a_gpu_proof(ctx, oracle, 10, 16, segment_params(12, 0, 2), [7])
    assert shape(v) == (2, 2, 2, 12) and v["hash_width"] == 24 and v["W"] == 16 and v["H"] == 12 and v["pubs"] == [7] and len(v["opened"]) == 40
    prove_and_compare(ctx, oracle, v, (1, 12, 4))


# ------------------------------------------------------------------ (3) refused before anything is proven
def test_prover_refusals_each_by_its_message(ctx):
    v = HA.honest_view(1, 1, 1, 3, 40, 7)
    R, F, b, Q = shape(v)
    prm = Params(1, 8, 2)
    key = ctx.fri16_head_key(v, prm)
    bump = lambda e: [(e[0] + 1) % P] + list(e[1:])
    try:
        assert verify_fri16_head(ctx.prove_fri16_head(key, v, prm), v["pubs"], R, F, b, Q, v["pow_bits"], v["W"], key.root, prm) == (0, 0)
        # a constant of the view that the head does not derive, named.  (fa, OFFN and OFFQ, zeta and zeta g_N are moved together: the constants must match each other first)
        fa = bump(v["consts"]["FA"])
        moved = dict(v["consts"], FA=fa, OFFN=HA.pyref.ext_pow(fa, v["W"]), OFFQ=HA.pyref.ext_pow(fa, 2 * v["W"]))
        with pytest.raises(ZkHipError, match="the constant fa derived from the head of the transcript is not the view's"):
            ctx.prove_fri16_head(key, dict(v, consts=moved), prm)
        zeta = bump(v["consts"]["ZETA"])
        g = HA.pyref.two_adic_generator(v["H"] - v["b"])
        with pytest.raises(ZkHipError, match="the constant zeta derived"):
            ctx.prove_fri16_head(key, dict(v, consts=dict(v["consts"], ZETA=zeta, ZNX=[c * g % P for c in zeta])), prm)
        for name, said in (("YL", "YL"), ("YN", "YN"), ("YQ", "YQ")):
            with pytest.raises(ZkHipError, match="the constant %s derived" % said):
                ctx.prove_fri16_head(key, dict(v, consts=dict(v["consts"], **{name: bump(v["consts"][name])})), prm)
        with pytest.raises(ZkHipError, match="the capacity the head of the transcript leaves is not the view's"):
            ctx.prove_fri16_head(key, dict(v, capacity=bump(v["capacity"])), prm)
        # an opened value or a public value that is not the proof's: the derived challenges move
        opened = [list(e) for e in v["opened"]]
        opened[5][2] = (opened[5][2] + 1) % P
        with pytest.raises(ZkHipError, match="the constant fa derived"):
            ctx.prove_fri16_head(key, dict(v, opened=opened), prm)
        with pytest.raises(ZkHipError, match="the constant fa derived"):
            ctx.prove_fri16_head(key, dict(v, pubs=bump(v["pubs"])), prm)
        opened[5][2] = P
        with pytest.raises(ZkHipError, match="the opened values must be canonical"):
            ctx.prove_fri16_head(key, dict(v, opened=opened), prm)
        with pytest.raises(ZkHipError, match="the inner public values must be canonical"):
            ctx.prove_fri16_head(key, dict(v, pubs=[P] + list(v["pubs"][1:])), prm)
        with pytest.raises(ZkHipError, match="more than 30 inner public values"):
            ctx.prove_fri16_head(key, dict(v, pubs=list(range(31))), prm)
        # what the row-paths machine refuses
        with pytest.raises(ZkHipError, match="width-16 hash"):
            ctx.prove_fri16_head(key, dict(v, hash_width=16), prm)
        trows = [list(r) for r in v["trows"]]
        trows[2][5] = (trows[2][5] + 1) % P
        with pytest.raises(ZkHipError, match="the reduced opening of query 2 computed from its rows and the constants is not the view's"):
            ctx.prove_fri16_head(key, dict(v, trows=trows), prm)
        moved = [[[(c + 1) % P if (qq, l, k) == (1, 2, 3) else c for k, c in enumerate(d)] for l, d in enumerate(p)] for qq, p in enumerate(v["tpaths"])]
        with pytest.raises(ZkHipError, match="query 1, trace tree: the opened row's path does not end in the root"):
            ctx.prove_fri16_head(key, dict(v, tpaths=moved), prm)
    finally:
        key.close()


# ------------------------------------------------------------------ (4) full size, measured and printed
def test_full_size_segment_measured(ctx):
    """one 2^20 x 128 segment at the RISC Zero parameters (50 queries, R = 3, 256 final coefficients, H = 22), outer (1, 50, 16): after one warm-up call each, host
    clock around calls that end in a synchronise -- the three head tables alone (137 head rows in front of the chain, 132 OPENED16 rows), the whole head proof, and
    the row-paths machine's proof of the same view in the same process (the difference is what the head costs).  Single measurements; printed, not asserted.  Both
    proofs are verified."""
    log_n, width, public = 20, 128, [1, 2, 3]
    sp = segment_params(50, 0, 8)
    t = ctx.gen_trace(SEED, 0, log_n, width)
    proof = ctx.prove_shard(t, log_n, width, public, sp)
    t.free()
    v, tv = fri16_view_shard(proof, log_n, width, public, sp), fri16_view_transcript(proof, log_n, width, public, sp)
    v = dict(v, capacity=tv["capacity"], witness=tv["witness"], pow_bits=tv["pow_bits"], **fri16_view_openings(proof, log_n, width, public, sp),
             **fri16_view_row_paths(proof, log_n, width, public, sp), **fri16_view_head(proof, log_n, width, public, sp))
    R, F, b, Q = shape(v)
    assert (R, F, b, Q, v["W"], v["H"]) == (3, 8, 2, 50, 128, 22) and v["hash_width"] == 24
    assert HA.head_rows(128, 3) == (3, 136)
    prm = Params(1, 50, 16)
    hkey, rkey = ctx.fri16_head_key(v, prm), ctx.fri16_rowpaths_key(v, prm)
    args = (R, F, b, Q, v["pow_bits"], v["W"], v["pubs"], v["troot"], v["qroot"], v["opened"], v["roots"], v["final_poly"], v["witness"])
    try:
        ctx.prove_fri16_head(hkey, v, prm)                           # warm-up (allocations, programs)
        ctx.prove_fri16_rowpaths(rkey, v, prm)
        ctx.fri16_head_gen_traces(*args)
        t0 = time.perf_counter()
        traces = ctx.fri16_head_gen_traces(*args)
        t1 = time.perf_counter()
        hproof = ctx.prove_fri16_head(hkey, v, prm)
        t2 = time.perf_counter()
        rproof = ctx.prove_fri16_rowpaths(rkey, v, prm)
        t3 = time.perf_counter()
        assert traces[3].tolist() == [[int(c) for c in v["consts"][n]] for n in OA.CONSTS] and traces[4].tolist() == [int(c) for c in v["capacity"]]
        assert hkey.root.tolist() == fri16_head_key_host(v, prm).tolist() and rkey.root.tolist() == fri16_rowpaths_key_host(v, prm).tolist()
        assert verify_fri16_head(hproof, v["pubs"], R, F, b, Q, v["pow_bits"], v["W"], hkey.root, prm) == (0, 0)
        assert verify_fri16_rowpaths(rproof, RPA.public_values(v), R, F, b, Q, v["pow_bits"], v["W"], rkey.root, prm) == (0, 0)
    finally:
        hkey.close(); rkey.close()
    print("fri16 head machine of a 2^20 x 128 segment: %d head rows, %d OPENED16 rows; the three head tables (with their downloads) %.3f ms, whole head proof %.3f ms "
          "(%d bytes); the row-paths machine's proof of the same view %.3f ms (%d bytes)"
          % (HA.head_rows(128, 3)[1], 132, 1e3 * (t1 - t0), 1e3 * (t2 - t1), hproof.size, 1e3 * (t3 - t2), rproof.size))
