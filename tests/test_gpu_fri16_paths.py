"""The fold-by-16 PATHS machine on the GPU (zktls_amd/csrc/fri16_chip.hip, the P24L trace kernel in hash.hip): the device's P24L table against
the Python restatement (tests/fri16_paths_air.py) word for word, the device key against the host key and the oracle's setup, proof bytes
against the oracle's generic keyed-machine prover on the restatement's arrays, what the prover refuses before proving, and one full-size
measurement beside the LAYERS-table machine."""
import functools
import time

import numpy as np
import pytest

import fri16_air as A
import fri16_paths_air as PA
from test_fri16_chip_cpu import FOLD16_GOLDEN, golden_view, shape_of
from test_fri16_paths_cpu import SMALL_SHAPES
from test_gpu_fri16_chip import SEED, segment_view
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import fri16_key_host, fri16_paths_key_host, fri16_view_shard, verify_fri16, verify_fri16_paths

pytestmark = pytest.mark.gpu
P = 2013265921


@functools.lru_cache(maxsize=None)
def random_view(shape):
    return PA.random_view(*shape, seed=7 * shape[0] + shape[1])


def check_trace(ctx, v):
    """the device's P24L table and path ends = the restatement's; -> the restatement's (trace, ends, counts)"""
    mine = PA.p24l_trace(v)
    buf, ln, ends = ctx.fri16_paths_gen_trace(v)
    got = buf.download().reshape(-1, PA.WIDTH_L)
    buf.free()
    assert got.shape == mine[0].shape == (1 << ln, PA.WIDTH_L)
    assert (got == mine[0]).all(), np.argwhere(got != mine[0])[:8]
    assert ends.tolist() == mine[1]
    assert all(e == [int(x) for x in v["roots"][p[0]]] for p, e in zip(PA.distinct_paths(v), mine[1]))
    return mine


# ------------------------------------------------------------------ (7) the device's P24L = the restatement's
@pytest.mark.parametrize("shape", SMALL_SHAPES + [(5, 1, 1, 9), (2, 6, 3, 3), (4, 8, 3, 16), (3, 8, 2, 50)])
def test_device_trace_of_random_views_equals_the_python_restatement(ctx, shape):
    check_trace(ctx, random_view(shape))


@pytest.mark.parametrize("name", FOLD16_GOLDEN)
def test_device_trace_of_the_golden_views_equals_the_python_restatement(ctx, name):
    check_trace(ctx, golden_view(name))


# ------------------------------------------------------------------ (8) device key = host key = oracle setup; proof bytes = the oracle's
def prove_and_compare(ctx, O, v, shape, p24l=None):
    R, F, b, Q = len(v["betas"]), v["F"], v["b"], len(v["queries"])
    main, pre, progs, tabs, pub = PA.machine(v, p24l)
    lns, ws, pws = shape_of(main, pre)
    prm, oprm = Params(*shape), O.default_params(*shape)
    key = ctx.fri16_paths_key(v, prm)
    try:
        assert key.root.tolist() == fri16_paths_key_host(v, prm).tolist() == O.machine_setup(pre, lns, oprm).tolist()
        proof = ctx.prove_fri16_paths(key, v, prm)
        assert proof.tobytes() == O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm).tobytes()
        assert verify_fri16_paths(proof, pub, R, F, b, Q, key.root, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tabs, pub, oprm) == 0
        bad = list(pub)
        bad[0] = (bad[0] + 1) % P
        assert verify_fri16_paths(proof, bad, R, F, b, Q, key.root, prm)[0] != 0
    finally:
        key.close()
    return proof


@pytest.mark.parametrize("shape", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_a_golden_view_equal_the_oracles(ctx, oracle, shape):
    prove_and_compare(ctx, oracle, golden_view("v8_groups_r0_lookup_8x16"), shape)


@pytest.mark.parametrize("code_width,shape", [(0, (1, 12, 4)), (4, (2, 7, 0))])
def test_trace_and_proof_bytes_of_a_gpu_segment_proofs_view(ctx, oracle, code_width, shape):
    """2^10 x 16, 50 queries, R = 2, four final coefficients, made on the GPU; code_width = 4: a version-8 proof (code / data groups)"""
    v = segment_view(ctx, oracle, 10, 16, segment_params(50, 0, 2, code_width), [7])
    assert len(v["betas"]) == 2 and len(v["queries"]) == 50 and v["hash_width"] == 24
    prove_and_compare(ctx, oracle, v, shape, check_trace(ctx, v))


# ------------------------------------------------------------------ (9) refused before anything is proven
def disagreeing_view(v):
    """queries 0 and 1 share their layer-0 row.  A row's fold is linear in its entries, fold = sum_j a_j e_j, so query 0's copy can hold another value where
    query 1 has its own entry (position p1) and compensate at a third position p2 (e_p2 -= a_p1 / a_p2): query 0 still folds to the same value, every
    chain still ends in the final polynomial -- and the two queries no longer hold the same row"""
    from pyref import ext_inv, ext_mul
    (i0, val0, sib0), (i1, _, _) = v["queries"][0], v["queries"][1]
    assert i0 >> 4 == i1 >> 4 and i0 != i1
    own, p1 = i0 & 15, i1 & 15
    p2 = [j for j in range(16) if j not in (own, p1)][0]
    row, lh, beta = i0 >> 4, v["H"] - 4, v["betas"][0]
    unit = lambda j: [[1, 0, 0, 0] if k == j else [0, 0, 0, 0] for k in range(16)]
    a1, a2 = (A.fold_row(row, lh, beta, unit(j))[1][3][0] for j in (p1, p2))
    entries = [list(e) for e in sib0[0]]
    entries.insert(own, list(val0))
    before = A.fold_row(row, lh, beta, entries)[1][3][0]
    entries[p1] = A.e_add(entries[p1], [1, 0, 0, 0])
    entries[p2] = A.e_sub(entries[p2], ext_mul(a1, ext_inv(a2)))
    assert A.fold_row(row, lh, beta, entries)[1][3][0] == before
    sibs = [[e for j, e in enumerate(entries) if j != own]] + [[list(e) for e in r] for r in sib0[1:]]
    return dict(v, queries=[(i0, val0, sibs)] + list(v["queries"][1:]))


def test_prover_refusals_name_query_and_layer(ctx):
    v = random_view((2, 2, 2, 11))
    R, Q = 2, 11
    prm = Params(1, 8, 2)
    key = ctx.fri16_paths_key(v, prm)
    try:
        assert verify_fri16_paths(ctx.prove_fri16_paths(key, v, prm), [c for bt in v["betas"] for c in bt], 2, 2, 2, Q, key.root, prm) == (0, 0)
        # one sibling digest of one path (query 3's alone: it shares its layer-1 row with no other query)
        rows1 = [q[0] >> 8 for q in v["queries"]]
        assert rows1.count(rows1[3]) == 1
        paths = [[list(pl) for pl in pq] for pq in v["paths"]]
        paths[3][1][8 * 2 + 3] = (paths[3][1][8 * 2 + 3] + 1) % P
        with pytest.raises(ZkHipError, match="query 3 layer 1 does not open"):
            ctx.prove_fri16_paths(key, dict(v, paths=paths), prm)
        # two queries that share a row (0 and 1 at layer 0) and bring different paths for it
        assert v["queries"][0][0] >> 4 == v["queries"][1][0] >> 4
        paths = [[list(pl) for pl in pq] for pq in v["paths"]]
        paths[1][0][5] = (paths[1][0][5] + 1) % P
        with pytest.raises(ZkHipError, match="query 1 layer 0 disagrees with query 0 about the path of a shared row"):
            ctx.prove_fri16_paths(key, dict(v, paths=paths), prm)
        # a root that is not the tree's (the key made for the true roots)
        roots = [list(r) for r in v["roots"]]
        roots[0][0] = (roots[0][0] + 1) % P
        with pytest.raises(ZkHipError, match="layer 0 does not open"):
            ctx.prove_fri16_paths(key, dict(v, roots=roots), prm)
        # one layer entry changed: the chain no longer ends in the final polynomial (refused as today, first)
        q = list(v["queries"])
        sibs = [[list(e) for e in row] for row in q[4][2]]
        sibs[1][6][2] = (sibs[1][6][2] + 1) % P
        with pytest.raises(ZkHipError, match="query 4 does not end in the final polynomial"):
            ctx.prove_fri16_paths(key, dict(v, queries=q[:4] + [(q[4][0], q[4][1], sibs)] + q[5:]), prm)
        one_index = dict(v, queries=q[:6] + [(q[6][0] ^ (1 << 7), q[6][1], q[6][2])] + q[7:])
        with pytest.raises(ZkHipError, match="query 6 does not end in the final polynomial"):
            ctx.prove_fri16_paths(key, one_index, prm)
        # two queries that disagree about the ENTRIES of a shared row while both chains stay intact
        with pytest.raises(ZkHipError, match="query 1 layer 0 disagrees with query 0 about a shared row"):
            ctx.prove_fri16_paths(key, disagreeing_view(v), prm)
        # a fold-16 view whose commitments are width-16 trees
        with pytest.raises(ZkHipError, match="width-16 hash"):
            ctx.prove_fri16_paths(key, dict(v, hash_width=16), prm)
    finally:
        key.close()


def test_a_width16_hash_fold16_proof_is_refused_here_and_taken_by_the_layers_machine(ctx, oracle):
    inner = Params(2, 50, 0, 0, 4, 2, 16)
    t = ctx.gen_trace(SEED, 0, 10, 16)
    proof = ctx.prove_shard(t, 10, 16, [1, 2, 3], inner)
    t.free()
    v = fri16_view_shard(proof, 10, 16, [1, 2, 3], inner)
    assert v["hash_width"] == 16
    prm = Params(1, 8, 2)
    with pytest.raises(ZkHipError, match="width-16 hash"):
        ctx.fri16_paths_key(v, prm)
    key = ctx.fri16_key(v, prm)
    try:
        assert verify_fri16(ctx.prove_fri16(key, v, prm), [c for bt in v["betas"] for c in bt], 2, 2, 2, 50, key.root, prm) == (0, 0)
    finally:
        key.close()


# ------------------------------------------------------------------ (10) full size, measured and printed
def test_full_size_segment_measured(ctx):
    """one 2^20 x 128 segment at the RISC Zero parameters (50 queries, R = 3, 256 final coefficients), outer (1, 50, 16): after one warm-up
    call each, host clock around calls that end in a synchronise -- the P24L table alone (which includes the FOLD16 rows it reads its leaves
    from, the uploads and the download of the path ends), the whole paths-machine proof, and the LAYERS-table machine's proof of the same view
    in the same process.  Single measurements; printed, not asserted.  Both proofs are verified on the host."""
    log_n, width = 20, 128
    sp = segment_params(50, 0, 8)
    t = ctx.gen_trace(SEED, 0, log_n, width)
    proof = ctx.prove_shard(t, log_n, width, [1, 2, 3], sp)
    t.free()
    v = fri16_view_shard(proof, log_n, width, [1, 2, 3], sp)
    R, F, b, Q = len(v["betas"]), v["F"], v["b"], len(v["queries"])
    assert (R, F, b, Q) == (3, 8, 2, 50) and v["hash_width"] == 24
    prm = Params(1, 50, 16)
    pub = [c for bt in v["betas"] for c in bt]
    pkey, lkey = ctx.fri16_paths_key(v, prm), ctx.fri16_key(v, prm)
    try:
        ctx.prove_fri16_paths(pkey, v, prm)                          # warm-up (allocations, programs)
        ctx.prove_fri16(lkey, v, prm)
        buf, ln, ends = ctx.fri16_paths_gen_trace(v)
        t0 = time.perf_counter()
        ctx.fri16_paths_gen_trace(v, out=buf)
        t1 = time.perf_counter()
        buf.free()
        pproof = ctx.prove_fri16_paths(pkey, v, prm)
        t2 = time.perf_counter()
        lproof = ctx.prove_fri16(lkey, v, prm)
        t3 = time.perf_counter()
        assert pkey.root.tolist() == fri16_paths_key_host(v, prm).tolist() and lkey.root.tolist() == fri16_key_host(v, prm).tolist()
        assert verify_fri16_paths(pproof, pub, R, F, b, Q, pkey.root, prm) == (0, 0)
        assert verify_fri16(lproof, pub, R, F, b, Q, lkey.root, prm) == (0, 0)
    finally:
        pkey.close(); lkey.close()
    rows = sum(4 + len(p[4]) for p in PA.distinct_paths(v))
    print("fri16 paths machine of a 2^20 x 128 segment: %d paths, %d P24L rows in 2^%d; P24L generation %.3f ms, whole paths proof %.3f ms (%d bytes); "
          "the LAYERS-table machine's proof of the same view %.3f ms (%d bytes)"
          % (len(ends), rows, ln, 1e3 * (t1 - t0), 1e3 * (t2 - t1), pproof.size, 1e3 * (t3 - t2), lproof.size))
