"""The fold-by-16 FRI machine on the GPU (zktls_amd/csrc/fri16_chip.hip): the two trace kernels against the Python restatement
(tests/fri16_air.py) word for word, the device key against the host key, proof bytes against the oracle's generic keyed-machine prover on the
restatement's arrays, the views of segment proofs made on the GPU (their layer openings through the width-24 Poseidon2 chip), what the
prover refuses before proving, and one full-size measurement."""
import functools
import time
import types

import numpy as np
import pytest

import fri16_air as A
import fri16_head_air as HA
import fri16_openings_air as OA
import fri16_rowpaths_air as RPA
import fri16_transcript_air as TA
import zktls_amd.device as D
from test_fri16_chip_cpu import RANDOM_SHAPES, FOLD16_GOLDEN, GOLDEN, golden_view, load, shape_of
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import fri16_key_host, fri16_view_shard, verify_fri16, verify_merkle_paths_p24

pytestmark = pytest.mark.gpu
SEED = 0x5A4B544C53
P = 2013265921


def shape_tuple(sp):
    return (sp.log_blowup, sp.num_queries, sp.pow_bits, sp.logup_pairs, sp.log_fold, sp.log_final, sp.hash_width, sp.code_width)


def segment_view(ctx, oracle, log_n, width, sp, public, shard=3):
    """a RISC Zero-shape segment proof made on the GPU (column-major trace) and its fold-16 view from the library, checked against the restatement's parse"""
    t = oracle.gen_trace(SEED, shard, log_n, width)
    cols = ctx.from_numpy(np.ascontiguousarray(t.T))
    proof = ctx.prove_segment(cols, log_n, width, public, sp)
    cols.free()
    v = fri16_view_shard(proof, log_n, width, public, sp)
    s = shape_tuple(sp)
    mine = A.parse_view(proof.tobytes(), log_n, width, public, s[0], s[1], s[2], logup_pairs=s[3], log_final=s[5], hash_width=s[6], code_width=s[7])
    assert v["betas"] == mine["betas"] and v["final_poly"] == mine["final_poly"] and v["roots"] == mine["roots"] and v["paths"] == mine["paths"]
    assert v["queries"] == [(i, list(x), [[list(e) for e in row] for row in sb]) for i, x, sb in mine["queries"]]
    return v


def check_traces(ctx, v):
    main, pre = A.tables(v)
    fold, lf, wf, final, ln = ctx.fri16_gen_traces(v)
    assert (1 << lf, wf) == main[A.FOLD16].shape and (1 << ln, A.FIN_MAIN) == main[A.FINAL].shape
    got_fold, got_final = fold.download().reshape(-1, wf), final.download().reshape(-1, A.FIN_MAIN)
    fold.free(); final.free()
    assert (got_fold == main[A.FOLD16]).all(), np.argwhere(got_fold != main[A.FOLD16])[:8]
    assert (got_final == main[A.FINAL]).all(), np.argwhere(got_final != main[A.FINAL])[:8]


# ------------------------------------------------------------------ (f) device traces = the restatement's
@pytest.mark.parametrize("R,F,b,Q", RANDOM_SHAPES + [(5, 1, 1, 9), (2, 6, 3, 3), (1, 7, 1, 2), (4, 8, 3, 16)])
def test_device_traces_of_random_views_equal_the_python_restatement(ctx, R, F, b, Q):
    check_traces(ctx, A.random_view(R, F, b, Q, seed=7 * R + F))


@pytest.mark.parametrize("name", FOLD16_GOLDEN)
def test_device_traces_of_the_golden_views_equal_the_python_restatement(ctx, name):
    check_traces(ctx, golden_view(name))


# ------------------------------------------------------------------ (g) proof bytes = the oracle's; device key = host key
def prove_and_compare(ctx, O, v, shape):
    R, F, b, Q = len(v["betas"]), v["F"], v["b"], len(v["queries"])
    main, pre, progs, tabs, pub = A.machine(v)
    lns, ws, pws = shape_of(main, pre)
    prm, oprm = Params(*shape), O.default_params(*shape)
    key = ctx.fri16_key(v, prm)
    try:
        assert key.root.tolist() == fri16_key_host(v, prm).tolist() == O.machine_setup(pre, lns, oprm).tolist()
        proof = ctx.prove_fri16(key, v, prm)
        assert proof.tobytes() == O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm).tobytes()
        assert verify_fri16(proof, pub, R, F, b, Q, key.root, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tabs, pub, oprm) == 0
        bad = list(pub)
        bad[0] = (bad[0] + 1) % P
        assert verify_fri16(proof, bad, R, F, b, Q, key.root, prm)[0] != 0
    finally:
        key.close()
    return proof


@pytest.mark.parametrize("shape", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_a_golden_view_equal_the_oracles(ctx, oracle, shape):
    prove_and_compare(ctx, oracle, golden_view("v8_groups_r0_lookup_8x16"), shape)


@pytest.mark.parametrize("code_width", [0, 4])
@pytest.mark.parametrize("shape", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_a_gpu_segment_proofs_view_equal_the_oracles(ctx, oracle, shape, code_width):
    """2^10 x 16, 50 queries, R = 2, four final coefficients; code_width = 4: a version-8 proof (code / data groups)"""
    v = segment_view(ctx, oracle, 10, 16, segment_params(50, 0, 2, code_width), [7])
    assert len(v["betas"]) == 2 and len(v["final_poly"]) == 4 and len(v["queries"]) == 50
    prove_and_compare(ctx, oracle, v, shape)


# ------------------------------------------------------------------ (h) the view's roots and paths are the ones a width-24 chip opens
def test_layer_openings_of_a_gpu_segment_proof_through_the_width24_chip(ctx, oracle):
    v = segment_view(ctx, oracle, 10, 16, segment_params(50, 0, 2), [7])
    R, H = len(v["betas"]), v["H"]
    prm = Params(1, 8, 4)
    for l in range(R):
        lh = H - 4 * (l + 1)
        rows = np.array([[c for e in ch[0][l]["entries"] for c in e] for ch in A.chains(v)], dtype=np.uint32)
        idx = np.array([ch[0][l]["row"] for ch in A.chains(v)], dtype=np.uint32)
        sibs = np.array([v["paths"][q][l] for q in range(50)], dtype=np.uint32).reshape(50, lh, 8)
        root = np.array(v["roots"][l], dtype=np.uint32)
        assert rows.shape == (50, 64)
        proof = ctx.prove_merkle_paths_p24(rows, sibs, idx, root, prm, row_width=64)
        assert verify_merkle_paths_p24(proof, root, 50, prm) == (0, 0)
        wrong = rows.copy()
        wrong[11, 9] = (int(wrong[11, 9]) + 1) % P
        with pytest.raises(ZkHipError):
            ctx.prove_merkle_paths_p24(wrong, sibs, idx, root, prm, row_width=64)


# ------------------------------------------------------------------ (i) refused before anything is proven
def test_prover_refuses_a_view_whose_chains_do_not_end_in_the_final_polynomial(ctx):
    v = A.random_view(2, 2, 2, 9, seed=2)
    prm = Params(1, 8, 2)
    key = ctx.fri16_key(v, prm)
    try:
        assert verify_fri16(ctx.prove_fri16(key, v, prm), [c for bt in v["betas"] for c in bt], 2, 2, 2, 9, key.root, prm) == (0, 0)
        q = list(v["queries"])
        sibs = [[list(e) for e in row] for row in q[4][2]]
        sibs[1][6][2] = (sibs[1][6][2] + 1) % P
        one_sibling = dict(v, queries=q[:4] + [(q[4][0], q[4][1], sibs)] + q[5:])
        with pytest.raises(ZkHipError, match="query 4 does not end in the final polynomial"):
            ctx.prove_fri16(key, one_sibling, prm)
        one_index = dict(v, queries=q[:6] + [(q[6][0] ^ (1 << 7), q[6][1], q[6][2])] + q[7:])
        with pytest.raises(ZkHipError, match="query 6 does not end in the final polynomial"):
            ctx.prove_fri16(key, one_index, prm)
        with pytest.raises(ZkHipError):
            ctx.fri16_key(one_sibling, prm)
    finally:
        key.close()


# ------------------------------------------------------------------ (i') every kind's entries refuse in their own name
@functools.lru_cache(maxsize=None)
def kind_view(kind):
    """the golden view the kind's own tests prove"""
    if kind in ("layers", "paths"):
        return golden_view("v8_groups_r0_lookup_8x16")
    if kind == "indices":
        return TA.golden_view("v8_groups_r0_lookup_8x16", GOLDEN, load)
    return {"openings": OA, "rowpaths": RPA}.get(kind, HA).golden_view("v3_r0_9x8", GOLDEN, load)


@pytest.mark.parametrize("kind,infix", [("layers", ""), ("paths", "_paths"), ("indices", "_indices"), ("openings", "_openings"), ("rowpaths", "_rowpaths"), ("head", "_head"),
                                        ("identity", "_identity"), ("lift", "_lift")])
def test_every_kinds_entries_refuse_in_their_own_name(ctx, kind, infix):
    """a null key is refused by the prove entry's argument checks (nothing is launched) with ZKHIP_ERR_INVALID and "<entry>: null argument"; from the paths machine on
    the key entry and the host key entry refuse an inner hash width of 16, each naming itself"""
    v, prm = kind_view(kind), Params(1, 8, 2)
    with pytest.raises(ZkHipError, match=r"^zkhip error -1: prove_fri16%s: null argument$" % infix) as e:
        getattr(ctx, "prove_fri16" + infix)(types.SimpleNamespace(handle=None), v, prm)
    assert e.value.code == -1
    if kind == "layers":
        return
    if kind == "lift":
        shape = (len(v["roots"]), v["F"], v["b"], len(v["queries"]), v["pow_bits"], v["W"], len(v["pubs"]))
        device, host = (lambda: ctx.fri16_lift_key(*shape, prm, hash_width=16)), (lambda: D.fri16_lift_key_host(*shape, prm, hash_width=16))
    else:
        w16 = dict(v, hash_width=16)
        device, host = (lambda: getattr(ctx, "fri16%s_key" % infix)(w16, prm)), (lambda: getattr(D, "fri16%s_key_host" % infix)(w16, prm))
    for call, name in ((device, "fri16%s_key: " % infix), (host, "fri16%s_key_host: " % infix)):
        with pytest.raises(ZkHipError, match="^zkhip error -1: " + name) as e:
            call()
        assert e.value.code == -1


# ------------------------------------------------------------------ (j) full size, measured and printed
def test_full_size_segment_measured(ctx):
    """one 2^20 x 128 segment at the RISC Zero parameters (50 queries, R = 3, 256 final coefficients): the time of the two trace kernels
    (upload, launches, the download of the chain ends) and of the whole proof, each after one warm-up call, host clock around calls that end
    in a synchronise; printed, not asserted.  The proof is verified on the host."""
    log_n, width = 20, 128
    sp = segment_params(50, 0, 8)
    t = ctx.gen_trace(SEED, 0, log_n, width)
    proof = ctx.prove_shard(t, log_n, width, [1, 2, 3], sp)
    t.free()
    v = fri16_view_shard(proof, log_n, width, [1, 2, 3], sp)
    R, F, b, Q = len(v["betas"]), v["F"], v["b"], len(v["queries"])
    assert (R, F, b, Q) == (3, 8, 2, 50)
    prm = Params(1, 50, 16)
    key = ctx.fri16_key(v, prm)
    try:
        ctx.prove_fri16(key, v, prm)                                 # warm-up (allocations, programs)
        bufs = ctx.fri16_gen_traces(v)
        t0 = time.perf_counter()
        ctx.fri16_gen_traces(v, out=(bufs[0], bufs[3]))
        t1 = time.perf_counter()
        bufs[0].free(); bufs[3].free()
        t2 = time.perf_counter()
        mproof = ctx.prove_fri16(key, v, prm)
        t3 = time.perf_counter()
        assert key.root.tolist() == fri16_key_host(v, prm).tolist()
        assert verify_fri16(mproof, [c for bt in v["betas"] for c in bt], R, F, b, Q, key.root, prm) == (0, 0)
    finally:
        key.close()
    print("fri16 machine of a 2^20 x 128 segment: %d fold rows in 2^%d, %d final rows in 2^%d; trace generation %.3f ms, whole proof %.3f ms, %d proof bytes"
          % (Q * R, bufs[1], Q << F, bufs[4], 1e3 * (t1 - t0), 1e3 * (t3 - t2), mproof.size))
