"""The width-24 Poseidon2 chip on the GPU: the on-device trace generator against the Python restatement (tests/poseidon2_24_air.py), proof
bytes against the oracle in both proof shapes, and openings of real RISC Zero-shape commitments proven in-circuit: a segment proof's trace
commitment and a matrix committed with zkhip_merkle_commit_p24_colmajor."""
import time

import numpy as np
import pytest

import poseidon2_24_air as A
import pyverify
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import p24chip_air, verify_merkle_paths_p24

pytestmark = pytest.mark.gpu
SEED = 0x5A4B544C53
R0_SHAPE = (2, 4, 0, 0, 4, 1, 24)           # blowup 4, fold 16, Poseidon2 width 24
P = 2013265921


def r0_shape(log_n, queries=4):
    """the RISC Zero shape (blowup 4, fold 16, Poseidon2 width 24) for a chip trace of 2^log_n rows: the final polynomial takes what folding
    by 16 leaves"""
    return (2, queries, 0, 0, 4, log_n % 4, 24)


def trace_log_n(n_paths, depth, row_width):
    return max(5, (n_paths * ((row_width + 15) // 16 + depth) - 1).bit_length())


@pytest.mark.parametrize("case", [(3, 0, 4, 1), (5, 4, 3, 2), (4, 8, 5, 3), (2, 12, 6, 4), (6, 16, 3, 5), (3, 28, 4, 6), (4, 64, 3, 7),
                                  (10, 20, 5, 8)])
def test_trace_equals_the_python_restatement(ctx, case):
    depth, row_width, n_paths, seed = case
    leaves, sibs, idx, root = A.sparse_tree_paths(depth, n_paths, row_width, seed)
    trace, roots = A.merkle_trace(leaves, sibs, idx, row_width=row_width)
    d, droots, log_n = ctx.p24chip_gen_merkle_trace(np.array(leaves, dtype=np.uint32), np.array(sibs, dtype=np.uint32), np.array(idx, dtype=np.uint32),
                                                    row_width=row_width)
    assert log_n == trace.shape[0].bit_length() - 1
    assert (droots == np.array(roots, dtype=np.uint32)).all() and all(r == root for r in roots)
    assert (d.download().reshape(-1, A.WIDTH) == trace).all()
    d.free()


@pytest.mark.parametrize("shape", [(1, 8, 4), R0_SHAPE])
def test_proof_bytes_equal_the_oracles(ctx, oracle, shape):
    O = oracle
    leaves, sibs, idx, root = A.sparse_tree_paths(4, 5, 20, 11)
    trace, _ = A.merkle_trace(leaves, sibs, idx, row_width=20)
    prm, oprm = Params(*shape), O.default_params(*shape)
    lv, sb, ix = np.array(leaves, dtype=np.uint32), np.array(sibs, dtype=np.uint32), np.array(idx, dtype=np.uint32)
    proof = ctx.prove_merkle_paths_p24(lv, sb, ix, root, prm, row_width=20)
    log_n = trace.shape[0].bit_length() - 1
    assert proof.tobytes() == O.prove_shard_air(A.program(), trace, root + [5], oprm).tobytes()
    assert verify_merkle_paths_p24(proof, root, 5, prm) == (0, 0)
    assert O.verify_shard_air(A.program(), proof, log_n, A.WIDTH, root + [5], oprm) == 0
    assert pyverify.verify(proof.tobytes(), log_n, A.WIDTH, root + [5], *shape, air=A.program()) is True
    # a path that does not end in the root is refused before anything is proven
    wrong = sb.copy()
    wrong[2, 1, 0] = (int(wrong[2, 1, 0]) + 1) % P
    with pytest.raises(ZkHipError):
        ctx.prove_merkle_paths_p24(lv, wrong, ix, root, prm, row_width=20)


def segment_openings(proof, log_n, width, public, prm_tuple):
    v = {}
    assert pyverify.verify(proof.tobytes(), log_n, width, public, *prm_tuple, view=v) is True
    ops = v["openings"]
    return (np.array([o["trow"] for o in ops], dtype=np.uint32), np.array([o["tpath"] for o in ops], dtype=np.uint32),
            np.array([o["index"] for o in ops], dtype=np.uint32), np.array(v["trace_root"], dtype=np.uint32),
            np.array([o["qrow"] for o in ops], dtype=np.uint32), np.array([o["qpath"] for o in ops], dtype=np.uint32), np.array(v["quot_root"], dtype=np.uint32))


def test_openings_of_a_segment_proof_in_circuit(ctx, oracle):
    """a RISC Zero-shape segment proof made on the GPU (2^10 x 16, column-major): every trace-commitment opening its verifier checks,
    proven through the chip against the proof's trace root"""
    log_n, width, lf = 10, 16, 6
    t = oracle.gen_trace(SEED, 3, log_n, width)
    cols = ctx.from_numpy(np.ascontiguousarray(t.T))
    sp = segment_params(50, 0, lf)
    proof = ctx.prove_segment(cols, log_n, width, [7], sp)
    shape = (sp.log_blowup, sp.num_queries, sp.pow_bits, sp.logup_pairs, sp.log_fold, sp.log_final, sp.hash_width)
    rows_, sibs, idx, troot, _, _, _ = segment_openings(proof, log_n, width, [7], shape)
    assert rows_.shape == (50, width) and sibs.shape == (50, log_n + 2, 8)
    cl = trace_log_n(50, log_n + 2, width)
    prm = Params(*r0_shape(cl))
    cproof = ctx.prove_merkle_paths_p24(rows_, sibs, idx, troot, prm, row_width=width)
    assert verify_merkle_paths_p24(cproof, troot, 50, prm) == (0, 0)
    assert pyverify.verify(cproof.tobytes(), cl, A.WIDTH, troot.tolist() + [50], *r0_shape(cl), air=p24chip_air()) is True
    # one opened value changed: the prover refuses
    bad = rows_.copy()
    bad[17, 5] = (int(bad[17, 5]) + 1) % P
    with pytest.raises(ZkHipError):
        ctx.prove_merkle_paths_p24(bad, sibs, idx, troot, prm, row_width=width)


def test_openings_of_a_hal_commitment_in_circuit(ctx, oracle):
    """zkhip_merkle_commit_p24_colmajor over a 2^12 x 20 matrix (rows of 20: a full block and a partial one); openings of several rows,
    read column-wise, proven against its root"""
    log_rows, cols = 12, 20
    rng = np.random.default_rng(12)
    m = rng.integers(0, P, (cols, 1 << log_rows)).astype(np.uint32)       # column-major: [cols][rows]
    tree = ctx.merkle_commit_p24_colmajor(ctx.from_numpy(m), cols, log_rows).download().reshape(-1, 8)
    assert (tree == oracle.merkle_tree_p24_colmajor(m)).all()
    levels, off = [], 0
    for l in range(log_rows + 1):
        levels.append(tree[off:off + (1 << (log_rows - l))])
        off += 1 << (log_rows - l)
    root = levels[-1][0]
    idx = rng.integers(0, 1 << log_rows, 24).astype(np.uint32)
    rows_ = np.ascontiguousarray(m[:, idx].T)
    sibs = np.stack([levels[l][(idx >> l) ^ 1] for l in range(log_rows)], axis=1)
    prm = Params(1, 20, 8)
    proof = ctx.prove_merkle_paths_p24(rows_, sibs, idx, root, prm, row_width=cols)
    assert verify_merkle_paths_p24(proof, root, 24, prm) == (0, 0)
    cl = trace_log_n(24, log_rows, cols)
    assert oracle.verify_shard_air(p24chip_air(), proof, cl, A.WIDTH, root.tolist() + [24], oracle.default_params(1, 20, 8)) == 0
    assert verify_merkle_paths_p24(proof, root, 23, prm)[0] != 0


def test_openings_of_a_full_size_segment_measured(ctx):
    """the openings of one 2^20 x 128 segment (50 queries; trace and quotient commitments) proven once; the split between trace generation and
    the rest of the proof is printed, not asserted"""
    log_n, width = 20, 128
    sp = segment_params(50, 0, 8)
    t = ctx.gen_trace(SEED, 0, log_n, width)
    proof = ctx.prove_shard(t, log_n, width, [1, 2, 3], sp)
    t.free()
    shape = (sp.log_blowup, sp.num_queries, sp.pow_bits, sp.logup_pairs, sp.log_fold, sp.log_final, sp.hash_width)
    trows, tsibs, idx, troot, qrows, qsibs, qroot = segment_openings(proof, log_n, width, [1, 2, 3], shape)
    for name, rows_, sibs, root in (("trace", trows, tsibs, troot), ("quotient", qrows, qsibs, qroot)):
        rw = rows_.shape[1]
        prm = Params(*r0_shape(trace_log_n(len(idx), sibs.shape[1], rw), 50))
        ctx.prove_merkle_paths_p24(rows_, sibs, idx, root, prm, row_width=rw)             # warm-up (allocations, program)
        t0 = time.perf_counter()
        d, roots, ln = ctx.p24chip_gen_merkle_trace(rows_, sibs, idx, row_width=rw)
        t1 = time.perf_counter()
        d.free()
        assert (roots == root).all()
        t2 = time.perf_counter()
        cproof = ctx.prove_merkle_paths_p24(rows_, sibs, idx, root, prm, row_width=rw)
        t3 = time.perf_counter()
        assert verify_merkle_paths_p24(cproof, root, len(idx), prm) == (0, 0)
        used = len(idx) * ((rw + 15) // 16 + sibs.shape[1])
        print("p24chip %s openings of a 2^20 x 128 segment: %d paths, row width %d, %d rows used of 2^%d; trace generation %.3f ms, "
              "whole proof %.3f ms (prove_shard_air part ~%.3f ms)" % (name, len(idx), rw, used, ln, 1e3 * (t1 - t0), 1e3 * (t3 - t2), 1e3 * ((t3 - t2) - (t1 - t0))))
