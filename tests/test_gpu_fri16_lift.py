"""The fold-by-16 LIFT machine on the GPU (zktls_amd/csrc/fri16_chip.hip, fri16_lift_tables_kernel in fri16_rows.cuh): the device's ROOTS and COEFFS main columns
against the Python restatement (tests/fri16_lift_air.py) word for word -- at the smallest and the largest tables, on random words and on edge words --, the device
key against the host key and the oracle's setup, proof bytes against the oracle's generic keyed-machine prover on the restatement's arrays, TWO segment proofs of
one shape under ONE key, the call from segment proof to lift proof, what the prover refuses before proving, and one full-size measurement beside the identity
machine."""
import time

import numpy as np
import pytest

import fri16_head_air as HA
import fri16_identity_air as IA
import fri16_lift_air as LA
from field_edges import assert_canonical, edge_canonical
from test_fri16_chip_cpu import GOLDEN, load, shape_of
from test_gpu_fri16_chip import SEED
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import (fri16_lift_key_host, fri16_view_head, fri16_view_openings, fri16_view_row_paths, fri16_view_shard, fri16_view_transcript, verify_fri16_identity,
                              verify_fri16_lift, verify_shard)

pytestmark = pytest.mark.gpu
P = 2013265921


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


def full_shape(v):
    return shape(v) + (v["pow_bits"], v["W"], len(v["pubs"]))


def full_view(proof, log_n, width, public, sp):
    """every fold-16 view of a segment proof, each from its own pass of the host verifier, in one dict: the long form of what the segment call does in one pass"""
    v, tv = fri16_view_shard(proof, log_n, width, public, sp), fri16_view_transcript(proof, log_n, width, public, sp)
    return dict(v, capacity=tv["capacity"], witness=tv["witness"], pow_bits=tv["pow_bits"], **fri16_view_openings(proof, log_n, width, public, sp),
                **fri16_view_row_paths(proof, log_n, width, public, sp), **fri16_view_head(proof, log_n, width, public, sp))


def gpu_segment(ctx, oracle, log_n, width, sp, public, shard=3):
    """a RISC Zero-shape segment proof of the synthetic AIR made on the GPU -> (proof bytes, its full view)"""
    t = oracle.gen_trace(SEED, shard, log_n, width)
    cols = ctx.from_numpy(np.ascontiguousarray(t.T))
    proof = ctx.prove_segment(cols, log_n, width, public, sp)
    cols.free()
    return proof, full_view(proof, log_n, width, public, sp)


# ------------------------------------------------------------------ (1) the device's tables = the restatement's
def compare_tables(ctx, R, F, roots, troot, qroot, final_poly):
    view = dict(roots=roots, troot=troot, qroot=qroot, final_poly=final_poly)
    lr_c = max(5, F)
    want_r, want_c = LA.roots_main(view, 0), LA.coeffs_main(view, lr_c)
    got_r, got_c = ctx.fri16_lift_gen_tables(R, F, 1, 2, roots, troot, qroot, final_poly)
    assert got_r.shape == want_r.shape == (32, 16) and got_c.shape == want_c.shape == (1 << lr_c, 8)
    assert (got_r == want_r).all(), ("ROOTS", np.argwhere(got_r != want_r)[:8])
    assert (got_c == want_c).all(), ("COEFFS", np.argwhere(got_c != want_c)[:8])
    assert not got_r[R + 2:].any() and not got_c[1 << F:].any() and not got_r[:, :8].any() and not got_c[:, :4].any()      # rows past the active ones, columns not its own: zero
    rb, cb = ctx.fri16_lift_gen_tables(R, F, 1, 2, roots, troot, qroot, final_poly, buffers=True)
    assert_canonical(rb), assert_canonical(cb)
    rb.free(), cb.free()


def draw(rng, R, F, pool=None):
    rnd = (lambda n: [int(x) for x in rng.integers(0, P, n)]) if pool is None else (lambda n: [pool[int(i)] for i in rng.integers(0, len(pool), n)])
    return [rnd(8) for _ in range(R)], rnd(8), rnd(8), [rnd(4) for _ in range(1 << F)]


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("F", [0, 1, 8])
def test_gen_tables_equal_the_python_restatement(ctx, R, F):
    """1, 2 and 256 coefficients (the smallest COEFFS, the first with a coefficient row of two, the largest); 3 and 7 active rows of ROOTS' 32"""
    compare_tables(ctx, R, F, *draw(np.random.default_rng([83, R, F]), R, F))


@pytest.mark.parametrize("R,F", [(1, 0), (5, 8)])
def test_gen_tables_on_edge_words(ctx, R, F):
    """every word 0, 1 or P - 1, as a canonical value and as the canonical value whose Montgomery word it is (so the kernel's output words are 0, 1 and P - 1)"""
    words = [0, 1, P - 1]
    pool = words + [int(x) for x in edge_canonical(words)]
    compare_tables(ctx, R, F, *draw(np.random.default_rng([89, R, F]), R, F, pool))
    for w in (0, P - 1, int(edge_canonical([P - 1])[0])):
        compare_tables(ctx, R, F, [[w] * 8] * R, [w] * 8, [w] * 8, [[w] * 4] * (1 << F))


def test_gen_tables_refuses_words_that_are_not_canonical(ctx):
    roots, troot, qroot, fp = draw(np.random.default_rng(97), 2, 1)
    with pytest.raises(ZkHipError, match="fri16_lift_gen_tables: values must be canonical"):
        ctx.fri16_lift_gen_tables(2, 1, 1, 2, [[P] + roots[0][1:], roots[1]], troot, qroot, fp)
    with pytest.raises(ZkHipError, match="fri16_lift_gen_tables: values must be canonical"):
        ctx.fri16_lift_gen_tables(2, 1, 1, 2, roots, troot, qroot, [fp[0], fp[1][:3] + [P]])
    with pytest.raises(ZkHipError, match="fri16_lift_gen_tables: the roots must be canonical"):
        ctx.fri16_lift_gen_tables(2, 1, 1, 2, roots, troot, [P] + qroot[1:], fp)


# ------------------------------------------------------------------ (2) device key = host key = oracle setup; proof bytes = the oracle's
def prove_and_compare(ctx, O, v, outer, key=None):
    R, F, b, Q, pb, W, NP = S = full_shape(v)
    main, pre, progs, tabs, pub = LA.machine(v)
    lns, ws, pws = shape_of(main, pre)
    prm, oprm = Params(*outer), O.default_params(*outer)
    own = key is None
    key = ctx.fri16_lift_key(*S, prm) if own else key
    try:
        assert key.root.tolist() == fri16_lift_key_host(*S, prm).tolist() == O.machine_setup(pre, lns, oprm).tolist()
        proof = ctx.prove_fri16_lift(key, v, prm)
        assert proof.tobytes() == O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm).tobytes()
        assert pub == [int(x) for x in v["pubs"]]
        assert verify_fri16_lift(proof, pub, R, F, b, Q, pb, W, key.root, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tabs, pub, oprm) == 0
        for k in range(len(pub)):                                # one inner public value changed
            bad = list(pub)
            bad[k] = (bad[k] + 1) % P
            assert verify_fri16_lift(proof, bad, R, F, b, Q, pb, W, key.root, prm)[0] != 0
    finally:
        if own:
            key.close()
    return proof


@pytest.mark.parametrize("outer", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_the_golden_view_equal_the_oracles(ctx, oracle, outer):
    prove_and_compare(ctx, oracle, HA.golden_view("v3_r0_9x8", GOLDEN, load), outer)


def test_proof_bytes_of_an_oracle_made_inner_proof_equal_the_oracles(ctx, oracle):
    prove_and_compare(ctx, oracle, IA.oracle_view(oracle, 1, 1, 1, 3, 40, 7, pow_bits=4), (1, 10, 2))


def test_two_gpu_segment_proofs_of_one_shape_under_one_key_and_the_segment_call(ctx, oracle):
    """2^10 x 16, 12 queries, R = 2, four final coefficients, one public value, two traces and two public values: ONE zkhip_machine_key proves both, one after the
    other; the second's bytes are what a fresh key gives (the key carries no state from proof to proof); the call from segment proof to lift proof gives the long
    form's bytes, and fails as the host verifier fails"""
    log_n, width, sp, outer = 10, 16, segment_params(12, 0, 2), (1, 12, 4)
    prm = Params(*outer)
    (p1, v1), (p2, v2) = gpu_segment(ctx, oracle, log_n, width, sp, [7], 3), gpu_segment(ctx, oracle, log_n, width, sp, [8], 4)
    S = full_shape(v1)
    assert S == full_shape(v2) == (2, 2, 2, 12, 0, 16, 1) and v1["troot"] != v2["troot"] and IA.identity_holds(v1) and IA.identity_holds(v2)
    key = ctx.fri16_lift_key(*S, prm)
    try:
        l1 = prove_and_compare(ctx, oracle, v1, outer, key)
        l2 = prove_and_compare(ctx, oracle, v2, outer, key)
        assert l1.tobytes() != l2.tobytes()
        assert verify_fri16_lift(l1, [8], *S[:6], key.root, prm)[0] != 0 and verify_fri16_lift(l2, [7], *S[:6], key.root, prm)[0] != 0
        fresh = ctx.fri16_lift_key(*S, prm)
        try:
            assert fresh.root.tolist() == key.root.tolist() and ctx.prove_fri16_lift(fresh, v2, prm).tobytes() == l2.tobytes()
        finally:
            fresh.close()
        assert ctx.prove_fri16_lift_segment(key, p1, log_n, width, [7], sp, prm).tobytes() == l1.tobytes()
        assert ctx.prove_fri16_lift_segment(key, p2, log_n, width, [8], sp, prm).tobytes() == l2.tobytes()
        bad = p1.copy()
        bad[bad.size // 2] ^= 1
        rc, _ = verify_shard(bad, log_n, width, [7], sp)
        assert rc != 0
        with pytest.raises(ZkHipError) as e:
            ctx.prove_fri16_lift_segment(key, bad, log_n, width, [7], sp, prm)
        assert e.value.code == rc
        with pytest.raises(ZkHipError) as e:                     # another public value: the transcript moves, the host verifier rejects
            ctx.prove_fri16_lift_segment(key, p1, log_n, width, [9], sp, prm)
        assert e.value.code == rc
        sp16 = Params(2, 12, 0, 0, 4, 2, 16)                     # the same shape committed with the width-16 hash
        t = ctx.gen_trace(SEED, 0, log_n, width)
        p16 = ctx.prove_shard(t, log_n, width, [7], sp16)
        t.free()
        assert verify_shard(p16, log_n, width, [7], sp16)[0] == 0
        with pytest.raises(ZkHipError, match="fri16_view_head: proofs with the width-16 hash are not taken"):
            ctx.prove_fri16_lift_segment(key, p16, log_n, width, [7], sp16, prm)
    finally:
        key.close()


# ------------------------------------------------------------------ (3) refused before anything is proven
def test_prover_refusals_each_by_its_message(ctx, oracle):
    prm = Params(1, 8, 2)
    bad = HA.honest_view(1, 1, 1, 3, 40, 7)                      # everything the head machine proves holds; no AIR holds between the columns
    v = IA.oracle_view(oracle, 1, 1, 1, 3, 40, 7, pow_bits=4)
    assert full_shape(bad) == full_shape(v)                      # (the one key serves both: the shape is the same)
    key = ctx.fri16_lift_key(*full_shape(v), prm)
    try:
        with pytest.raises(ZkHipError, match="prove_fri16_lift: the inner proof's AIR identity at zeta does not hold"):
            ctx.prove_fri16_lift(key, bad, prm)
        opened = [list(e) for e in v["opened"]]
        opened[5][2] = (opened[5][2] + 1) % P
        with pytest.raises(ZkHipError, match="prove_fri16_lift: the constant fa derived from the head of the transcript is not the view's"):
            ctx.prove_fri16_lift(key, dict(v, opened=opened), prm)
        with pytest.raises(ZkHipError, match="prove_fri16_lift: more than 30 inner public values"):
            ctx.prove_fri16_lift(key, dict(v, pubs=list(range(31))), prm)
        with pytest.raises(ZkHipError, match="width-16 hash"):
            ctx.prove_fri16_lift(key, dict(v, hash_width=16), prm)
        roots = [list(r) for r in v["roots"]]
        roots[0][3] = P                                          # a root word >= P
        with pytest.raises(ZkHipError, match="prove_fri16_lift: values must be canonical"):
            ctx.prove_fri16_lift(key, dict(v, roots=roots), prm)
        fp = [list(c) for c in v["final_poly"]]
        fp[1][0] = P + 1                                         # a coefficient word >= P
        with pytest.raises(ZkHipError, match="prove_fri16_lift: values must be canonical"):
            ctx.prove_fri16_lift(key, dict(v, final_poly=fp), prm)
        with pytest.raises(ZkHipError, match="prove_fri16_lift: the roots must be canonical"):
            ctx.prove_fri16_lift(key, dict(v, troot=[P] + list(v["troot"][1:])), prm)
        roots[0][3] = (v["roots"][0][3] + 1) % P                 # a canonical root that is not the proof's: the challenges it draws are not the view's
        with pytest.raises(ZkHipError, match="prove_fri16_lift: the challenges are not the ones the transcript draws"):
            ctx.prove_fri16_lift(key, dict(v, roots=roots), prm)
    finally:
        key.close()
    with pytest.raises(ZkHipError, match="width-24"):
        ctx.fri16_lift_key(*full_shape(v), prm, hash_width=16)


# ------------------------------------------------------------------ (4) full size, measured and printed
def test_full_size_segment_measured(ctx):
    """one 2^20 x 128 segment at the RISC Zero parameters (50 queries, R = 3, 256 final coefficients, H = 22, NP = 3), outer (1, 50, 16): after one warm-up call
    each, host clock around calls that end in a synchronise -- the lift proof beside the identity proof of the same view, the lift key beside the identity key, in
    the same process.  Single measurements; printed, not asserted.  Both proofs are verified."""
    log_n, width, public = 20, 128, [1, 2, 3]
    sp = segment_params(50, 0, 8)
    t = ctx.gen_trace(SEED, 0, log_n, width)
    proof = ctx.prove_shard(t, log_n, width, public, sp)
    t.free()
    v = full_view(proof, log_n, width, public, sp)
    R, F, b, Q, pb, W, NP = S = full_shape(v)
    assert (R, F, b, Q, W, v["H"], NP) == (3, 8, 2, 50, 128, 22, 3) and v["hash_width"] == 24
    prm = Params(1, 50, 16)
    lkey, ikey = ctx.fri16_lift_key(*S, prm), ctx.fri16_identity_key(v, prm)          # warm-up of both key calls
    try:
        ctx.prove_fri16_lift(lkey, v, prm)                           # warm-up (allocations, programs)
        ctx.prove_fri16_identity(ikey, v, prm)
        t0 = time.perf_counter()
        lproof = ctx.prove_fri16_lift(lkey, v, prm)
        t1 = time.perf_counter()
        iproof = ctx.prove_fri16_identity(ikey, v, prm)
        t2 = time.perf_counter()
        lkey2 = ctx.fri16_lift_key(*S, prm)
        t3 = time.perf_counter()
        ikey2 = ctx.fri16_identity_key(v, prm)
        t4 = time.perf_counter()
        assert lkey2.root.tolist() == lkey.root.tolist() == fri16_lift_key_host(*S, prm).tolist() and ikey2.root.tolist() == ikey.root.tolist()
        lkey2.close(); ikey2.close()
        assert verify_fri16_lift(lproof, v["pubs"], R, F, b, Q, pb, W, lkey.root, prm) == (0, 0)
        assert verify_fri16_identity(iproof, v["pubs"], R, F, b, Q, pb, W, ikey.root, prm) == (0, 0)
        assert lproof.size > iproof.size                            # the twelve main columns' openings
    finally:
        lkey.close(); ikey.close()
    print("fri16 lift machine of a 2^20 x 128 segment: lift proof %.3f ms (%d bytes), identity proof of the same view %.3f ms (%d bytes); lift key %.3f ms, identity "
          "key %.3f ms" % (1e3 * (t1 - t0), lproof.size, 1e3 * (t2 - t1), iproof.size, 1e3 * (t3 - t2), 1e3 * (t4 - t3)))
