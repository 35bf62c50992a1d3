"""The fold-by-16 IDENTITY machine on the GPU (zktls_amd/csrc/fri16_chip.hip, fri16_identity_rows_kernel in fri16_rows.cuh): the device's AIR16 and SCALARS16 tables
and the two accumulators against the Python restatement (tests/fri16_identity_air.py) word for word from random inputs -- at the group counts inside, filling and
straddling a wave of 64 lanes, two waves and the full workgroup of 256, at 26 squarings, and on edge words --, the device key against the host key and the oracle's
setup, proof bytes against the oracle's generic keyed-machine prover on the restatement's arrays, what the prover refuses before proving, and one full-size
measurement beside the head machine."""
import time

import numpy as np
import pytest

import fri16_head_air as HA
import fri16_identity_air as IA
from field_edges import edge_canonical
from test_fri16_chip_cpu import GOLDEN, load, shape_of
from test_gpu_fri16_chip import SEED
from test_gpu_fri16_head import head_view_of_a_gpu_proof
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import (fri16_head_key_host, fri16_identity_key_host, fri16_view_head, fri16_view_openings, fri16_view_row_paths, fri16_view_shard,
                              fri16_view_transcript, verify_fri16_head, verify_fri16_identity)

pytestmark = pytest.mark.gpu
P = 2013265921
RAW = (2, 0, 1, 2)                                            # R, F, log_blowup, Q of the raw tests: n = 8 squarings
DEEP = (5, 6, 1, 1)                                           # n = 26 squarings, the most a fold-16 shape has
# G = W / 4 groups: 2, 4; 62 / 64 / 66 inside, filling and straddling a wave; 126 / 128 / 130 two waves; 254 / 256 the full workgroup
WIDTHS = [8, 16, 248, 256, 264, 504, 512, 520, 1016, 1024]
NP = 3


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


def compare_with_the_restatement(ctx, S, W, alpha, zeta, opened):
    R, F, b, Q = S
    n = 4 * R + F
    amain, acco = IA.air16_main(opened, alpha, zeta, W, n)
    smain, prod = IA.scalars16_main(opened, alpha, zeta, W, n)
    air, sc, accs = ctx.fri16_identity_gen_traces(R, F, b, Q, 4, W, NP, alpha, zeta, opened)
    assert air.shape == amain.shape == (1 << max(6, (W // 4 - 1).bit_length()), 56) and sc.shape == smain.shape == (128, 4 * (17 + n))
    assert (air == amain).all(), ("AIR16", np.argwhere(air != amain)[:8])
    assert (sc == smain).all(), ("SCALARS16", np.argwhere(sc != smain)[:8])
    assert accs.tolist() == [acco, prod]
    return acco, prod


def random_inputs(rng, W, pool=None):
    rnd = (lambda n: [int(x) for x in rng.integers(0, P, n)]) if pool is None else (lambda n: [pool[int(i)] for i in rng.integers(0, len(pool), n)])
    return rnd(4), rnd(4), [rnd(4) for _ in range(2 * W + 8)]


# ------------------------------------------------------------------ (1) the device's tables and accumulators = the restatement's
@pytest.mark.parametrize("W", WIDTHS)
def test_gen_traces_equal_the_python_restatement(ctx, W):
    compare_with_the_restatement(ctx, RAW, W, *random_inputs(np.random.default_rng([53, W]), W))


def test_gen_traces_at_26_squarings(ctx):
    compare_with_the_restatement(ctx, DEEP, 8, *random_inputs(np.random.default_rng(59), 8))


@pytest.mark.parametrize("W", [8, 264, 1024])
def test_gen_traces_on_edge_words(ctx, W):
    """every input drawn from the words 0, 1, P - 1, (P - 1) / 2, (P + 1) / 2 -- as canonical values and as the canonical values whose Montgomery words they are"""
    words = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]
    pool = words + [int(x) for x in edge_canonical(words)]
    compare_with_the_restatement(ctx, RAW, W, *random_inputs(np.random.default_rng([61, W]), W, pool))


def test_gen_traces_on_all_zero_and_all_p_minus_1_opened_values(ctx):
    alpha, zeta, _ = random_inputs(np.random.default_rng(67), 16)
    acco, prod = compare_with_the_restatement(ctx, RAW, 16, alpha, zeta, [[0] * 4] * 40)
    assert prod == [0, 0, 0, 0] and acco != [0, 0, 0, 0]             # no quotient; the constants K1 .. K3 alone in the fold
    compare_with_the_restatement(ctx, RAW, 16, alpha, zeta, [[P - 1] * 4] * 40)
    compare_with_the_restatement(ctx, RAW, 520, alpha, zeta, [[P - 1] * 4] * 1048)


def test_gen_traces_refuses_bad_arguments(ctx):
    R, F, b, Q = RAW
    alpha, zeta, opened = random_inputs(np.random.default_rng(71), 16)
    with pytest.raises(ZkHipError, match="the opened values must be canonical"):
        ctx.fri16_identity_gen_traces(R, F, b, Q, 4, 16, NP, alpha, zeta, [[P, 0, 0, 0]] + opened[1:])
    with pytest.raises(ZkHipError, match="the challenges must be canonical"):
        ctx.fri16_identity_gen_traces(R, F, b, Q, 4, 16, NP, [P] + alpha[1:], zeta, opened)
    with pytest.raises(ZkHipError, match="zeta is 1"):
        ctx.fri16_identity_gen_traces(R, F, b, Q, 4, 16, NP, alpha, [1, 0, 0, 0], opened)


# ------------------------------------------------------------------ (2) device key = host key = oracle setup; proof bytes = the oracle's
def prove_and_compare(ctx, O, v, outer):
    R, F, b, Q = shape(v)
    pb, W = v["pow_bits"], v["W"]
    main, pre, progs, tabs, pub = IA.machine(v)
    lns, ws, pws = shape_of(main, pre)
    prm, oprm = Params(*outer), O.default_params(*outer)
    key = ctx.fri16_identity_key(v, prm)
    try:
        assert key.root.tolist() == fri16_identity_key_host(v, prm).tolist() == O.machine_setup(pre, lns, oprm).tolist()
        proof = ctx.prove_fri16_identity(key, v, prm)
        assert proof.tobytes() == O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm).tobytes()
        assert pub == [int(x) for x in v["pubs"]]
        assert verify_fri16_identity(proof, pub, R, F, b, Q, pb, W, key.root, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tabs, pub, oprm) == 0
        for k in range(len(pub)):                                # one inner public value changed
            bad = list(pub)
            bad[k] = (bad[k] + 1) % P
            assert verify_fri16_identity(proof, bad, R, F, b, Q, pb, W, key.root, prm)[0] != 0
    finally:
        key.close()
    return proof


@pytest.mark.parametrize("outer", [(1, 12, 4), (2, 7, 0)])
def test_proof_bytes_of_the_golden_view_equal_the_oracles(ctx, oracle, outer):
    prove_and_compare(ctx, oracle, HA.golden_view("v3_r0_9x8", GOLDEN, load), outer)


def test_proof_bytes_of_an_oracle_made_inner_proof_equal_the_oracles(ctx, oracle):
    """W = 40, NP = 7: ten groups, an inner proof the oracle's shard prover makes here"""
    prove_and_compare(ctx, oracle, IA.oracle_view(oracle, 1, 1, 1, 3, 40, 7, pow_bits=4), (1, 10, 2))


def test_proof_bytes_of_a_gpu_segment_proofs_view(ctx, oracle):
    """2^10 x 16, 12 queries, R = 2, four final coefficients, one public value, made on the GPU"""
    v = head_view_of_a_gpu_proof(ctx, oracle, 10, 16, segment_params(12, 0, 2), [7])
    assert shape(v) == (2, 2, 2, 12) and v["W"] == 16 and IA.identity_holds(v)
    prove_and_compare(ctx, oracle, v, (1, 12, 4))


# ------------------------------------------------------------------ (3) refused before anything is proven
def test_prover_refuses_columns_that_satisfy_no_air_and_a_tampered_opened_value(ctx, oracle):
    prm = Params(1, 8, 2)
    bad = HA.honest_view(1, 1, 1, 3, 40, 7)                      # everything the head machine proves holds; no AIR holds between the columns
    key = ctx.fri16_identity_key(bad, prm)
    try:
        with pytest.raises(ZkHipError, match="prove_fri16_identity: the inner proof's AIR identity at zeta does not hold"):
            ctx.prove_fri16_identity(key, bad, prm)
    finally:
        key.close()
    hkey = ctx.fri16_head_key(bad, prm)                          # ... and the head machine proves that very view
    try:
        R, F, b, Q = shape(bad)
        assert verify_fri16_head(ctx.prove_fri16_head(hkey, bad, prm), bad["pubs"], R, F, b, Q, bad["pow_bits"], bad["W"], hkey.root, prm) == (0, 0)
    finally:
        hkey.close()
    v = IA.oracle_view(oracle, 1, 1, 1, 3, 40, 7, pow_bits=4)
    key = ctx.fri16_identity_key(v, prm)
    try:
        opened = [list(e) for e in v["opened"]]
        opened[5][2] = (opened[5][2] + 1) % P                    # the challenges the head derives move with it: refused as the head prover refuses it
        with pytest.raises(ZkHipError, match="prove_fri16_identity: the constant fa derived from the head of the transcript is not the view's"):
            ctx.prove_fri16_identity(key, dict(v, opened=opened), prm)
        with pytest.raises(ZkHipError, match="prove_fri16_identity: more than 30 inner public values"):
            ctx.prove_fri16_identity(key, dict(v, pubs=list(range(31))), prm)
        with pytest.raises(ZkHipError, match="width-16 hash"):
            ctx.prove_fri16_identity(key, dict(v, hash_width=16), prm)
    finally:
        key.close()


# ------------------------------------------------------------------ (4) full size, measured and printed
def test_full_size_segment_measured(ctx):
    """one 2^20 x 128 segment at the RISC Zero parameters (50 queries, R = 3, 256 final coefficients, H = 22; 32 groups, 20 squarings), outer (1, 50, 16): after one
    warm-up call each, host clock around calls that end in a synchronise -- the two identity tables alone, the whole identity proof, and the head machine's proof of
    the same view in the same process (the difference is what the identity costs).  Single measurements; printed, not asserted.  Both proofs are verified."""
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
    prm = Params(1, 50, 16)
    h = HA.head_of(v)
    ikey, hkey = ctx.fri16_identity_key(v, prm), ctx.fri16_head_key(v, prm)
    args = (R, F, b, Q, v["pow_bits"], v["W"], len(v["pubs"]), h["alpha"], h["zeta"], v["opened"])
    try:
        ctx.prove_fri16_identity(ikey, v, prm)                       # warm-up (allocations, programs)
        ctx.prove_fri16_head(hkey, v, prm)
        ctx.fri16_identity_gen_traces(*args)
        t0 = time.perf_counter()
        traces = ctx.fri16_identity_gen_traces(*args)
        t1 = time.perf_counter()
        iproof = ctx.prove_fri16_identity(ikey, v, prm)
        t2 = time.perf_counter()
        hproof = ctx.prove_fri16_head(hkey, v, prm)
        t3 = time.perf_counter()
        assert traces[2][0].tolist() == traces[2][1].tolist()        # the identity holds: the two accumulators are one value
        assert ikey.root.tolist() == fri16_identity_key_host(v, prm).tolist() and hkey.root.tolist() == fri16_head_key_host(v, prm).tolist()
        assert verify_fri16_identity(iproof, v["pubs"], R, F, b, Q, v["pow_bits"], v["W"], ikey.root, prm) == (0, 0)
        assert verify_fri16_head(hproof, v["pubs"], R, F, b, Q, v["pow_bits"], v["W"], hkey.root, prm) == (0, 0)
    finally:
        ikey.close(); hkey.close()
    print("fri16 identity machine of a 2^20 x 128 segment: 32 AIR16 groups, 20 squarings; the two identity tables (with their downloads) %.3f ms, whole identity proof "
          "%.3f ms (%d bytes); the head machine's proof of the same view %.3f ms (%d bytes)" % (1e3 * (t1 - t0), 1e3 * (t2 - t1), iproof.size, 1e3 * (t3 - t2), hproof.size))
