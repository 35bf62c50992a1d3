"""zkhip_prove_fri16_lift_batch on the GPU: every proof of a batch is the unbatched prover's bytes (zkhip_prove_fri16_lift_segment under a key made on a plain
context) -- through the lock-step lanes and through one context per worker --, the launches of a batch really merge, the shape's key stays with the pooled
contexts, one bad member fails alone, and the batch feeds the join.  Every job has its own trace seed and public values: a member that read another member's
argument slot would make other bytes.  The shapes are the smallest the lift is proven at (tests/test_gpu_fri16_lift.py)."""
import ctypes as C
import time

import numpy as np
import pytest

import fri16_identity_air as IA
from test_gpu_fri16_chip import SEED
from zktls_amd import _lib
from zktls_amd._lib import Params, segment_params
from zktls_amd.device import fri16_lift_key_host, lockstep_stats, prove_fri16_lift_batch, set_lockstep, verify_fri16_lift, verify_shard

pytestmark = pytest.mark.gpu
INVALID = -1
OUTER = Params(1, 12, 4)
# (log_n, width, segment parameters, public values per job, lift shape R F b Q pow_bits W NP)
BIG = dict(log_n=10, width=16, sp=segment_params(12, 0, 2), S=(2, 2, 2, 12, 0, 16, 1))
SMALL = dict(log_n=5, width=40, sp=Params(1, 3, 4, 0, 4, 1, 24), S=(1, 1, 1, 3, 4, 40, 7))


@pytest.fixture
def lockstep():
    yield set_lockstep
    set_lockstep(16, 6)                                       # the library's defaults


@pytest.fixture(scope="module")
def made(ctx, oracle):
    """the segments and their unbatched lift proofs, each made once: made(shape, n) -> (segment proofs, public values, lift proofs, vk) of jobs 0 .. n - 1"""
    store = {}

    def get(shape, n):
        name = "big" if shape is BIG else "small"
        segs, pubs, lifts, key = store.setdefault(name, ([], [], [], []))
        if not key:
            key.append(ctx.fri16_lift_key(*shape["S"], OUTER))
        for i in range(len(segs), n):
            if shape is BIG:                                  # a GPU segment proof of the synthetic AIR, as test_gpu_fri16_lift.gpu_segment makes it
                pub = [7 + i]
                t = oracle.gen_trace(SEED, 3 + i, shape["log_n"], shape["width"])
                cols = ctx.from_numpy(np.ascontiguousarray(t.T))
                seg = ctx.prove_segment(cols, shape["log_n"], shape["width"], pub, shape["sp"])
                cols.free()
            else:                                             # 2^5 x 40, R = 1, F = 1, grinding: the oracle's shard prover (test_gpu_fri16_lift's second shape)
                seg, log_n, pub, prm = IA.oracle_proof(oracle, 1, 1, 1, 3, 40, 7, seed=1 + i, pow_bits=4)
                assert log_n == shape["log_n"] and tuple(prm) == (1, 3, 4, 0, 4, 1, 24)
            assert verify_shard(seg, shape["log_n"], shape["width"], pub, shape["sp"])[0] == 0
            segs.append(seg); pubs.append(pub)
            lifts.append(ctx.prove_fri16_lift_segment(key[0], seg, shape["log_n"], shape["width"], pub, shape["sp"], OUTER))
        return segs[:n], pubs[:n], lifts[:n], key[0].root

    yield get
    for _, _, _, key in store.values():
        for k in key:
            k.close()


def batch(shape, segs, pubs, **kw):
    return prove_fri16_lift_batch([0], segs, shape["log_n"], shape["width"], pubs, shape["sp"], OUTER, **kw)


def check_batch(shape, segs, pubs, lifts, vk, got):
    proofs, statuses, bvk = got
    R, F, b, Q, pb, W, NP = shape["S"]
    assert statuses == [0] * len(segs)
    assert bvk.tolist() == vk.tolist() == fri16_lift_key_host(*shape["S"], OUTER).tolist()
    for i, (p, want) in enumerate(zip(proofs, lifts)):
        assert p.tobytes() == want.tobytes(), "job %d of %d: not the unbatched prover's bytes" % (i, len(segs))
        assert verify_fri16_lift(p, pubs[i], R, F, b, Q, pb, W, bvk, OUTER) == (0, 0)
        if len(segs) > 1:
            assert verify_fri16_lift(p, pubs[(i + 1) % len(segs)], R, F, b, Q, pb, W, bvk, OUTER)[0] != 0      # its neighbour's public values


@pytest.mark.parametrize("n", [1, 2, 5, 17])
def test_every_proof_of_a_batch_is_the_unbatched_provers(ctx, made, lockstep, n):
    """1: the route outside the lanes (no launch goes through a batcher); 2: the smallest batch; 5: an odd one; 17: more than one batch of 16 -- two lanes, cuts of 8 and 9"""
    segs, pubs, lifts, vk = made(BIG, n)
    if n == 17:
        lockstep(16, 2)
    s0 = lockstep_stats()
    got = batch(BIG, segs, pubs)
    s1 = lockstep_stats()
    check_batch(BIG, segs, pubs, lifts, vk, got)
    assert (s1[1] - s0[1] == 0) == (n == 1), (n, s0, s1)


def test_the_small_shape_with_grinding_and_seven_public_values(ctx, made):
    segs, pubs, lifts, vk = made(SMALL, 5)
    check_batch(SMALL, segs, pubs, lifts, vk, batch(SMALL, segs, pubs))


def test_both_routes_give_the_same_bytes(ctx, made, lockstep):
    segs, pubs, lifts, vk = made(BIG, 5)
    lockstep(0, 0)                                            # lanes off: one context per worker
    s0 = lockstep_stats()
    off = batch(BIG, segs, pubs, in_flight=2)
    assert lockstep_stats()[1] == s0[1]
    lockstep(16, 6)
    on = batch(BIG, segs, pubs)
    assert lockstep_stats()[1] > s0[1]
    check_batch(BIG, segs, pubs, lifts, vk, off)
    check_batch(BIG, segs, pubs, lifts, vk, on)


def test_the_launches_of_a_batch_merge(ctx, made, lockstep):
    """17 jobs on two lanes are batches of 8 and 9: a launch every member asks for is ONE launch per batch, so the member requests are 17 / 2 = 8.5 times the merged
    launches when nothing splits.  Members do split for a launch or two (the number of distinct layer paths is the segment's own, and the size of a copy follows it),
    and the driver may cut a rendezvous: the bound is half of what a batch of 8 gives."""
    segs, pubs, lifts, vk = made(BIG, 17)
    lockstep(16, 2)
    s0 = lockstep_stats()
    got = batch(BIG, segs, pubs)
    s1 = lockstep_stats()
    launches, requests, mixed = s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]
    print("fri16 lift batch of 17 (cuts of 8 and 9): %d member requests in %d merged launches (x %.2f; every launch shared: x %.2f), %d mixed rounds"
          % (requests, launches, requests / max(launches, 1), 17 / 2, mixed))
    check_batch(BIG, segs, pubs, lifts, vk, got)
    assert launches > 0 and requests >= launches * 8 // 2, (launches, requests, mixed)


def test_the_key_stays_with_the_pooled_contexts(ctx, made, lockstep):
    """a second call of the same shape in the same process: same bytes, and fewer member requests than the first by the key's setup (the preprocessed columns'
    LDEs and their tree), which only contexts without the shape's key run.  The pool is emptied first, so every context of the first call is fresh."""
    segs, pubs, lifts, vk = made(BIG, 5)
    _lib.load().zkhip_release_cached_contexts()
    s0 = lockstep_stats()
    t0 = time.perf_counter()
    first = batch(BIG, segs, pubs)
    t1 = time.perf_counter()
    s1 = lockstep_stats()
    second = batch(BIG, segs, pubs)
    t2 = time.perf_counter()
    s2 = lockstep_stats()
    check_batch(BIG, segs, pubs, lifts, vk, first)
    check_batch(BIG, segs, pubs, lifts, vk, second)
    r1, r2 = s1[1] - s0[1], s2[1] - s1[1]
    print("fri16 lift batch of 5, fresh contexts: %d member requests, %.1f ms; again on the pooled contexts: %d member requests, %.1f ms"
          % (r1, 1e3 * (t1 - t0), r2, 1e3 * (t2 - t1)))
    assert 0 < r2 < r1, (r1, r2)
    third = batch(BIG, segs, pubs)                            # and the requests of a keyed call do not move
    assert lockstep_stats()[1] - s2[1] == r2
    check_batch(BIG, segs, pubs, lifts, vk, third)


def test_one_bad_member_fails_alone(ctx, made):
    L = _lib.load()
    segs, pubs, lifts, vk = made(BIG, 5)
    bad = segs[2].copy()
    bad[bad.size // 2] ^= 1                                   # the host verifier refuses it: nothing of job 2 reaches the device
    rc, _ = verify_shard(bad, BIG["log_n"], BIG["width"], pubs[2], BIG["sp"])
    assert rc != 0
    with_bad = segs[:2] + [bad] + segs[3:]
    with pytest.raises(_lib.ZkHipError) as e:
        batch(BIG, with_bad, pubs)
    assert e.value.code == rc
    proofs, statuses, bvk = batch(BIG, with_bad, pubs, raise_on_error=False)
    assert statuses == [0, 0, rc, 0, 0] and proofs[2].size == 0
    assert bvk.tolist() == vk.tolist()
    for i in (0, 1, 3, 4):
        assert proofs[i].tobytes() == lifts[i].tobytes()
    # a buffer one byte short: that job alone, by message
    room = L.zkhip_fri16_lift_proof_size(*BIG["S"], C.byref(OUTER))
    assert room >= max(p.size for p in lifts)
    caps = [room] * 5
    caps[1] = room - 1
    proofs, statuses, _ = batch(BIG, segs, pubs, raise_on_error=False, proof_caps=caps)
    msg = L.zkhip_last_error()
    assert statuses == [0, INVALID, 0, 0, 0] and proofs[1].size == 0
    assert b"prove_fri16_lift_batch: proof buffer too small" in msg
    for i in (0, 2, 3, 4):
        assert proofs[i].tobytes() == lifts[i].tobytes()
    # segments committed with the width-16 hash: the view's refusal
    sp16 = Params(2, 12, 0, 0, 4, 2, 16)
    t = ctx.gen_trace(SEED, 0, BIG["log_n"], BIG["width"])
    p16 = ctx.prove_shard(t, BIG["log_n"], BIG["width"], [7], sp16)
    t.free()
    assert verify_shard(p16, BIG["log_n"], BIG["width"], [7], sp16)[0] == 0
    with pytest.raises(_lib.ZkHipError, match="fri16_view_head: proofs with the width-16 hash are not taken"):
        prove_fri16_lift_batch([0], [p16, p16], BIG["log_n"], BIG["width"], [[7], [7]], sp16, OUTER)


def test_verify_inside_the_call(ctx, made):
    segs, pubs, lifts, vk = made(BIG, 5)
    check_batch(BIG, segs, pubs, lifts, vk, batch(BIG, segs, pubs, verify=True))
    check_batch(BIG, segs[:1], pubs[:1], lifts[:1], vk, batch(BIG, segs[:1], pubs[:1], verify=True))      # (outside the lanes: checked on the worker's thread)


def test_batch_lifted_proofs_go_into_the_join(ctx, made):
    """four segments: lift batch + join = the one-call entry's bytes"""
    segs, pubs, lifts, vk = made(BIG, 4)
    proofs, statuses, _ = batch(BIG, segs, pubs)
    assert statuses == [0] * 4
    S = BIG["S"]
    lkey, jkey = ctx.fri16_lift_key(*S, OUTER), ctx.fri16_join_setup(*S, 4, OUTER, OUTER)
    try:
        joined = ctx.prove_fri16_join(jkey, *S, proofs, pubs, OUTER, OUTER)
        want = ctx.prove_fri16_join_segments(lkey, jkey, segs, BIG["log_n"], BIG["width"], pubs, BIG["sp"], OUTER, OUTER)
        assert joined.tobytes() == want.tobytes()
    finally:
        lkey.close(); jkey.close()
