"""The TREE above the join of fold-16 lift proofs on the GPU (zktls_amd/csrc/fri16_chip.hip: zkhip_prove_fri16_join_batch, zkhip_fri16_tree_*, zkhip_prove_fri16_tree).
GPU-made segment proofs at 2^10 x 16 with 12 queries (tests/test_gpu_fri16_join.py's shape; lift (1, 12, 4), join and top (1, 8, 2)) are lifted once per module, then:
the joins of a batch against zkhip_prove_fri16_join one by one; the tree's top against zkhip_prove_machine_verifier on the join machine's description assembled here,
under device and host witnesses (the top over joins runs machine mode's witness kernels -- mrec_chains16_kernel, mrec_rowsum_query_kernel and, from four joins on,
mrec_eval_rows_kernel -- at an inner machine of ten chips); the host check from (shape, public values, keys); padding, refusals, two logical devices."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_fri16_join import eval_log_rows
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import (InnerMachine, fri16_join_key_host, fri16_lift_inner_machine, fri16_tree_key_host, machine_verifier_describe, prove_fri16_join_batch,
                              recursion_witnesses_on_host, verify_fri16_tree, verify_machine_recursive)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5A4B544C53
LOG_N, WIDTH = 10, 16
LIFT, JOIN, TOP = Params(1, 12, 4), Params(1, 8, 2), Params(1, 8, 2)
PUBS = [[7], [8], [9], [10]]
_CASE = {}


def case(ctx, oracle):
    """four GPU-made segment proofs and their lift proofs, made once"""
    if _CASE:
        return _CASE
    sp = segment_params(12, 0, 2)
    S = ((LOG_N - int(sp.log_final)) // 4, int(sp.log_final), int(sp.log_blowup), int(sp.num_queries), int(sp.pow_bits), WIDTH, 1)      # (R, F, log_blowup, Q, grinding bits, W, NP)
    assert S == (2, 2, 2, 12, 0, 16, 1)
    lkey = ctx.fri16_lift_key(*S, LIFT)
    lifted = []
    for pub, shard in zip(PUBS, (3, 4, 5, 6)):
        cols = ctx.from_numpy(np.ascontiguousarray(oracle.gen_trace(SEED, shard, LOG_N, WIDTH).T))
        seg = ctx.prove_segment(cols, LOG_N, WIDTH, pub, sp)
        cols.free()
        lifted.append(ctx.prove_fri16_lift_segment(lkey, seg, LOG_N, WIDTH, pub, sp, LIFT))
    lkey.close()
    _CASE.update(S=S, lifted=lifted, lift_machine=fri16_lift_inner_machine(*S, LIFT))
    return _CASE


def join_machine(c, J, join_vk):
    """the join machine of (shape, join size) assembled from the public describe entry: what the fri16_tree entries build inside"""
    chips = []
    for which in range(10):
        prog, ln, mw, pw = machine_verifier_describe(c["lift_machine"], which, 0, J)
        chips.append(dict(ln=ln, W=mw, Pw=pw, prog=prog, tab=machine_verifier_describe(c["lift_machine"], which, 1, J)[0]))
    return InnerMachine(chips, join_vk, JOIN.num_queries, JOIN.pow_bits, J * c["S"][6])


def tree_of(ctx, c, lifted, pubs, J, devices=None, in_flight=4):
    """joins one by one and the top by the generic entry, then the tree in one call under device and host witnesses: every byte equal -> (top, joins, jvk, tkey root, jm)"""
    S = c["S"]
    n_joins = len(lifted) // J
    jkey = ctx.fri16_join_setup(*S, J, LIFT, JOIN)
    jvk = jkey.root.tolist()
    assert jvk == fri16_join_key_host(*S, J, LIFT, JOIN).tolist()
    jm = join_machine(c, J, jvk)
    tkey = ctx.fri16_tree_setup(*S, J, jvk, n_joins, LIFT, JOIN, TOP)
    gkey = ctx.machine_verifier_setup(jm, TOP, n_joins)
    prev = recursion_witnesses_on_host(0)
    try:
        assert tkey.root.tolist() == gkey.root.tolist() == fri16_tree_key_host(*S, J, jvk, n_joins, LIFT, JOIN, TOP).tolist()
        one = [ctx.prove_fri16_join(jkey, *S, lifted[J * j:J * j + J], pubs[J * j:J * j + J], LIFT, JOIN) for j in range(n_joins)]
        jpubs = [[v for p in pubs[J * j:J * j + J] for v in p] for j in range(n_joins)]
        want = ctx.prove_machine_verifier(gkey, jm, one, jpubs, TOP)
        top, joins = ctx.prove_fri16_tree(tkey, *S, lifted, J, pubs, jvk, LIFT, JOIN, TOP, devices=devices, in_flight=in_flight)
        assert [x.tobytes() for x in joins] == [x.tobytes() for x in one]
        assert top.tobytes() == want.tobytes()               # a shape call, not a second prover
        recursion_witnesses_on_host(1)
        htop, hjoins = ctx.prove_fri16_tree(tkey, *S, lifted, J, pubs, jvk, LIFT, JOIN, TOP, devices=devices, in_flight=in_flight)
        assert htop.tobytes() == top.tobytes() and [x.tobytes() for x in hjoins] == [x.tobytes() for x in one]      # the host's walk of every witness table
    finally:
        recursion_witnesses_on_host(prev)
        jkey.close(), gkey.close()
    return top, joins, jvk, tkey, jm


def test_four_segments_in_joins_of_two(ctx, oracle):
    c = case(ctx, oracle)
    S, lifted = c["S"], c["lifted"]
    top, joins, jvk, tkey, jm = tree_of(ctx, c, lifted, PUBS, 2)
    try:
        for in_flight in (1, 3):
            batch, bvk = prove_fri16_join_batch(lifted, 2, PUBS, *S, LIFT, JOIN, in_flight=in_flight, verify=True)
            assert bvk.tolist() == jvk and [x.tobytes() for x in batch] == [x.tobytes() for x in joins]
        flat = [v for p in PUBS for v in p]
        assert verify_fri16_tree(top, PUBS, *S, 2, jvk, 2, tkey.root, LIFT, JOIN, TOP) == (0, 0)
        assert verify_machine_recursive(jm, top, flat, tkey.root, TOP, 2) == (0, 0)
        assert verify_fri16_tree(top, [PUBS[0], PUBS[2], PUBS[1], PUBS[3]], *S, 2, jvk, 2, tkey.root, LIFT, JOIN, TOP)[0] != 0      # two segments' public values exchanged
        again, _ = ctx.prove_fri16_tree(tkey, *S, lifted, 2, PUBS, jvk, LIFT, JOIN, TOP)
        assert again.tobytes() == top.tobytes()
    finally:
        tkey.close()


def test_four_segments_in_joins_of_one_eval_rows_from_the_kernel(ctx, oracle):
    c = case(ctx, oracle)
    S, lifted = c["S"], c["lifted"]
    jm = join_machine(c, 1, [0] * 8)
    assert eval_log_rows(jm, 4) >= 16                        # 2^15 rows or more: the top's EVAL rows are mrec_eval_rows_kernel's
    assert eval_log_rows(jm, 2) == eval_log_rows(jm, 3) == 15
    top, joins, jvk, tkey, _ = tree_of(ctx, c, lifted, PUBS, 1)
    try:
        assert len(joins) == 4
        assert verify_fri16_tree(top, PUBS, *S, 1, jvk, 4, tkey.root, LIFT, JOIN, TOP) == (0, 0)
        assert verify_fri16_tree(top, [PUBS[1], PUBS[0]] + PUBS[2:], *S, 1, jvk, 4, tkey.root, LIFT, JOIN, TOP)[0] != 0
    finally:
        tkey.close()


def test_three_segments_padded_by_the_caller_and_five_refused(ctx, oracle):
    c = case(ctx, oracle)
    S, lifted = c["S"], c["lifted"]
    padded, pubs = lifted[:3] + [lifted[2]], PUBS[:3] + [PUBS[2]]
    top, joins, jvk, tkey, _ = tree_of(ctx, c, padded, pubs, 2)
    try:
        assert verify_fri16_tree(top, pubs, *S, 2, jvk, 2, tkey.root, LIFT, JOIN, TOP) == (0, 0)
        assert verify_fri16_tree(top, PUBS, *S, 2, jvk, 2, tkey.root, LIFT, JOIN, TOP)[0] != 0            # (the fourth segment is not in it)
        with pytest.raises(ZkHipError, match="prove_fri16_tree: the number of lift proofs must be a positive multiple of proofs_per_join, not 5 for joins of 2"):
            ctx.prove_fri16_tree(tkey, *S, lifted + [lifted[0]], 2, PUBS + [PUBS[0]], jvk, LIFT, JOIN, TOP)
        with pytest.raises(ZkHipError, match="prove_fri16_join_batch: the number of lift proofs must be a positive multiple of proofs_per_join, not 5 for joins of 2"):
            prove_fri16_join_batch(lifted + [lifted[0]], 2, PUBS + [PUBS[0]], *S, LIFT, JOIN)
    finally:
        tkey.close()


def test_a_bad_lift_proof_names_its_join_and_a_wrong_join_key_is_refused(ctx, oracle):
    c = case(ctx, oracle)
    S, lifted = c["S"], c["lifted"]
    jkey = ctx.fri16_join_setup(*S, 2, LIFT, JOIN)
    jvk = jkey.root.tolist()
    tkey = ctx.fri16_tree_setup(*S, 2, jvk, 2, LIFT, JOIN, TOP)
    try:
        bad = lifted[3].copy()
        bad[bad.size // 2] ^= 1
        with pytest.raises(ZkHipError) as alone:
            ctx.prove_fri16_join(jkey, *S, [lifted[2], bad], PUBS[2:], LIFT, JOIN)
        with pytest.raises(ZkHipError, match="prove_fri16_tree: join 1: .*proof 1[: ]") as e:
            ctx.prove_fri16_tree(tkey, *S, lifted[:3] + [bad], 2, PUBS, jvk, LIFT, JOIN, TOP)
        assert e.value.code == alone.value.code != 0          # machine mode's code
        with pytest.raises(ZkHipError, match="prove_fri16_join_batch: join 1: .*proof 1[: ]") as e:
            prove_fri16_join_batch(lifted[:3] + [bad], 2, PUBS, *S, LIFT, JOIN)
        assert e.value.code == alone.value.code
        other = list(jvk)
        other[2] = (other[2] + 1) % 2013265921
        with pytest.raises(ZkHipError, match="prove_fri16_tree: join_vk is not the key of joins of 2 lift proofs of this shape"):
            ctx.prove_fri16_tree(tkey, *S, lifted, 2, PUBS, other, LIFT, JOIN, TOP)
        with pytest.raises(ZkHipError, match="prove_fri16_tree: join_vk is not the key of joins of 2"):      # the key of another join size
            ctx.prove_fri16_tree(tkey, *S, lifted, 2, PUBS, fri16_join_key_host(*S, 1, LIFT, JOIN), LIFT, JOIN, TOP)
        with pytest.raises(ZkHipError, match=r"prove_fri16_tree: public_values holds n_joins x proofs_per_join x n_inner_public words in segment order \(4 here\), not 3"):
            ctx.prove_fri16_tree(tkey, *S, lifted, 2, PUBS[:3], jvk, LIFT, JOIN, TOP)
    finally:
        jkey.close(), tkey.close()


def test_the_tree_over_two_logical_devices_gives_the_same_bytes():
    """tests/checks/fri16_tree_logical.py in a fresh process: the A/B build's two logical devices on the one GPU (tests/test_gpu_multirank.py's way -- the shipped library
    has one ordinal per GPU and refuses a list that names it twice), joins dealt over [0, 1] against [0]"""
    env = dict(os.environ)
    env["ZKHIP_LOGICAL_DEVICES"] = "2"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "fri16_tree_logical.py")], env=env, cwd=ROOT, timeout=600, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert r["logical_devices"] == 2 and r["joins_over_two_devices_same_bytes"] is True and r["top_over_two_devices_same_bytes"] is True and r["top_accepted"] is True
