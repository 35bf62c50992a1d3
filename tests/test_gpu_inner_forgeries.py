"""Forged inner proofs (tests/inner_forgeries.py) against the recursion provers on the GPU.  In the default setting the Merkle openings, the FRI layer openings and the
fold chains of an inner proof are checked by device kernels alone (csrc/hash.hip mrec_chains16_kernel and p2r_chains16_kernel, csrc/machine_verifier.inl
mrec_fold_kernel, the shard verifier's root and final comparisons): honest proofs never show what those kernels do when a check fails.  Here every forgery of the
catalogue goes through the prover under zkhip_recursion_witnesses_on_host(0) and (1): the call is refused with ZKHIP_ERR_VERIFY, the message names the forged proof
and a check of the forgery's own set; a forgery that breaks ONE check gets the same phrase under both settings; after the refusals an honest call returns the bytes
it returned before them.  tests/test_inner_forgeries_cpu.py holds the catalogue to the Python references and asserts the lanes these shapes cover."""
import time

import numpy as np
import pytest

import inner_forgeries as IF
from inner_forgery_shapes import JOIN, LIFT, LIFT_LOG_N, LIFT_WIDTH, case_factory, lift_machine, lift_shape
from zktls_amd._lib import Params, ZkHipError
from zktls_amd.device import InnerMachine, recursion_witnesses_on_host

pytestmark = pytest.mark.gpu
ERR_VERIFY = -6
OUTER = Params(1, 20, 8)


@pytest.fixture(scope="module")
def cases(oracle):
    return case_factory(oracle)


def blobs(proofs):
    return [np.frombuffer(bytes(p), dtype=np.uint8) for p in proofs]


MACHINE, SHARD = "prove_machine_verifier", "prove_shard_verifier"


def names_proof(msg, entry, p):
    """the entry's own refusal, "<entry>: proof p rejected: ..." (handed on from a proof's fill it stands behind "proof p: "), or -- the shard verifier under host
    witnesses -- the host verifier's pass over proof p handed on: "proof p: proof rejected (check N)" """
    return ("%s: proof %d rejected: " % (entry, p)) in msg or (entry == SHARD and ("proof %d: proof rejected (check " % p) in msg)


def phrase_of(msg):
    return msg.split("rejected: ")[-1] if "rejected: " in msg else msg.split(": ")[-1]


def refused(prove, proofs):
    """-> (code, message) of the refusal under the current setting"""
    with pytest.raises(ZkHipError) as e:
        prove(blobs(proofs))
    return e.value.code, str(e.value)


def run_catalogue(prove, proofs, entries, phrases, entry):
    """every forgery under both witness settings; the honest bytes before and after.  phrases: {setting: {phrase: checks}}.  Every finding is collected, so that one
    run shows them all."""
    found, seen = [], {}
    prev = recursion_witnesses_on_host(0)
    try:
        t0 = time.time()
        honest = prove(blobs(proofs)).tobytes()
        for f in entries:
            bad = [IF.forge(pr, f.off) if p == f.p else pr for p, pr in enumerate(proofs)]
            tails = []
            for setting in (0, 1):
                recursion_witnesses_on_host(setting)
                code, msg = refused(prove, bad)
                tails.append(phrase_of(msg))
                seen.setdefault((f.kind, setting), set()).add(phrase_of(msg))
                if code != ERR_VERIFY or not names_proof(msg, entry, f.p):
                    found.append(("code or proof index", f, setting, code, msg))
                elif IF.TRANSCRIPT not in f.breaks and not IF.phrase_fits(phrases[setting], msg, f.breaks):
                    found.append(("a phrase outside the set", f, setting, code, msg))
            if len(f.breaks) == 1 and IF.TRANSCRIPT not in f.breaks and tails[0] != tails[1]:
                found.append(("the settings disagree on a single check", f, tails))
        recursion_witnesses_on_host(0)
        after = prove(blobs(proofs)).tobytes()
        print("%d forgeries x 2 settings + 2 honest calls: %.2f s" % (len(entries), time.time() - t0))
        for k in sorted(seen):
            print("  %-12s setting %d: %s" % (k[0], k[1], sorted(seen[k])))
    finally:
        recursion_witnesses_on_host(prev)
    assert not found, "\n".join(repr(x) for x in found[:40])
    assert after == honest, "an honest call after the refusals returns other bytes than before them"
    return honest


def lower_proof_is_named(prove, proofs, f0, f1, phrases, entry):
    """both proofs of a join forged, f0 in proof 0 and f1 in proof 1: proof 0 is named, for f0's check, under both settings"""
    assert (f0.p, f1.p) == (0, 1)
    prev = recursion_witnesses_on_host(0)
    try:
        for setting in (0, 1):
            recursion_witnesses_on_host(setting)
            code, msg = refused(prove, [IF.forge(proofs[0], f0.off), IF.forge(proofs[1], f1.off)])
            assert code == ERR_VERIFY and names_proof(msg, entry, 0) and not names_proof(msg, entry, 1), (setting, msg)
            assert IF.phrase_fits(phrases[setting], msg, f0.breaks), (setting, msg)
    finally:
        recursion_witnesses_on_host(prev)


MACHINE_BOTH = {0: IF.MACHINE_PHRASES, 1: IF.MACHINE_PHRASES}


# ---------------------------------------------------------------------------------------------------------------- machine mode, oracle-made inner proofs
@pytest.mark.parametrize("name", ["byte", "mixed", "wide"])
def test_machine_mode_refuses_every_forgery_under_both_witness_settings(ctx, cases, name):
    """byte: two proofs x three queries of the two-chip byte machine (the shape of test_device_witnesses_and_the_hosts_walk_give_one_proof; 66 chains: a partial last
    workgroup).  mixed: two proofs x three queries of the SP1-shaped machine of four heights (injection rows, a shorter height's digest waiting in LDS, the key's tree
    shorter than the domain and checked against the key, not a proof word).  wide: two proofs x 33 queries -- (proof, query) lanes 63, 64, 65 of the fold and row-sum
    kernels on either side of their first workgroup, 41 workgroups of chains"""
    c = cases(name)
    im = InnerMachine(c.chips, c.vk, c.q, c.pb, len(c.pubs[0]))
    key = ctx.machine_verifier_setup(im, OUTER, len(c.proofs))
    try:
        run_catalogue(lambda proofs: ctx.prove_machine_verifier(key, im, proofs, c.pubs, OUTER), c.proofs, c.entries, MACHINE_BOTH, MACHINE)
    finally:
        key.close()


def test_two_forged_proofs_name_the_lower_one_and_two_forgeries_in_one_proof_are_one_refusal(ctx, cases):
    c = cases("byte")
    im = InnerMachine(c.chips, c.vk, c.q, c.pb, len(c.pubs[0]))
    key = ctx.machine_verifier_setup(im, OUTER, 2)
    prove = lambda proofs: ctx.prove_machine_verifier(key, im, proofs, c.pubs, OUTER)
    paths = [f for f in c.entries if f.kind == "commit path" and f.field[0] == "tpath"]
    layers = [f for f in c.entries if f.kind == "layer path"]
    prev = recursion_witnesses_on_host(0)
    try:
        honest = prove(blobs(c.proofs)).tobytes()
        for setting in (0, 1):
            recursion_witnesses_on_host(setting)
            # a main path digest in proof 1, a layer path digest in proof 0: proof 0 is named, with the layer's phrase
            f1, f0 = next(f for f in paths if f.p == 1), next(f for f in layers if f.p == 0)
            code, msg = refused(prove, [IF.forge(c.proofs[0], f0.off), IF.forge(c.proofs[1], f1.off)])
            assert code == ERR_VERIFY and names_proof(msg, MACHINE, 0) and "proof 1 rejected" not in msg, (setting, msg)
            assert IF.phrase_fits(IF.MACHINE_PHRASES, msg, f0.breaks), (setting, msg)
            # one opening and one layer path in proof 1, different queries: both chains refuse in one launch; whichever wrote first is reported
            a, b = next(f for f in paths if f.p == 1 and f.q == 0), next(f for f in layers if f.p == 1 and f.q == 2)
            code, msg = refused(prove, [c.proofs[0], IF.forge_many(c.proofs[1], [a.off, b.off])])
            assert code == ERR_VERIFY and names_proof(msg, MACHINE, 1), (setting, msg)
            assert IF.phrase_fits(IF.MACHINE_PHRASES, msg, a.breaks | b.breaks), (setting, msg)
        recursion_witnesses_on_host(0)
        assert prove(blobs(c.proofs)).tobytes() == honest
    finally:
        recursion_witnesses_on_host(prev)
        key.close()


# ---------------------------------------------------------------------------------------------------------------- the lift and the join: GPU-made inner proofs
@pytest.fixture(scope="module")
def lifted(ctx, oracle):
    """two GPU-made segment proofs, lifted: made once"""
    sp, S = lift_shape()
    pubs = [[7], [8]]
    lkey = ctx.fri16_lift_key(*S, LIFT)
    out = []
    for pub, shard in zip(pubs, (3, 4)):
        cols = ctx.from_numpy(np.ascontiguousarray(oracle.gen_trace(IF.SEED, shard, LIFT_LOG_N, LIFT_WIDTH).T))
        seg = ctx.prove_segment(cols, LIFT_LOG_N, LIFT_WIDTH, pub, sp)
        cols.free()
        out.append(ctx.prove_fri16_lift_segment(lkey, seg, LIFT_LOG_N, LIFT_WIDTH, pub, sp, LIFT).tobytes())
    lkey.close()
    return out, pubs


def test_the_join_refuses_a_forged_lift_proof(ctx, lifted):
    """zkhip_prove_fri16_join over two lift proofs (thirteen chips; EVAL's rows from the device kernel): a main path digest, a layer path digest and a sibling, in
    proof 0's first query and in proof 1's last"""
    proofs, pubs = lifted
    _, S = lift_shape()
    chips, vk, sh = lift_machine(2)
    lay = IF.MachineLayout(sh)
    assert all(len(p) == 4 * lay.words for p in proofs)
    entries = []
    for p, q in ((0, 0), (1, sh.Q - 1)):
        sites = IF.machine_query_sites(lay, p, q)
        entries += [next(f for f in sites if f.kind == "commit path" and f.field[0] == "tpath" and f.field[1] > 0), next(f for f in sites if f.kind == "layer path" and f.field[2] > 0),
                    next(f for f in sites if f.kind == "sibling")]
    jkey = ctx.fri16_join_setup(*S, 2, LIFT, JOIN)
    try:
        prove = lambda ps: ctx.prove_fri16_join(jkey, *S, ps, pubs, LIFT, JOIN)
        run_catalogue(prove, proofs, entries, MACHINE_BOTH, MACHINE)
        lower_proof_is_named(prove, proofs, entries[1], entries[3], MACHINE_BOTH, MACHINE)       # a layer path in proof 0, a main path in proof 1
    finally:
        jkey.close()


# ---------------------------------------------------------------------------------------------------------------- the shard verifier
@pytest.mark.parametrize("name", ["shard", "shard-air", "shard-5"])
def test_the_shard_verifier_refuses_every_forgery_under_both_witness_settings(ctx, cases, name):
    """two 2^6 x 16 shard proofs of three queries, plain and air mode (48 chains: whole workgroups of the chain kernel), and two 2^5 x 16 ones (42: a partial one).  Its chain kernel (csrc/hash.hip p2r_chains16_kernel, sixteen lanes per chain) hands every chain's root back and the
    host compares: under device witnesses a layer's path is reported like a commitment's ("an opening does not end in its root"), and the finals of the fold kernel
    are compared before the roots; under host witnesses the host's verifier pass (paths not hashed) refuses a chain's end by its reason code.  The phrases are
    recorded per setting in inner_forgeries.SHARD_PHRASES."""
    c = cases(name)
    iprm, jprm = Params(1, c.q, c.pb), Params(1, 4, 2)
    key = ctx.shard_verifier_setup(c.log_n, c.width, c.q, c.pb, 3, jprm, n_proofs=2, program=c.prog)
    try:
        prove = lambda proofs: ctx.prove_shard_verifier(key, proofs, c.log_n, c.width, c.pubs, iprm, jprm, program=c.prog)
        run_catalogue(prove, c.proofs, c.entries, IF.SHARD_PHRASES, SHARD)
        # both proofs forged: the proof index the root comparison derives from the chain's number is the LOWER one's -- a layer's chain of proof 0 (its chains stand
        # first in a proof's list) against a quotient opening of proof 1, and a quotient opening of proof 0 (the last chain of its list) against a layer of proof 1
        one = IF.single(c.entries)
        lay0, quo1 = next(f for f in one if f.p == 0 and f.kind == "layer path"), next(f for f in one if f.p == 1 and f.field[0] == "qpath")
        quo0, lay1 = next(f for f in one if f.p == 0 and f.field[0] == "qpath" and f.q == c.q - 1), next(f for f in one if f.p == 1 and f.kind == "layer path" and f.q == 0)
        lower_proof_is_named(prove, c.proofs, lay0, quo1, IF.SHARD_PHRASES, SHARD)
        lower_proof_is_named(prove, c.proofs, quo0, lay1, IF.SHARD_PHRASES, SHARD)
    finally:
        key.close()
