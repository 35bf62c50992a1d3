"""Forged inner proofs (tests/inner_forgeries.py) on the CPU: the catalogue's offsets are the fields the Python verifiers name; each forgery is refused by the
Python reference, by the library's stand-alone host verifier and by the host walk of the recursion prover (machine mode: zkhip_machine_verifier_host_tables) -- every
time for a reason that belongs to the forgery's own set of checks; and the catalogue covers what the device tests (tests/test_gpu_inner_forgeries.py) rely on.

The host walk has three forms (csrc/machine_verifier.inl fill_proof): sixteen queries in lockstep (AVX-512; a partial last group), one query after the other, and a
few threads over the queries.  Three queries reach the first two, thirty-three (groups of 16, 16 and 1; queries 0, 15, 16, 31, 32 forged) the first and the third;
zkhip_host_simd(0) switches the lockstep form off.  The forms that ran are printed."""
import numpy as np
import pytest

import inner_forgeries as IF
from inner_forgery_shapes import LIFT, case_factory, lift_machine, lift_shape
import pyref
import pyverify
import pyverify_chips
from pyverify import Reject

ERR_VERIFY = -6
MACHINES = ["byte", "mixed", "wide"]


SHARDS = ["shard", "shard-air", "shard-5"]


@pytest.fixture(scope="module")
def cases(oracle):
    return case_factory(oracle)


@pytest.fixture(scope="module")
def remembered_permutations():
    """a forged proof shares all but a few Poseidon2 permutations with the honest one: the reference's permutation (plain integers, explicit matrices) is computed
    once per input state.  The reference itself is unchanged."""
    plain, seen = pyref.poseidon2, {}

    def poseidon2(state):
        key = tuple(state)
        if key not in seen:
            seen[key] = tuple(plain(list(state)))
        return list(seen[key])
    pyref.poseidon2 = poseidon2
    yield
    pyref.poseidon2 = plain


def py_machine(c, proof, pub, view=None):
    return pyverify_chips.verify(proof, c.lns, c.widths, pub, log_blowup=1, num_queries=c.q, pow_bits=c.pb, programs=c.progs, tables=c.tabs, pre_widths=c.pws,
                                 pre_root=c.vk, view=view)


def py_shard(c, proof, pub, view=None):
    return pyverify.verify(proof, c.log_n, c.width, pub, log_blowup=1, num_queries=c.q, pow_bits=c.pb, air=c.prog, view=view)


def forged_list(c, f):
    return [IF.forge(pr, f.off) if p == f.p else pr for p, pr in enumerate(c.proofs)]


# ---------------------------------------------------------------------------------------------------------------- the offsets
@pytest.mark.parametrize("name", MACHINES)
def test_machine_offsets_are_the_fields_of_the_python_view(cases, remembered_permutations, name):
    c = cases(name)
    for p, proof in enumerate(c.proofs):
        view = {}
        assert py_machine(c, proof, c.pubs[p], view) is True
        w = IF.words_of(proof)
        assert len(w) == c.lay.words
        mine = [f for f in c.entries if f.p == p]
        assert mine
        for f in mine:
            assert w[f.off] == IF.machine_view_word(view, f), f
        assert len({f.off for f in mine}) == len(mine)                             # no site twice
        assert w[c.lay.witness] == view["witness"] and w[c.lay.cum:c.lay.cum + 4] == view["cumsum"][0] and w[c.lay.proot:c.lay.proot + 8] == view["perm_root"]


@pytest.mark.parametrize("name", SHARDS)
def test_shard_offsets_are_the_fields_of_the_python_view(cases, remembered_permutations, name):
    c = cases(name)
    for p, proof in enumerate(c.proofs):
        view = {}
        assert py_shard(c, proof, c.pubs[p], view) is True
        w = IF.words_of(proof)
        assert len(w) == c.lay.words
        mine = [f for f in c.entries if f.p == p]
        for f in mine:
            assert w[f.off] == IF.shard_view_word(view, f), f
        assert len({f.off for f in mine}) == len(mine) and w[c.lay.witness] == view["witness"]


# ---------------------------------------------------------------------------------------------------------------- the reference rejects
@pytest.mark.parametrize("proof", [0, 1])
@pytest.mark.parametrize("name", MACHINES + SHARDS)
def test_the_python_reference_rejects_every_forgery_for_a_reason_of_its_set(cases, remembered_permutations, name, proof):
    c = cases(name)
    verify = py_shard if name.startswith("shard") else py_machine
    for f in [f for f in c.entries if f.p == proof]:
        with pytest.raises(Reject) as e:
            verify(c, IF.forge(c.proofs[f.p], f.off), c.pubs[f.p])
        reason = str(e.value)
        if IF.TRANSCRIPT not in f.breaks:
            assert IF.check_of_reject(reason) in f.breaks, (f, reason)


# ---------------------------------------------------------------------------------------------------------------- the library's stand-alone host verifier
@pytest.mark.parametrize("name", MACHINES + SHARDS)
def test_the_stand_alone_host_verifier_rejects_every_forgery_for_a_reason_of_its_set(cases, name):
    from zktls_amd._lib import Params
    from zktls_amd.device import verify_machine_keyed, verify_shard, verify_shard_air
    c = cases(name)
    prm = Params(1, c.q, c.pb)

    def verdict(proof, pub):
        blob = np.frombuffer(proof, dtype=np.uint8)
        if name in ("shard", "shard-5"):
            return verify_shard(blob, c.log_n, c.width, pub, prm)
        if name == "shard-air":
            return verify_shard_air(c.prog, blob, c.log_n, c.width, pub, prm)
        return verify_machine_keyed(blob, c.lns, c.widths, c.pws, c.vk, c.progs, c.tabs, pub, prm)
    for p, proof in enumerate(c.proofs):
        assert verdict(proof, c.pubs[p]) == (0, 0)
    for f in c.entries:
        rc, why = verdict(IF.forge(c.proofs[f.p], f.off), c.pubs[f.p])
        assert rc == ERR_VERIFY, f
        if IF.TRANSCRIPT not in f.breaks:
            assert IF.check_of_code(why) in f.breaks, (f, why)


# ---------------------------------------------------------------------------------------------------------------- the prover's host walk
def walk_forms(n_queries, n_proofs):
    """the forms of the host walk this build and this CPU reach at this query count: [(zkhip_host_simd setting, name)]"""
    from zktls_amd import _lib
    forms = []
    if _lib.load().zkhip_selftest_host_simd(None, None) == 1:
        forms.append((1, "sixteen queries in lockstep (AVX-512)"))
    threads = 1 if n_proofs >= 16 else 16 // n_proofs
    forms.append((0, "one query after the other" if threads == 1 or n_queries < 4 else "a few threads over the queries"))
    return forms


@pytest.mark.parametrize("name", MACHINES)
def test_the_host_walk_names_the_proof_and_a_check_of_the_set(cases, name):
    from zktls_amd import _lib
    from zktls_amd.device import InnerMachine, machine_verifier_host_tables, machine_verifier_key_host
    c = cases(name)
    im = InnerMachine(c.chips, c.vk, c.q, c.pb, len(c.pubs[0]))
    assert machine_verifier_key_host(im, _lib.Params(1, 20, 8), len(c.proofs)).size == 8        # the machine takes this (proofs, queries) shape
    L = _lib.load()
    blobs = lambda proofs: [np.frombuffer(p, dtype=np.uint8) for p in proofs]
    prev = L.zkhip_host_simd(1)
    try:
        for setting, form in walk_forms(c.q, len(c.proofs)):
            L.zkhip_host_simd(setting)
            print("host walk, %s, Q = %d: %s; %d forgeries" % (name, c.q, form, len(c.entries)))
            assert machine_verifier_host_tables(im, blobs(c.proofs), c.pubs, 0) is not None
            for f in c.entries:
                assert machine_verifier_host_tables(im, blobs(forged_list(c, f)), c.pubs, 0) is None, f
                msg = L.zkhip_last_error().decode()
                assert "proof %d rejected: " % f.p in msg, (f, msg)
                if IF.TRANSCRIPT not in f.breaks:
                    assert IF.phrase_fits(IF.MACHINE_PHRASES, msg, f.breaks), (f, msg)
    finally:
        L.zkhip_host_simd(prev)


# ---------------------------------------------------------------------------------------------------------------- what the device tests rely on
def test_the_catalogue_covers_the_chain_kernels_lanes(cases):
    """the chain kernel gives a chain sixteen lanes: four chains to a wavefront (its refusal picks the chain's own sixteen bits out of the wavefront's ballot), sixteen
    to a workgroup.  Over the shapes the device tests run, the forgeries that break ONE commitment opening and those that break ONE layer opening each sit in every
    group of a wavefront (gid mod 4) and in the first and the last chain of a workgroup (gid mod 16); every shape forges its first chain (a commitment's) and its last
    (a layer's); and a shape's chain count is no multiple of sixteen, so its last workgroup is partial."""
    shapes = [cases(n) for n in MACHINES]
    openings = [f for c in shapes for f in IF.single(c.entries) if f.kind == "commit path"]
    layers = [f for c in shapes for f in IF.single(c.entries) if f.kind == "layer path"]
    for group in (openings, layers):
        assert {f.gid % 4 for f in group} == {0, 1, 2, 3}
        assert {0, 15} <= {f.gid % 16 for f in group}
    for c in shapes:
        mine = IF.single(c.entries)
        assert 0 in {f.gid for f in mine if f.kind == "commit path"} and c.lay.n_chains - 1 in {f.gid for f in mine if f.kind == "layer path"}
        assert all(0 <= f.gid < c.lay.n_chains for f in c.entries if f.gid is not None)
    byte, mixed, wide = shapes
    assert byte.lay.n_chains % 16 != 0                                            # (the shape of test_device_witnesses_and_the_hosts_walk_give_one_proof: no other q needed)
    assert len(mixed.sh.hs) == 4 and mixed.sh.tree_hs["E"][0] < mixed.sh.H        # injection rows; the key tree shorter than the proof's domain
    assert any(f.kind == "row word" and IF.LAYER(0) not in f.breaks for f in mixed.entries)      # rows of a shorter height: their digest is injected mid-path
    # the wide shape: (proof, query) lanes 63, 64 and the last carry a sibling forgery; many workgroups of chains
    lanes = {wide.lay.lane(f.p, f.q) for f in wide.entries if f.kind == "sibling"}
    assert wide.sh.NP * wide.sh.Q >= 66 and {63, 64, wide.sh.NP * wide.sh.Q - 1} <= lanes and wide.lay.n_chains > 16 * 16
    # the shard verifier's chain list: its chain kernel has the same sixteen-lane form (csrc/hash.hip p2r_chains16_kernel)
    # (two proofs of three queries at 2^6: 48 chains, whole workgroups; at 2^5: 42, a partial last one).  Each class, as above
    shards = [cases(n) for n in SHARDS]
    for kind in ("commit path", "layer path"):
        group = [f for c in shards for f in IF.single(c.entries) if f.kind == kind]
        assert {f.gid % 4 for f in group} == {0, 1, 2, 3} and {0, 15} <= {f.gid % 16 for f in group}, kind
    for c in shards:
        one = IF.single(c.entries)
        assert 0 in {f.gid for f in one if f.kind == "layer path"} and c.lay.n_chains - 1 in {f.gid for f in one if f.kind == "commit path"}
    assert [c.lay.n_chains % 16 for c in shards] == [0, 0, 10]
    print("forgeries per shape: " + ", ".join("%s %d" % (n, len(cases(n).entries)) for n in MACHINES + SHARDS))


def test_the_lift_machines_layout_has_the_length_of_a_lift_proof():
    """the device tests forge GPU-made lift proofs (thirteen chips): the catalogue's layout of that machine, from the library's description of it, ends where the
    library says a lift proof ends"""
    import ctypes as C
    from zktls_amd import _lib
    _, S = lift_shape()
    chips, vk, sh = lift_machine(2)
    lay = IF.MachineLayout(sh)
    L = _lib.load()
    L.zkhip_fri16_lift_proof_size.restype = C.c_size_t
    assert 4 * lay.words == L.zkhip_fri16_lift_proof_size(*S[:4], S[4], S[5], S[6], C.byref(LIFT))
    sites = IF.machine_query_sites(lay, 1, sh.Q - 1)
    assert max(f.off for f in sites) < lay.words and lay.layer_gid(1, sh.Q - 1, sh.R - 1) == lay.n_chains - 1
