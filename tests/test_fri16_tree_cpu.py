"""The TREE above the join of fold-16 lift proofs (zktls_amd/csrc/fri16_chip.hip: zkhip_prove_fri16_join_batch, zkhip_fri16_tree_*, zkhip_prove_fri16_tree,
zkhip_verify_fri16_tree -- shape calls over machine mode, one level above the zkhip_fri16_join_* entries), CPU side: the symbols and prototypes against the binding; the
top's key against zkhip_machine_verifier_key_host on the join machine's description assembled HERE from zkhip_machine_verifier_describe with the join's key as root; the
key as a function of the join size, the number of joins and the join's key; the two bounds against a search over zkhip_machine_verifier_proof_size on the assembled
description; every refusal by its message; and ONE TREE END TO END WITHOUT A GPU -- the two oracle lift proofs of tests/test_fri16_join_cpu.py's case, two joins of one
proof each and the top over them proven by the oracle from zkhip_machine_verifier_host_tables, zkhip_verify_fri16_tree on (shape, public values, keys)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import recursion_machine as RM
import test_fri16_join_cpu as TJ
import test_fri16_lift_cpu as TL
from zktls_amd import _lib, device
from zktls_amd._lib import Params
from zktls_amd.device import (InnerMachine, fri16_join_key_host, fri16_join_max_proofs, fri16_lift_inner_machine, fri16_tree_key_host, fri16_tree_max_join,
                              fri16_tree_max_joins, fri16_tree_proof_size, machine_verifier_describe, machine_verifier_host_tables, machine_verifier_key_host,
                              prove_fri16_join_batch, verify_fri16_tree)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = TJ.P
LIFT, JOIN, TOP = TJ.LIFT, TJ.JOIN, (1, 3, 0)               # the twin lift proofs' outer parameters, the joins', the top's
SMALL = (2, 2, 2, 12, 0, 16, 1)                              # (R, F, b, Q, grinding bits, W, NP): 2^10 x 16 segments with 12 queries, tests/test_gpu_fri16_tree.py's shape
SMALL_PRM = ((1, 12, 4), (1, 8, 2), (1, 8, 2))               # its lift, join and top parameters
FULL = (3, 8, 2, 50, 0, 128, 9)                              # 2^20 x 128 segments at ZKHIP_PARAMS_RISC0
FULL_PRM = ((1, 100, 16),) * 3
NAMES = ["zkhip_prove_fri16_join_batch", "zkhip_fri16_tree_max_join", "zkhip_fri16_tree_max_joins", "zkhip_fri16_tree_key_host", "zkhip_fri16_tree_setup",
         "zkhip_fri16_tree_proof_size", "zkhip_prove_fri16_tree", "zkhip_verify_fri16_tree"]
SHAPE8 = ["R", "F", "log_blowup", "n_queries", "inner_hash_width", "inner_pow_bits", "trace_width", "n_inner_public"]
TREE7 = ["lift_prm", "proofs_per_join", "join_prm", "join_vk", "n_joins", "top_prm"]
WANT = {
    "zkhip_prove_fri16_join_batch": ["devices", "n_devices"] + SHAPE8 + ["lift_prm", "lift_proofs", "lens", "n_proofs", "proofs_per_join", "public_values", "n_public_total",
                                                                         "join_prm", "in_flight_per_device", "verify", "joined", "joined_stride", "joined_lens", "vk"],
    "zkhip_fri16_tree_max_join": SHAPE8 + ["lift_prm", "join_prm"],
    "zkhip_fri16_tree_max_joins": SHAPE8 + ["lift_prm", "proofs_per_join", "join_prm"],
    "zkhip_fri16_tree_key_host": SHAPE8 + TREE7 + ["vk"],
    "zkhip_fri16_tree_setup": ["ctx"] + SHAPE8 + TREE7 + ["key", "vk"],
    "zkhip_fri16_tree_proof_size": SHAPE8 + TREE7,
    "zkhip_prove_fri16_tree": ["ctx", "top_key"] + SHAPE8 + ["lift_prm", "devices", "n_devices", "lift_proofs", "lens", "n_proofs", "proofs_per_join", "public_values",
                                                            "n_public_total", "join_prm", "join_vk", "top_prm", "in_flight_per_device", "joined", "joined_stride", "joined_lens",
                                                            "out", "cap", "len"],
    "zkhip_verify_fri16_tree": SHAPE8 + ["lift_prm", "proofs_per_join", "join_prm", "join_vk", "n_joins", "proof", "len", "public_values", "n_public_total", "top_vk", "top_prm",
                                         "reason"],
}
_DESC, _CASE = {}, {}


def last_error():
    return _lib.load().zkhip_last_error().decode()


def prm(t):
    return Params(*t)


def join_machine(S, J, join_vk, lift, join):
    """the JOIN machine of (shape, join size) as an InnerMachine, put together HERE: the ten chips machine mode describes over the lift machine at n_proofs = J, the
    join's key as root, the join's queries and proof-of-work bits, J x NP public values -- what the fri16_tree entries build inside"""
    k = (S, lift, J)
    if k not in _DESC:
        im = fri16_lift_inner_machine(*S, prm(lift))
        chips = []
        for which in range(10):
            prog, ln, mw, pw = machine_verifier_describe(im, which, 0, J)
            chips.append(dict(ln=ln, W=mw, Pw=pw, prog=prog, tab=machine_verifier_describe(im, which, 1, J)[0]))
        _DESC[k] = chips if all(c["prog"].size for c in chips) else None
    chips = _DESC[k]
    return InnerMachine(chips, join_vk, join[1], join[2], J * S[6]) if chips else None


def takes(S, J, n_joins, lift, join, top):
    jm = join_machine(S, J, [0] * 8, lift, join)
    return jm is not None and _lib.load().zkhip_machine_verifier_proof_size(jm.desc, n_joins, C.byref(prm(top))) > 0


def largest(ok, hi):
    """the largest n in 1 .. hi with ok(n), by bisection (what is bounded grows with n); 0: not even 1"""
    if not ok(1):
        return 0
    lo = 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


# ------------------------------------------------------------------ (1) the symbols
def test_exports_prototypes_and_python_signatures_agree():
    L = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zkhip_chips.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
        assert m, "include/zkhip_chips.h does not declare " + name
        args = [a.strip() for a in m.group(2).split(",")]
        assert [re.sub(r"\[.*?\]", "", a).split()[-1].lstrip("*") for a in args] == WANT[name], name
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(args), name
        for a, t in zip(args, fn.argtypes):
            assert ("*" in a or "[" in a) == (hasattr(t, "contents") or t is C.c_void_p), (name, a)      # pointers face pointers, position by position
            if "size_t" in a and "*" not in a:
                assert t is C.c_size_t, (name, a)
        assert (fn.restype is C.c_size_t) == (m.group(1) == "size_t"), name
    assert "STILL OUTSIDE: a tree above the join" not in open(os.path.join(ROOT, "include", "zkhip_chips.h")).read()
    # the Python entries named after them
    shape = ["R", "F", "log_blowup", "n_queries", "pow_bits", "W", "NP"]
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(device.prove_fri16_join_batch)[:3] == ["lift_proofs", "proofs_per_join", "public_values"] and par(device.prove_fri16_join_batch)[3:10] == shape
    assert par(device.fri16_tree_max_join)[:7] == shape and par(device.fri16_tree_max_joins)[:8] == shape + ["proofs_per_join"]
    for f in (device.fri16_tree_key_host, device.fri16_tree_proof_size):
        assert par(f)[:10] == shape + ["proofs_per_join", "join_vk", "n_joins"]
    assert par(device.verify_fri16_tree)[:13] == ["proof", "public_values"] + shape + ["proofs_per_join", "join_vk", "n_joins", "top_vk"]
    assert par(device.Context.fri16_tree_setup)[1:11] == shape + ["proofs_per_join", "join_vk", "n_joins"]
    assert par(device.Context.prove_fri16_tree)[1:13] == ["top_key"] + shape + ["lift_proofs", "proofs_per_join", "public_values", "join_vk"]


# ------------------------------------------------------------------ (2) the key
def test_tree_key_equals_machine_modes_on_the_assembled_description_and_moves_with_its_arguments():
    S = TJ.args_of(TJ.KEY_SHAPES[0])                         # (the smaller shape: every key below is a host commitment of the top's preprocessed traces)
    lift, join, top = prm(LIFT), prm(JOIN), prm(TOP)
    jvk = {J: fri16_join_key_host(*S, J, lift, join).tolist() for J in (1, 2)}
    vk = fri16_tree_key_host(*S, 1, jvk[1], 2, lift, join, top).tolist()
    jm = join_machine(S, 1, jvk[1], LIFT, JOIN)
    assert vk == machine_verifier_key_host(jm, top, 2).tolist()
    assert fri16_tree_proof_size(*S, 1, jvk[1], 2, lift, join, top) == _lib.load().zkhip_machine_verifier_proof_size(jm.desc, 2, C.byref(top)) > 0
    # the join size, the number of joins, the joins' key
    vk2 = fri16_tree_key_host(*S, 2, jvk[2], 2, lift, join, top).tolist()
    assert vk2 != vk and vk2 == machine_verifier_key_host(join_machine(S, 2, jvk[2], LIFT, JOIN), top, 2).tolist()
    assert fri16_tree_key_host(*S, 1, jvk[1], 3, lift, join, top).tolist() != vk
    other = list(jvk[1])
    other[5] = (other[5] + 1) % P
    assert fri16_tree_key_host(*S, 1, other, 2, lift, join, top).tolist() != vk
    assert fri16_tree_key_host(*S, 1, jvk[2], 2, lift, join, top).tolist() != vk


# ------------------------------------------------------------------ (3) the bounds, computed
def test_small_shape_bounds_agree_with_a_search_on_the_assembled_description():
    lift, join, top = SMALL_PRM
    most = fri16_join_max_proofs(*SMALL, prm(lift))
    assert most >= 2
    got = fri16_tree_max_join(*SMALL, prm(lift), prm(join))
    assert got == largest(lambda J: takes(SMALL, J, 1, lift, join, top), most) >= 2
    for J in (1, 2):
        joins = fri16_tree_max_joins(*SMALL, J, prm(lift), prm(join))
        assert joins == largest(lambda n: takes(SMALL, J, n, lift, join, top), 64) == 64      # (the issue's table: 2, 3 or 64 joins of 1 or 2 are taken)
        for n in (2, 3, 64):
            assert 179196 <= fri16_tree_proof_size(*SMALL, J, [0] * 8, n, prm(lift), prm(join), prm(top)) <= 212508


def test_full_shape_bounds_agree_with_a_search_on_the_assembled_description():
    lift, join, top = FULL_PRM
    most = fri16_join_max_proofs(*FULL, prm(lift))
    assert most == 64
    got = fri16_tree_max_join(*FULL, prm(lift), prm(join))
    assert 32 <= got < 64                                     # 32 joinable, 64 refused
    assert takes(FULL, 32, 2, lift, join, top) and not takes(FULL, 64, 1, lift, join, top)
    assert takes(FULL, got, 1, lift, join, top) and not takes(FULL, got + 1, 1, lift, join, top)
    joins = fri16_tree_max_joins(*FULL, 16, prm(lift), prm(join))
    assert 16 <= joins <= 63
    assert takes(FULL, 16, joins, lift, join, top) and not takes(FULL, 16, joins + 1, lift, join, top)
    assert fri16_tree_max_joins(*FULL, 32, prm(lift), prm(join)) >= 16                                   # 512 segments in all
    # a join of 64 under a top: refused by every entry with a message that names the bound
    assert fri16_tree_max_joins(*FULL, 64, prm(lift), prm(join)) == 0
    assert "fri16_tree_max_joins: no top takes a join of 64 lift proofs of this shape" in last_error() and "2^21" in last_error()
    assert fri16_tree_proof_size(*FULL, 64, [0] * 8, 2, prm(lift), prm(join), prm(top)) == 0 and "fri16_tree_proof_size: no top takes a join of 64" in last_error()
    with pytest.raises(_lib.ZkHipError, match="fri16_tree_key_host: no top takes a join of 64"):
        fri16_tree_key_host(*FULL, 64, [0] * 8, 2, prm(lift), prm(join), prm(top))
    # more joins than the top takes
    assert fri16_tree_proof_size(*FULL, 16, [0] * 8, joins + 1, prm(lift), prm(join), prm(top)) == 0
    assert "fri16_tree_proof_size: 1 .. %d joins of 16 lift proofs of this shape go under one top, not %d" % (joins, joins + 1) in last_error()


# ------------------------------------------------------------------ (4) refusals, by message
def test_every_refusal_names_its_entry_and_the_bound():
    L = _lib.load()
    S = TJ.args_of(TJ.KEY_SHAPES[0])
    lift, join, top = prm(LIFT), prm(JOIN), prm(TOP)
    most = fri16_join_max_proofs(*S, lift)
    joins = fri16_tree_max_joins(*S, 1, lift, join)
    assert 2 <= joins <= 64
    for n in (0, joins + 1):
        with pytest.raises(_lib.ZkHipError, match="fri16_tree_key_host: 1 .. %d joins of 1 lift proofs of this shape go under one top, not %d" % (joins, n)):
            fri16_tree_key_host(*S, 1, [0] * 8, n, lift, join, top)
        assert fri16_tree_proof_size(*S, 1, [0] * 8, n, lift, join, top) == 0 and "joins of 1 lift proofs" in last_error()
        rc, why = verify_fri16_tree(np.zeros(64, dtype=np.uint8), [[0] * S[6]] * n, *S, 1, [0] * 8, n, [0] * 8, lift, join, top)
        assert rc != 0 and why == 1 and "verify_fri16_tree: 1 .. %d joins of 1 lift proofs" % joins in last_error()
    # a join size no join takes keeps the join's message, in the tree entry's name
    for J in (0, most + 1):
        with pytest.raises(_lib.ZkHipError, match="fri16_tree_key_host: 1 .. %d lift proofs of this shape go into one join, not %d" % (most, J)):
            fri16_tree_key_host(*S, J, [0] * 8, 2, lift, join, top)
        assert fri16_tree_max_joins(*S, J, lift, join) == 0 and "fri16_tree_max_joins: 1 .. %d lift proofs of this shape" % most in last_error()
    # shapes the lift refuses keep the lift's message
    with pytest.raises(_lib.ZkHipError, match="width-24"):
        fri16_tree_key_host(*S, 1, [0] * 8, 2, lift, join, top, hash_width=16)
    assert fri16_tree_max_join(*S, lift, join, hash_width=16) == 0 and "width-24" in last_error()
    assert fri16_tree_max_join(1, 0, 1, 4, 4, 8, 0, lift, join) == 0 and "1 .. 30 inner public values" in last_error()
    # the public values: n_joins x proofs_per_join x n_inner_public words
    rc, why = verify_fri16_tree(np.zeros(64, dtype=np.uint8), [[0] * 7, [0] * 7, [0] * 6], *TJ.args_of(TL.TWIN), 1, [0] * 8, 3, [0] * 8, lift, join, top)
    assert rc != 0 and why == 1 and "verify_fri16_tree: public_values holds n_joins x proofs_per_join x n_inner_public words in segment order (21 here), not 20" in last_error()
    # the batch: a number of lift proofs that is no positive multiple of the join size, before any device is asked for
    dummy = [np.zeros(64, dtype=np.uint8)] * 5
    for n, J in ((5, 2), (0, 2), (3, 0)):
        with pytest.raises(_lib.ZkHipError, match="prove_fri16_join_batch: the number of lift proofs must be a positive multiple of proofs_per_join, not %d for joins of %d" % (n, J)):
            prove_fri16_join_batch(dummy[:n], J, [[0]] * n, *S, lift, join)
    with pytest.raises(_lib.ZkHipError, match=r"prove_fri16_join_batch: public_values holds n_proofs x n_inner_public words in proof order \(4 here\), not 3"):
        prove_fri16_join_batch(dummy[:4], 2, [[0]] * 3, *S, lift, join)
    with pytest.raises(_lib.ZkHipError, match="prove_fri16_join_batch: 1 .. %d lift proofs of this shape go into one join, not %d" % (most, most + 1)):
        prove_fri16_join_batch(dummy[:1] * (2 * most + 2), most + 1, [[0]] * (2 * most + 2), *S, lift, join)
    vk = np.zeros(8, dtype=np.uint32)
    assert L.zkhip_prove_fri16_join_batch(None, 0, *S[:4], 24, *S[4:], C.byref(lift), None, None, 2, 1, None, 2, C.byref(join), 0, 0, None, 0, None,
                                          vk.ctypes.data_as(_lib.u32p)) == -1 and "prove_fri16_join_batch: null argument" in last_error()
    assert L.zkhip_prove_fri16_tree(None, None, *S[:4], 24, *S[4:], C.byref(lift), None, 0, None, None, 2, 1, None, 2, C.byref(join), None, C.byref(top), 0, None, 0, None,
                                    None, 0, None) != 0


# ------------------------------------------------------------------ (5) end to end without a GPU
def oracle_proof_of(O, im, proofs, pubs, params):
    """the machine-mode machine over len(proofs) proofs of `im`: its ten main tables from the host entry (the Poseidon2 chip's 360 columns computed by
    tests/test_fri16_join_cpu.py), the oracle's keyed-machine proof of them and the oracle's key -> (proof, vk)"""
    n = len(proofs)
    mains, pres, progs, tabs, lns = [], [], [], [], []
    for i in range(10):
        prog, ln, mw, pw = machine_verifier_describe(im, i, 0, n)
        got = machine_verifier_host_tables(im, proofs, pubs, i)
        assert got is not None, (i, last_error())
        if mw == RM.P2_MAIN:
            rows = got.reshape(-1, 18)
            got = TJ.p2r_columns(rows[:, :16].astype(np.uint64), rows[:, 16], rows[:, 17], ln)
        pre = machine_verifier_describe(im, i, 2, n)[0]
        mains.append(got.reshape(1 << ln, mw))
        pres.append(pre.reshape(1 << ln, pw) if pw else None)
        progs.append(prog)
        tabs.append(machine_verifier_describe(im, i, 1, n)[0])
        lns.append(ln)
    flat = [int(v) for pub in pubs for v in pub]
    return O.prove_machine_keyed(mains, pres, progs, tabs, flat, O.default_params(*params)), O.machine_setup(pres, lns, O.default_params(*params))


def tree_case(oracle):
    """tests/test_fri16_join_cpu.py's two oracle lift proofs of the twin shape -> two joins of ONE proof each at (1, 3, 0) -> the top over the two joins at (1, 3, 0), every
    level proven by the oracle from the library's host tables.  (The twin shape is the smaller of the shapes of which two different lift proofs exist.)"""
    if _CASE:
        return _CASE
    c = TJ.join_case(oracle)
    S, lifted, pubs = c["S"], c["proofs"], c["pubs"]
    joins, jvks = [], []
    for p in range(2):
        jp, jvk = oracle_proof_of(oracle, c["im"], [lifted[p]], [pubs[p]], JOIN)
        joins.append(jp)
        jvks.append(jvk.tolist())
    assert jvks[0] == jvks[1] == fri16_join_key_host(*S, 1, prm(LIFT), prm(JOIN)).tolist()
    jm = join_machine(S, 1, jvks[0], LIFT, JOIN)
    top, tvk = oracle_proof_of(oracle, jm, joins, pubs, TOP)
    _CASE.update(S=S, pubs=pubs, jvk=jvks[0], top=top, tvk=tvk.tolist(), joins=joins)
    return _CASE


def test_two_joins_and_the_top_over_them_without_a_gpu(oracle):
    c = tree_case(oracle)
    S, pubs, jvk, top = c["S"], c["pubs"], c["jvk"], c["top"]
    lift, join, tp = prm(LIFT), prm(JOIN), prm(TOP)
    tvk = fri16_tree_key_host(*S, 1, jvk, 2, lift, join, tp).tolist()
    assert tvk == c["tvk"]                                    # the oracle's commitment to the preprocessed traces the library describes
    assert top.size == fri16_tree_proof_size(*S, 1, jvk, 2, lift, join, tp)
    check = lambda pv, J=1, k=jvk, n=2, t=tvk: verify_fri16_tree(top, pv, *S, J, k, n, t, lift, join, tp)
    assert check(pubs) == (0, 0)
    assert check([pubs[1], pubs[0]])[0] != 0                  # the joins' public values exchanged
    changed = [list(pubs[0]), list(pubs[1])]
    changed[1][3] = (changed[1][3] + 1) % P
    assert check(changed)[0] != 0                             # one public word
    assert check(pubs + [pubs[0]], n=3, t=fri16_tree_key_host(*S, 1, jvk, 3, lift, join, tp))[0] != 0      # another n_joins
    assert check(pubs[:1], n=1, t=fri16_tree_key_host(*S, 1, jvk, 1, lift, join, tp))[0] != 0
    other = list(jvk)
    other[0] = (other[0] + 1) % P
    assert check(pubs, k=other)[0] != 0                       # another join_vk, under the top key that made the proof and under its own
    assert check(pubs, k=other, t=fri16_tree_key_host(*S, 1, other, 2, lift, join, tp))[0] != 0
    jvk2 = fri16_join_key_host(*S, 2, lift, join).tolist()    # the key of another join size: one join of both segments
    assert check(pubs, J=2, k=jvk2, n=1, t=fri16_tree_key_host(*S, 2, jvk2, 1, lift, join, tp))[0] != 0
    assert check(pubs, k=jvk2)[0] != 0
