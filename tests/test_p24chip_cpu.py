"""The width-24 Poseidon2 chip (RISC Zero-shape commitments), CPU side: the product's program against the independent Python restatement
(tests/poseidon2_24_air.py, on tests/pyref.py's poseidon2_24), Python traces against every constraint, what the constraints catch, real
openings of golden RISC Zero-shape proofs, and proofs of the oracle checked by the host verifier and by tests/pyverify.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import poseidon2_24_air as A
import pyref
import pyverify
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import p24chip_air, verify_merkle_paths_p24, verify_shard_air

P = 2013265921
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "oracle_kat.json")))["golden_proof_files"]
R0_SHAPE = (2, 4, 0, 0, 4, 1, 24)           # blowup 4, fold 16, Poseidon2 width 24 (a 2^5-row trace: one final coefficient bit)


def test_program_equals_the_python_restatement(oracle):
    prog = A.program()
    assert prog.tolist() == p24chip_air().tolist()
    assert oracle.air_validate(prog, A.WIDTH, A.N_PUBLIC) == 1 and oracle.air_log_quotient_degree(prog) == 1
    assert A.WIDTH == 540 and A.WIDTH % 4 == 0 and prog[3] == 577


def test_program_follows_the_width24_tables(tmp_path):
    """the round constants are coefficients of the program: another width-24 table set, another program; the width-16 chip's is untouched"""
    from zktls_amd.device import p2chip_air
    L = _lib.load()
    before, before16 = p24chip_air(), p2chip_air()
    params = json.load(open(os.path.join(HERE, "golden", "poseidon2_24_params.json")))
    f = {"width": 24, "name": "test/p24chip", "external_rc": params["external_rc"], "internal_rc": list(params["internal_rc"]), "internal_diag": params["internal_diag"]}
    f["internal_rc"][5] = (f["internal_rc"][5] + 1) % P
    path = tmp_path / "p24.json"
    path.write_text(json.dumps(f))
    try:
        assert L.zkhip_load_poseidon2_params(str(path).encode()) == 0
        other = p24chip_air()
        assert other.size == before.size and other.tolist() != before.tolist()
        assert p2chip_air().tolist() == before16.tolist()
    finally:
        L.zkhip_reset_poseidon2_params()
    assert p24chip_air().tolist() == before.tolist()


@pytest.mark.parametrize("case", [(1, 0, 2, 1), (2, 4, 3, 2), (3, 8, 5, 3), (4, 12, 4, 4), (5, 16, 3, 5), (6, 28, 3, 6), (7, 64, 2, 7),
                                  (10, 0, 6, 8), (10, 20, 3, 9), (9, 12, 7, 10)])
def test_trace_satisfies_every_constraint(case):
    """random trees, every row width class (no sponge row, one partial block, one full block, full + partial, several blocks), several
    paths, padding behind them; the roots are pyref's sponge24 / compress24 roots"""
    depth, row_width, n_paths, seed = case
    leaves, sibs, idx, root = A.sparse_tree_paths(depth, n_paths, row_width, seed)
    trace, roots = A.merkle_trace(leaves, sibs, idx, row_width=row_width)
    assert all(r == root for r in roots)
    assert all(pyverify.Hash(24).root_from_path(l, i, s) == root for l, i, s in zip(leaves, idx, sibs)) if row_width else True
    used = n_paths * ((row_width + 15) // 16 + depth)
    assert trace.shape == (max(32, 1 << (used - 1).bit_length()), A.WIDTH)
    assert A.check_constraints(A.program(), trace, root + [n_paths]) == []
    assert trace[:, A.END].sum() == n_paths and trace[:, A.SS].sum() == (n_paths if row_width else 0)
    # another count or another root is not this trace's statement
    assert A.check_constraints(A.program(), trace, root + [n_paths + 1]) != []
    assert A.check_constraints(A.program(), trace, [root[0] ^ 1] + root[1:] + [n_paths]) != []


def test_what_the_constraints_catch():
    """each single-cell change breaks at least one constraint"""
    prog = A.program()
    # two paths over rows of 20 values (a full block, then a partial block of 4) and two over rows of 8 (one partial block)
    l20, s20, i20, r20 = A.sparse_tree_paths(3, 2, 20, 21)
    t20, _ = A.merkle_trace(l20, s20, i20, row_width=20)
    l8, s8, i8, r8 = A.sparse_tree_paths(3, 2, 8, 22)
    t8, _ = A.merkle_trace(l8, s8, i8, row_width=8)
    assert A.check_constraints(prog, t20, r20 + [2]) == [] and A.check_constraints(prog, t8, r8 + [2]) == []
    # t20: row 0 SS (16 values), row 1 SPG absorbing 4 (groups 1..3 carried), rows 2..4 compression
    assert t20[0, A.SS] == 1 and t20[1, A.SPG] == 1 and t20[1, A.G[1]] == 0 and t20[1, A.C[1]] == 1 and t20[2, A.CH] == 1
    assert t8[0, A.SS] == 1 and t8[0, A.G[1]] == 1 and t8[0, A.G[2]] == 0

    def broken(t, pub, row, col, delta=1):
        bad = t.copy()
        bad[row, col] = (int(bad[row, col]) + delta) % P
        return A.check_constraints(prog, bad, pub) != []
    bit2 = (i20[0] >> 0) & 1
    sib_col = A.IN + (0 if bit2 else 8) + 3                   # where the sibling sits in the first compression row
    assert broken(t20, r20 + [2], 2, sib_col), "a sibling word"
    assert broken(t20, r20 + [2], 3, A.BIT), "a direction bit"
    assert broken(t20, r20 + [2], 0, A.IN + 7), "an absorbed word (first block)"
    assert broken(t20, r20 + [2], 1, A.IN + 2), "an absorbed word (partial block)"
    assert broken(t20, r20 + [2], 1, A.IN + 9), "a carried-over rate word on a partial block"
    assert broken(t20, r20 + [2], 1, A.IN + 20), "a capacity word that does not follow"
    assert broken(t20, r20 + [2], 1, A.G[2]), "a non-prefix group pattern (G2 without G1)"
    assert broken(t8, r8 + [2], 0, A.IN + 9), "a non-absorbed rate word on a first sponge row"
    assert broken(t8, r8 + [2], 0, A.IN + 17), "a nonzero capacity on a first sponge row"
    assert broken(t20, r20 + [2], 3, A.IN + 18), "a nonzero capacity on a compression row"
    assert broken(t20, r20 + [2], 4, A.CNT), "a CNT skip"
    assert broken(t20, r20 + [2], 1, A.C[2], P - 1), "a carry flag that does not match SPG (1 - G)"
    assert broken(t20, r20 + [2], 4, A.X3E(6) + 5), "a forged intermediate"
    assert broken(t20, r20 + [2], 4, A.SBP(12)), "a forged internal round"
    # a non-prefix pattern written consistently (G1 = 0, G2 = 1 with C1, C2 to match) is still refused by the prefix constraint
    bad = t8.copy()
    bad[0, A.G[1]], bad[0, A.G[2]] = 0, 1
    assert A.check_constraints(prog, bad, r8 + [2]) != []


def golden_openings(name):
    g = GOLDEN[name]
    v = {}
    b = open(os.path.join(HERE, "golden", "proofs", name + ".bin"), "rb").read()
    assert pyverify.verify(b, g["log_n"], g["width"], g["public"], *g["shape"], view=v) is True
    return g, v


@pytest.mark.parametrize("name,which", [("v3_r0_9x8", "trace"), ("v3_r0_9x8", "quot"), ("v8_groups_r0_lookup_8x16", "quot")])
def test_openings_of_golden_r0_proofs(name, which):
    """the openings a RISC Zero-shape proof's verifier checks, through the chip: every one ends in the root the proof commits to"""
    g, v = golden_openings(name)
    ops = v["openings"]
    rows_ = [o["trow" if which == "trace" else "qrow"] for o in ops]
    sibs = [o["tpath" if which == "trace" else "qpath"] for o in ops]
    idx = [o["index"] for o in ops]
    root = v["trace_root" if which == "trace" else "quot_root"]
    rw = len(rows_[0])
    assert rw % 4 == 0 and len(sibs[0]) == g["log_n"] + g["shape"][0]
    trace, roots = A.merkle_trace(rows_, sibs, idx, row_width=rw)
    assert all(r == root for r in roots)
    assert A.check_constraints(A.program(), trace, root + [len(ops)]) == []


@pytest.mark.parametrize("shape", [(1, 6, 4), R0_SHAPE])
def test_host_verifier_on_oracle_proofs(oracle, shape):
    O = oracle
    leaves, sibs, idx, root = A.sparse_tree_paths(3, 3, 20, 31)
    trace, _ = A.merkle_trace(leaves, sibs, idx, row_width=20)
    assert trace.shape == (32, A.WIDTH)
    prog, pub = A.program(), root + [3]
    oprm, prm = O.default_params(*shape), Params(*shape)
    proof = O.prove_shard_air(prog, trace, pub, oprm)
    assert O.verify_shard_air(prog, proof, 5, A.WIDTH, pub, oprm) == 0
    assert verify_merkle_paths_p24(proof, root, 3, prm) == (0, 0)
    assert verify_shard_air(prog, proof, 5, A.WIDTH, pub, prm) == (0, 0)
    assert pyverify.verify(proof.tobytes(), 5, A.WIDTH, pub, *shape, air=prog) is True
    # another root, another count, one flipped byte
    assert verify_merkle_paths_p24(proof, [root[0] ^ 1] + root[1:], 3, prm)[0] != 0
    assert verify_merkle_paths_p24(proof, root, 2, prm)[0] != 0
    flipped = proof.copy()
    flipped[len(flipped) // 2] ^= 1
    assert verify_merkle_paths_p24(flipped, root, 3, prm)[0] != 0
    with pytest.raises(pyverify.Reject):
        pyverify.verify(proof.tobytes(), 5, A.WIDTH, root + [2], *shape, air=prog)
    with pytest.raises(pyverify.Reject):
        pyverify.verify(flipped.tobytes(), 5, A.WIDTH, pub, *shape, air=prog)


def test_entries_check_their_arguments():
    L = _lib.load()
    prm = Params(1, 10, 4)
    assert L.zkhip_merkle_paths_p24_proof_size(0, 4, 0, C.byref(prm)) == 0
    assert L.zkhip_merkle_paths_p24_proof_size(4, 0, 0, C.byref(prm)) == 0
    assert L.zkhip_merkle_paths_p24_proof_size(4, 33, 0, C.byref(prm)) == 0
    assert L.zkhip_merkle_paths_p24_proof_size(1 << 22, 2, 0, C.byref(prm)) == 0
    assert L.zkhip_merkle_paths_p24_proof_size(100, 10, 6, C.byref(prm)) == 0            # not a multiple of 4
    assert L.zkhip_merkle_paths_p24_proof_size(100, 10, 1028, C.byref(prm)) == 0         # wider than 1024
    assert L.zkhip_merkle_paths_p24_proof_size(100, 10, 0, C.byref(prm)) > 0
    assert L.zkhip_merkle_paths_p24_proof_size(100, 10, 20, C.byref(prm)) > L.zkhip_merkle_paths_p24_proof_size(100, 10, 0, C.byref(prm))
    z = (C.c_uint32 * 8)()
    got = C.c_size_t(0)
    buf = (C.c_uint8 * 16)()
    assert L.zkhip_prove_merkle_paths_p24(None, z, 0, z, z, 1, 1, z, C.byref(prm), buf, 16, C.byref(got)) != 0
    assert L.zkhip_p24chip_gen_merkle_trace(None, z, 0, z, z, 1, 1, 5, None, 540, z) != 0
    assert L.zkhip_verify_merkle_paths_p24(buf, 16, z, 1, C.byref(prm), None) != 0
