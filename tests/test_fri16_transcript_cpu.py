"""The fold-by-16 INDICES machine (zktls_amd/csrc/fri16_chip.hip: the paths machine with the Fiat-Shamir transcript inside -- P2T, SAMPLES, FOLD16B and the
buses that carry challenges and indices), CPU side: the library's programs and interaction tables against the Python restatement
(tests/fri16_transcript_air.py); the restatement's traces under every constraint and every bus in plain integers; the key without a GPU, which holds no index
and no challenge; the machine under the oracle's prover and the library's verifier; the transcript view of the committed fold-16 proofs; and forgeries, each
built here and shown rejected BY WHAT (a named constraint or a bus)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fri16_air as A
import fri16_paths_air as PA
import fri16_transcript_air as TA
import fri_air as FA
import poseidon2_24_air as P24
from test_fri16_chip_cpu import FOLD16_GOLDEN, GOLDEN, combined, load, shape_of, violations
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import (fri16_describe, fri16_indices_describe, fri16_indices_key_host, fri16_paths_describe, fri16_view_transcript, verify_fri16_indices)

P = 2013265921


@functools.lru_cache(maxsize=None)
def view_of(which):
    """a committed fixture by name, or an honest random instance by (R, F, b, Q)"""
    return TA.golden_view(which, GOLDEN, load) if isinstance(which, str) else TA.honest_view(*which)


@functools.lru_cache(maxsize=None)
def machine_of(which):
    return TA.machine(view_of(which))


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


# ------------------------------------------------------------------ (1) programs and interaction tables
@pytest.mark.parametrize("which", TA.HONEST_SHAPES + FOLD16_GOLDEN)
def test_describe_equals_the_python_restatement(oracle, which):
    if isinstance(which, str):
        v = view_of(which)
        R, F, b, Q, pb = shape(v) + (v["pow_bits"],)
    else:
        R, F, b, Q, pb = which + (TA.POW_BITS,)
    progs, tabs, lrs, o, mains = TA.programs(R, F, b, pb), TA.interactions(R), TA.log_rows(R, F, b, Q), TA.order(R, F, b, Q), TA.main_widths(F + b)
    assert sorted(o) == list(range(8)) and all(lrs[o[i]] >= lrs[o[i + 1]] for i in range(7))
    for which_, t in enumerate(o):
        prog, ln, mw, pw, table = fri16_indices_describe(R, F, b, Q, pb, which_, 0)
        tab = fri16_indices_describe(R, F, b, Q, pb, which_, 1)[0]
        assert (table, ln, mw, pw) == (t, lrs[t], mains[t], TA.PRE_WIDTHS[t])
        assert prog.tolist() == progs[t].tolist()
        assert tab.tolist() == tabs[t].tolist()
        assert oracle.air_validate(prog, mw + pw, TA.N_PUBLIC) == 1
        assert oracle.air_log_quotient_degree(prog) == 1
        assert int(tab[1]) <= 64 and mw % 4 == 0 and pw % 4 == 0


@pytest.mark.parametrize("S", [(1, 1, 1, 8), (2, 2, 2, 11), (3, 8, 2, 50)])
def test_final_and_p24l_are_the_paths_machines_and_fold16b_differs_in_the_beta_constraints_and_one_interaction(S):
    """FINAL and P24L: word for word but the public-value count in the header (word 4; every program of a machine names the machine's count)"""
    R, F, b, Q = S
    mine = {d[4]: (d[0], fri16_indices_describe(R, F, b, Q, 4, w, 1)[0]) for w, d in ((w, fri16_indices_describe(R, F, b, Q, 4, w, 0)) for w in range(8))}
    theirs = {d[4]: (d[0], fri16_paths_describe(R, F, b, Q, w, 1)[0]) for w, d in ((w, fri16_paths_describe(R, F, b, Q, w, 0)) for w in range(6))}
    for t in (TA.FINAL, TA.P24L):
        a, c = mine[t][0].tolist(), theirs[t][0].tolist()
        assert a[4] == 8 and c[4] == 4 * R and a[:4] + a[5:] == c[:4] + c[5:]
        assert mine[t][1].tolist() == theirs[t][1].tolist()
    fold = {d[4]: d[0] for d in (fri16_describe(R, F, b, Q, w, 0) for w in range(5))}[A.FOLD16]
    old, new = TA.constraints_of(fold), TA.constraints_of(mine[TA.FOLD16B][0])
    gone = [c for c in old if c not in new]
    assert len(gone) == 4 and [c for c in new if c not in old] == [] and len(new) == len(old) - 4
    for c, (sel, terms) in enumerate(gone):                  # BETA_c - sum_l L_l public[4 l + c]
        assert sel == 0 and terms[0] == (1, [A.BETA + c]) and [t[1] for t in terms[1:]] == [[A.L + l, (2 << 30) | (4 * l + c)] for l in range(R)]
    assert [c for c in old if c in new] == new                # the order of the others is kept
    to, tn = list(TA._entries(theirs[PA.FOLD16][1])), list(TA._entries(mine[TA.FOLD16B][1]))
    assert tn[:-1] == to and tn[-1] == (1, A.ACTIVE, TA.BUS_BF16, [A.LN, A.BETA, A.BETA + 1, A.BETA + 2, A.BETA + 3])


# ------------------------------------------------------------------ (2) constraints and buses
@pytest.mark.parametrize("which", TA.HONEST_SHAPES + FOLD16_GOLDEN)
def test_restated_traces_satisfy_every_constraint_and_balance_every_bus(which):
    v = view_of(which)
    assert A.consistent(v)
    main, pre, progs, tabs, pub = machine_of(which)
    assert violations(main, pre, progs, tabs, pub) == ([], {})
    R, F, b, Q = shape(v)
    C_, S_, NT = TA.chain_rows(R, F, Q)
    if which == (1, 0, 1, 4):
        assert (C_, S_, NT) == (0, 1, 2)                      # F = 0: coefficient and witness in one row
    if which == (1, 1, 1, 7):
        assert (C_, S_) == (1, 1)                             # one coefficient row; the eight slots fill one SAMPLES row exactly
    if which == (1, 1, 1, 8):
        assert (C_, S_) == (1, 2)                             # a ninth slot alone in a second row
    if which == (2, 2, 2, 11):
        assert (C_, S_) == (2, 2)


# ------------------------------------------------------------------ (3) the key and the machine under the oracle's prover
@pytest.mark.parametrize("which", [(1, 0, 1, 4), (2, 2, 2, 11)] + FOLD16_GOLDEN)
def test_host_key_equals_the_oracles_setup_and_holds_no_index_and_no_challenge(oracle, which):
    v = view_of(which)
    main, pre, progs, tabs, pub = machine_of(which)
    lns = shape_of(main, pre)[0]
    o = TA.order(*shape(v))
    kt = TA.key_tables(v)
    assert all((pre[i] is None and kt[t] is None) or (pre[i] == kt[t]).all() for i, t in enumerate(o))
    other = dict(v, betas=[[(c + 5) % P for c in bt] for bt in v["betas"]], queries=[((i + 1) % (1 << v["H"]), val, sb) for i, val, sb in v["queries"]])
    for sh in ((1, 12, 4), (2, 7, 0)):
        root = oracle.machine_setup(pre, lns, oracle.default_params(*sh)).tolist()
        assert fri16_indices_key_host(v, Params(*sh)).tolist() == root
        assert fri16_indices_key_host(other, Params(*sh)).tolist() == root
    moved = dict(v, queries=[(i, [(val[0] + (q == 0)) % P] + list(val[1:]), sb) for q, (i, val, sb) in enumerate(v["queries"])])
    assert fri16_indices_key_host(moved, Params(1, 12, 4)).tolist() != oracle.machine_setup(pre, lns, oracle.default_params(1, 12, 4)).tolist()
    assert fri16_indices_key_host(dict(v, pow_bits=v["pow_bits"] + 1), Params(1, 12, 4)).tolist() == oracle.machine_setup(pre, lns, oracle.default_params(1, 12, 4)).tolist()


@pytest.mark.parametrize("which,sh", [((1, 1, 1, 8), (1, 10, 2)), ("v3_r0_9x8", (2, 7, 0)), ("v8_groups_r0_lookup_8x16", (1, 12, 4))])
def test_the_oracle_proves_the_restated_arrays_and_the_library_verifies(oracle, which, sh):
    O = oracle
    v = view_of(which)
    R, F, b, Q = shape(v)
    pb = v["pow_bits"]
    main, pre, progs, tabs, pub = machine_of(which)
    lns, ws, pws = shape_of(main, pre)
    oprm, prm = O.default_params(*sh), Params(*sh)
    root = O.machine_setup(pre, lns, oprm)
    assert fri16_indices_key_host(v, prm).tolist() == root.tolist()
    proof = O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm)
    assert _lib.load().zkhip_fri16_indices_proof_size(R, F, b, Q, pb, C.byref(prm)) == proof.size
    assert O.verify_machine_keyed(proof, lns, ws, pws, root, progs, tabs, pub, oprm) == 0
    assert verify_fri16_indices(proof, pub, R, F, b, Q, pb, root, prm)[0] == 0
    bad = list(pub)
    bad[5] = (bad[5] + 1) % P
    assert verify_fri16_indices(proof, bad, R, F, b, Q, pb, root, prm)[0] != 0                      # one capacity word changed
    bad_root = root.copy()
    bad_root[3] = (int(bad_root[3]) + 1) % P
    assert verify_fri16_indices(proof, pub, R, F, b, Q, pb, bad_root, prm)[0] != 0                  # a changed key
    assert verify_fri16_indices(proof, pub, R, F, b, Q, pb + 1, root, prm)[0] != 0                  # the grinding bits are part of the statement: another machine


# ------------------------------------------------------------------ (4) the transcript view of the committed proofs
@pytest.mark.parametrize("name", FOLD16_GOLDEN)
def test_view_transcript_of_a_golden_proof_equals_the_restatement(name):
    g = GOLDEN[name]
    prm = Params(*g["shape"])
    mine = view_of(name)
    got = fri16_view_transcript(load(name), g["log_n"], g["width"], g["public"], prm)
    assert got["roots"] == mine["roots"] and got["betas"] == mine["betas"]
    assert got["capacity"] == mine["capacity"] and got["pending"] == 0 and got["witness"] == mine["witness"] and got["pow_bits"] == mine["pow_bits"]
    words = np.frombuffer(load(name).tobytes(), dtype=np.uint32).copy()
    words[-1] ^= 1
    with pytest.raises(_lib.ZkHipError):                      # fails like zkhip_fri16_view_shard
        fri16_view_transcript(words.view(np.uint8), g["log_n"], g["width"], g["public"], prm)
    with pytest.raises(_lib.ZkHipError):                      # a fold-by-2 shape
        fri16_view_transcript(load(name), g["log_n"], g["width"], g["public"], Params(1, 100, 16))


# ------------------------------------------------------------------ (5) forgeries, and what rejects each
class Forge:
    """a machine's arrays by table number; caught(): names of the failing constraints ("P2T: ...", "SAMPLES: ...", or the table's name) and unbalanced buses"""
    NAMES = ["FOLD16B", "FINAL", "P24L", "QUERIES", "COEFFS", "ROOTS", "P2T", "SAMPLES"]

    def __init__(self, view, honest=True):
        self.v = view
        self.o = TA.order(*shape(view))
        self.at = {t: i for i, t in enumerate(self.o)}
        self.main, self.pre, self.progs, self.tabs, self.pub = TA.machine(view, honest=honest)

    def caught(self, fn=None, table=None, in_pre=False):
        m, p = [x.copy() for x in self.main], [None if x is None else x.copy() for x in self.pre]
        if fn is not None:
            fn((p if in_pre else m)[self.at[table]])
        names = set()
        for i, (rows, prog) in enumerate(zip(combined(m, p), self.progs)):
            t = self.o[i]
            for c, _ in P24.check_constraints(prog, rows, self.pub):
                names.add("P2T: " + TA.p2t_constraint_names()[c] if t == TA.P2T
                          else "SAMPLES: " + TA.samples_constraint_names(self.v["pow_bits"])[c] if t == TA.SAMPLES else self.NAMES[t])
        return names, {bus for bus, _ in A.bus_balance(m, p, self.tabs)}


@pytest.fixture(scope="module")
def honest():
    f = Forge(view_of((2, 2, 2, 11)))
    assert f.caught() == (set(), set())
    return f


def test_a_beta_changed_in_one_fold16b_row_is_caught_by_the_beta_bus(honest):
    """with B2, B4, B8 and the folds of that row recomputed a forger still has to receive (layer, beta') -- which ROOTS does not send"""
    def change(t):
        t[0, A.BETA] = (int(t[0, A.BETA]) + 1) % P
    names, buses = honest.caught(change, TA.FOLD16B)
    assert TA.BUS_BF16 in buses and names == {"FOLD16B"}
    # the whole layer under another challenge, ROOTS' main row included: what ROOTS then receives from the transcript row is not what it holds
    def change_roots(t):
        t[0, 1] = (int(t[0, 1]) + 1) % P
    names, buses = honest.caught(change_roots, TA.ROOTS)
    assert names == set() and buses == {TA.BUS_TB, TA.BUS_BF16}


def test_a_challenge_sent_from_a_padding_row_of_roots_is_caught_by_roots_own_constraint(honest):
    """ROOTS' padding rows have layer number 0 in their (zero) preprocessed cells and receive nothing from the transcript; their main cells are the prover's.
    Layer 0's send moved there, with another challenge, and the layer-0 rows of FOLD16B taking that challenge: every bus balances (a forger would refold, so
    FOLD16B's own arithmetic is no defence) -- what rejects it is fold rows (1 - LISTED) = 0 in ROOTS"""
    v = honest.v
    Q = len(v["queries"])
    beta2 = [(int(c) + 1) % P for c in v["betas"][0]]
    m, p = [x.copy() for x in honest.main], [None if x is None else x.copy() for x in honest.pre]
    roots, fold = m[honest.at[TA.ROOTS]], m[honest.at[TA.FOLD16B]]
    assert not p[honest.at[TA.ROOTS]][31].any()
    roots[0, 5], roots[31, 1:5], roots[31, 5] = 0, beta2, Q
    layer0 = fold[:, A.L] == 1
    assert layer0.sum() == Q
    fold[layer0, A.BETA:A.BETA + 4] = beta2
    assert A.bus_balance(m, p, honest.tabs) == {}
    at = honest.at[TA.ROOTS]
    bad = P24.check_constraints(honest.progs[at], combined(m, p)[at], honest.pub)
    assert bad == [(1, 31)]
    # the same move without the other challenge: still refused
    m2 = [x.copy() for x in honest.main]
    m2[at][0, 5], m2[at][31, 1:5], m2[at][31, 5] = 0, v["betas"][0], Q
    assert A.bus_balance(m2, p, honest.tabs) == {} and P24.check_constraints(honest.progs[at], combined(m2, p)[at], honest.pub) == [(1, 31)]


def test_one_querys_index_changed_with_its_chain_refolded_is_caught_by_the_index_bus():
    """query 3 walks the chain of query 5 (index, reduced opening, rows, paths: every fold and every path holds); SAMPLES keeps sending (3, the drawn index)"""
    v = view_of((2, 2, 2, 11))
    assert v["queries"][3][0] != v["queries"][5][0]
    q, pt = list(v["queries"]), list(v["paths"])
    q[3], pt[3] = q[5], pt[5]
    names, buses = Forge(dict(v, queries=q, paths=pt), honest=False).caught()
    assert names == set() and buses == {FA.BUS_I}


def test_the_indices_of_two_queries_swapped_are_caught_by_the_index_bus():
    v = view_of((2, 2, 2, 11))
    q, pt = list(v["queries"]), list(v["paths"])
    q[0], q[4], pt[0], pt[4] = q[4], q[0], pt[4], pt[0]
    assert q[0][0] != q[4][0]
    names, buses = Forge(dict(v, queries=q, paths=pt), honest=False).caught()
    assert names == set() and buses == {FA.BUS_I}


def test_a_witness_whose_proof_of_work_word_has_a_low_bit_set_is_caught_by_samples():
    v = view_of((1, 1, 1, 8))
    R, F, b, Q = shape(v)
    w = v["witness"]
    while True:                                              # the next witness whose word fails the proof of work
        w += 1
        ch = TA.chain(v["capacity"], v["roots"], v["final_poly"], w, F, Q)
        if ch["words"][0][0] & ((1 << v["pow_bits"]) - 1):
            break
    names, buses = Forge(dict(v, witness=w), honest=False).caught()
    assert "SAMPLES: proof of work" in names and not any(n.startswith("P2T") for n in names)
    assert FA.BUS_I in buses                                  # ... and the indices that follow are other ones


def test_a_coefficient_changed_in_coeffs_only_is_caught_by_both_of_its_buses(honest):
    def change(t):
        t[1, 2] = (int(t[1, 2]) + 1) % P
    names, buses = honest.caught(change, TA.COEFFS, in_pre=True)
    assert names == set() and buses == {A.BUS_COEF, TA.BUS_CT}


def test_a_non_canonical_decomposition_of_a_sampled_word_is_caught_by_the_canonical_form_constraint():
    """the word plus P written in bits: the bits still sum to the word mod P, the index read off them is another one"""
    H, Q = 12, 7
    words = [[5 << 4, 1 << 20, (1 << 27) - 2, 77, 0, 123456, 9, 3]]              # (word 0 is the proof-of-work word: its low 4 bits are zero)
    pre, main, _ = FA.samples_tables(H - 1, Q, words, 5, base=3)
    prog = FA.samples_program(H - 1, None, 4, TA.N_PUBLIC)
    names = TA.samples_constraint_names(4)
    rows = np.concatenate([pre, main], axis=1)
    assert P24.check_constraints(prog, rows, [0] * 8) == []
    for j in (1, 2, 3):
        w = words[0][j] + P
        assert w < 1 << 31
        forged = main.copy()
        bits = [(w >> i) & 1 for i in range(31)]
        forged[0, FA.S_BITS + 31 * j:FA.S_BITS + 31 * j + 31] = bits
        forged[0, FA.S_H1 + j], forged[0, FA.S_H2 + j], forged[0, FA.S_HH + j] = bits[30] & bits[29], bits[28] & bits[27], bits[30] & bits[29] & bits[28] & bits[27]
        forged[0, FA.S_IDX + j] = w & ((1 << H) - 1)
        assert forged[0, FA.S_IDX + j] != main[0, FA.S_IDX + j]
        bad = P24.check_constraints(prog, np.concatenate([pre, forged], axis=1), [0] * 8)
        assert {names[c] for c, _ in bad} == {"canonical"} and {r for _, r in bad} == {0}


# ------------------------------------------------------------------ (6) argument checks
def test_entry_point_argument_checks():
    lib = _lib.load()
    u32p = _lib.u32p
    prm = Params(1, 8, 2)
    v = view_of((1, 1, 1, 8))
    bt, fp, ix, vl, sb, rt, pt, cp = TA.view_arrays(v)
    p = lambda a: a.ctypes.data_as(u32p)
    vk = np.zeros(8, dtype=np.uint32)
    S = (1, 1, 1, 8)
    assert lib.zkhip_fri16_indices_key_host(*S, 24, 4, p(fp), p(vl), p(rt), C.byref(prm), p(vk)) == 0
    assert vk.tolist() == fri16_indices_key_host(v, prm).tolist()
    b8 = np.zeros(8, dtype=np.uint8).ctypes.data_as(_lib.u8p)
    for bad in ((0, 2, 2, 5), (6, 2, 2, 5), (2, 9, 2, 5), (2, 2, 0, 5), (2, 2, 2, 0), (2, 2, 2, 1025), (5, 8, 3, 5)):
        assert lib.zkhip_fri16_indices_key_host(*bad, 24, 4, p(fp), p(vl), p(rt), C.byref(prm), p(vk)) == -1 and b"fri16" in lib.zkhip_last_error()
        assert lib.zkhip_fri16_indices_proof_size(*bad, 4, C.byref(prm)) == 0
        assert lib.zkhip_fri16_indices_describe(*bad, 4, 0, 0, None, 0, None, None, None, None) == 0
        assert lib.zkhip_verify_fri16_indices(b8, 8, *bad, 4, p(cp), p(vk), C.byref(prm), None) != 0
    for pb in (-1, 31):                                      # inner_pow_bits in [0, 30]
        assert lib.zkhip_fri16_indices_key_host(*S, 24, pb, p(fp), p(vl), p(rt), C.byref(prm), p(vk)) == -1 and b"inner_pow_bits" in lib.zkhip_last_error()
        assert lib.zkhip_fri16_indices_proof_size(*S, pb, C.byref(prm)) == 0
    for hw in (16, 0):
        assert lib.zkhip_fri16_indices_key_host(*S, hw, 4, p(fp), p(vl), p(rt), C.byref(prm), p(vk)) == -1 and b"width-16 hash" in lib.zkhip_last_error()
    for k in range(3):
        args = [p(fp), p(vl), p(rt)]
        args[k] = None
        assert lib.zkhip_fri16_indices_key_host(*S, 24, 4, *args, C.byref(prm), p(vk)) == -1 and b"null" in lib.zkhip_last_error()
    bad = rt.copy(); bad[3] = P
    assert lib.zkhip_fri16_indices_key_host(*S, 24, 4, p(fp), p(vl), p(bad), C.byref(prm), p(vk)) == -1 and b"canonical" in lib.zkhip_last_error()
    assert lib.zkhip_fri16_indices_describe(*S, 4, 8, 0, None, 0, None, None, None, None) == 0 and lib.zkhip_fri16_indices_describe(*S, 4, 7, 0, None, 0, None, None, None, None) > 0
    # without a context the device entries refuse (no fallback)
    assert lib.zkhip_fri16_indices_key(None, *S, 24, 4, p(fp), p(vl), p(rt), C.byref(prm), None, p(vk)) == -1
    assert lib.zkhip_fri16_indices_gen_traces(None, *S, 4, p(cp), p(rt), p(fp), 0, None, None, p(bt), p(ix)) == -1
    assert lib.zkhip_fri16_samples_gen_trace(None, 12, 8, p(bt), None) == -1
    assert lib.zkhip_prove_fri16_indices(None, None, *S, 24, 4, p(bt), p(fp), p(ix), p(vl), p(sb), p(rt), p(pt), p(cp), 0, C.byref(prm), None, 0, None) == -1
    assert lib.zkhip_verify_fri16_indices(None, 0, *S, 4, p(cp), p(vk), C.byref(prm), None) != 0
