"""The fold-by-16 LIFT machine (zktls_amd/csrc/fri16_chip.hip: the identity machine with the roots and the final coefficients out of the key), CPU side: the
library's programs, interaction tables and host key against the Python restatement (tests/fri16_lift_air.py) and the oracle's setup; the eleven tables that do
not change against the identity machine's words; the heights over the shape space; THE KEY AS A FUNCTION OF THE SHAPE -- two different inner proofs of one shape
under one key, each accepted with its own public values and rejected with the other's; the restatement's traces under every constraint and every bus in plain
integers; and forgeries, each built here on an honest trace and shown rejected BY WHAT (a named constraint or a bus)."""
import ctypes as C

import numpy as np
import pytest

import fri16_air as A
import fri16_head_air as HA
import fri16_identity_air as IA
import fri16_lift_air as LA
import fri16_paths_air as PA
import fri16_transcript_air as TA
import poseidon2_24_air as P24
from test_fri16_chip_cpu import GOLDEN, combined, load, shape_of, violations
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import fri16_identity_describe, fri16_identity_key_host, fri16_lift_describe, fri16_lift_key_host, verify_fri16_lift

P = 2013265921
GOLDEN_NAME = "v3_r0_9x8"
# (R, F, b, Q, W, NP): the shapes of the identity machine's CPU file
SHAPES = [(1, 0, 1, 4, 8, 1), (1, 1, 1, 3, 40, 7), (1, 0, 2, 4, 16, 3), (2, 1, 2, 3, 8, 3), (1, 0, 1, 2, 264, 6), (1, 2, 2, 5, 1024, 30)]
TWIN = SHAPES[1]                                             # the shape of which two different inner proofs are made
POW_BITS = 4
_VIEWS, _MACHINES = {}, {}


def view_of(oracle, which, seed=1):
    k = (which, seed)
    if k not in _VIEWS:
        _VIEWS[k] = HA.golden_view(which, GOLDEN, load) if isinstance(which, str) else IA.oracle_view(oracle, *which, seed=seed, pow_bits=POW_BITS)
    return _VIEWS[k]


def machine_of(oracle, which, seed=1):
    k = (which, seed)
    if k not in _MACHINES:
        _MACHINES[k] = LA.machine(view_of(oracle, which, seed))
    return _MACHINES[k]


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


def full_shape(v):
    return shape(v) + (v["pow_bits"], v["W"], len(v["pubs"]))


# ------------------------------------------------------------------ (1) programs, interaction tables
@pytest.mark.parametrize("which", [GOLDEN_NAME] + SHAPES)
def test_describe_equals_the_python_restatement(oracle, which):
    if isinstance(which, str):
        R, F, b, Q, pb, W, NP = full_shape(view_of(oracle, which))
    else:
        R, F, b, Q, W, NP = which
        pb = POW_BITS
    n = 4 * R + F
    progs, tabs, lrs, o, mains = LA.programs(R, F, b, pb, W, NP), LA.interactions(R, F + b, n), LA.log_rows(R, F, b, Q, W, NP), LA.order(R, F, b, Q, W, NP), LA.main_widths(F + b, n)
    assert mains[LA.ROOTS] == 16 and mains[LA.COEFFS] == 8
    for which_, t in enumerate(o):
        prog, ln, mw, pw, table = fri16_lift_describe(R, F, b, Q, pb, W, NP, which_, 0)
        tab = fri16_lift_describe(R, F, b, Q, pb, W, NP, which_, 1)[0]
        assert (table, ln, mw, pw) == (t, lrs[t], mains[t], LA.PRE_WIDTHS[t])
        assert prog.tolist() == progs[t].tolist(), LA.NAMES[t]
        assert tab.tolist() == tabs[t].tolist(), LA.NAMES[t]
        assert int(prog[4]) == NP
        assert oracle.air_validate(prog, mw + pw, NP) == 1
        assert oracle.air_log_quotient_degree(prog) == 1
    with pytest.raises(_lib.ZkHipError):
        fri16_lift_describe(R, F, b, Q, pb, W, NP, 13, 0)


@pytest.mark.parametrize("S", [(1, 1, 1, 8, 8, 3), (2, 2, 2, 11, 24, 6), (3, 8, 2, 50, 128, 30)])
def test_the_eleven_other_tables_keep_the_identity_machines_words(S):
    """FOLD16C FINAL P24L QUERY16H P2TH SAMPLES ROWSUM16H P24R OPENED16 AIR16 SCALARS16.  Exceptions: NONE -- no word of a program or an interaction table encodes
    the kind, and the public-value count (word 4 of a program) is the same NP in both kinds.  ROOTS and COEFFS are the two that change, and how is pinned here"""
    R, F, b, Q, W, NP = S
    mine = {d[4]: (d, fri16_lift_describe(R, F, b, Q, 4, W, NP, w, 1)[0]) for w, d in ((w, fri16_lift_describe(R, F, b, Q, 4, W, NP, w, 0)) for w in range(13))}
    theirs = {d[4]: (d, fri16_identity_describe(R, F, b, Q, 4, W, NP, w, 1)[0]) for w, d in ((w, fri16_identity_describe(R, F, b, Q, 4, W, NP, w, 0)) for w in range(13))}
    assert sorted(mine) == sorted(theirs) == list(range(13)) and len(LA.UNCHANGED) == 11
    for t in range(13):
        (prog, ln, mw, pw, _), tab = mine[t]
        (prog_i, ln_i, mw_i, pw_i, _), tab_i = theirs[t]
        assert (ln, pw) == (ln_i, pw_i), LA.NAMES[t]
        if t in LA.UNCHANGED:
            assert mw == mw_i and prog.tolist() == prog_i.tolist() and tab.tolist() == tab_i.tolist(), LA.NAMES[t]
    e, ei = list(TA._entries(mine[LA.ROOTS][1])), list(TA._entries(theirs[LA.ROOTS][1]))
    assert [x[:3] for x in e] == [x[:3] for x in ei]                         # the same buses under the same multiplicities, in the same order
    RM = HA.ROOTS_PRE
    for (_, _, bus, cols), (_, _, _, cols_i) in zip(e, ei):
        assert cols == [RM + 8 + c - 2 if 2 <= c <= 9 else c for c in cols_i], bus
    assert (mine[LA.ROOTS][0][2], theirs[LA.ROOTS][0][2]) == (16, 8)
    cons = TA.constraints_of(mine[LA.ROOTS][0][0])
    assert cons[:2] == TA.constraints_of(theirs[LA.ROOTS][0][0]) and len(cons) == 3          # the first-row identity still names main column 7: a spare column
    e, ei = list(TA._entries(mine[LA.COEFFS][1])), list(TA._entries(theirs[LA.COEFFS][1]))
    assert [x[:3] for x in e] == [x[:3] for x in ei] == [(0, 5, A.BUS_COEF), (0, 6, TA.BUS_CT)]      # both multiplicities preprocessed
    assert all(cols == [0, 12, 13, 14, 15] for _, _, _, cols in e)
    assert (mine[LA.COEFFS][0][2], theirs[LA.COEFFS][0][2]) == (8, 4)
    assert TA.constraints_of(mine[LA.COEFFS][0][0]) == TA.constraints_of(theirs[LA.COEFFS][0][0])  # ... and COEFFS' names main column 3, as before


def test_the_heights_are_the_identity_machines_over_the_sweep():
    """R 1..5 x F 0..8 x log_blowup 1..2 x Q x W x NP: every table as tall as in the identity machine, so the eight-tables-of-one-height rule refuses no shape"""
    lib = _lib.load()
    taken = 0
    for R in range(1, 6):
        for F in range(0, 9):
            for b in (1, 2):
                if not A.shape_ok(R, F, b, 1):
                    continue
                for Q in (1, 2, 50, 100, 1024):
                    for W in (8, 16, 24, 128, 1024):
                        for NP in (3, 30):
                            lrs = IA.log_rows(R, F, b, Q, W, NP)
                            assert LA.log_rows(R, F, b, Q, W, NP) == lrs and LA.shape_ok(R, F, b, Q, 4, W, NP)
                            o = LA.order(R, F, b, Q, W, NP)
                            for which in (12,):
                                ln, li = C.c_int(0), C.c_int(-1)
                                n = lib.zkhip_fri16_lift_describe(R, F, b, Q, 4, W, NP, which, 1, None, 0, C.byref(ln), None, None, None)
                                lib.zkhip_fri16_identity_describe(R, F, b, Q, 4, W, NP, which, 1, None, 0, C.byref(li), None, None, None)
                                assert n > 0 and ln.value == li.value == lrs[o[which]], (R, F, b, Q, W, NP, lib.zkhip_last_error())
                            taken += 1
    assert taken > 4000
    assert lib.zkhip_fri16_lift_describe(1, 0, 1, 4, 4, 8, 0, 0, 0, None, 0, None, None, None, None) == 0 and b"1 .. 30 inner public values" in lib.zkhip_last_error()


# ------------------------------------------------------------------ (2) the key is a function of the shape
def key_of(oracle, S, sh):
    R, F, b, Q, pb, W, NP = S
    kt = LA.shape_key_tables(R, F, b, Q, pb, W, NP)
    o, lrs = LA.order(R, F, b, Q, W, NP), LA.log_rows(R, F, b, Q, W, NP)
    return oracle.machine_setup([kt[t] for t in o], [lrs[t] for t in o], oracle.default_params(*sh))


@pytest.mark.parametrize("which", [GOLDEN_NAME] + SHAPES[:4])
def test_host_key_equals_the_oracles_setup_on_the_shapes_tables(oracle, which):
    S = full_shape(view_of(oracle, which))
    for sh in ((1, 12, 4), (2, 7, 0)):
        assert fri16_lift_key_host(*S, Params(*sh)).tolist() == key_of(oracle, S, sh).tolist()
    kt, vt = LA.shape_key_tables(*S), LA.key_tables(view_of(oracle, which))
    assert all((a is None and c is None) or (a == c).all() for a, c in zip(kt, vt))
    R = S[0]
    assert not kt[LA.ROOTS][:, 3:10].any() and kt[LA.ROOTS][:, LA.RT_ACT].tolist() == [1] * (R + 2) + [0] * (32 - R - 2) and not kt[LA.COEFFS][:, 1:5].any()


def test_two_inner_proofs_of_one_shape_share_one_key(oracle):
    O = oracle
    v1, v2 = view_of(oracle, TWIN, 1), view_of(oracle, TWIN, 2)
    S = full_shape(v1)
    assert full_shape(v2) == S and v1["roots"] != v2["roots"] and v1["troot"] != v2["troot"] and v1["final_poly"] != v2["final_poly"] and v1["pubs"] != v2["pubs"]
    R, F, b, Q, pb, W, NP = S
    sh = (1, 10, 2)
    oprm, prm = O.default_params(*sh), Params(*sh)
    vk = fri16_lift_key_host(*S, prm)
    assert vk.tolist() == key_of(oracle, S, sh).tolist()
    proofs = []
    for seed, v in ((1, v1), (2, v2)):
        main, pre, progs, tabs, pub = machine_of(oracle, TWIN, seed)
        lns, ws, pws = shape_of(main, pre)
        assert O.machine_setup(pre, lns, oprm).tolist() == vk.tolist()                      # the restatement's key tables of THIS view: the one key
        proof = O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm)
        assert _lib.load().zkhip_fri16_lift_proof_size(R, F, b, Q, pb, W, NP, C.byref(prm)) == proof.size
        assert O.verify_machine_keyed(proof, lns, ws, pws, vk, progs, tabs, pub, oprm) == 0
        proofs.append((proof, pub))
    for i in range(2):
        proof, pub = proofs[i]
        assert verify_fri16_lift(proof, pub, R, F, b, Q, pb, W, vk, prm) == (0, 0)
        assert verify_fri16_lift(proof, proofs[1 - i][1], R, F, b, Q, pb, W, vk, prm)[0] != 0      # the other proof's public values
    for k in range(7):                                       # any one shape argument changed: another key
        T = list(S)
        T[k] += 8 if k == 5 else 1
        assert fri16_lift_key_host(*T, prm).tolist() != vk.tolist(), k
    # the contrast that shows what moved: the identity machine needs a key per inner proof
    assert fri16_identity_key_host(v1, prm).tolist() != fri16_identity_key_host(v2, prm).tolist()
    with pytest.raises(_lib.ZkHipError, match="width-24"):
        fri16_lift_key_host(*S, prm, hash_width=16)


# ------------------------------------------------------------------ (3) constraints and buses
@pytest.mark.parametrize("which", [GOLDEN_NAME, TWIN])
def test_restated_traces_satisfy_every_constraint_and_balance_every_bus(oracle, which):
    v = view_of(oracle, which)
    main, pre, progs, tabs, pub = machine_of(oracle, which)
    assert pub == [int(x) for x in v["pubs"]]
    assert violations(main, pre, progs, tabs, pub) == ([], {})


# ------------------------------------------------------------------ (4) forgeries, and what rejects each
class Forge:
    """a machine's arrays by table number; caught(): names of the failing constraints ("<table>: <name>") and the unbalanced buses"""
    NAMED = (LA.ROOTS, LA.COEFFS, HA.P2TH)

    def __init__(self, view):
        self.v = view
        R, F, b, Q = shape(view)
        self.R, self.F, self.Q, self.W, self.NP, self.n = R, F, Q, view["W"], len(view["pubs"]), 4 * R + F
        self.o = LA.order(R, F, b, Q, self.W, self.NP)
        self.at = {t: i for i, t in enumerate(self.o)}
        self.main, self.pre, self.progs, self.tabs, self.pub = LA.machine(view)

    def caught(self, fn=None):
        m, p = [x.copy() for x in self.main], [None if x is None else x.copy() for x in self.pre]
        if fn is not None:
            out = fn({t: m[i] for t, i in self.at.items()}, {t: p[i] for t, i in self.at.items()})
            for t, arr in (out or {}).items():               # a table made anew
                m[self.at[t]] = arr
        names = set()
        for i, (rows, prog) in enumerate(zip(combined(m, p), self.progs)):
            t = self.o[i]
            cn = LA.constraint_names(t, self.W, self.NP, self.n, self.v["pow_bits"]) if t in self.NAMED else None
            for c, _ in P24.check_constraints(prog, rows, self.pub):
                names.add(LA.NAMES[t] + (": " + cn[c] if cn else ""))
        return names, {bus for bus, _ in A.bus_balance(m, p, self.tabs)}


@pytest.fixture(scope="module")
def honest(oracle):
    f = Forge(view_of(oracle, TWIN))
    assert f.caught() == (set(), set()) and (f.R, f.F) == (1, 1)
    return f


ROOT = LA.RL_ROOT
COEF = LA.CL_C


def bump(arr, r, c):
    arr[r, c] = (int(arr[r, c]) + 1) % P


def test_a_layer_root_word_changed_in_roots_only_is_caught_by_the_transcript_bus(honest):
    names, buses = honest.caught(lambda m, p: bump(m[LA.ROOTS], 0, ROOT + 2))
    assert names == set() and TA.BUS_TR0 in buses and TA.BUS_TR1 not in buses


def test_the_same_word_changed_in_the_transcript_too_is_caught_by_the_path_end_bus(honest):
    """ROOTS' word and P2TH's input changed alike and the chain rehashed from there: the transcript buses carry the forged root on both sides, and no path of
    P24L ends in it"""
    v = honest.v
    roots = [list(r) for r in v["roots"]]
    roots[0][2] = (roots[0][2] + 1) % P
    h = HA.head_of(v)
    ch = TA.chain(v["capacity"], roots, v["final_poly"], v["witness"], v["F"], honest.Q)

    def fn(m, p):
        bump(m[LA.ROOTS], 0, ROOT + 2)
        return {HA.P2TH: HA.p2th_main(h["inputs"] + ch["inputs"], m[HA.P2TH].shape[0].bit_length() - 1)}
    names, buses = honest.caught(fn)
    assert not any(n.startswith("ROOTS") or n.startswith("P2TH") for n in names)
    assert TA.BUS_TR0 not in buses and TA.BUS_TR1 not in buses and PA.BUS_RT0 in buses and PA.BUS_RT1 not in buses


def test_a_trace_root_word_changed_in_roots_only_is_caught_by_the_head_bus(honest):
    names, buses = honest.caught(lambda m, p: bump(m[LA.ROOTS], honest.R, ROOT + 5))
    assert names == set() and HA.BUS_HR in buses and PA.BUS_RT1 in buses and TA.BUS_TR1 not in buses      # (the tree rows are not LISTED: no transcript tuple)


def test_a_coefficient_changed_in_coeffs_only_is_caught_by_both_its_buses(honest):
    names, buses = honest.caught(lambda m, p: bump(m[LA.COEFFS], 1, COEF + 1))
    assert names == set() and buses == {A.BUS_COEF, TA.BUS_CT}


def test_a_coefficient_changed_in_coeffs_and_final_is_caught_by_the_transcripts_bus(honest):
    n = 1 << honest.F

    def fn(m, p):
        bump(m[LA.COEFFS], 1, COEF + 1)
        for q in range(honest.Q):                            # FINAL's row of coefficient j in block q is n - 1 - j
            bump(m[HA.FINAL], q * n + n - 1 - 1, A.FC - A.FIN_PRE + 1)      # (A.FC counts from the combined row's first column)
    _, buses = honest.caught(fn)
    assert A.BUS_COEF not in buses and TA.BUS_CT in buses


def test_a_padding_row_that_receives_a_path_end_is_caught_by_the_act_constraint(honest):
    """a row behind the R + 2 active ones with ENDS = 1 and a digest of the forger's choice: its tuple is (LN 0, DEP 0, digest) with nothing preprocessed about
    the digest -- only ENDS (1 - ACT) = 0 keeps it from receiving"""
    def fn(m, p):
        m[LA.ROOTS][honest.R + 3, 0] = 1
        m[LA.ROOTS][honest.R + 3, ROOT:ROOT + 8] = [5, 6, 7, 8, 9, 10, 11, 12]
    names, buses = honest.caught(fn)
    assert names == {"ROOTS: ENDS (1 - ACT) = 0"} and buses == {PA.BUS_RT0, PA.BUS_RT1}
    names, _ = honest.caught(lambda m, p: m[LA.ROOTS].__setitem__((honest.R + 3, slice(ROOT, ROOT + 8)), 9))      # the digest alone: the row receives nothing
    assert names == set() and _ == set()


def test_a_padding_row_of_coeffs_that_holds_a_value_sends_nothing(honest):
    def fn(m, p):
        m[LA.COEFFS][(1 << honest.F) + 1, COEF:COEF + 4] = [1, 2, 3, 4]
    assert honest.caught(fn) == (set(), set())
    pre = honest.pre[honest.at[LA.COEFFS]]
    assert not pre[1 << honest.F:, 5:7].any()                # both multiplicities are preprocessed, and zero there


def test_the_first_row_identities_pin_no_moved_word(honest):
    """root word 7 and coefficient word 3 are non-zero on row 0 of the honest trace, and it is accepted: the identities name the spare columns"""
    rm, cm = honest.main[honest.at[LA.ROOTS]], honest.main[honest.at[LA.COEFFS]]
    assert rm[0, ROOT + 7] != 0 and cm[0, COEF + 3] != 0 and rm.shape[1] - 1 == ROOT + 7 and cm.shape[1] - 1 == COEF + 3
    assert honest.caught() == (set(), set())
    names, _ = honest.caught(lambda m, p: m[LA.ROOTS].__setitem__((0, LA.ROOTS_SPARE), 1))
    assert names == {"ROOTS: row 0: the spare column is zero"}
    names, _ = honest.caught(lambda m, p: m[LA.COEFFS].__setitem__((0, LA.COEFFS_SPARE), 1))
    assert names == {"COEFFS: row 0: the spare column is zero"}
