"""The fold-by-16 IDENTITY machine (zktls_amd/csrc/fri16_chip.hip: the head machine with the AIR identity at zeta inside), CPU side: the library's programs,
interaction tables and host key against the Python restatement (tests/fri16_identity_air.py) and the oracle's setup; the head machine's eleven tables against
the head machine's words; the restatement's traces under every constraint and every bus in plain integers; the machine under the oracle's prover and the
library's verifier; the rule of table heights over the shape space; and forgeries, each built here on an honest trace and shown rejected BY WHAT (a named
constraint or a bus).  Honest instances must satisfy the AIR: the committed v3_r0_9x8 and proofs the oracle's shard prover makes here."""
import ctypes as C

import numpy as np
import pytest

import fri16_air as A
import fri16_head_air as HA
import fri16_identity_air as IA
import fri16_transcript_air as TA
import poseidon2_24_air as P24
import pyverify
from test_fri16_chip_cpu import GOLDEN, combined, load, shape_of, violations
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import fri16_head_describe, fri16_identity_describe, fri16_identity_key_host, fri16_view_head, verify_fri16_identity

P = 2013265921
GOLDEN_NAME = "v3_r0_9x8"
# (R, F, b, Q, W, NP): the oracle proves each and pyverify accepts it; G = 2, 10, 4, 2, 66 and 256 groups, NP up to 30
SHAPES = [(1, 0, 1, 4, 8, 1), (1, 1, 1, 3, 40, 7), (1, 0, 2, 4, 16, 3), (2, 1, 2, 3, 8, 3), (1, 0, 1, 2, 264, 6), (1, 2, 2, 5, 1024, 30)]
HONEST = SHAPES[:2]
POW_BITS = 4
_VIEWS, _MACHINES = {}, {}


def view_of(oracle, which):
    if which not in _VIEWS:
        _VIEWS[which] = HA.golden_view(which, GOLDEN, load) if isinstance(which, str) else IA.oracle_view(oracle, *which, pow_bits=POW_BITS)
    return _VIEWS[which]


def machine_of(oracle, which):
    if which not in _MACHINES:
        _MACHINES[which] = IA.machine(view_of(oracle, which))
    return _MACHINES[which]


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


# ------------------------------------------------------------------ (1) programs, interaction tables, key
@pytest.mark.parametrize("which", [GOLDEN_NAME] + SHAPES)
def test_describe_equals_the_python_restatement(oracle, which):
    if isinstance(which, str):
        v = view_of(oracle, which)
        R, F, b, Q, pb, W, NP = shape(v) + (v["pow_bits"], v["W"], len(v["pubs"]))
    else:
        R, F, b, Q, W, NP = which
        pb = POW_BITS
    n = 4 * R + F
    progs, tabs, lrs, o, mains = IA.programs(R, F, b, pb, W, NP), IA.interactions(R, F + b, n), IA.log_rows(R, F, b, Q, W, NP), IA.order(R, F, b, Q, W, NP), IA.main_widths(F + b, n)
    assert sorted(o) == list(range(13)) and all(lrs[o[i]] >= lrs[o[i + 1]] for i in range(12))
    assert lrs[IA.AIR16] == max(6, A.lg(W // 4)) and lrs[IA.SCALARS16] == 7 and mains[IA.AIR16] == 56 and mains[IA.SCALARS16] == 4 * (17 + n)
    for which_, t in enumerate(o):
        prog, ln, mw, pw, table = fri16_identity_describe(R, F, b, Q, pb, W, NP, which_, 0)
        tab = fri16_identity_describe(R, F, b, Q, pb, W, NP, which_, 1)[0]
        assert (table, ln, mw, pw) == (t, lrs[t], mains[t], IA.PRE_WIDTHS[t])
        assert prog.tolist() == progs[t].tolist(), IA.NAMES[t]
        assert tab.tolist() == tabs[t].tolist(), IA.NAMES[t]
        assert int(prog[4]) == NP
        assert oracle.air_validate(prog, mw + pw, NP) == 1
        assert oracle.air_log_quotient_degree(prog) == 1
        assert int(tab[1]) <= 64 and mw % 4 == 0 and pw % 4 == 0
        if t in (IA.AIR16, IA.SCALARS16, HA.OPENED16, HA.P2TH):      # every multiplicity is preprocessed
            assert all(mult < pw for _, mult, _, _ in TA._entries(tab))
    with pytest.raises(_lib.ZkHipError):
        fri16_identity_describe(R, F, b, Q, pb, W, NP, 13, 0)


@pytest.mark.parametrize("S", [(1, 1, 1, 8, 8, 3), (2, 2, 2, 11, 24, 6), (3, 8, 2, 50, 128, 30)])
def test_the_eleven_head_tables_keep_their_words(S):
    R, F, b, Q, W, NP = S
    mine = {d[4]: (d, fri16_identity_describe(R, F, b, Q, 4, W, NP, w, 1)[0]) for w, d in ((w, fri16_identity_describe(R, F, b, Q, 4, W, NP, w, 0)) for w in range(13))}
    theirs = {d[4]: (d, fri16_head_describe(R, F, b, Q, 4, W, NP, w, 1)[0]) for w, d in ((w, fri16_head_describe(R, F, b, Q, 4, W, NP, w, 0)) for w in range(11))}
    assert sorted(mine) == list(range(13)) and sorted(theirs) == list(range(11))
    for t in range(11):
        (prog, ln, mw, pw, _), tab = mine[t]
        (prog_h, ln_h, mw_h, pw_h, _), tab_h = theirs[t]
        assert (ln, mw) == (ln_h, mw_h), IA.NAMES[t]
        if t == HA.OPENED16:
            assert (pw, pw_h) == (12, 8)
            assert [(s, len(ts)) for s, ts in TA.constraints_of(prog)] == [(s, len(ts)) for s, ts in TA.constraints_of(prog_h)]      # the same constraints, four columns on
            assert len(list(TA._entries(tab))) == len(list(TA._entries(tab_h))) + 2
        else:
            assert pw == pw_h and prog.tolist() == prog_h.tolist(), IA.NAMES[t]
            if t == HA.P2TH:
                e, eh = list(TA._entries(tab)), list(TA._entries(tab_h))
                assert e[:-1] == eh and e[-1][:3] == (0, IA.PH_AM, IA.BUS_ALPHA)
            else:
                assert tab.tolist() == tab_h.tolist(), IA.NAMES[t]
    assert not any(v >> 30 == 2 for t in (IA.AIR16, IA.SCALARS16) for _, ts in TA.constraints_of(mine[t][0][0]) for _, vs in ts for v in vs), "no public value is named in the new tables"


@pytest.mark.parametrize("which", [GOLDEN_NAME] + SHAPES[:4])
def test_host_key_equals_the_oracles_setup_and_holds_no_opened_word(oracle, which):
    v = view_of(oracle, which)
    R, F, b, Q = shape(v)
    o = IA.order(R, F, b, Q, v["W"], len(v["pubs"]))
    kt = IA.key_tables(v)
    pre = [kt[t] for t in o]
    lns = IA.log_rows(R, F, b, Q, v["W"], len(v["pubs"]))
    lns = [lns[t] for t in o]
    sh = (1, 12, 4)
    root = oracle.machine_setup(pre, lns, oracle.default_params(*sh)).tolist()
    assert fri16_identity_key_host(v, Params(*sh)).tolist() == root
    if which in (GOLDEN_NAME, SHAPES[0]):
        assert fri16_identity_key_host(v, Params(2, 7, 0)).tolist() == oracle.machine_setup(pre, lns, oracle.default_params(2, 7, 0)).tolist()
        # other opened values, public VALUES and challenges under the same roots and the same NP: the same key
        other = dict(v, opened=[[1, 2, 3, 4]] * (2 * v["W"] + 8), pubs=[(c + 9) % P for c in v["pubs"]], betas=[[(c + 5) % P for c in bt] for bt in v["betas"]],
                     consts={k: [(c + 1) % P for c in e] for k, e in v["consts"].items()}, alpha=[5, 6, 7, 8], capacity=[(c + 1) % P for c in v["capacity"]])
        assert fri16_identity_key_host(other, Params(*sh)).tolist() == root
        for name in ("troot", "qroot"):                      # either root changed: another key
            moved = dict(v, **{name: [(v[name][0] + 1) % P] + list(v[name][1:])})
            assert fri16_identity_key_host(moved, Params(*sh)).tolist() != root
        assert fri16_identity_key_host(dict(v, pubs=list(v["pubs"]) + [5]), Params(*sh)).tolist() != root          # another NP: another key


def test_the_oracles_proofs_are_accepted_and_read_as_the_view_says(oracle):
    """the inner proofs made here: pyverify accepts them, zkhip_fri16_view_head hands out what the restatement reads, and their AIR identity holds in plain integers"""
    for S in HONEST:
        proof, log_n, pubs, s = IA.oracle_proof(oracle, *S, pow_bits=POW_BITS)
        assert pyverify.verify(proof.tobytes(), log_n, S[4], pubs, log_blowup=s[0], num_queries=s[1], pow_bits=s[2], logup_pairs=0, log_fold=4, log_final=s[5], hash_width=24)
        v = view_of(oracle, S)
        if log_n >= 5:                                       # (the library's view entries take proofs of 2^5 rows and more)
            assert fri16_view_head(proof, log_n, S[4], pubs, Params(*s)) == {k: v[k] for k in ("opened", "alpha", "pubs")}
        assert HA.head_of(v)["alpha"] == v["alpha"] and IA.identity_holds(v)
    assert IA.identity_holds(view_of(oracle, GOLDEN_NAME))
    assert not IA.identity_holds(HA.honest_view(1, 0, 1, 4, 8, 1))      # random columns satisfy no AIR


# ------------------------------------------------------------------ (2) constraints and buses; the oracle's prover, the library's verifier
@pytest.mark.parametrize("which", [GOLDEN_NAME] + HONEST)
def test_restated_traces_satisfy_every_constraint_and_balance_every_bus(oracle, which):
    v = view_of(oracle, which)
    assert A.consistent(v)
    main, pre, progs, tabs, pub = machine_of(oracle, which)
    assert pub == [int(x) for x in v["pubs"]]
    assert violations(main, pre, progs, tabs, pub) == ([], {})


@pytest.mark.parametrize("which,sh", [(HONEST[0], (1, 10, 2)), (GOLDEN_NAME, (2, 7, 0))])
def test_the_oracle_proves_the_restated_arrays_and_the_library_verifies(oracle, which, sh):
    O = oracle
    v = view_of(oracle, which)
    R, F, b, Q = shape(v)
    pb, W, NP = v["pow_bits"], v["W"], len(v["pubs"])
    main, pre, progs, tabs, pub = machine_of(oracle, which)
    lns, ws, pws = shape_of(main, pre)
    oprm, prm = O.default_params(*sh), Params(*sh)
    root = O.machine_setup(pre, lns, oprm)
    assert fri16_identity_key_host(v, prm).tolist() == root.tolist()
    proof = O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm)
    assert _lib.load().zkhip_fri16_identity_proof_size(R, F, b, Q, pb, W, NP, C.byref(prm)) == proof.size
    assert O.verify_machine_keyed(proof, lns, ws, pws, root, progs, tabs, pub, oprm) == 0
    assert verify_fri16_identity(proof, pub, R, F, b, Q, pb, W, root, prm)[0] == 0
    for k in range(NP):                                      # any inner public value changed
        bad = list(pub)
        bad[k] = (bad[k] + 1) % P
        assert verify_fri16_identity(proof, bad, R, F, b, Q, pb, W, root, prm)[0] != 0, k
    bad_root = root.copy()
    bad_root[3] = (int(bad_root[3]) + 1) % P
    assert verify_fri16_identity(proof, pub, R, F, b, Q, pb, W, bad_root, prm)[0] != 0
    assert verify_fri16_identity(proof, pub + [0], R, F, b, Q, pb, W, root, prm)[0] != 0


# ------------------------------------------------------------------ (3) heights over the shape space
def test_no_shape_of_the_sweep_has_nine_tables_of_one_height():
    """the floors 2^6 (AIR16) and 2^7 (SCALARS16): over R 1..5 x F 0..8 x log_blowup 1..2 x Q x W x NP no shape the fold-16 machines take has nine of the thirteen
    tables at one height, so the refusal (kept, with its message) meets none of them"""
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
                            assert max(lrs.count(h) for h in set(lrs)) <= 8 and IA.shape_ok(R, F, b, Q, 4, W, NP), (R, F, b, Q, W, NP)
                            ln = C.c_int(0)
                            n = lib.zkhip_fri16_identity_describe(R, F, b, Q, 4, W, NP, 12, 1, None, 0, C.byref(ln), None, None, None)
                            assert n > 0 and ln.value == lrs[IA.order(R, F, b, Q, W, NP)[12]], (R, F, b, Q, W, NP, lib.zkhip_last_error())
                            taken += 1
    assert taken > 4000
    assert lib.zkhip_fri16_identity_describe(1, 0, 1, 4, 4, 8, 0, 0, 0, None, 0, None, None, None, None) == 0 and b"1 .. 30 inner public values" in lib.zkhip_last_error()


# ------------------------------------------------------------------ (4) forgeries, and what rejects each
class Forge:
    """a machine's arrays by table number; caught(): names of the failing constraints ("<table>: <name>") and the unbalanced buses"""
    NAMED = (HA.P2TH, HA.QUERY16H, HA.ROWSUM16H, IA.AIR16, IA.SCALARS16)

    def __init__(self, view, scalars_acc=None):
        self.v = view
        R, F, b, Q = shape(view)
        self.W, self.NP, self.n = view["W"], len(view["pubs"]), 4 * R + F
        self.o = IA.order(R, F, b, Q, self.W, self.NP)
        self.at = {t: i for i, t in enumerate(self.o)}
        self.main, self.pre, self.progs, self.tabs, self.pub = IA.machine(view, scalars_acc=scalars_acc)
        self.head = HA.head_of(view)
        self.G = self.W // 4

    def caught(self, fn=None):
        m, p = [x.copy() for x in self.main], [None if x is None else x.copy() for x in self.pre]
        if fn is not None:
            out = fn({t: m[i] for t, i in self.at.items()}, {t: p[i] for t, i in self.at.items()})
            for t, arr in (out or {}).items():               # a table made anew
                m[self.at[t]] = arr
        names = set()
        for i, (rows, prog) in enumerate(zip(combined(m, p), self.progs)):
            t = self.o[i]
            cn = IA.constraint_names(t, self.W, self.NP, self.n, self.v["pow_bits"]) if t in self.NAMED else None
            for c, _ in P24.check_constraints(prog, rows, self.pub):
                names.add(IA.NAMES[t] + (": " + cn[c] if cn else ""))
        return names, {bus for bus, _ in A.bus_balance(m, p, self.tabs)}

    def air_anew(self, opened=None, alpha=None):
        lr = self.main[self.at[IA.AIR16]].shape[0].bit_length() - 1
        return IA.air16_main(self.v["opened"] if opened is None else opened, self.head["alpha"] if alpha is None else alpha, self.head["zeta"], self.W, self.n, lr)[0]

    def scalars_anew(self, opened=None, zeta=None, acc=None):
        return IA.scalars16_main(self.v["opened"] if opened is None else opened, self.head["alpha"], self.head["zeta"] if zeta is None else zeta, self.W, self.n, acc)[0]


@pytest.fixture(scope="module")
def honest(oracle):
    """W = 40, NP = 7: ten groups; four sponge rows up to alpha, so the loc rows are OPENED16's rows 5 .. 24, the nxt rows 25 .. 44, the quotient rows 45 .. 48"""
    f = Forge(view_of(oracle, HONEST[1]))
    assert f.caught() == (set(), set()) and f.G == 10
    return f


def sc(f, name):
    c = IA.scalars_cols(f.n)[0][name]
    return slice(c, c + 4)


def ai(name):
    return slice(IA.AI[name], IA.AI[name] + 4)


def test_a_changed_in_one_air16_row_is_caught_by_the_value_bus(honest):
    """AIR16 made anew from the changed value, every constraint of its own holding: OPENED16 sent another word (and the accumulator moved with it)"""
    opened = [list(e) for e in honest.v["opened"]]
    opened[8][2] = (opened[8][2] + 1) % P                     # a of group 2
    names, buses = honest.caught(lambda m, p: {IA.AIR16: honest.air_anew(opened)})
    assert names == set() and IA.BUS_OH0 in buses and IA.BUS_OH1 not in buses and IA.BUS_ACC in buses


def test_dn_taken_from_the_even_nxt_row_is_caught_by_its_key(honest):
    """DN of group 1 is nxt[5] where nxt[7] belongs: the value lies in the second half of an EVEN nxt row, which sends nothing, and the row's key names the odd one"""
    W = honest.W
    opened = [list(e) for e in honest.v["opened"]]
    opened[W + 7] = list(opened[W + 5])
    names, buses = honest.caught(lambda m, p: {IA.AIR16: honest.air_anew(opened)})
    assert names == set() and IA.BUS_OH1 in buses and IA.BUS_OH0 not in buses
    pre = honest.pre[honest.at[HA.OPENED16]]
    nxt = pre[W // 2:W]
    assert not nxt[:, IA.OQ_H0].any() and nxt[:, IA.OQ_H1].tolist() == [0, 1] * (W // 4)


def test_another_alpha_throughout_air16_is_caught_by_the_first_row_receive(honest):
    alpha = [(c + 1) % P for c in honest.head["alpha"]]
    names, buses = honest.caught(lambda m, p: {IA.AIR16: honest.air_anew(alpha=alpha)})
    assert names == set() and IA.BUS_KA in buses and IA.BUS_KSELT not in buses


def test_alpha_changed_in_one_row_is_caught_by_the_transition_constraint(honest):
    def fn(m, p):
        m[IA.AIR16][3, ai("ALPHA")] = [(c + 1) % P for c in honest.head["alpha"]]
    names, buses = honest.caught(fn)
    assert "AIR16: ALPHA' = ALPHA" in names and IA.BUS_KA not in buses


def test_accin_of_row_1_that_is_not_acco_of_row_0_is_caught(honest):
    def fn(m, p):
        m[IA.AIR16][1, ai("ACCIN")] = [(int(c) + 1) % P for c in m[IA.AIR16][1, ai("ACCIN")]]
    names, _ = honest.caught(fn)
    assert "AIR16: ACCIN' = ACCO" in names and "AIR16: ACCIN = 0 on the first row" not in names


def test_acco_sent_from_another_row_is_caught_by_the_last_flag(honest):
    """SCALARS16 takes the accumulator of the last group but one: only the LAST row sends, and its flag is preprocessed"""
    tab = honest.tabs[honest.at[IA.AIR16]]
    assert [e for e in TA._entries(tab) if e[2] == IA.BUS_ACC][0][:2] == (0, IA.AP_LAST)
    pre = honest.pre[honest.at[IA.AIR16]]
    assert pre[:, IA.AP_LAST].tolist() == [0] * (honest.G - 1) + [1] + [0] * (pre.shape[0] - honest.G)
    acc = [int(c) for c in honest.main[honest.at[IA.AIR16]][honest.G - 2, ai("ACCO")]]
    names, buses = honest.caught(lambda m, p: {IA.SCALARS16: honest.scalars_anew(acc=acc)})
    assert IA.BUS_ACC in buses


def test_a_zeta_in_scalars16_that_is_not_the_drawn_one_is_caught_by_the_bus_from_p2th(honest):
    zeta = [(c + 1) % P for c in honest.head["zeta"]]
    names, buses = honest.caught(lambda m, p: {IA.SCALARS16: honest.scalars_anew(zeta=zeta)})
    assert HA.BUS_ZETA in buses and not any(n.startswith("SCALARS16: squaring") or "INVF" in n for n in names)
    assert honest.pre[honest.at[HA.P2TH]][HA.head_rows(honest.W, honest.NP)[0], HA.PH_ZM] == 2     # zeta has two receivers in this key


def test_one_wrong_squaring_is_caught(honest):
    def fn(m, p):
        m[IA.SCALARS16][:, sc(honest, "ZP2")] = [(int(c) + 1) % P for c in m[IA.SCALARS16][0, sc(honest, "ZP2")]]
    names, _ = honest.caught(fn)
    assert "SCALARS16: squaring" in names and "SCALARS16: every row repeats row 0" not in names


def test_a_wrong_invf_is_caught(honest):
    def fn(m, p):
        m[IA.SCALARS16][:, sc(honest, "INVF")] = [(int(c) + 1) % P for c in m[IA.SCALARS16][0, sc(honest, "INVF")]]
    names, _ = honest.caught(fn)
    assert "SCALARS16: (ZETA - 1) INVF = 1" in names


def test_a_changed_qz_is_caught_by_the_value_bus(honest):
    W = honest.W
    opened = [list(e) for e in honest.v["opened"]]
    opened[2 * W + 3][0] = (opened[2 * W + 3][0] + 1) % P      # QZ_3: the second half of the second quotient row
    names, buses = honest.caught(lambda m, p: {IA.SCALARS16: honest.scalars_anew(opened)})
    assert not any(n.startswith("SCALARS16") for n in names) and IA.BUS_OH1 in buses and IA.BUS_OH0 not in buses


def test_a_padding_row_of_scalars16_that_is_not_row_0_is_caught(honest):
    def fn(m, p):
        m[IA.SCALARS16][5, sc(honest, "QUO")] = [1, 2, 3, 4]
    names, buses = honest.caught(fn)
    assert "SCALARS16: every row repeats row 0" in names and buses == set()
    def zero(m, p):
        m[IA.SCALARS16][1:] = 0
    assert "SCALARS16: every row repeats row 0" in honest.caught(zero)[0]


def test_an_all_zero_padding_row_of_air16_satisfies_the_program_and_moves_nothing(honest):
    main, pre = honest.main[honest.at[IA.AIR16]], honest.pre[honest.at[IA.AIR16]]
    assert not main[honest.G:].any() and not pre[honest.G:].any()


def test_columns_that_satisfy_no_air_are_rejected_with_every_table_filled_honestly():
    """the one that matters: an inner proof whose opened columns are low-degree and consistently opened -- everything the head machine proves -- and satisfy no
    AIR.  With SCALARS16 taking AIR16's accumulator the identity's own constraint fails; with QUO (zeta^N - 1) there, the accumulator bus does not balance"""
    v = HA.honest_view(1, 1, 1, 3, 40, 7)
    assert not IA.identity_holds(v)
    names, buses = Forge(v, scalars_acc="air").caught()
    assert names == {"SCALARS16: ACC = QUO (ZP_n - 1)"} and buses == set()
    names, buses = Forge(v).caught()
    assert names == set() and buses == {IA.BUS_ACC}
