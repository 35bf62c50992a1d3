"""The fold-by-16 HEAD machine (zktls_amd/csrc/fri16_chip.hip: the row-paths machine with the head of the transcript inside), CPU side: the library's programs,
interaction tables and host key against the Python restatement (tests/fri16_head_air.py) and the oracle's setup; the six unchanged tables against the row-paths
machine's words; the restatement's traces under every constraint and every bus in plain integers; the machine under the oracle's prover and the library's verifier;
the head view of the committed fold-16 proofs; the rule of table heights over the shape space; and forgeries, each built here on an honest trace and shown
rejected BY WHAT (a named constraint or a bus)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fri16_air as A
import fri16_head_air as HA
import fri16_openings_air as OA
import fri16_rowpaths_air as RPA
import fri16_transcript_air as TA
import poseidon2_24_air as P24
import poseidon2_air as P2
import pyref
import recursion_air as RA
from test_fri16_chip_cpu import GOLDEN, combined, load, shape_of, violations
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import fri16_head_describe, fri16_head_key_host, fri16_rowpaths_describe, fri16_view_head, verify_fri16_head

P = 2013265921
GOLDEN_NAME = "v3_r0_9x8"
HONEST = [(1, 0, 1, 4, 8, 1), (1, 1, 1, 3, 40, 7)]           # (R, F, b, Q, W, NP): 19 and 25 stream words up to alpha (partial rows of three words and of one)
# shapes for the words alone (no trace is made): NP = 6 and 30 give 24 and 48 stream words, no partial row; 7 a partial row of one word; W up to 128
SHAPES = [(1, 0, 1, 4, 8, 1), (1, 1, 1, 3, 40, 7), (2, 2, 2, 11, 8, 6), (2, 0, 1, 3, 40, 14), (3, 8, 2, 50, 128, 30), (1, 0, 1, 4, 128, 3)]
KEY_SHAPES = [(1, 0, 1, 4, 8, 1), (1, 1, 1, 3, 40, 7), (1, 0, 1, 4, 8, 6), (1, 0, 1, 4, 40, 14), (1, 1, 1, 3, 8, 30), (1, 0, 1, 4, 128, 3)]      # small domains: the views are made in Python


@functools.lru_cache(maxsize=None)
def view_of(which):
    """a committed fixture by name, or an honest synthetic instance by (R, F, b, Q, W, NP)"""
    return HA.golden_view(which, GOLDEN, load) if isinstance(which, str) else HA.honest_view(*which)


@functools.lru_cache(maxsize=None)
def machine_of(which):
    return HA.machine(view_of(which))


@functools.lru_cache(maxsize=None)
def key_view(R, F, b, Q, W, NP):
    """a view for the KEY alone: the row-paths machine's honest view (roots, final coefficients) and NP public values -- nothing else reaches the key"""
    return dict(RPA.honest_view(R, F, b, Q, W), pubs=list(range(1, NP + 1)))


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


# ------------------------------------------------------------------ (1) programs, interaction tables, key
@pytest.mark.parametrize("which", [GOLDEN_NAME] + SHAPES)
def test_describe_equals_the_python_restatement(oracle, which):
    if isinstance(which, str):
        v = view_of(which)
        R, F, b, Q, pb, W, NP = shape(v) + (v["pow_bits"], v["W"], len(v["pubs"]))
        assert NP == 3 and HA.head_rows(W, NP) == (3, 3 + 1 + W + 4)      # 21 stream words: a partial third row
    else:
        R, F, b, Q, W, NP = which
        pb = TA.POW_BITS
    progs, tabs, lrs, o, mains = HA.programs(R, F, b, pb, W, NP), HA.interactions(R, F + b), HA.log_rows(R, F, b, Q, W, NP), HA.order(R, F, b, Q, W, NP), HA.main_widths(F + b)
    assert sorted(o) == list(range(11)) and all(lrs[o[i]] >= lrs[o[i + 1]] for i in range(10))
    assert lrs[HA.OPENED16] == A.lg(W + 4, 6) and lrs[HA.P2TH] == A.lg(HA.head_rows(W, NP)[1] + TA.chain_rows(R, F, Q)[2])
    for which_, t in enumerate(o):
        prog, ln, mw, pw, table = fri16_head_describe(R, F, b, Q, pb, W, NP, which_, 0)
        tab = fri16_head_describe(R, F, b, Q, pb, W, NP, which_, 1)[0]
        assert (table, ln, mw, pw) == (t, lrs[t], mains[t], HA.PRE_WIDTHS[t])
        assert prog.tolist() == progs[t].tolist(), HA.NAMES[t]
        assert tab.tolist() == tabs[t].tolist(), HA.NAMES[t]
        assert int(prog[4]) == NP
        assert oracle.air_validate(prog, mw + pw, NP) == 1
        assert oracle.air_log_quotient_degree(prog) == 1      # degree 3 with the selector
        assert int(tab[1]) <= 64 and mw % 4 == 0 and pw % 4 == 0
        for _, mult, _, _ in TA._entries(tab):                # every multiplicity of the head is preprocessed (ROOTS' fold rows and P24's flags are the kinds' before)
            if t in (HA.P2TH, HA.OPENED16, HA.QUERY16H, HA.ROWSUM16H):
                assert mult < pw


@pytest.mark.parametrize("S", [(1, 1, 1, 8, 8, 3), (2, 2, 2, 11, 24, 6), (3, 8, 2, 50, 128, 30)])
def test_six_tables_are_the_row_paths_machines_word_for_word(S):
    R, F, b, Q, W, NP = S
    mine = {d[4]: (d[0], fri16_head_describe(R, F, b, Q, 4, W, NP, w, 1)[0]) for w, d in ((w, fri16_head_describe(R, F, b, Q, 4, W, NP, w, 0)) for w in range(11))}
    theirs = {d[4]: (d[0], fri16_rowpaths_describe(R, F, b, Q, 4, W, w, 1)[0]) for w, d in ((w, fri16_rowpaths_describe(R, F, b, Q, 4, W, w, 0)) for w in range(10))}
    for t in HA.UNCHANGED:
        a, c = mine[t][0].tolist(), theirs[t][0].tolist()
        assert (a[4], c[4]) == (NP, 40) and a[:4] + a[5:] == c[:4] + c[5:], HA.NAMES[t]       # the public-value count in the header, and nothing else
        assert mine[t][1].tolist() == theirs[t][1].tolist(), HA.NAMES[t]
    # the three replaced programs keep what the issue says they keep
    q_new, q_old = TA.constraints_of(mine[HA.QUERY16H][0]), TA.constraints_of(theirs[RPA.QUERY16][0])
    assert q_new[36:] == q_old[28:] and len(q_new) == len(q_old) + 8                          # the eight products; 28 c' = c, ZNX, OFFQ where 28 "= public" stood
    r_new, r_old = TA.constraints_of(mine[HA.ROWSUM16H][0]), TA.constraints_of(theirs[RPA.ROWSUM16][0])
    assert len(r_new) == len(r_old)
    p_new, p_old = TA.constraints_of(mine[HA.P2TH][0]), TA.constraints_of(theirs[RPA.P2T][0])
    assert len(p_new) == len(p_old) + 8 + NP
    assert not any(v >> 30 == 2 for t in (HA.QUERY16H, HA.ROWSUM16H, HA.OPENED16, HA.ROOTS) for _, ts in TA.constraints_of(mine[t][0]) for _, vs in ts for v in vs), \
        "no public value is named outside P2TH"


@pytest.mark.parametrize("which", [GOLDEN_NAME] + KEY_SHAPES)
def test_host_key_equals_the_oracles_setup_and_holds_no_opened_word(oracle, which):
    v = view_of(which) if isinstance(which, str) else key_view(*which)
    R, F, b, Q = shape(v)
    o = HA.order(R, F, b, Q, v["W"], len(v["pubs"]))
    kt = HA.key_tables(v)
    pre = [kt[t] for t in o]
    lns = HA.log_rows(R, F, b, Q, v["W"], len(v["pubs"]))
    lns = [lns[t] for t in o]
    sh = (1, 12, 4)
    root = oracle.machine_setup(pre, lns, oracle.default_params(*sh)).tolist()
    assert fri16_head_key_host(v, Params(*sh)).tolist() == root
    if which in (GOLDEN_NAME, KEY_SHAPES[0]):
        assert fri16_head_key_host(v, Params(2, 7, 0)).tolist() == oracle.machine_setup(pre, lns, oracle.default_params(2, 7, 0)).tolist()
        # other rows, paths, values, challenges, constants, capacity, opened values and public VALUES under the same roots and the same NP: the same key
        other = dict(v, trows=[[(c + 1) % P for c in r] for r in v["trows"]], consts={k: [(c + 1) % P for c in e] for k, e in v["consts"].items()},
                     capacity=[(c + 1) % P for c in v["capacity"]], pubs=[(c + 9) % P for c in v["pubs"]], opened=[[1, 2, 3, 4]] * (2 * v["W"] + 8),
                     betas=[[(c + 5) % P for c in bt] for bt in v["betas"]])
        assert fri16_head_key_host(other, Params(*sh)).tolist() == root
        for name in ("troot", "qroot"):                      # either root changed: another key
            moved = dict(v, **{name: [(v[name][0] + 1) % P] + list(v[name][1:])})
            assert fri16_head_key_host(moved, Params(*sh)).tolist() != root
        assert fri16_head_key_host(dict(v, pubs=list(v["pubs"]) + [5]), Params(*sh)).tolist() != root          # another NP: another header, another key
        assert fri16_head_key_host(dict(v, pow_bits=v["pow_bits"] + 1), Params(*sh)).tolist() != root


def test_the_head_of_the_chain_is_the_committed_proofs_transcript():
    """the restated duplex rules against pyverify's own transcript of the committed proof: alpha, and -- through the views of the machines before -- the capacity
    the commit phase finds and all eight constants"""
    v = view_of(GOLDEN_NAME)
    h = HA.head_of(v)
    assert h["alpha"] == v["alpha"] and h["capacity"] == [int(c) for c in v["capacity"]]
    got = HA.derived_consts(v, h)
    assert all(got[n] == [int(c) for c in v["consts"][n]] for n in OA.CONSTS)
    R, F, b, Q = shape(v)
    assert len(h["inputs"]) == HA.head_rows(v["W"], 3)[1] and h["inputs"][0] == HA.header(R, F, b, Q, v["pow_bits"], v["W"], 3)[:8] + [0] * 8
    for NP in range(0, 31):                                  # the row count of the head at every NP: ceil((18 + NP) / 8) + 1 + W + 4
        pubs, rnd = list(range(NP)), list(range(8))
        hc = HA.head_chain(HA.header(1, 0, 1, 4, 4, 8, NP), rnd, pubs, rnd, [[1, 2, 3, 4]] * 24)
        assert len(hc["inputs"]) == -(-(18 + NP) // 8) + 1 + 12
        k = (18 + NP) % 8
        if k:                                                # the partial row keeps the previous output's rate words behind its own
            a = HA.head_rows(8, NP)[0]
            assert hc["inputs"][a - 1][k:] == [int(x) for x in pyref.poseidon2(hc["inputs"][a - 2])][k:]


# ------------------------------------------------------------------ (2) constraints and buses; the oracle's prover, the library's verifier
@pytest.mark.parametrize("which", [GOLDEN_NAME] + HONEST)
def test_restated_traces_satisfy_every_constraint_and_balance_every_bus(which):
    v = view_of(which)
    assert A.consistent(v)
    main, pre, progs, tabs, pub = machine_of(which)
    assert pub == [int(x) for x in v["pubs"]]                 # the inner proof's own public values and nothing else
    assert violations(main, pre, progs, tabs, pub) == ([], {})


@pytest.mark.parametrize("which,sh", [(HONEST[0], (1, 10, 2)), (HONEST[1], (1, 10, 2)), (GOLDEN_NAME, (2, 7, 0))])
def test_the_oracle_proves_the_restated_arrays_and_the_library_verifies(oracle, which, sh):
    O = oracle
    v = view_of(which)
    R, F, b, Q = shape(v)
    pb, W, NP = v["pow_bits"], v["W"], len(v["pubs"])
    main, pre, progs, tabs, pub = machine_of(which)
    lns, ws, pws = shape_of(main, pre)
    oprm, prm = O.default_params(*sh), Params(*sh)
    root = O.machine_setup(pre, lns, oprm)
    assert fri16_head_key_host(v, prm).tolist() == root.tolist()
    proof = O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm)
    assert _lib.load().zkhip_fri16_head_proof_size(R, F, b, Q, pb, W, NP, C.byref(prm)) == proof.size
    assert O.verify_machine_keyed(proof, lns, ws, pws, root, progs, tabs, pub, oprm) == 0
    assert verify_fri16_head(proof, pub, R, F, b, Q, pb, W, root, prm)[0] == 0
    for k in range(NP):                                      # any inner public value changed
        bad = list(pub)
        bad[k] = (bad[k] + 1) % P
        assert verify_fri16_head(proof, bad, R, F, b, Q, pb, W, root, prm)[0] != 0, k
    bad_root = root.copy()
    bad_root[3] = (int(bad_root[3]) + 1) % P
    assert verify_fri16_head(proof, pub, R, F, b, Q, pb, W, bad_root, prm)[0] != 0
    assert verify_fri16_head(proof, pub + [0], R, F, b, Q, pb, W, root, prm)[0] != 0                  # another NP: another machine


# ------------------------------------------------------------------ (3) the head view of the committed proofs
def test_view_head_of_the_golden_proof_equals_the_restatements_parse():
    g = GOLDEN[GOLDEN_NAME]
    prm = Params(*g["shape"])
    mine = view_of(GOLDEN_NAME)
    got = fri16_view_head(load(GOLDEN_NAME), g["log_n"], g["width"], g["public"], prm)
    assert got == {k: mine[k] for k in ("opened", "alpha", "pubs")}
    assert len(got["opened"]) == 2 * g["width"] + 8
    words = np.frombuffer(load(GOLDEN_NAME).tobytes(), dtype=np.uint32).copy()
    words[-1] ^= 1
    with pytest.raises(_lib.ZkHipError):                      # fails like zkhip_fri16_view_shard
        fri16_view_head(words.view(np.uint8), g["log_n"], g["width"], g["public"], prm)
    with pytest.raises(_lib.ZkHipError, match="fold-by-16"):  # a fold-by-2 shape
        fri16_view_head(load(GOLDEN_NAME), g["log_n"], g["width"], g["public"], Params(1, 100, 16))
    words = np.frombuffer(load(GOLDEN_NAME).tobytes(), dtype=np.uint32).copy()
    words[1] = 7
    with pytest.raises(_lib.ZkHipError, match="program"):     # a version-7 proof says so in its second word
        fri16_view_head(words.view(np.uint8), g["log_n"], g["width"], g["public"], prm)


def test_view_head_refuses_lookup_pairs_a_code_group_and_the_width_16_hash(oracle):
    name = "v8_groups_r0_lookup_8x16"
    g = GOLDEN[name]
    with pytest.raises(_lib.ZkHipError, match="lookup pairs"):
        fri16_view_head(load(name), g["log_n"], g["width"], g["public"], Params(*g["shape"]))
    log_n, w = 8, 16
    s8 = (2, 3, 0, 0, 4, 0, 24, 4)                            # version 8: the first four columns under a commitment of their own
    proof = oracle.prove_shard(oracle.gen_trace(7, 5, log_n, w), [1, 2, 3], oracle.default_params(*s8))
    with pytest.raises(_lib.ZkHipError, match="code group"):
        fri16_view_head(proof, log_n, w, [1, 2, 3], Params(*s8))
    s16 = (2, 3, 0, 0, 4, 0, 16)                              # fold by 16 with the width-16 hash
    proof = oracle.prove_shard(oracle.gen_trace(7, 5, log_n, w), [1, 2, 3], oracle.default_params(*s16))
    with pytest.raises(_lib.ZkHipError, match="width-16 hash"):
        fri16_view_head(proof, log_n, w, [1, 2, 3], Params(*s16))


# ------------------------------------------------------------------ (4) heights over the shape space
def test_at_most_eight_tables_of_one_height_over_the_shape_space():
    """the rule: a shape is taken exactly when NP is 1 .. 30 and no height is shared by more than 8 of the eleven tables.  The sweep reports what is refused: every
    shape at NP = 0 (by its own message), and the shapes it counts below by the height rule"""
    lib = _lib.load()
    taken, by_np, by_height = 0, 0, []
    for R in range(1, 6):
        for F in range(0, 9):
            for b in (1, 2):
                if not A.shape_ok(R, F, b, 1):
                    continue
                for Q in (1, 2, 50, 100, 1024):
                    for W in (8, 16, 24, 128, 1024):
                        for NP in (0, 3, 30):
                            ln = C.c_int(0)
                            n = lib.zkhip_fri16_head_describe(R, F, b, Q, 4, W, NP, 10, 1, None, 0, C.byref(ln), None, None, None)
                            if NP == 0:
                                assert n == 0 and b"1 .. 30 inner public values" in lib.zkhip_last_error()
                                by_np += 1
                                continue
                            lrs = HA.log_rows(R, F, b, Q, W, NP)
                            ok = max(lrs.count(h) for h in set(lrs)) <= 8
                            assert ok == HA.shape_ok(R, F, b, Q, 4, W, NP)
                            if ok:
                                assert n > 0 and ln.value == lrs[HA.order(R, F, b, Q, W, NP)[10]]
                                taken += 1
                            else:
                                assert n == 0 and b"at most 8 tables of one height" in lib.zkhip_last_error()
                                by_height.append((R, F, b, Q, W, NP))
    print("fri16 head machine: %d shapes taken, %d refused for NP = 0, %d refused by the height rule %s" % (taken, by_np, len(by_height), by_height[:8]))
    assert taken + len(by_height) == 2 * by_np and taken > 4000
    rule = lambda lrs: max(lrs.count(h) for h in set(lrs)) <= HA.MAX_SAME_HEIGHT
    assert rule([5] * 8 + [6, 6, 6]) and not rule([5] * 9 + [6, 6]) and not rule([7] * 11)


# ------------------------------------------------------------------ (5) forgeries, and what rejects each
class Forge:
    """a machine's arrays by table number; caught(): names of the failing constraints ("<table>: <name>") and the unbalanced buses"""
    NAMED = (HA.P2TH, HA.QUERY16H, HA.ROWSUM16H, HA.OPENED16)

    def __init__(self, view):
        self.v = view
        R, F, b, Q = shape(view)
        self.W, self.NP, self.log_n = view["W"], len(view["pubs"]), 4 * R + F
        self.o = HA.order(R, F, b, Q, self.W, self.NP)
        self.at = {t: i for i, t in enumerate(self.o)}
        self.main, self.pre, self.progs, self.tabs, self.pub = HA.machine(view)
        self.a, self.hd = HA.head_rows(self.W, self.NP)
        self.head = HA.head_of(view)

    def caught(self, fn=None):
        m, p = [x.copy() for x in self.main], [None if x is None else x.copy() for x in self.pre]
        if fn is not None:
            out = fn({t: m[i] for t, i in self.at.items()}, {t: p[i] for t, i in self.at.items()})
            for t, arr in (out or {}).items():               # a table made anew
                m[self.at[t]] = arr
        names = set()
        for i, (rows, prog) in enumerate(zip(combined(m, p), self.progs)):
            t = self.o[i]
            cn = HA.constraint_names(t, self.W, self.NP, self.log_n, self.v["pow_bits"]) if t in self.NAMED else None
            for c, _ in P24.check_constraints(prog, rows, self.pub):
                names.add(HA.NAMES[t] + (": " + cn[c] if cn else ""))
        return names, {bus for bus, _ in A.bus_balance(m, p, self.tabs)}

    def p2th_row(self, r, change):
        """P2TH with row r's input state changed and the row's permutation made anew (the rows behind it stay)"""
        def fn(m, p):
            s = list(self.head["inputs"][r])
            change(s)
            m[HA.P2TH][r] = np.array(P2.row(s)[0][:TA.T_WIDTH], dtype=np.uint64).astype(np.uint32)
        return fn

    def opened_made_anew(self, opened, fa=None):
        lr = self.main[self.at[HA.OPENED16]].shape[0].bit_length() - 1
        return HA.opened16_main(opened, self.head["fa"] if fa is None else fa, self.W, lr)[0]


@pytest.fixture(scope="module")
def honest():
    """W = 40, NP = 7: 25 stream words -- four rows up to alpha, the fourth partial with one word; the quotient root on row 4; rows 5 .. 48 the opened values"""
    f = Forge(view_of(HONEST[1]))
    assert f.caught() == (set(), set()) and (f.a, f.hd) == (4, 49)
    return f


def col(m, name):
    c = RA.query_cols()[name] - OA.Q16_PRE
    return slice(c, c + 4)


def test_an_opened_word_changed_in_opened16_only_is_caught_by_the_opened_value_bus(honest):
    """OPENED16 made anew from the changed value, every constraint of its own holding: P2TH absorbed another word (and the sum moved with it)"""
    opened = [list(e) for e in honest.v["opened"]]
    opened[6][1] = (opened[6][1] + 1) % P                     # row 3, first half
    names, buses = honest.caught(lambda m, p: {HA.OPENED16: honest.opened_made_anew(opened)})
    assert names == set() and HA.BUS_OV0 in buses and HA.BUS_OV1 not in buses and HA.BUS_YL in buses


def test_two_opened16_rows_swapped_are_caught_by_the_row_number_in_the_tuple(honest):
    opened = [list(e) for e in honest.v["opened"]]
    opened[4:6], opened[6:8] = opened[6:8], opened[4:6]       # rows 2 and 3 of the first segment
    names, buses = honest.caught(lambda m, p: {HA.OPENED16: honest.opened_made_anew(opened)})
    assert names == set() and {HA.BUS_OV0, HA.BUS_OV1} <= buses


def test_yl_changed_in_query16hs_whole_column_is_caught_by_the_first_row_receive(honest):
    def fn(m, p):
        m[HA.QUERY16H][:, col(m, "YL")] = [(int(c) + 1) % P for c in honest.v["consts"]["YL"]]
    names, buses = honest.caught(fn)
    assert HA.BUS_YL in buses and not any("' = " in n for n in names)       # one constant down the table still; P1 no longer fits, which a forger could mend


def test_a_constant_changed_in_one_query16h_row_is_caught_by_the_transition_constraint(honest):
    def fn(m, p):
        m[HA.QUERY16H][1, col(m, "YQ")] = [(int(c) + 1) % P for c in honest.v["consts"]["YQ"]]
    names, buses = honest.caught(fn)
    assert "QUERY16H: YQ' = YQ" in names and HA.BUS_YQ not in buses


def test_another_fa_throughout_rowsum16h_is_caught_by_its_first_row_receive(honest):
    v = honest.v
    fa = [(int(c) + 1) % P for c in v["consts"]["FA"]]
    lr = honest.main[honest.at[HA.ROWSUM16H]].shape[0].bit_length() - 1
    rs = OA.opening_traces(v["H"], v["W"], v["trows"], v["qrows"], dict(v["consts"], FA=fa), [q[0] for q in v["queries"]], lr)[0]
    names, buses = honest.caught(lambda m, p: {HA.ROWSUM16H: rs})
    assert not any(n.startswith("ROWSUM16H") for n in names) and HA.BUS_FA in buses


def test_a_zeta_in_query16h_that_is_not_the_drawn_one_is_caught_by_the_bus_from_p2th(honest):
    zeta = [(int(c) + 1) % P for c in honest.v["consts"]["ZETA"]]
    g = pyref.two_adic_generator(honest.log_n)

    def fn(m, p):
        m[HA.QUERY16H][:, col(m, "ZETA")], m[HA.QUERY16H][:, col(m, "ZNX")] = zeta, [c * g % P for c in zeta]
    names, buses = honest.caught(fn)
    assert HA.BUS_ZETA in buses and "QUERY16H: ZNX = g ZETA" not in names and "QUERY16H: ZETA' = ZETA" not in names


def test_znx_that_is_not_g_zeta_and_offq_that_is_not_offn_squared_are_caught_by_their_constraints(honest):
    def znx(m, p):
        m[HA.QUERY16H][:, col(m, "ZNX")] = [(int(c) + 1) % P for c in honest.v["consts"]["ZNX"]]
    assert "QUERY16H: ZNX = g ZETA" in honest.caught(znx)[0]

    def offq(m, p):
        m[HA.QUERY16H][:, col(m, "OFFQ")] = [(int(c) + 1) % P for c in honest.v["consts"]["OFFQ"]]
    assert "QUERY16H: OFFQ = OFFN OFFN" in honest.caught(offq)[0]


def test_pw_carried_into_the_next_segment_is_caught_on_the_segments_first_row(honest):
    """the row where the values at zeta g begin takes PW from the row before it; everything else on the row follows from that PW"""
    W = honest.W

    def fn(m, p):
        t = m[HA.OPENED16]
        r = W // 2
        pw = [int(c) for c in t[r - 1, HA.OP_PWN:HA.OP_PWN + 4]]
        pt = pyref.ext_mul(pw, [int(c) for c in t[r, HA.OP_T:HA.OP_T + 4]])
        t[r, HA.OP_PW:HA.OP_PW + 4], t[r, HA.OP_PT:HA.OP_PT + 4], t[r, HA.OP_Y:HA.OP_Y + 4] = pw, pt, pt
        t[r, HA.OP_PWN:HA.OP_PWN + 4] = pyref.ext_mul(pw, [int(c) for c in t[r, HA.OP_FA2:HA.OP_FA2 + 4]])
    names, _ = honest.caught(fn)
    assert "OPENED16: PW = 1 on a segment's first row" in names and "OPENED16: PT = PW T" not in names


def test_a_header_word_changed_in_p2th_is_caught_by_the_header_pin(honest):
    def q_minus_one(s):
        assert s[3] == len(honest.v["queries"])
        s[3] -= 1
    names, _ = honest.caught(honest.p2th_row(0, q_minus_one))
    assert "P2TH: header pin" in names and "P2TH: permutation" not in names


def test_a_public_word_in_p2th_that_is_not_the_proofs_is_caught_by_the_public_pin(honest):
    def change(s):
        assert s[2] == honest.v["pubs"][0]                    # stream word 18: row 2, word 2
        s[2] = (s[2] + 1) % P
    names, _ = honest.caught(honest.p2th_row(2, change))
    assert "P2TH: public pin" in names and "P2TH: permutation" not in names
    def last(s):
        assert s[0] == honest.v["pubs"][6]                    # the partial row's one word
        s[0] = (s[0] + 1) % P
    assert "P2TH: public pin" in honest.caught(honest.p2th_row(3, last))[0]


def test_root_words_in_p2th_that_are_not_roots_are_caught_by_the_root_bus(honest):
    def troot(s):
        assert s[2:8] == honest.v["troot"][:6]                # the trace root sits at stream words 10 .. 17: 6 + 2 over rows 1 and 2
        s[4] = (s[4] + 1) % P
    names, buses = honest.caught(honest.p2th_row(1, troot))
    assert HA.BUS_HR in buses and not any("pin" in n for n in names)

    def troot_tail(s):
        assert s[:2] == honest.v["troot"][6:]
        s[1] = (s[1] + 1) % P
    assert HA.BUS_HR in honest.caught(honest.p2th_row(2, troot_tail))[1]

    def qroot(s):
        assert s[:8] == honest.v["qroot"]
        s[7] = (s[7] + 1) % P
    assert HA.BUS_HR in honest.caught(honest.p2th_row(honest.a, qroot))[1]


def test_a_kept_rate_word_changed_on_the_partial_row_is_caught_by_the_chain(honest):
    def change(s):
        s[5] = (s[5] + 1) % P                                 # 25 stream words: row 3 absorbs one word and keeps seven
    names, _ = honest.caught(honest.p2th_row(3, change))
    assert "P2TH: K: kept rate words follow" in names and "P2TH: public pin" not in names


def test_a_non_zero_capacity_on_row_0_is_caught(honest):
    def change(s):
        assert s[8:] == [0] * 8
        s[11] = 1
    names, _ = honest.caught(honest.p2th_row(0, change))
    assert "P2TH: row 0: the capacity is zero" in names and "P2TH: header pin" not in names


def test_a_padding_row_of_opened16_cannot_send(honest):
    """every multiplicity of OPENED16 is a preprocessed column, zero on a padding row: whatever a prover writes there -- here two values with the T that fits them,
    every constraint holding -- reaches no bus"""
    tab = honest.tabs[honest.at[HA.OPENED16]]
    assert all(mult < HA.OPN_PRE for _, mult, _, _ in TA._entries(tab))
    pre = honest.pre[honest.at[HA.OPENED16]]
    r = honest.W + 4 + 3
    assert not pre[honest.W + 4:].any()

    def fn(m, p):
        t = m[HA.OPENED16]
        v0, v1 = [5, 6, 7, 8], [9, 10, 11, 12]
        t[r, HA.OP_V:HA.OP_V + 8] = v0 + v1
        t[r, HA.OP_T:HA.OP_T + 4] = A.e_add(v0, pyref.ext_mul([int(c) for c in t[r, HA.OP_FA:HA.OP_FA + 4]], v1))
    assert honest.caught(fn) == (set(), set())
