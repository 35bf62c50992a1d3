"""The fold-by-16 OPENINGS machine (zktls_amd/csrc/fri16_chip.hip: the indices machine with the reduced openings computed in-circuit -- FOLD16C, QUERY16,
ROWSUM16 and the preprocessed ROWS table), CPU side: the library's programs and interaction tables against the Python restatement (tests/fri16_openings_air.py);
the restatement's traces under every constraint and every bus in plain integers; the key without a GPU, which holds the opened rows and no reduced opening; the
machine under the oracle's prover and the library's verifier; the openings view of the committed fold-16 proofs; and forgeries, each built here and shown
rejected BY WHAT (a named constraint or a bus)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fri16_air as A
import fri16_openings_air as OA
import fri16_paths_air as PA
import fri16_transcript_air as TA
import fri_air as FA
import poseidon2_24_air as P24
import pyref
import recursion_air as RA
from test_fri16_chip_cpu import GOLDEN, combined, load, shape_of, violations
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import (fri16_indices_describe, fri16_openings_describe, fri16_openings_key_host, fri16_view_openings, fri16_view_shard, verify_fri16_openings)

P = 2013265921
GOLDEN_NAME = "v3_r0_9x8"
SMALL = [(1, 0, 1, 4, 8), (2, 2, 2, 11, 24)]                # honest synthetic views (H <= 12: the restatement evaluates the whole domain)


@functools.lru_cache(maxsize=None)
def view_of(which):
    """a committed fixture by name, or an honest synthetic instance by (R, F, b, Q, W)"""
    return OA.golden_view(which, GOLDEN, load) if isinstance(which, str) else OA.honest_view(*which)


@functools.lru_cache(maxsize=None)
def machine_of(which):
    return OA.machine(view_of(which))


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


# ------------------------------------------------------------------ (1) programs and interaction tables
@pytest.mark.parametrize("which", [GOLDEN_NAME] + OA.HONEST_SHAPES)
def test_describe_equals_the_python_restatement(oracle, which):
    if isinstance(which, str):
        v = view_of(which)
        R, F, b, Q, pb, W = shape(v) + (v["pow_bits"], v["W"])
    else:
        R, F, b, Q, W = which
        pb = TA.POW_BITS
    progs, tabs, lrs, o, mains = OA.programs(R, F, b, pb), OA.interactions(R, F + b), OA.log_rows(R, F, b, Q, W), OA.order(R, F, b, Q, W), OA.main_widths(F + b)
    assert sorted(o) == list(range(10)) and all(lrs[o[i]] >= lrs[o[i + 1]] for i in range(9))
    assert lrs[OA.ROWSUM16] == A.lg(Q * (W // 8 + 1), 6) and lrs[OA.ROWS] == A.lg(Q * (W + 8) // 4, 6) and lrs[OA.QUERY16] == A.lg(Q)
    assert max(lrs.count(h) for h in set(lrs)) <= 8          # a keyed machine takes at most 8 tables of one height
    for which_, t in enumerate(o):
        prog, ln, mw, pw, table = fri16_openings_describe(R, F, b, Q, pb, W, which_, 0)
        tab = fri16_openings_describe(R, F, b, Q, pb, W, which_, 1)[0]
        assert (table, ln, mw, pw) == (t, lrs[t], mains[t], OA.PRE_WIDTHS[t])
        assert prog.tolist() == progs[t].tolist(), OA.NAMES[t]
        assert tab.tolist() == tabs[t].tolist(), OA.NAMES[t]
        assert oracle.air_validate(prog, mw + pw, OA.N_PUBLIC) == 1
        assert oracle.air_log_quotient_degree(prog) == 1
        assert int(tab[1]) <= 64 and mw % 4 == 0 and pw % 4 == 0


@pytest.mark.parametrize("S", [(1, 1, 1, 8, 8), (2, 2, 2, 11, 24), (3, 8, 2, 50, 128)])
def test_six_tables_are_the_indices_machines_and_fold16c_differs_in_one_column_one_constraint_and_one_send(S):
    """FINAL, P24L, COEFFS, ROOTS, P2T and SAMPLES: word for word but the public-value count in the header (word 4); FOLD16C: FOLD16B's constraints in their
    order, then XQ = X sum_j O_j w_16^bitrev(j, 4) on every row; the width grows by the column and three unused cells; the send on a chain's first row takes XQ"""
    R, F, b, Q, W = S
    lf = F + b
    mine = {d[4]: (d[0], fri16_openings_describe(R, F, b, Q, 4, W, w, 1)[0]) for w, d in ((w, fri16_openings_describe(R, F, b, Q, 4, W, w, 0)) for w in range(10))}
    theirs = {d[4]: (d[0], fri16_indices_describe(R, F, b, Q, 4, w, 1)[0]) for w, d in ((w, fri16_indices_describe(R, F, b, Q, 4, w, 0)) for w in range(8))}
    for t in (OA.FINAL, OA.P24L, OA.COEFFS, OA.ROOTS, OA.P2T, OA.SAMPLES):
        a, c = mine[t][0].tolist(), theirs[t][0].tolist()
        assert a[4] == 40 and c[4] == 8 and a[:4] + a[5:] == c[:4] + c[5:], OA.NAMES[t]
        assert mine[t][1].tolist() == theirs[t][1].tolist(), OA.NAMES[t]
    new, old = mine[OA.FOLD16C][0].tolist(), theirs[TA.FOLD16B][0].tolist()
    assert new[2] == old[2] + 4 == A.width_of(lf) + 4 and new[3] == old[3] + 1 and new[4] == 40
    cn, co = TA.constraints_of(new), TA.constraints_of(old)
    assert cn[:-1] == co
    sel, terms = cn[-1]
    XQ = A.width_of(lf)
    assert sel == 0 and terms[0] == (1, [XQ]) and len(terms) == 17
    w16 = pyref.two_adic_generator(4)
    for j in range(16):
        assert terms[1 + j] == (P - pow(w16, pyref.bitrev(j, 4), P), [A.X, A.OF + j])                 # degree 2; a zero row satisfies it
    tn, to = list(TA._entries(mine[OA.FOLD16C][1])), list(TA._entries(theirs[TA.FOLD16B][1]))
    assert len(tn) == len(to)
    diff = [(x, y) for x, y in zip(tn, to) if x != y]
    assert diff == [((0, A.L, A.BUS_Q16, [A.IDX, XQ, A.OWN, A.OWN + 1, A.OWN + 2, A.OWN + 3]), (0, A.L, A.BUS_Q16, [A.IDX, A.OWN, A.OWN + 1, A.OWN + 2, A.OWN + 3]))]


def test_query16_and_rowsum16_keep_the_shard_verifiers_product_and_horner_constraints():
    """the eight product constraints are those of recursion_air.query_program and the Horner / NOTFIRST / first-block constraints those of rowsum_program (same
    polynomials: the preprocessed columns have other numbers, QUERY16's coincide); the carried-constant transitions are gone, every constant is tied to a public value"""
    sh = RA.Shape(5, 8, 4, 3, 3)
    theirs = TA.constraints_of(RA.query_program(sh))
    mine = TA.constraints_of(OA.query16_program())
    assert len(theirs) == len(mine) == 28 + 32 and theirs[28:] == mine[28:]
    m = RA.query_cols()
    for i, name in enumerate(RA.QUERY_CONSTS):
        for c in range(4):
            assert mine[4 * i + c] == (0, [(1, [m[name] + c]), (P - 1, [(2 << 30) | (OA.PUB[name] + c)])])
    ren = {RA.RP_NOTFIRST: OA.RP_NOTFIRST, RA.RP_ACT: OA.RP_ACT}
    def moved(cons):                                          # recursion_air's ROWSUM constraint on ROWSUM16's columns
        sel, terms = cons
        f = lambda v: (v & ~0xffff) | (ren[v & 0xffff] if (v & 0xffff) < RA.RS_PRE else (v & 0xffff) - RA.RS_PRE + OA.RS16_PRE)
        return sel, [(c, [f(v) for v in vs]) for c, vs in terms]
    theirs = [moved(c) for c in TA.constraints_of(RA.rowsum_program(sh))[4:]]              # (the first four carry FA from row to row)
    mine = TA.constraints_of(OA.rowsum16_program())
    assert theirs == mine[4:] and len(mine) == 4 + 32 + 4 + 4
    for c in range(4):
        assert mine[c] == (0, [(1, [OA.RS16_PRE + RA.RS_FA + c]), (P - 1, [(2 << 30) | (OA.PUB["FA"] + c)])])


# ------------------------------------------------------------------ (2) constraints and buses
@pytest.mark.parametrize("which", [GOLDEN_NAME] + SMALL)
def test_restated_traces_satisfy_every_constraint_and_balance_every_bus(which):
    v = view_of(which)
    assert A.consistent(v)
    main, pre, progs, tabs, pub = machine_of(which)
    assert len(pub) == 40 and pub[:8] == [int(c) for c in v["capacity"]]
    assert violations(main, pre, progs, tabs, pub) == ([], {})


def test_the_synthetic_views_quotient_rows_are_solved_from_a_nonsingular_system():
    """four words of a quotient row are free, the other four come from the 4 x 4 system in 1, fa, fa^2, fa^3: not singular for the fa drawn"""
    for which in SMALL:
        v = view_of(which)
        rng = np.random.default_rng(5)
        for q, (index, value, _) in enumerate(v["queries"]):
            row = OA.solve_quotient_row(index, v["H"], v["trows"][q], v["consts"], value, rng)
            assert row is not None
            forged = dict(v, qrows=[row if i == q else r for i, r in enumerate(v["qrows"])])
            assert OA.reduced_openings(forged)[q] == list(value)
    singular = dict(view_of(SMALL[0])["consts"], FA=[5, 0, 0, 0])                     # fa in the base field: 1, fa, fa^2, fa^3 span one dimension
    v = view_of(SMALL[0])
    assert OA.solve_quotient_row(v["queries"][0][0], v["H"], v["trows"][0], singular, v["queries"][0][1], np.random.default_rng(1)) is None


# ------------------------------------------------------------------ (3) the key and the machine under the oracle's prover
@pytest.mark.parametrize("which", [GOLDEN_NAME] + SMALL)
def test_host_key_equals_the_oracles_setup_and_holds_the_rows_and_no_reduced_opening(oracle, which):
    v = view_of(which)
    main, pre, progs, tabs, pub = machine_of(which)
    lns = shape_of(main, pre)[0]
    o = OA.order(*shape(v), v["W"])
    kt = OA.key_tables(v)
    assert all((pre[i] is None and kt[t] is None) or (pre[i] == kt[t]).all() for i, t in enumerate(o))
    sh = (1, 12, 4)
    root = oracle.machine_setup(pre, lns, oracle.default_params(*sh)).tolist()
    assert fri16_openings_key_host(v, Params(*sh)).tolist() == root
    assert fri16_openings_key_host(v, Params(2, 7, 0)).tolist() == oracle.machine_setup(pre, lns, oracle.default_params(2, 7, 0)).tolist()
    # one row word changed: among the indices machine's inputs only `values` would change -- and this key changes
    moved = dict(v, trows=[[(r[0] + (q == 0)) % P] + list(r[1:]) for q, r in enumerate(v["trows"])])
    assert OA.reduced_openings(moved)[0] != OA.reduced_openings(v)[0] and OA.reduced_openings(moved)[1:] == OA.reduced_openings(v)[1:]
    assert fri16_openings_key_host(moved, Params(*sh)).tolist() != root
    moved_q = dict(v, qrows=[list(r[:7]) + [(r[7] + (q == len(v["qrows"]) - 1)) % P] for q, r in enumerate(v["qrows"])])
    assert fri16_openings_key_host(moved_q, Params(*sh)).tolist() != root
    # the same rows with other `values`, other indices, other challenges, other constants: the same key
    other = dict(v, betas=[[(c + 5) % P for c in bt] for bt in v["betas"]], consts={k: [(c + 1) % P for c in e] for k, e in v["consts"].items()},
                 queries=[((i + 1) % (1 << v["H"]), [(c + 3) % P for c in val], sb) for i, val, sb in v["queries"]])
    assert fri16_openings_key_host(other, Params(*sh)).tolist() == root


@pytest.mark.parametrize("which,sh", [((1, 0, 1, 4, 8), (1, 10, 2)), (GOLDEN_NAME, (2, 7, 0))])
def test_the_oracle_proves_the_restated_arrays_and_the_library_verifies(oracle, which, sh):
    O = oracle
    v = view_of(which)
    R, F, b, Q = shape(v)
    pb, W = v["pow_bits"], v["W"]
    main, pre, progs, tabs, pub = machine_of(which)
    lns, ws, pws = shape_of(main, pre)
    oprm, prm = O.default_params(*sh), Params(*sh)
    root = O.machine_setup(pre, lns, oprm)
    assert fri16_openings_key_host(v, prm).tolist() == root.tolist()
    proof = O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm)
    assert _lib.load().zkhip_fri16_openings_proof_size(R, F, b, Q, pb, W, C.byref(prm)) == proof.size
    assert O.verify_machine_keyed(proof, lns, ws, pws, root, progs, tabs, pub, oprm) == 0
    assert verify_fri16_openings(proof, pub, R, F, b, Q, pb, W, root, prm)[0] == 0
    for k in range(40):                                      # any one of the 40 public values changed
        bad = list(pub)
        bad[k] = (bad[k] + 1) % P
        assert verify_fri16_openings(proof, bad, R, F, b, Q, pb, W, root, prm)[0] != 0, k
    bad_root = root.copy()
    bad_root[3] = (int(bad_root[3]) + 1) % P
    assert verify_fri16_openings(proof, pub, R, F, b, Q, pb, W, bad_root, prm)[0] != 0
    assert verify_fri16_openings(proof, pub, R, F, b, Q, pb, 256, root, prm)[0] != 0                 # a trace width under which ROWSUM16 and ROWS are taller: another machine


# ------------------------------------------------------------------ (4) the openings view of the committed proofs
def test_view_openings_of_the_golden_proof_equals_the_restatements_parse_and_gives_the_reduced_openings():
    g = GOLDEN[GOLDEN_NAME]
    prm = Params(*g["shape"])
    mine = view_of(GOLDEN_NAME)
    got = fri16_view_openings(load(GOLDEN_NAME), g["log_n"], g["width"], g["public"], prm)
    assert got["W"] == mine["W"] and got["trows"] == mine["trows"] and got["qrows"] == mine["qrows"]
    assert got["consts"] == {k: [int(c) for c in e] for k, e in mine["consts"].items()}
    shard = fri16_view_shard(load(GOLDEN_NAME), g["log_n"], g["width"], g["public"], prm)
    redone = OA.reduced_openings(dict(shard, **got))
    assert redone == [[int(c) for c in q[1]] for q in shard["queries"]]
    words = np.frombuffer(load(GOLDEN_NAME).tobytes(), dtype=np.uint32).copy()
    words[-1] ^= 1
    with pytest.raises(_lib.ZkHipError):                      # fails like zkhip_fri16_view_shard
        fri16_view_openings(words.view(np.uint8), g["log_n"], g["width"], g["public"], prm)
    with pytest.raises(_lib.ZkHipError, match="fold-by-16"):  # a fold-by-2 shape
        fri16_view_openings(load(GOLDEN_NAME), g["log_n"], g["width"], g["public"], Params(1, 100, 16))


def test_view_openings_refuses_lookup_pairs_and_takes_a_group_order_proof_without_them(oracle):
    name = "v8_groups_r0_lookup_8x16"
    g = GOLDEN[name]
    with pytest.raises(_lib.ZkHipError, match="lookup pairs"):
        fri16_view_openings(load(name), g["log_n"], g["width"], g["public"], Params(*g["shape"]))
    log_n, w, s = 8, 16, (2, 3, 0, 0, 4, 0, 24, 4)           # version 8 (the first four columns under a commitment of their own), no lookups
    proof = oracle.prove_shard(oracle.gen_trace(7, 5, log_n, w), [1, 2, 3], oracle.default_params(*s))
    assert np.frombuffer(proof.tobytes(), dtype=np.uint32)[1] == 8
    got = fri16_view_openings(proof, log_n, w, [1, 2, 3], Params(*s))
    mine = OA.parse_openings(proof.tobytes(), log_n, w, [1, 2, 3], s)
    assert got["trows"] == mine["trows"] and got["qrows"] == mine["qrows"] and got["consts"] == {k: [int(c) for c in e] for k, e in mine["consts"].items()}
    shard = fri16_view_shard(proof, log_n, w, [1, 2, 3], Params(*s))
    assert OA.reduced_openings(dict(shard, **got)) == [[int(c) for c in q[1]] for q in shard["queries"]]


# ------------------------------------------------------------------ (5) forgeries, and what rejects each
class Forge:
    """a machine's arrays by table number; caught(): names of the failing constraints ("QUERY16: ...", "ROWSUM16: ...", or the table's name) and unbalanced buses"""
    def __init__(self, view, honest=True):
        self.v = view
        self.o = OA.order(*shape(view), view["W"])
        self.at = {t: i for i, t in enumerate(self.o)}
        self.main, self.pre, self.progs, self.tabs, self.pub = OA.machine(view, honest=honest)

    def caught(self, fn=None, pub=None):
        m, p = [x.copy() for x in self.main], [None if x is None else x.copy() for x in self.pre]
        if fn is not None:
            fn({t: m[i] for t, i in self.at.items()}, {t: p[i] for t, i in self.at.items()})
        names = set()
        for i, (rows, prog) in enumerate(zip(combined(m, p), self.progs)):
            t = self.o[i]
            cn = OA.constraint_names(t, self.v["pow_bits"])
            for c, _ in P24.check_constraints(prog, rows, self.pub if pub is None else pub):
                names.add(OA.NAMES[t] + (": " + cn[c] if cn and t in (OA.QUERY16, OA.ROWSUM16) else ""))
        return names, {bus for bus, _ in A.bus_balance(m, p, self.tabs)}


@pytest.fixture(scope="module")
def honest():
    f = Forge(view_of((2, 2, 2, 11, 24)))
    assert f.caught() == (set(), set())
    return f


M0, QM = OA.RS16_PRE, RA.query_cols()
QC = lambda name: QM[name] - OA.Q16_PRE                      # a QUERY16 main column


def redo_rowsum(t, r0, n, fa):
    """the Horner cells of ROWSUM16 rows r0 .. r0 + n - 1 (one segment) recomputed from their V cells"""
    acc = [0, 0, 0, 0]
    for r in range(r0, r0 + n):
        t[r, RA.RS_ACCIN:RA.RS_ACCIN + 4] = acc
        steps = RA._horner8(acc, [int(x) for x in t[r, RA.RS_V:RA.RS_V + 8]], fa)
        for s in range(8):
            t[r, RA.RS_T + 4 * s:RA.RS_T + 4 * s + 4] = steps[s]
        acc = steps[0]
    return acc


def test_a_row_word_changed_in_rowsum16_only_is_caught_by_the_rows_bus(honest):
    """with the Horner cells of the query's segment, AT and everything behind it in QUERY16 recomputed, the forger still has to send (tag, K, words) -- which ROWS,
    the key's table, does not receive"""
    v = honest.v
    def change(m, p):
        t = m[OA.ROWSUM16]
        t[1, RA.RS_V + 2] = (int(t[1, RA.RS_V + 2]) + 1) % P
        at = redo_rowsum(t, 0, v["W"] // 8, v["consts"]["FA"])
        m[OA.QUERY16][0, QC("AT"):QC("AT") + 4] = at
    names, buses = honest.caught(change)
    assert OA.BUS_ROW in buses and not any(n.startswith("ROWSUM16") for n in names)
    def change_only(m, p):
        t = m[OA.ROWSUM16]
        t[1, RA.RS_V + 2] = (int(t[1, RA.RS_V + 2]) + 1) % P
    names, buses = honest.caught(change_only)
    assert "ROWSUM16: Horner" in names and OA.BUS_ROW in buses


def test_at_of_two_queries_swapped_is_caught_by_the_query_number_in_the_tuple(honest):
    def change(m, p):
        t = m[OA.QUERY16]
        a, b = t[0, QC("AT"):QC("AT") + 4].copy(), t[1, QC("AT"):QC("AT") + 4].copy()
        assert a.tolist() != b.tolist()
        t[0, QC("AT"):QC("AT") + 4], t[1, QC("AT"):QC("AT") + 4] = b, a
    names, buses = honest.caught(change)
    assert OA.BUS_AT16 in buses and OA.BUS_AQ16 not in buses            # (q, AT) is keyed by the query number: the multiset of sums alone would balance


def test_ro_changed_in_query16_with_the_chain_refolded_from_it_is_caught_by_query16s_sum_constraint():
    """query 2 enters layer 0 with another value: its own entry, OWN and the four fold steps of its FOLD16C row are redone from it (every constraint of FOLD16C holds)
    and QUERY16 takes the value the row sends, so the bus between them balances.  What rejects it: RO = P1 + P2O + P3O in QUERY16 (and, further down, the row's
    entries are no longer the committed ones and its fold no longer meets the final polynomial: the layer bus and FINAL's)"""
    f = Forge(view_of((1, 2, 2, 4, 8)))
    v = f.v
    index, value, sibs = v["queries"][2]
    forged = [(value[0] + 1) % P] + list(value[1:])
    def change(m, p):
        t = m[OA.FOLD16C]
        row, own = index >> 4, index & 15
        entries = [list(e) for e in sibs[0]]
        entries.insert(own, forged)
        _, stages = A.fold_row(row, v["H"] - 4, v["betas"][0], entries)
        t[2, A.E + 4 * own:A.E + 4 * own + 4] = forged
        t[2, A.OWN:A.OWN + 4] = forged
        for base, stage in zip(A.STEP_OUT, stages):
            for k, e in enumerate(stage):
                t[2, base + 4 * k:base + 4 * k + 4] = e
        m[OA.QUERY16][2, QC("RO"):QC("RO") + 4] = forged
    names, buses = f.caught(change)
    assert names == {"QUERY16: RO = P1 + P2O + P3O"} and A.BUS_Q16 not in buses and buses == {A.BUS_L16, A.BUS_FIN16}
    def change_query_only(m, p):                             # QUERY16 alone: the bus from FOLD16C's first row does not balance either
        m[OA.QUERY16][2, QC("RO"):QC("RO") + 4] = forged
    names, buses = f.caught(change_query_only)
    assert names == {"QUERY16: RO = P1 + P2O + P3O"} and buses == {A.BUS_Q16}


def test_xq_of_another_index_with_idx_kept_is_caught_by_fold16cs_xq_constraint(honest):
    v = honest.v
    R, lf = len(v["roots"]), v["F"] + v["b"]
    XQ = OA.xq_col(lf)
    other = OA.point(v["queries"][1][0] ^ 1, v["H"])
    def change(m, p):
        m[OA.FOLD16C][R * 1, XQ] = other
        m[OA.QUERY16][1, QC("XQ")] = other
        vals = OA.query_values(v["queries"][1][0], v["H"], [int(c) for c in m[OA.QUERY16][1, QC("AT"):QC("AT") + 4]], [int(c) for c in m[OA.QUERY16][1, QC("AQ"):QC("AQ") + 4]],
                               v["consts"])
        assert vals["XQ"] != other
    names, buses = honest.caught(change)
    assert "FOLD16C" in names and buses == set()             # the bus carries (IDX, XQ, RO) and balances: only the constraint XQ = X sum O_j w_16^.. ties XQ to the index
    at = honest.at[OA.FOLD16C]
    m = [x.copy() for x in honest.main]
    m[at][R, XQ] = other
    bad = P24.check_constraints(honest.progs[at], m[at], honest.pub)
    assert bad == [(len(TA.constraints_of(honest.progs[at])) - 1, R)]


def test_i1_zero_with_p1_and_p3_zero_is_caught_by_the_inverse_constraint(honest):
    def change(m, p):
        t = m[OA.QUERY16]
        for name in ("I1", "P1", "P3", "P3O"):
            t[0, QC(name):QC(name) + 4] = 0
        t[0, QC("RO"):QC("RO") + 4] = t[0, QC("P2O"):QC("P2O") + 4]
    names, buses = honest.caught(change)
    assert "QUERY16: I1 (x - zeta) = 1" in names and not any(n.startswith("QUERY16: P") or n.startswith("QUERY16: RO") for n in names)


def test_a_constant_changed_in_one_row_is_caught_by_the_tie_to_the_public_value(honest):
    def change(m, p):
        t = m[OA.QUERY16]
        t[3, QC("YN") + 1] = (int(t[3, QC("YN") + 1]) + 1) % P
    names, _ = honest.caught(change)
    assert "QUERY16: YN = its public value" in names
    def change_pad(m, p):                                    # a padding row too: the tie holds on every row
        t = m[OA.QUERY16]
        t[31, QC("OFFQ")] = (int(t[31, QC("OFFQ")]) + 1) % P
    assert "QUERY16: OFFQ = its public value" in honest.caught(change_pad)[0]
    def change_fa(m, p):
        t = m[OA.ROWSUM16]
        t[5, RA.RS_FA] = (int(t[5, RA.RS_FA]) + 1) % P
    assert "ROWSUM16: FA = its public value" in honest.caught(change_fa)[0]


def test_a_nonzero_accin_on_a_querys_first_block_is_caught(honest):
    v = honest.v
    per = v["W"] // 8 + 1
    def change(m, p):
        t = m[OA.ROWSUM16]
        r = per * 2                                          # query 2's first block
        acc = [7, 0, 0, 0]
        for k in range(per - 1):
            t[r + k, RA.RS_ACCIN:RA.RS_ACCIN + 4] = acc
            steps = RA._horner8(acc, [int(x) for x in t[r + k, RA.RS_V:RA.RS_V + 8]], v["consts"]["FA"])
            for s in range(8):
                t[r + k, RA.RS_T + 4 * s:RA.RS_T + 4 * s + 4] = steps[s]
            acc = steps[0]
    names, _ = honest.caught(change)
    assert "ROWSUM16: ACCIN = 0 on a first block" in names and "ROWSUM16: Horner" not in names and "ROWSUM16: ACCIN follows" not in names


def test_a_padding_row_of_rowsum16_cannot_send_a_sum_because_its_multiplicities_are_preprocessed(honest):
    """(q, T_0) goes to QUERY16 with the multiplicities LAST0 / LAST1, and the rows go to ROWS with ACT: preprocessed columns, zero on every padding row -- the key
    fixes them, no main cell can turn a padding row into a sender"""
    v = honest.v
    used = len(v["queries"]) * (v["W"] // 8 + 1)
    pre = honest.pre[honest.at[OA.ROWSUM16]]
    assert not pre[used:].any() and pre[:used, OA.RP_ACT].all()
    for sign, mult, bus, cols in TA._entries(honest.tabs[honest.at[OA.ROWSUM16]]):
        assert sign == 0 and mult < OA.RS16_PRE              # every multiplicity of the table is a preprocessed column
    for sign, mult, bus, cols in TA._entries(honest.tabs[honest.at[OA.QUERY16]]):
        assert sign == 1 and mult == OA.QP_ACT
    def change(m, p):                                        # main cells of a padding row are the prover's: nothing moves
        m[OA.ROWSUM16][used + 1, RA.RS_T:RA.RS_T + 4] = [1, 2, 3, 4]
    names, buses = honest.caught(change)
    assert buses == set() and names == {"ROWSUM16: Horner"}


# ------------------------------------------------------------------ (6) argument checks
def test_entry_point_argument_checks():
    lib = _lib.load()
    u32p = _lib.u32p
    prm = Params(1, 8, 2)
    v = view_of((1, 0, 1, 4, 8))
    bt, fp, ix, vl, sb, rt, pt, cp, tr, qr, cs = OA.view_arrays(v)
    p = lambda a: a.ctypes.data_as(u32p)
    vk = np.zeros(8, dtype=np.uint32)
    S = (1, 0, 1, 4)
    assert lib.zkhip_fri16_openings_key_host(*S, 24, 4, 8, p(fp), p(tr), p(qr), p(rt), C.byref(prm), p(vk)) == 0
    assert vk.tolist() == fri16_openings_key_host(v, prm).tolist()
    pub = np.array(OA.public_values(v), dtype=np.uint32)
    b8 = np.zeros(8, dtype=np.uint8).ctypes.data_as(_lib.u8p)
    for bad in ((0, 2, 2, 5), (6, 2, 2, 5), (2, 9, 2, 5), (2, 2, 0, 5), (2, 2, 2, 0), (2, 2, 2, 1025), (5, 8, 3, 5)):
        assert lib.zkhip_fri16_openings_key_host(*bad, 24, 4, 8, p(fp), p(tr), p(qr), p(rt), C.byref(prm), p(vk)) == -1 and b"fri16" in lib.zkhip_last_error()
        assert lib.zkhip_fri16_openings_proof_size(*bad, 4, 8, C.byref(prm)) == 0
        assert lib.zkhip_fri16_openings_describe(*bad, 4, 8, 0, 0, None, 0, None, None, None, None) == 0
        assert lib.zkhip_verify_fri16_openings(b8, 8, *bad, 4, 8, p(pub), p(vk), C.byref(prm), None) != 0
    for W in (0, 4, 12, 1032):                               # the trace width: 8 .. 1024 in multiples of 8
        assert lib.zkhip_fri16_openings_key_host(*S, 24, 4, W, p(fp), p(tr), p(qr), p(rt), C.byref(prm), p(vk)) == -1 and b"trace width" in lib.zkhip_last_error()
        assert lib.zkhip_fri16_openings_proof_size(*S, 4, W, C.byref(prm)) == 0
        assert lib.zkhip_fri16_openings_describe(*S, 4, W, 0, 0, None, 0, None, None, None, None) == 0
    for pb in (-1, 31):
        assert lib.zkhip_fri16_openings_key_host(*S, 24, pb, 8, p(fp), p(tr), p(qr), p(rt), C.byref(prm), p(vk)) == -1 and b"inner_pow_bits" in lib.zkhip_last_error()
    for hw in (16, 0):
        assert lib.zkhip_fri16_openings_key_host(*S, hw, 4, 8, p(fp), p(tr), p(qr), p(rt), C.byref(prm), p(vk)) == -1 and b"width-16 hash" in lib.zkhip_last_error()
    for k in range(4):
        args = [p(fp), p(tr), p(qr), p(rt)]
        args[k] = None
        assert lib.zkhip_fri16_openings_key_host(*S, 24, 4, 8, *args, C.byref(prm), p(vk)) == -1 and b"null" in lib.zkhip_last_error()
    for k, arr in ((1, tr), (2, qr)):
        bad = arr.copy(); bad[3] = P
        args = [p(fp), p(tr), p(qr), p(rt)]
        args[k] = p(bad)
        assert lib.zkhip_fri16_openings_key_host(*S, 24, 4, 8, *args, C.byref(prm), p(vk)) == -1 and b"canonical" in lib.zkhip_last_error()
    assert lib.zkhip_fri16_openings_describe(*S, 4, 8, 10, 0, None, 0, None, None, None, None) == 0 and lib.zkhip_fri16_openings_describe(*S, 4, 8, 9, 0, None, 0, None, None, None, None) > 0
    assert lib.zkhip_fri16_view_openings(None, 0, 9, 8, None, 0, C.byref(prm), p(tr), p(qr), p(cs)) == -1
    assert lib.zkhip_fri16_view_openings(b8, 8, 9, 8, None, 0, C.byref(prm), None, p(qr), p(cs)) == -1 and b"null" in lib.zkhip_last_error()
    # without a context the device entries refuse (no fallback)
    assert lib.zkhip_fri16_openings_key(None, *S, 24, 4, 8, p(fp), p(tr), p(qr), p(rt), C.byref(prm), None, p(vk)) == -1
    assert lib.zkhip_fri16_openings_gen_traces(None, *S, 4, 8, p(tr), p(qr), p(cs), p(ix), None, None, p(vl)) == -1
    assert lib.zkhip_prove_fri16_openings(None, None, *S, 24, 4, 8, p(bt), p(fp), p(ix), p(vl), p(sb), p(rt), p(pt), p(cp), 0, p(tr), p(qr), p(cs), C.byref(prm), None, 0, None) == -1
    assert lib.zkhip_verify_fri16_openings(None, 0, *S, 4, 8, p(pub), p(vk), C.byref(prm), None) != 0
