"""The fold-by-16 ROW-PATHS machine (zktls_amd/csrc/fri16_chip.hip: the openings machine with the width-24 chip variant P24R where the preprocessed ROWS table
stood), CPU side: the library's programs and interaction tables against the Python restatement (tests/fri16_rowpaths_air.py); the eight unchanged tables against
the openings machine's words; the restatement's traces under every constraint and every bus in plain integers; the key without a GPU, which holds roots and no
opened word; the machine under the oracle's prover and the library's verifier; the row-paths view of the committed fold-16 proofs; the rule of table heights over
the shape space; and forgeries, each built here and shown rejected BY WHAT (a named constraint or a bus)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fri16_air as A
import fri16_openings_air as OA
import fri16_paths_air as PA
import fri16_rowpaths_air as RPA
import fri16_transcript_air as TA
import poseidon2_24_air as P24
import pyref
import recursion_air as RA
from test_fri16_chip_cpu import GOLDEN, combined, load, shape_of, violations
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import (fri16_openings_describe, fri16_rowpaths_describe, fri16_rowpaths_key_host, fri16_view_row_paths, verify_fri16_rowpaths)

P = 2013265921
GOLDEN_NAME = "v3_r0_9x8"
SHARED = (1, 0, 1, 4, 8, 4)                                  # (R, F, b, Q, W, seed): an honest view in which two queries draw one index (H = 5)


@functools.lru_cache(maxsize=None)
def view_of(which):
    """a committed fixture by name, or an honest synthetic instance by (R, F, b, Q, W[, seed])"""
    return RPA.golden_view(which, GOLDEN, load) if isinstance(which, str) else RPA.honest_view(*which)


@functools.lru_cache(maxsize=None)
def machine_of(which):
    return RPA.machine(view_of(which))


def shape(v):
    return len(v["roots"]), v["F"], v["b"], len(v["queries"])


# ------------------------------------------------------------------ (1) programs and interaction tables
@pytest.mark.parametrize("which", [GOLDEN_NAME] + RPA.HONEST_SHAPES + [(3, 8, 2, 50, 128)])
def test_describe_equals_the_python_restatement(oracle, which):
    if isinstance(which, str):
        v = view_of(which)
        R, F, b, Q, pb, W = shape(v) + (v["pow_bits"], v["W"])
    else:
        R, F, b, Q, W = which
        pb = TA.POW_BITS
    H = 4 * R + F + b
    progs, tabs, lrs, o, mains = RPA.programs(R, F, b, pb), RPA.interactions(R, F + b), RPA.log_rows(R, F, b, Q, W), RPA.order(R, F, b, Q, W), RPA.main_widths(F + b)
    assert sorted(o) == list(range(10)) and all(lrs[o[i]] >= lrs[o[i + 1]] for i in range(9))
    assert lrs[RPA.P24R] == A.lg(Q * ((W + 15) // 16 + 1 + 2 * H), 6) and lrs[RPA.ROOTS] == 5 and R + 2 <= 7
    for which_, t in enumerate(o):
        prog, ln, mw, pw, table = fri16_rowpaths_describe(R, F, b, Q, pb, W, which_, 0)
        tab = fri16_rowpaths_describe(R, F, b, Q, pb, W, which_, 1)[0]
        assert (table, ln, mw, pw) == (t, lrs[t], mains[t], RPA.PRE_WIDTHS[t])
        assert prog.tolist() == progs[t].tolist(), RPA.NAMES[t]
        assert tab.tolist() == tabs[t].tolist(), RPA.NAMES[t]
        assert oracle.air_validate(prog, mw + pw, RPA.N_PUBLIC) == 1
        assert oracle.air_log_quotient_degree(prog) == 1      # degree 3 with the selector
        assert int(tab[1]) <= 64 and mw % 4 == 0 and pw % 4 == 0


@pytest.mark.parametrize("S", [(1, 1, 1, 8, 8), (2, 2, 2, 11, 24), (3, 8, 2, 50, 128)])
def test_eight_tables_are_the_openings_machines_word_for_word_and_query16_gains_two_sends(S):
    R, F, b, Q, W = S
    mine = {d[4]: (d[0], fri16_rowpaths_describe(R, F, b, Q, 4, W, w, 1)[0]) for w, d in ((w, fri16_rowpaths_describe(R, F, b, Q, 4, W, w, 0)) for w in range(10))}
    theirs = {d[4]: (d[0], fri16_openings_describe(R, F, b, Q, 4, W, w, 1)[0]) for w, d in ((w, fri16_openings_describe(R, F, b, Q, 4, W, w, 0)) for w in range(10))}
    for t in RPA.UNCHANGED:                                  # programs AND interaction tables, ROOTS' among them
        assert mine[t][0].tolist() == theirs[t][0].tolist(), RPA.NAMES[t]
        assert mine[t][1].tolist() == theirs[t][1].tolist(), RPA.NAMES[t]
    assert mine[RPA.QUERY16][0].tolist() == theirs[OA.QUERY16][0].tolist()              # QUERY16: the program unchanged
    tn, to = list(TA._entries(mine[RPA.QUERY16][1])), list(TA._entries(theirs[OA.QUERY16][1]))
    idx = RA.query_cols()["IDX"]
    assert tn[:len(to)] == to and tn[len(to):] == [(0, OA.QP_ACT, RPA.BUS_TAG, [2, 4, idx]), (0, OA.QP_ACT, RPA.BUS_TAG, [3, 5, idx])]
    # P24R: P24L's chip part (permutation, flags, CNT) constraint for constraint, then its own; every multiplicity of a receive is tied to the flags
    cr, cl = TA.constraints_of(mine[RPA.P24R][0]), TA.constraints_of(mine[RPA.P24L][0])
    n_chip = RPA.constraint_names(RPA.P24R).index("M0 = SS + SPG")
    assert cr[:n_chip] == cl[:n_chip] and PA.constraint_names()[n_chip] == "Z boolean"
    assert int(mine[RPA.P24R][0][2]) == 552 == int(mine[RPA.P24L][0][2])
    ent = list(TA._entries(mine[RPA.P24R][1]))
    assert [(s, m, bus) for s, m, bus, _ in ent] == [(1, RPA.R_M0, OA.BUS_ROW), (1, P24.G[1], OA.BUS_ROW), (1, P24.G[2], OA.BUS_ROW), (1, P24.G[3], OA.BUS_ROW),
                                                    (1, P24.SS, RPA.BUS_TAG), (0, P24.END, PA.BUS_RT0), (0, P24.END, PA.BUS_RT1)]


# ------------------------------------------------------------------ (2) constraints and buses
@pytest.mark.parametrize("which", [GOLDEN_NAME] + RPA.HONEST_SHAPES + [SHARED])
def test_restated_traces_satisfy_every_constraint_and_balance_every_bus(which):
    v = view_of(which)
    assert A.consistent(v)
    main, pre, progs, tabs, pub = machine_of(which)
    assert len(pub) == 40 and pub[:8] == [int(c) for c in v["capacity"]]
    assert violations(main, pre, progs, tabs, pub) == ([], {})
    if which == SHARED:                                      # two queries draw one index: a path each, none shared
        idx = [q[0] for q in v["queries"]]
        assert len(set(idx)) < len(idx)
        t = main[RPA.order(*shape(v), v["W"]).index(RPA.P24R)]
        assert int(t[:, P24.END].sum()) == 2 * len(idx) and int(t[:, P24.SS].sum()) == 2 * len(idx)


def test_the_restated_leaf_hash_is_the_overwrite_mode_sponge_at_every_block_shape():
    """a lone half block, a lone full block, full + half, two full + half: the sponge rows' last output is pyref.sponge24 of the words"""
    rng = np.random.default_rng(3)
    for W in (8, 16, 24, 40):
        leaf = [int(x) for x in rng.integers(0, P, W)]
        rows, digest = RPA.path_rows(0, 0, 1, 0, leaf, [])
        assert len(rows) == (W + 15) // 16 and digest == pyref.sponge24(leaf)
        assert [r[RPA.R_LSP] for r in rows] == [0] * (len(rows) - 1) + [1] and [r[RPA.R_BL] for r in rows] == list(range(len(rows)))
        assert [r[P24.G[1]] + r[P24.G[2]] + r[P24.G[3]] for r in rows][-1] == (1 if W % 16 == 8 else 3)


# ------------------------------------------------------------------ (3) the key and the machine under the oracle's prover
@pytest.mark.parametrize("which", [GOLDEN_NAME, (1, 0, 1, 4, 8), (2, 0, 1, 3, 40)])
def test_host_key_equals_the_oracles_setup_and_holds_roots_and_no_opened_word(oracle, which):
    v = view_of(which)
    main, pre, progs, tabs, pub = machine_of(which)
    lns = shape_of(main, pre)[0]
    o = RPA.order(*shape(v), v["W"])
    kt = RPA.key_tables(v)
    assert all((pre[i] is None and kt[t] is None) or (pre[i] == kt[t]).all() for i, t in enumerate(o))
    sh = (1, 12, 4)
    root = oracle.machine_setup(pre, lns, oracle.default_params(*sh)).tolist()
    assert fri16_rowpaths_key_host(v, Params(*sh)).tolist() == root
    assert fri16_rowpaths_key_host(v, Params(2, 7, 0)).tolist() == oracle.machine_setup(pre, lns, oracle.default_params(2, 7, 0)).tolist()
    # other rows, paths, indices, values, challenges and constants under the same roots: the same key
    other = dict(v, trows=[[(c + 1) % P for c in r] for r in v["trows"]], qrows=[[(c + 2) % P for c in r] for r in v["qrows"]],
                 tpaths=[[[(c + 3) % P for c in d] for d in p] for p in v["tpaths"]], betas=[[(c + 5) % P for c in bt] for bt in v["betas"]],
                 consts={k: [(c + 1) % P for c in e] for k, e in v["consts"].items()},
                 queries=[((i + 1) % (1 << v["H"]), [(c + 3) % P for c in val], sb) for i, val, sb in v["queries"]])
    assert fri16_rowpaths_key_host(other, Params(*sh)).tolist() == root
    for name in ("troot", "qroot"):                          # either root changed: another key
        moved = dict(v, **{name: [(v[name][0] + 1) % P] + list(v[name][1:])})
        assert fri16_rowpaths_key_host(moved, Params(*sh)).tolist() != root


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
    assert fri16_rowpaths_key_host(v, prm).tolist() == root.tolist()
    proof = O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm)
    assert _lib.load().zkhip_fri16_rowpaths_proof_size(R, F, b, Q, pb, W, C.byref(prm)) == proof.size
    assert O.verify_machine_keyed(proof, lns, ws, pws, root, progs, tabs, pub, oprm) == 0
    assert verify_fri16_rowpaths(proof, pub, R, F, b, Q, pb, W, root, prm)[0] == 0
    for k in (0, 7, 8, 23, 39):                              # a public value changed
        bad = list(pub)
        bad[k] = (bad[k] + 1) % P
        assert verify_fri16_rowpaths(proof, bad, R, F, b, Q, pb, W, root, prm)[0] != 0, k
    bad_root = root.copy()
    bad_root[3] = (int(bad_root[3]) + 1) % P
    assert verify_fri16_rowpaths(proof, pub, R, F, b, Q, pb, W, bad_root, prm)[0] != 0
    assert verify_fri16_rowpaths(proof, pub, R, F, b, Q, pb, 1024, root, prm)[0] != 0                # a trace width under which the tables are taller: another machine


# ------------------------------------------------------------------ (4) the row-paths view of the committed proofs
def test_view_row_paths_of_the_golden_proof_equals_the_restatements_parse():
    g = GOLDEN[GOLDEN_NAME]
    prm = Params(*g["shape"])
    mine = view_of(GOLDEN_NAME)
    got = fri16_view_row_paths(load(GOLDEN_NAME), g["log_n"], g["width"], g["public"], prm)
    assert got == {k: mine[k] for k in ("tpaths", "qpaths", "troot", "qroot")}
    H = mine["H"]
    assert all(len(p) == H for p in got["tpaths"] + got["qpaths"])
    for q, (index, _, _) in enumerate(mine["queries"]):      # each path ends in its root, by the restatement's hash
        for leaf, path, root in ((mine["trows"][q], got["tpaths"][q], got["troot"]), (mine["qrows"][q], got["qpaths"][q], got["qroot"])):
            d = pyref.sponge24(leaf)
            for lvl, sib in enumerate(path):
                d = pyref.compress24(sib, d) if (index >> lvl) & 1 else pyref.compress24(d, sib)
            assert d == root
    words = np.frombuffer(load(GOLDEN_NAME).tobytes(), dtype=np.uint32).copy()
    words[-1] ^= 1
    with pytest.raises(_lib.ZkHipError):                      # fails like zkhip_fri16_view_shard
        fri16_view_row_paths(words.view(np.uint8), g["log_n"], g["width"], g["public"], prm)
    with pytest.raises(_lib.ZkHipError, match="fold-by-16"):  # a fold-by-2 shape
        fri16_view_row_paths(load(GOLDEN_NAME), g["log_n"], g["width"], g["public"], Params(1, 100, 16))


def test_view_row_paths_refuses_lookup_pairs_a_commitment_of_the_proofs_own_and_the_width_16_hash(oracle):
    name = "v8_groups_r0_lookup_8x16"
    g = GOLDEN[name]
    with pytest.raises(_lib.ZkHipError, match="lookup pairs"):
        fri16_view_row_paths(load(name), g["log_n"], g["width"], g["public"], Params(*g["shape"]))
    log_n, w = 8, 16
    s8 = (2, 3, 0, 0, 4, 0, 24, 4)                            # version 8: the first four columns under a commitment of their own
    proof = oracle.prove_shard(oracle.gen_trace(7, 5, log_n, w), [1, 2, 3], oracle.default_params(*s8))
    with pytest.raises(_lib.ZkHipError, match="commitment of their own"):
        fri16_view_row_paths(proof, log_n, w, [1, 2, 3], Params(*s8))
    s16 = (2, 3, 0, 0, 4, 0, 16)                              # fold by 16 with the width-16 hash
    proof = oracle.prove_shard(oracle.gen_trace(7, 5, log_n, w), [1, 2, 3], oracle.default_params(*s16))
    with pytest.raises(_lib.ZkHipError, match="width-16 hash"):
        fri16_view_row_paths(proof, log_n, w, [1, 2, 3], Params(*s16))


# ------------------------------------------------------------------ (5) heights over the shape space
def test_at_most_eight_tables_of_one_height_over_the_shape_space():
    """the rule: a shape is taken exactly when no height is shared by more than 8 of the ten tables.  NO shape of this space is refused, and none the openings
    machine takes can be: ROOTS always has 2^5 rows, P24R and ROWSUM16 at least 2^6, and SAMPLES has fewer rows than QUERY16 from 2^6 on, so at most eight tables
    ever meet.  The refusal in the library (and its message) is therefore a guard that this sweep shows to be unreachable, not a path it exercises; the rule itself
    is exercised on height lists below"""
    lib = _lib.load()
    taken = refused = 0
    for R in range(1, 6):
        for F in range(0, 9):
            for b in (1, 2):
                if not A.shape_ok(R, F, b, 1):
                    continue
                for Q in (1, 2, 50, 100, 1024):
                    for W in (8, 16, 24, 128, 1024):
                        lrs = RPA.log_rows(R, F, b, Q, W)
                        ok = max(lrs.count(h) for h in set(lrs)) <= 8
                        assert ok == RPA.shape_ok(R, F, b, Q, 4, W)
                        ln = C.c_int(0)
                        n = lib.zkhip_fri16_rowpaths_describe(R, F, b, Q, 4, W, 9, 1, None, 0, C.byref(ln), None, None, None)
                        if ok:
                            assert n > 0 and ln.value == lrs[RPA.order(R, F, b, Q, W)[9]]
                            taken += 1
                        else:
                            assert n == 0 and b"at most 8 tables of one height" in lib.zkhip_last_error()
                            refused += 1
    assert taken > 2000 and refused == 0
    # the rule on height lists, as shape_ok applies it
    rule = lambda lrs: max(lrs.count(h) for h in set(lrs)) <= RPA.MAX_SAME_HEIGHT
    assert rule([5] * 8 + [6, 6]) and not rule([5] * 9 + [6]) and not rule([7] * 10) and rule([9, 8, 8, 7, 7, 6, 6, 5, 5, 5])


# ------------------------------------------------------------------ (6) forgeries, and what rejects each
class Forge:
    """a machine's arrays by table number; caught(): names of the failing constraints ("P24R: <name>", "ROOTS: #<number>", or the table's name) and unbalanced buses"""
    def __init__(self, view):
        self.v = view
        self.o = RPA.order(*shape(view), view["W"])
        self.at = {t: i for i, t in enumerate(self.o)}
        self.main, self.pre, self.progs, self.tabs, self.pub = RPA.machine(view)

    def caught(self, fn=None):
        m, p = [x.copy() for x in self.main], [None if x is None else x.copy() for x in self.pre]
        if fn is not None:
            out = fn({t: m[i] for t, i in self.at.items()}, {t: p[i] for t, i in self.at.items()})
            for t, arr in (out or {}).items():               # a table made anew
                m[self.at[t]] = arr
        names = set()
        for i, (rows, prog) in enumerate(zip(combined(m, p), self.progs)):
            t = self.o[i]
            cn = RPA.constraint_names(t, self.v["pow_bits"])
            for c, _ in P24.check_constraints(prog, rows, self.pub):
                names.add(RPA.NAMES[t] + (": " + cn[c] if cn and t in (RPA.P24R, RPA.QUERY16, RPA.ROWSUM16) else ": #%d" % c if t == RPA.ROOTS else ""))
        return names, {bus for bus, _ in A.bus_balance(m, p, self.tabs)}


def specs_of(v):
    """the paths of a view as the trace builder below takes them: [dict(tag, lnr, index, blocks, sibs)]"""
    R, W = len(v["roots"]), v["W"]
    out = []
    for q, (index, _, _) in enumerate(v["queries"]):
        for tree, (leaf, sibs) in enumerate(((v["trows"][q], v["tpaths"][q]), (v["qrows"][q], v["qpaths"][q]))):
            leaf = [int(x) for x in leaf]
            out.append(dict(tag=2 * q + tree, lnr=R + tree, index=index, blocks=[leaf[k:k + 16] for k in range(0, len(leaf), 16)], sibs=sibs))
    return out


def trace_from(specs, lr):
    """P24R from path specs, every flag derived the way an honest prover derives it BUT for what a spec overrides: blocks of any sizes (multiples of 4 words, partial
    ones anywhere), bl0 (the first block's number), ix (the IX / KP cells of the sponge rows), lnr, level0 (the level of the first compression row)"""
    rows = []
    for p, s in enumerate(specs):
        out, nb, index = [0] * 24, len(s["blocks"]), s["index"]
        ix = s.get("ix", index)
        for k, blk in enumerate(s["blocks"]):
            state = [int(x) for x in blk] + (out[len(blk):16] if k else [0] * (16 - len(blk))) + out[16:]
            r, out = P24.row(state, 0, 0, 0, p, 1 if k else 0, 0 if k else 1, len(blk) // 4 - 1)
            rows.append(r + RPA.tail(s["tag"], s["lnr"], 2 * ix, 0, ix, s.get("bl0", 0) + k, int(k == nb - 1), 1))
        digest = out[:8]
        for lvl, sib in enumerate(s["sibs"]):
            bit, end = (index >> lvl) & 1, 1 if lvl == len(s["sibs"]) - 1 else 0
            sib = [int(x) for x in sib]
            r, out = P24.row((sib + digest if bit else digest + sib) + [0] * 8, bit, 1, end, p + end)
            rows.append(r + RPA.tail(s["tag"], s["lnr"], index >> lvl, lvl + 1))
            digest = out[:8]
        s["end"] = digest
    pad = P24.row([0] * 24)[0]
    pad[P24.CNT] = len(specs)
    rows += [pad + RPA.tail()] * ((1 << lr) - len(rows))
    return np.array(rows, dtype=np.uint64).astype(np.uint32)


def p24r_names(names):
    return {n for n in names if n.startswith("P24R")}


@pytest.fixture(scope="module")
def honest():
    """W = 40: two full blocks and a half one"""
    f = Forge(view_of((2, 0, 1, 3, 40)))
    assert f.caught() == (set(), set())
    lr = f.main[f.at[RPA.P24R]].shape[0].bit_length() - 1
    assert (trace_from(specs_of(f.v), lr) == f.main[f.at[RPA.P24R]]).all()
    f.lr = lr
    return f


@pytest.fixture(scope="module")
def twin():
    """the same view with query 0's trace row ALSO committed at a second index, one bit away from the drawn one: a valid path to the trace root exists there"""
    v = view_of((2, 0, 1, 3, 40))
    idx = [q[0] for q in v["queries"]]
    other = next(idx[0] ^ (1 << k) for k in range(v["H"]) if idx[0] ^ (1 << k) not in idx)
    leaves = {i: [int(x) for x in v["trows"][q]] for q, i in enumerate(idx)}
    leaves[other] = leaves[idx[0]]
    root, node = RPA.sparse_tree(leaves, v["H"], [7, 0, 24])
    path = lambda i: [node(lvl, (i >> lvl) ^ 1) for lvl in range(v["H"])]
    f = Forge(dict(v, troot=root, tpaths=[path(i) for i in idx]))
    assert f.caught() == (set(), set())
    f.lr = f.main[f.at[RPA.P24R]].shape[0].bit_length() - 1
    f.other, f.other_path = other, path(other)
    return f


def test_a_row_word_changed_in_p24r_only_and_rehashed_is_caught_by_the_roots_bus(honest):
    """every constraint of P24R holds on the rehashed path; its end is another digest, which ROOTS -- the key's table -- does not receive (and the changed group is
    not one ROWSUM16 sends)"""
    specs = specs_of(honest.v)
    specs[2]["blocks"][1][5] = (specs[2]["blocks"][1][5] + 1) % P
    trace = trace_from(specs, honest.lr)
    assert specs[2]["end"] != honest.v["troot"]
    names, buses = honest.caught(lambda m, p: {RPA.P24R: trace})
    assert names == set() and buses == {PA.BUS_RT0, PA.BUS_RT1, OA.BUS_ROW}


def test_the_same_word_changed_in_rowsum16_only_is_caught_by_the_row_bus(honest):
    v = honest.v
    per = v["W"] // 8 + 1
    def change(m, p):
        t = m[RPA.ROWSUM16]
        r = per * 1 + (v["W"] // 8 - 1 - 2)                  # query 1, words 16..23: block 2 of the trace, counted from the last
        assert t[r, RA.RS_V:RA.RS_V + 8].tolist() == [int(x) for x in v["trows"][1][16:24]]
        t[r, RA.RS_V + 5] = (int(t[r, RA.RS_V + 5]) + 1) % P
    names, buses = honest.caught(change)
    assert OA.BUS_ROW in buses and PA.BUS_RT0 not in buses and p24r_names(names) == set()


def test_a_path_opened_at_another_index_with_ix_changed_is_caught_by_the_index_bus(twin):
    """the row IS committed at the other index too: the path ends in the trace root and every group is the one ROWSUM16 sends; only (TAG, LNR, IX) is not what
    QUERY16 sends for the tag"""
    specs = specs_of(twin.v)
    specs[0] = dict(specs[0], index=twin.other, sibs=twin.other_path)
    trace = trace_from(specs, twin.lr)
    assert specs[0]["end"] == twin.v["troot"]
    names, buses = twin.caught(lambda m, p: {RPA.P24R: trace})
    assert names == set() and buses == {RPA.BUS_TAG}


def test_ix_kept_but_a_bit_flipped_is_caught_by_the_kp_recurrence(twin):
    specs = specs_of(twin.v)
    specs[0] = dict(specs[0], index=twin.other, sibs=twin.other_path, ix=twin.v["queries"][0][0])
    trace = trace_from(specs, twin.lr)
    assert specs[0]["end"] == twin.v["troot"]
    names, buses = twin.caught(lambda m, p: {RPA.P24R: trace})
    assert names == {"P24R: KP = 2 KP' + BIT"} and buses == set()


def test_a_trace_tagged_path_that_carries_the_quotient_trees_number_is_caught_by_the_tag_tree_tuple(honest):
    R = len(honest.v["roots"])
    specs = specs_of(honest.v)
    specs[0]["lnr"] = R + 1
    trace = trace_from(specs, honest.lr)
    names, buses = honest.caught(lambda m, p: {RPA.P24R: trace})
    assert names == set() and RPA.BUS_TAG in buses           # (and ROOTS receives the trace root under the quotient tree's number: its bus too)
    assert buses == {RPA.BUS_TAG, PA.BUS_RT0, PA.BUS_RT1}


def test_a_leaf_whose_middle_block_is_partial_is_caught_by_the_row_bus(honest):
    """blocks of 16, 8, 16 words over the same 40: every constraint holds (a partial block is the chip's), the groups (tag, 6) and (tag, 7) are never received
    and (tag, 10), (tag, 11) are received without being sent"""
    specs = specs_of(honest.v)
    leaf = [w for blk in specs[0]["blocks"] for w in blk]
    specs[0]["blocks"] = [leaf[:16], leaf[16:24], leaf[24:40]]
    trace = trace_from(specs, honest.lr)
    names, buses = honest.caught(lambda m, p: {RPA.P24R: trace})
    assert names == set() and OA.BUS_ROW in buses and RPA.BUS_TAG not in buses


def test_a_leaf_cut_one_block_short_with_lsp_set_early_is_caught_by_the_row_bus(honest):
    specs = specs_of(honest.v)
    specs[0]["blocks"] = specs[0]["blocks"][:2]              # the two full blocks; LSP on the second
    trace = trace_from(specs, honest.lr)
    assert int(trace[1, RPA.R_LSP]) == 1 and int(trace[2, P24.CH]) == 1
    names, buses = honest.caught(lambda m, p: {RPA.P24R: trace})
    assert names == set() and OA.BUS_ROW in buses and RPA.BUS_TAG not in buses


def test_a_chain_that_starts_at_block_one_is_caught_by_bl_zero_on_ss(honest):
    """the first block skipped, the chain started at the second one under its true number"""
    specs = specs_of(honest.v)
    specs[0]["blocks"], specs[0]["bl0"] = specs[0]["blocks"][1:], 1
    trace = trace_from(specs, honest.lr)
    assert trace[0, RPA.R_K:RPA.R_K + 4].tolist() == [4, 5, 6, 7]
    names, buses = honest.caught(lambda m, p: {RPA.P24R: trace})
    assert names == {"P24R: SS: BL = 0"}


def test_a_chain_that_begins_on_the_first_row_without_an_ss_row_is_caught_by_the_chips_first_row_constraints(honest):
    """a chain's start is pinned by transitions (SPG' = M0 - LSP, CH' = LSP + CH - END), which the table's first row has no predecessor for: there the chip's own
    FIRST-row constraints CH = 0 and SPG = 0, which P24R keeps from the stand-alone chip as P24L does, leave SS, or a padding row, as the only starts"""
    names = RPA.constraint_names(RPA.P24R)
    cons = RPA.p24r_constraints()
    first = [(n, terms) for n, sel, terms in cons if sel == 1]
    assert [n for n, _ in first] == ["first row", "first row", "CNT"] and first[0][1] == [(1, [P24.CH])] and first[1][1] == [(1, [P24.SPG])]
    def continuing(m, p):                                    # row 0 made a continuing sponge row (block 1 of a chain whose block 0 is nowhere)
        t = m[RPA.P24R]
        t[0, P24.SS], t[0, P24.SPG], t[0, RPA.R_BL] = 0, 1, 1
    got, _ = honest.caught(continuing)
    assert "P24R: first row" in got
    def compression(m, p):                                   # row 0 made a compression row
        t = m[RPA.P24R]
        t[0, P24.SS], t[0, RPA.R_M0], t[0, P24.CH] = 0, 0, 1
    got, _ = honest.caught(compression)
    assert "P24R: first row" in got
    assert names.count("first row") == 2


def test_two_children_passed_as_a_one_block_leaf_are_caught_by_the_depth_in_roots_tuple():
    """W = 16: pyref.sponge24 over one full block IS pyref.compress24 of its halves, so the children of the node above query 0's leaf pass for a leaf whose path
    has H - 1 compression rows and ends in the trace root -- under DEP = H - 1, which ROOTS does not list"""
    f = Forge(view_of((1, 0, 1, 4, 16)))
    v = f.v
    H, index = v["H"], v["queries"][0][0]
    leaf, sib0 = pyref.sponge24(v["trows"][0]), [int(x) for x in v["tpaths"][0][0]]
    children = sib0 + leaf if index & 1 else leaf + sib0
    assert pyref.sponge24(children) == pyref.compress24(children[:8], children[8:])
    specs = specs_of(v)
    specs[0] = dict(specs[0], index=index >> 1, blocks=[children], sibs=v["tpaths"][0][1:])
    lr = f.main[f.at[RPA.P24R]].shape[0].bit_length() - 1
    trace = trace_from(specs, lr)
    assert specs[0]["end"] == v["troot"] and int(trace[H - 1, P24.END]) == 1 and int(trace[H - 1, RPA.R_DEP]) == H - 1
    names, buses = f.caught(lambda m, p: {RPA.P24R: trace})
    assert names == set() and {PA.BUS_RT0, PA.BUS_RT1} <= buses
    # ... and the tuples ROOTS is left with: the trace root under depth H - 1 sent, under depth H not
    m = [x.copy() for x in f.main]
    m[f.at[RPA.P24R]] = trace
    R = len(v["roots"])
    left = {tup for bus, tup in A.bus_balance(m, f.pre, f.tabs) if bus == PA.BUS_RT0}
    assert left == {(R, H - 1) + tuple(v["troot"][:4]), (R, H) + tuple(v["troot"][:4])}


def test_a_bit_past_the_depth_in_the_index_is_caught_at_the_end_row(honest):
    v = honest.v
    specs = specs_of(v)
    specs[0]["index"] = specs[0]["index"] + (1 << v["H"])    # the same H path bits, one more above them
    trace = trace_from(specs, honest.lr)
    assert specs[0]["end"] == v["troot"]
    names, buses = honest.caught(lambda m, p: {RPA.P24R: trace})
    assert names == {"P24R: END: KP = BIT"} and buses == {RPA.BUS_TAG}


def test_fold_rows_on_the_trace_roots_row_of_roots_is_caught_by_the_existing_roots_constraint(honest):
    R = len(honest.v["roots"])
    def change(m, p):
        assert int(p[RPA.ROOTS][R, 10]) == 0 and int(p[RPA.ROOTS][R - 1, 10]) == 1 and int(m[RPA.ROOTS][R, 0]) == len(honest.v["queries"])
        m[RPA.ROOTS][R, 5] = 1
    names, buses = honest.caught(change)
    assert names == {"ROOTS: #1"} and buses == {TA.BUS_BF16}                         # FOLDROWS (1 - LISTED) = 0


def test_a_padding_row_with_m0_set_is_caught_by_m0_equals_ss_plus_spg(honest):
    def change(m, p):
        t = m[RPA.P24R]
        assert not t[-2, 528:531].any() and not t[-2, 532:].any()                    # a padding row: no flag, the tail zero (CNT counts on)
        t[-2, RPA.R_M0] = 1
    names, buses = honest.caught(change)
    assert "P24R: M0 = SS + SPG" in names and buses == {OA.BUS_ROW}


# ------------------------------------------------------------------ (7) argument checks
def test_entry_point_argument_checks():
    lib = _lib.load()
    u32p = _lib.u32p
    prm = Params(1, 8, 2)
    v = view_of((1, 0, 1, 4, 8))
    bt, fp, ix, vl, sb, rt, pt, cp, tr, qr, cs, tp, qp, tro, qro = RPA.view_arrays(v)
    p = lambda a: a.ctypes.data_as(u32p)
    vk = np.zeros(8, dtype=np.uint32)
    S = (1, 0, 1, 4)
    assert lib.zkhip_fri16_rowpaths_key_host(*S, 24, 4, 8, p(fp), p(rt), p(tro), p(qro), C.byref(prm), p(vk)) == 0
    assert vk.tolist() == fri16_rowpaths_key_host(v, prm).tolist()
    pub = np.array(RPA.public_values(v), dtype=np.uint32)
    b8 = np.zeros(8, dtype=np.uint8).ctypes.data_as(_lib.u8p)
    for bad in ((0, 2, 2, 5), (6, 2, 2, 5), (2, 9, 2, 5), (2, 2, 0, 5), (2, 2, 2, 0), (2, 2, 2, 1025), (5, 8, 3, 5)):
        assert lib.zkhip_fri16_rowpaths_key_host(*bad, 24, 4, 8, p(fp), p(rt), p(tro), p(qro), C.byref(prm), p(vk)) == -1 and b"fri16" in lib.zkhip_last_error()
        assert lib.zkhip_fri16_rowpaths_proof_size(*bad, 4, 8, C.byref(prm)) == 0
        assert lib.zkhip_fri16_rowpaths_describe(*bad, 4, 8, 0, 0, None, 0, None, None, None, None) == 0
        assert lib.zkhip_verify_fri16_rowpaths(b8, 8, *bad, 4, 8, p(pub), p(vk), C.byref(prm), None) != 0
    for W in (0, 4, 12, 1032):
        assert lib.zkhip_fri16_rowpaths_key_host(*S, 24, 4, W, p(fp), p(rt), p(tro), p(qro), C.byref(prm), p(vk)) == -1 and b"trace width" in lib.zkhip_last_error()
    for hw in (16, 0):
        assert lib.zkhip_fri16_rowpaths_key_host(*S, hw, 4, 8, p(fp), p(rt), p(tro), p(qro), C.byref(prm), p(vk)) == -1 and b"width-16 hash" in lib.zkhip_last_error()
    for k in range(4):
        args = [p(fp), p(rt), p(tro), p(qro)]
        args[k] = None
        assert lib.zkhip_fri16_rowpaths_key_host(*S, 24, 4, 8, *args, C.byref(prm), p(vk)) == -1 and b"null" in lib.zkhip_last_error()
    for k, arr in ((2, tro), (3, qro)):
        bad = arr.copy(); bad[3] = P
        args = [p(fp), p(rt), p(tro), p(qro)]
        args[k] = p(bad)
        assert lib.zkhip_fri16_rowpaths_key_host(*S, 24, 4, 8, *args, C.byref(prm), p(vk)) == -1 and b"canonical" in lib.zkhip_last_error()
    assert lib.zkhip_fri16_rowpaths_describe(*S, 4, 8, 10, 0, None, 0, None, None, None, None) == 0 and lib.zkhip_fri16_rowpaths_describe(*S, 4, 8, 9, 0, None, 0, None, None, None, None) > 0
    assert lib.zkhip_fri16_view_row_paths(None, 0, 9, 8, None, 0, C.byref(prm), p(tp), p(qp), p(tro), p(qro)) == -1
    assert lib.zkhip_fri16_view_row_paths(b8, 8, 9, 8, None, 0, C.byref(prm), None, p(qp), p(tro), p(qro)) == -1 and b"null" in lib.zkhip_last_error()
    # without a context the device entries refuse (no fallback)
    assert lib.zkhip_fri16_rowpaths_key(None, *S, 24, 4, 8, p(fp), p(rt), p(tro), p(qro), C.byref(prm), None, p(vk)) == -1
    assert lib.zkhip_fri16_rowpaths_gen_trace(None, *S, 4, 8, p(tr), p(qr), p(ix), p(tp), p(qp), None, p(vl)) == -1
    assert lib.zkhip_prove_fri16_rowpaths(None, None, *S, 24, 4, 8, p(bt), p(fp), p(ix), p(vl), p(sb), p(rt), p(pt), p(cp), 0, p(tr), p(qr), p(cs), p(tp), p(qp), p(tro), p(qro),
                                          C.byref(prm), None, 0, None) == -1
    assert lib.zkhip_verify_fri16_rowpaths(None, 0, *S, 4, 8, p(pub), p(vk), C.byref(prm), None) != 0
