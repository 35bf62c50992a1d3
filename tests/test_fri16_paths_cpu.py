"""The fold-by-16 PATHS machine (zktls_amd/csrc/fri16_chip.hip: a layer-paths variant of the width-24 Poseidon2 chip, P24L, where the LAYERS
table stood, and the preprocessed ROOTS table), CPU side: the library's programs and interaction tables against the Python restatement
(tests/fri16_paths_air.py); the restatement's traces under every constraint and every bus in plain integers; what tampering the machine
catches and BY WHAT (a named constraint or a bus), the forged one-block leaf among it; the key without a GPU, which holds the layer roots and
no layer value; the machine under the oracle's prover and three verifiers; the argument checks of the new entries."""
import ctypes as C
import functools

import numpy as np
import pytest

import fri16_air as A
import fri16_paths_air as PA
import poseidon2_24_air as P24
import pyref
import pyverify_chips
from test_fri16_chip_cpu import FOLD16_GOLDEN, golden_view, shape_of, violations
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import fri16_describe, fri16_paths_describe, fri16_paths_key_host, verify_fri16_paths, verify_machine_keyed

P = 2013265921
SMALL_SHAPES = [(1, 0, 1, 4), (2, 2, 2, 11)]            # (R, F, log_blowup, queries)


@functools.lru_cache(maxsize=None)
def view_of(which):
    """a committed fixture by name, or a random view by (R, F, b, Q) with sparse Merkle trees"""
    return golden_view(which) if isinstance(which, str) else PA.random_view(*which, seed=7 * which[0] + which[1])


@functools.lru_cache(maxsize=None)
def machine_of(which):
    return PA.machine(view_of(which))


# ------------------------------------------------------------------ (1) programs and interaction tables
@pytest.mark.parametrize("R", [1, 2, 3, 5])
@pytest.mark.parametrize("lf", [2, 3, 10])
def test_program_and_table_words_equal_the_python_restatement(oracle, R, lf):
    b = 2
    F, Q = lf - b, 50
    if 4 * R + lf > 27:                      # no domain of 2^30 points: refused, with a message
        with pytest.raises(_lib.ZkHipError):
            fri16_paths_describe(R, F, b, Q, 0, 0)
        assert b"2^27" in _lib.load().zkhip_last_error()
        return
    progs, tabs, lrs, o = PA.programs(R, lf), PA.interactions(R), PA.log_rows(R, F, b, Q), PA.order(R, F, b, Q)
    mains = PA.main_widths(lf)
    assert sorted(o) == list(range(6)) and all(lrs[o[i]] >= lrs[o[i + 1]] for i in range(5)) and lrs[PA.ROOTS] == 5
    today = {}
    for which in range(5):
        prog, _, _, _, table = fri16_describe(R, F, b, Q, which, 0)
        today[table] = (prog.tolist(), fri16_describe(R, F, b, Q, which, 1)[0].tolist())
    for which, t in enumerate(o):
        prog, ln, mw, pw, table = fri16_paths_describe(R, F, b, Q, which, 0)
        tab = fri16_paths_describe(R, F, b, Q, which, 1)[0]
        assert (table, ln, mw, pw) == (t, lrs[t], mains[t], PA.PRE_WIDTHS[t])
        assert prog.tolist() == progs[t].tolist()
        assert tab.tolist() == tabs[t].tolist()
        if t in (PA.FOLD16, PA.FINAL, PA.QUERIES, PA.COEFFS):                       # FOLD16 and the others are today's, word for word
            assert (prog.tolist(), tab.tolist()) == today[t]
        assert oracle.air_validate(prog, mw + pw, 4 * R) == 1
        assert oracle.air_log_quotient_degree(prog) == 1                            # degree 3 with the selectors
        assert int(tab[1]) <= 64 and mw % 4 == 0 and pw % 4 == 0
    if (R, lf) == (3, 10):                   # the RISC Zero parameters on a 2^20-row segment: at most 2 700 rows in a 2^12-row table
        assert PA.depths(R, F, b) == [18, 14, 10] and Q * sum(4 + d for d in PA.depths(R, F, b)) == 2700 and lrs[PA.P24L] == 12


def test_a_sponge_over_one_block_is_the_compression_of_its_halves():
    """why the leaf length is pinned: without it an inner node's two children pass for a leaf one level up"""
    rng = np.random.default_rng(1)
    l, r = ([int(x) for x in rng.integers(0, P, 8)] for _ in range(2))
    assert pyref.sponge24(l + r) == pyref.compress24(l, r)


# ------------------------------------------------------------------ (2) constraints and buses
@pytest.mark.parametrize("which", FOLD16_GOLDEN + SMALL_SHAPES)
def test_restated_traces_satisfy_every_constraint_and_balance_every_bus(which):
    v = view_of(which)
    assert A.consistent(v)
    main, pre, progs, tabs, pub = machine_of(which)
    assert violations(main, pre, progs, tabs, pub) == ([], {})
    paths = PA.distinct_paths(v)
    if which == "v3_r0_9x8":
        assert len(paths) == 6 and sum(4 + len(p[4]) for p in paths) == 54 and main[0].shape == (64, PA.WIDTH_L)
    if which == "v8_groups_r0_lookup_8x16":                                          # one row shared by two queries: M = 2 in a committed fixture
        assert len(paths) == 5 and sum(4 + len(p[4]) for p in paths) == 42 and sorted(p[3] for p in paths) == [1, 1, 1, 1, 2]
    if not isinstance(which, str) and which[3] > 1:
        assert max(p[3] for p in paths) >= 2


# ------------------------------------------------------------------ (3) what tampering is caught, and by what
class Tamper:
    """a machine's arrays by table number, with P24L's failing constraints BY NAME and the unbalanced buses after a change"""

    def __init__(self, which):
        self.v = view_of(which)
        R, Q = len(self.v["betas"]), len(self.v["queries"])
        self.o = PA.order(R, self.v["F"], self.v["b"], Q)
        self.at = {t: i for i, t in enumerate(self.o)}
        self.main, self.pre, self.progs, self.tabs, self.pub = machine_of(which)
        self.names = PA.constraint_names()
        self.paths = PA.distinct_paths(self.v)
        self.starts = np.concatenate([[0], np.cumsum([4 + len(p[4]) for p in self.paths])]).astype(int)

    def caught(self, fn, table=PA.P24L, in_pre=False):
        """-> (names of P24L's failing constraints -- or "FOLD16" / "FINAL" if one of theirs fails --, buses that do not balance)"""
        m, p = [x.copy() for x in self.main], [None if x is None else x.copy() for x in self.pre]
        fn((p if in_pre else m)[self.at[table]])
        names = {self.names[c] for c, r in P24.check_constraints(self.progs[self.at[PA.P24L]], m[self.at[PA.P24L]], self.pub)}
        if table == PA.FOLD16 and P24.check_constraints(self.progs[self.at[PA.FOLD16]], m[self.at[PA.FOLD16]], self.pub):
            names.add("FOLD16")
        return names, {bus for bus, _ in A.bus_balance(m, p, self.tabs)}

    def put_path(self, t, p, rows):
        t[self.starts[p]:self.starts[p] + len(rows)] = np.array(rows, dtype=np.uint64).astype(np.uint32)


@pytest.fixture(scope="module")
def tm():
    t = Tamper((2, 2, 2, 11))
    assert t.caught(lambda x: None) == (set(), set())
    return t


def test_every_kind_of_single_cell_in_the_tail_and_flag_columns_is_caught(tm):
    """on the rows of a path: a sponge row, the first compression row, one in the middle, the END row.  (On padding rows LN, KP and DEP are free:
    nothing is sent or received there.)"""
    p = max(range(len(tm.paths)), key=lambda i: len(tm.paths[i][4]))             # a deep path
    s, depth = tm.starts[p], len(tm.paths[p][4])
    assert depth >= 4
    rows = {"first sponge row": s, "third sponge row": s + 2, "first compression row": s + 4, "a middle compression row": s + 5, "the END row": s + 3 + depth}
    flags = [P24.BIT, P24.CH, P24.END, P24.SPG, P24.SS, P24.G[1], P24.G[2], P24.G[3], P24.C[1], P24.C[2], P24.C[3]] + [PA.L_Z + k for k in range(4)]
    values = [P24.CNT, PA.L_LN, PA.L_KP, PA.L_M, PA.L_DEP] + [PA.L_K + i for i in range(4)]
    seen = set()
    for what, r in rows.items():
        for c in flags:
            names, buses = tm.caught(lambda t: t.__setitem__((r, c), 1 - int(t[r, c])))
            assert names, "a flipped flag in column %d on %s" % (c, what)
            seen |= names
        for c in values:
            names, buses = tm.caught(lambda t: t.__setitem__((r, c), (int(t[r, c]) + 1) % P))
            assert names or buses, "a changed value in column %d on %s" % (c, what)
            seen |= names
    for name in ("Z0 = SS", "SPG = Z1 + Z2 + Z3", "leaf blocks are full: G = SS + SPG", "leaf rows step: Z' = Z", "path shape: CH' = Z3 + CH - END",
                 "LN constant along a path", "KP constant on a leaf", "KP = 2 KP' + BIT", "END: KP = BIT", "sponge rows: DEP = 0", "DEP' = DEP + 1",
                 "M on sponge rows only", "K", "CNT", "C", "D", "END on a compression row"):
        assert name in seen, name


def test_an_entry_changed_in_fold16_but_not_in_the_leaf_is_caught_by_the_bus(tm):
    own = tm.v["queries"][0][0] & 15
    c = A.E + 4 * ((own + 1) % 16) + 1
    names, buses = tm.caught(lambda t: t.__setitem__((0, c), (int(t[0, c]) + 1) % P), table=PA.FOLD16)
    assert A.BUS_L16 in buses and "FOLD16" in names          # the leaf no longer receives what FOLD16 sends (and the fold no longer follows)


def test_two_entries_of_a_leaf_exchanged_are_caught(tm):
    """the whole path recomputed over the exchanged leaf, so that every row is a permutation and every digest follows: the keys no longer
    match FOLD16's, and the path ends elsewhere"""
    l, row, leaf, mult, sibs = tm.paths[0]
    swapped = leaf[4:8] + leaf[0:4] + leaf[8:]
    names, buses = tm.caught(lambda t: tm.put_path(t, 0, PA.path_rows(0, l, row, swapped, mult, sibs)[0]))
    assert names == set() and buses == {A.BUS_L16, PA.BUS_RT0, PA.BUS_RT1}


def test_kp_changed_on_a_leaf_is_caught(tm):
    """the four sponge rows moved to the neighbouring row index, keys included"""
    s = tm.starts[0]

    def move(t):
        for k in range(4):
            t[s + k, PA.L_KP] += 2
            t[s + k, PA.L_K:PA.L_K + 4] += 16
    names, buses = tm.caught(move)
    assert names == {"KP = 2 KP' + BIT"} and A.BUS_L16 in buses


def test_a_bit_flipped_with_the_children_swapped_to_match_is_caught(tm):
    """a path that takes the wrong side at one level, every row recomputed from there: each row is a permutation, D and the digests follow --
    the index walk does not, and the path ends elsewhere"""
    l, row, leaf, mult, sibs = tm.paths[0]
    rows, _ = PA.path_rows(0, l, row ^ 2, leaf, mult, sibs)                      # bit 1 flipped along the whole walk ...
    honest = PA.path_rows(0, l, row, leaf, mult, sibs)[0]
    for r in range(len(rows)):                                                   # ... but KP, K and DEP as the honest path holds them
        rows[r][PA.L_LN:] = honest[r][PA.L_LN:]
    names, buses = tm.caught(lambda t: tm.put_path(t, 0, rows))
    assert "KP = 2 KP' + BIT" in names and {PA.BUS_RT0, PA.BUS_RT1} <= buses


def test_a_root_word_changed_in_roots_is_caught(tm):
    names, buses = tm.caught(lambda t: t.__setitem__((1, PA.RT_ROOT + 5), (int(t[1, PA.RT_ROOT + 5]) + 1) % P), table=PA.ROOTS, in_pre=True)
    assert names == set() and buses == {PA.BUS_RT1}
    names, buses = tm.caught(lambda t: t.__setitem__((0, PA.RT_DEP), int(t[0, PA.RT_DEP]) - 1), table=PA.ROOTS, in_pre=True)
    assert buses == {PA.BUS_RT0, PA.BUS_RT1}                                     # the depth in the tuple pins the number of levels


def test_dep_off_by_one_is_caught(tm):
    s, depth = tm.starts[0], len(tm.paths[0][4])

    def shift(t):
        t[s + 4:s + 4 + depth, PA.L_DEP] += 1
    names, buses = tm.caught(shift)
    assert names == {"DEP' = DEP + 1"} and buses == {PA.BUS_RT0, PA.BUS_RT1}


def test_m_raised_on_one_leaf_is_caught(tm):
    s = tm.starts[0]

    def raise_m(t):
        t[s:s + 4, PA.L_M] += 1
    names, buses = tm.caught(raise_m)
    assert names == set() and buses == {A.BUS_L16}


def test_the_forged_one_block_leaf_is_rejected_by_the_leaf_shape(tm):
    """the forgery the leaf-shape constraints exist for: a path whose "leaf" is ONE sponge row absorbing the two children of a real inner node
    of layer l (the leaf's parent), climbing lh - 1 levels to the TRUE root.  Every row is a permutation, the capacity and digest chaining
    hold, the walk of the index is consistent one level up -- what rejects it is the leaf shape (the row after a leaf's first row must be its
    second: Z1' = Z0, and only a leaf's fourth row or a compression row is continued by a compression row), and with DEP counted honestly
    the tuple (layer, lh - 1, root) that no ROOTS row lists."""
    l, row, leaf, mult, sibs = tm.paths[0]
    digest = pyref.sponge24(leaf)
    children = (sibs[0] + digest) if row & 1 else (digest + sibs[0])
    node = row >> 1
    r0, out = P24.row(children + [0] * 8, 0, 0, 0, 0, 0, 1, 3)                   # SS, G1 = G2 = G3 = 1: a full first block and no second
    assert out[:8] == pyref.compress24(children[:8], children[8:])
    rows = [r0 + PA.tail(l, 2 * node, 0, 0, 0, 16 * node)]
    d = out[:8]
    for lvl, sib in enumerate(sibs[1:]):
        bit, end = (node >> lvl) & 1, 1 if lvl == len(sibs) - 2 else 0
        r, out = P24.row((sib + d if bit else d + sib) + [0] * 8, bit, 1, end, end)
        rows.append(r + PA.tail(l, node >> lvl, 0, lvl + 1))
        d = out[:8]
    assert d == [int(x) for x in tm.v["roots"][l]]                               # it does reach the true root

    def forge(t):
        """in the padding, behind the honest paths; CNT runs on"""
        at, n = int(tm.starts[-1]), len(tm.paths)
        for i, r in enumerate(rows):
            r[P24.CNT] = n + (1 if i == len(rows) - 1 else 0)
        t[at:at + len(rows)] = np.array(rows, dtype=np.uint64).astype(np.uint32)
        t[at + len(rows):, P24.CNT] = n + 1
    names, buses = tm.caught(forge)
    assert names == {"leaf rows step: Z' = Z", "path shape: CH' = Z3 + CH - END"} and buses == {PA.BUS_RT0, PA.BUS_RT1}


# ------------------------------------------------------------------ (4) the key: the roots and no layer value
@pytest.mark.parametrize("which", FOLD16_GOLDEN + SMALL_SHAPES[1:])
def test_host_key_equals_the_oracles_setup_and_does_not_depend_on_siblings(oracle, which):
    v = view_of(which)
    main, pre, progs, tabs, pub = machine_of(which)
    lns = shape_of(main, pre)[0]
    R, Q = len(v["betas"]), len(v["queries"])
    o = PA.order(R, v["F"], v["b"], Q)
    kt = PA.key_tables(v)
    assert all((pre[i] is None and kt[t] is None) or (pre[i] == kt[t]).all() for i, t in enumerate(o))      # the key's tables need no chain and no path
    other = dict(v, queries=[(i, val, [[[(c + 1) % P for c in e] for e in row] for row in sb]) for i, val, sb in v["queries"]],
                 paths=[[[(c + 3) % P for c in pl] for pl in pq] for pq in v["paths"]], betas=[[(c + 5) % P for c in bt] for bt in v["betas"]])
    for shape in ((1, 12, 4), (2, 7, 0)):
        root = oracle.machine_setup(pre, lns, oracle.default_params(*shape)).tolist()
        assert fri16_paths_key_host(v, Params(*shape)).tolist() == root
        assert fri16_paths_key_host(other, Params(*shape)).tolist() == root
    moved = dict(v, roots=[[(c + (1 if (l, j) == (R - 1, 7) else 0)) % P for j, c in enumerate(rt)] for l, rt in enumerate(v["roots"])])
    assert fri16_paths_key_host(moved, Params(1, 12, 4)).tolist() != oracle.machine_setup(pre, lns, oracle.default_params(1, 12, 4)).tolist()


# ------------------------------------------------------------------ (5) the machine under the oracle's prover and three verifiers
@pytest.mark.parametrize("which,shape", [("v8_groups_r0_lookup_8x16", (1, 12, 4)), ("v3_r0_9x8", (2, 7, 0)), ((2, 2, 2, 11), (1, 10, 2)), ((2, 2, 2, 11), (2, 7, 0))])
def test_machine_under_the_oracle_prover_and_three_verifiers(oracle, which, shape):
    O = oracle
    v = view_of(which)
    R, F, b, Q = len(v["betas"]), v["F"], v["b"], len(v["queries"])
    main, pre, progs, tabs, pub = machine_of(which)
    lns, ws, pws = shape_of(main, pre)
    oprm, prm = O.default_params(*shape), Params(*shape)
    root = O.machine_setup(pre, lns, oprm)
    assert fri16_paths_key_host(v, prm).tolist() == root.tolist()
    proof = O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm)
    assert _lib.load().zkhip_fri16_paths_proof_size(R, F, b, Q, C.byref(prm)) == proof.size

    def three(pub_, root_):
        x = O.verify_machine_keyed(proof, lns, ws, pws, root_, progs, tabs, pub_, oprm) == 0
        y = verify_fri16_paths(proof, pub_, R, F, b, Q, root_, prm)[0] == 0
        try:
            z = pyverify_chips.verify(proof.tobytes(), lns, ws, pub_, shape[0], shape[1], shape[2], programs=progs, tables=tabs, pre_widths=pws,
                                      pre_root=[int(c) for c in root_]) is True
        except Exception:
            z = False
        return x, y, z
    assert three(pub, root) == (True, True, True)
    assert verify_machine_keyed(proof, lns, ws, pws, root, progs, tabs, pub, prm) == (0, 0)
    bad_pub = list(pub)
    bad_pub[5 % len(pub)] = (bad_pub[5 % len(pub)] + 1) % P
    assert three(bad_pub, root) == (False, False, False)                         # one challenge changed
    moved = dict(v, roots=[[(c + (1 if (l, j) == (0, 2) else 0)) % P for j, c in enumerate(rt)] for l, rt in enumerate(v["roots"])])
    bad_root = fri16_paths_key_host(moved, prm)                                  # one root word changed, hence the key
    assert bad_root.tolist() != root.tolist() and three(pub, bad_root) == (False, False, False)
    assert verify_fri16_paths(proof, pub, R, F, b, Q + 40, root, prm)[0] != 0    # the query count is part of the shape: another machine


# ------------------------------------------------------------------ (6) argument checks
def test_entry_point_argument_checks():
    lib = _lib.load()
    u32p = _lib.u32p
    prm = Params(1, 8, 2)
    v = view_of((2, 2, 2, 11))
    bt, fp, ix, vl, sb, rt, pt = PA.view_arrays(v)
    p = lambda a: a.ctypes.data_as(u32p)
    vk = np.zeros(8, dtype=np.uint32)
    S = (2, 2, 2, 11)
    assert lib.zkhip_fri16_paths_key_host(*S, 24, p(fp), p(ix), p(vl), p(rt), C.byref(prm), p(vk)) == 0
    assert vk.tolist() == fri16_paths_key_host(v, prm).tolist()
    b8 = np.zeros(8, dtype=np.uint8).ctypes.data_as(_lib.u8p)
    for shape in ((0, 2, 2, 5), (6, 2, 2, 5), (2, 9, 2, 5), (2, 8, 4, 5), (2, 2, 0, 5), (2, 2, 2, 0), (2, 2, 2, 1025), (5, 8, 3, 5)):
        assert lib.zkhip_fri16_paths_key_host(*shape, 24, p(fp), p(ix), p(vl), p(rt), C.byref(prm), p(vk)) == -1 and b"fri16" in lib.zkhip_last_error()
        assert lib.zkhip_fri16_paths_proof_size(*shape, C.byref(prm)) == 0
        assert lib.zkhip_fri16_paths_describe(*shape, 0, 0, None, 0, None, None, None, None) == 0
        assert lib.zkhip_verify_fri16_paths(b8, 8, *shape, p(bt), p(vk), C.byref(prm), None) != 0
    # a fold-16 proof with the width-16 hash: refused with its message by every entry that takes a view (zkhip_prove_fri16 keeps taking it)
    for hw in (16, 0):
        assert lib.zkhip_fri16_paths_key_host(*S, hw, p(fp), p(ix), p(vl), p(rt), C.byref(prm), p(vk)) == -1
        assert b"width-16 hash" in lib.zkhip_last_error() and b"zkhip_prove_fri16" in lib.zkhip_last_error()
    with pytest.raises(_lib.ZkHipError, match="width-16 hash"):
        fri16_paths_key_host(dict(v, hash_width=16), prm)
    # NULLs
    for k in range(4):
        args = [p(fp), p(ix), p(vl), p(rt)]
        args[k] = None
        assert lib.zkhip_fri16_paths_key_host(*S, 24, *args, C.byref(prm), p(vk)) == -1 and b"null" in lib.zkhip_last_error()
    assert lib.zkhip_fri16_paths_key_host(*S, 24, p(fp), p(ix), p(vl), p(rt), None, p(vk)) == -1
    assert lib.zkhip_fri16_paths_key_host(*S, 24, p(fp), p(ix), p(vl), p(rt), C.byref(prm), None) == -1
    assert lib.zkhip_fri16_paths_proof_size(*S, None) == 0 and lib.zkhip_fri16_paths_proof_size(*S, C.byref(prm)) > 0
    assert lib.zkhip_fri16_paths_describe(*S, 6, 0, None, 0, None, None, None, None) == 0 and lib.zkhip_fri16_paths_describe(*S, 0, 2, None, 0, None, None, None, None) == 0
    assert lib.zkhip_fri16_paths_describe(*S, 5, 0, None, 0, None, None, None, None) > 0
    # a non-canonical word, an index with too many bits
    bad = rt.copy(); bad[3] = P
    assert lib.zkhip_fri16_paths_key_host(*S, 24, p(fp), p(ix), p(vl), p(bad), C.byref(prm), p(vk)) == -1 and b"canonical" in lib.zkhip_last_error()
    bad = ix.copy(); bad[0] |= 1 << 12
    assert lib.zkhip_fri16_paths_key_host(*S, 24, p(fp), p(bad), p(vl), p(rt), C.byref(prm), p(vk)) == -1 and b"index" in lib.zkhip_last_error()
    # without a context the device entries refuse (no fallback)
    n = C.c_size_t(0)
    assert lib.zkhip_fri16_paths_key(None, *S, 24, p(fp), p(ix), p(vl), p(rt), C.byref(prm), None, p(vk)) == -1
    assert lib.zkhip_fri16_paths_gen_trace(None, *S, 24, p(bt), p(fp), p(ix), p(vl), p(sb), p(pt), None, 0, None, 0, C.byref(n)) == -1
    assert lib.zkhip_prove_fri16_paths(None, None, *S, 24, p(bt), p(fp), p(ix), p(vl), p(sb), p(rt), p(pt), C.byref(prm), None, 0, None) == -1
    assert lib.zkhip_verify_fri16_paths(None, 0, *S, p(bt), p(vk), C.byref(prm), None) != 0
