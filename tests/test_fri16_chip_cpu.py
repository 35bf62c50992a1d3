"""The fold-by-16 FRI machine (zktls_amd/csrc/fri16_chip.hip: the FOLD16 and FINAL chips with the preprocessed LAYERS / QUERIES / COEFFS
tables), CPU side: the library's programs and interaction tables against the independent Python restatement (tests/fri16_air.py); the view
of the two fold-16 golden proofs as the library's verifier hands it out and as the restatement parses it; the restatement's traces under
every constraint and every bus in plain integers; what single cells the constraints catch; the key without a GPU; and the machine on the
restated arrays under the oracle's prover and three verifiers."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fri16_air as A
import poseidon2_24_air as P24
import pyverify_chips
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import fri16_describe, fri16_key_host, fri16_view_shard, fri_view_shard, verify_fri16, verify_machine_keyed

P = 2013265921
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "oracle_kat.json")))["golden_proof_files"]
FOLD16_GOLDEN = ["v3_r0_9x8", "v8_groups_r0_lookup_8x16"]
RANDOM_SHAPES = [(1, 0, 1, 4), (2, 2, 2, 11), (3, 8, 2, 50)]            # (R, F, log_blowup, queries)


def load(name):
    return np.frombuffer(open(os.path.join(HERE, "golden", "proofs", name + ".bin"), "rb").read(), dtype=np.uint8)


def golden_view(name):
    g = GOLDEN[name]
    s = g["shape"]
    return A.parse_view(load(name).tobytes(), g["log_n"], g["width"], g["public"], s[0], s[1], s[2], logup_pairs=s[3], log_final=s[5], hash_width=s[6],
                        code_width=s[7] if len(s) > 7 else 0)


def shape_of(traces, pre):
    return ([t.shape[0].bit_length() - 1 for t in traces], [t.shape[1] for t in traces], [0 if p is None else p.shape[1] for p in pre])


def combined(main, pre):
    return [m if p is None else np.concatenate([p, m], axis=1) for m, p in zip(main, pre)]


def violations(main, pre, progs, tabs, pub):
    """(constraint failures, unbalanced bus tuples) of a machine's arrays"""
    bad = [(i, c, r) for i, (rows, prog) in enumerate(zip(combined(main, pre), progs)) for c, r in P24.check_constraints(prog, rows, pub)]
    return bad, A.bus_balance(main, pre, tabs)


def constraints_of(prog):
    """a constraint program's words -> [(selector, [(coefficient, [variables])])]"""
    prog = [int(x) for x in prog]
    out, p = [], 6
    for _ in range(prog[3]):
        sel, nt = prog[p], prog[p + 1]
        p += 2
        terms = []
        for _ in range(nt):
            d = prog[p + 1]
            terms.append((prog[p], prog[p + 2:p + 2 + d]))
            p += 2 + d
        out.append((sel, terms))
    return out


# ------------------------------------------------------------------ (a) programs and interaction tables
@pytest.mark.parametrize("R", [1, 2, 3, 5])
@pytest.mark.parametrize("lf", [2, 3, 10])
def test_program_and_table_words_equal_the_python_restatement(oracle, R, lf):
    """every (R, lf) pair; R = 5 with lf = 10 is a domain of 2^30 points, which BabyBear (two-adicity 27) does not have: its program would need a
    2^30-th root of unity, so that one shape must be REFUSED, and is checked as such"""
    b = 2
    F, Q = lf - b, 50
    if 4 * R + lf > 27:                      # R = 5, lf = 10: the field has no domain of 2^30 points -- refused, with a message
        assert not A.shape_ok(R, F, b, Q)
        with pytest.raises(_lib.ZkHipError):
            fri16_describe(R, F, b, Q, 0, 0)
        assert b"2^27" in _lib.load().zkhip_last_error()
        return
    progs, tabs, lrs, o = A.programs(R, lf), A.interactions(R), A.log_rows(R, F, Q), A.order(R, F, Q)
    mains = [A.width_of(lf), A.FIN_MAIN, A.TAB_MAIN, A.TAB_MAIN, A.TAB_MAIN]
    pres = [0, A.FIN_PRE, A.LAY_PRE, A.Q_PRE, A.C_PRE]
    assert sorted(o) == list(range(5)) and all(lrs[o[i]] >= lrs[o[i + 1]] for i in range(4))
    for which, t in enumerate(o):
        prog, ln, mw, pw, table = fri16_describe(R, F, b, Q, which, 0)
        tab = fri16_describe(R, F, b, Q, which, 1)[0]
        assert (table, ln, mw, pw) == (t, lrs[t], mains[t], pres[t])
        assert prog.tolist() == progs[t].tolist()
        assert tab.tolist() == tabs[t].tolist()
        assert oracle.air_validate(prog, mw + pw, 4 * R) == 1
        assert oracle.air_log_quotient_degree(prog) == 1          # degree 3 with the selectors: outer blowup 2 is enough
        assert int(tab[1]) <= 64 and mw % 4 == 0 and pw % 4 == 0


# ------------------------------------------------------------------ (b) the view
@pytest.mark.parametrize("name", FOLD16_GOLDEN)
def test_view_of_a_golden_fold16_proof_equals_the_restatements_parse(name):
    g = GOLDEN[name]
    b = load(name)
    prm = Params(*g["shape"])
    mine = golden_view(name)
    got = fri16_view_shard(b, g["log_n"], g["width"], g["public"], prm)
    assert got["betas"] == mine["betas"] and got["final_poly"] == mine["final_poly"] and got["roots"] == mine["roots"]
    assert got["queries"] == [(i, list(v), [[list(e) for e in row] for row in s]) for i, v, s in mine["queries"]]
    assert got["paths"] == mine["paths"]
    assert (got["F"], got["b"], got["H"]) == (mine["F"], mine["b"], mine["H"]) and len(got["queries"]) == g["shape"][1]
    assert A.consistent(mine)                                  # every chain refolds to the Horner value, by the restatement's arithmetic
    A.chains(mine, check=True)                                 # ... at the points of the pair-by-pair fold
    # a proof with one flipped sibling word is refused: the FRI part of the last query is the tail of the proof
    H, R = mine["H"], len(mine["betas"])
    tail = sum(60 + 8 * (H - 4 * (l + 1)) for l in range(R))
    words = np.frombuffer(b.tobytes(), dtype=np.uint32).copy()
    assert int(words[len(words) - tail]) == mine["queries"][-1][2][0][0][0]
    words[len(words) - tail] ^= 1                              # the last query's first sibling word
    with pytest.raises(_lib.ZkHipError):
        fri16_view_shard(words.view(np.uint8), g["log_n"], g["width"], g["public"], prm)
    # the fold-by-2 view keeps refusing these proofs
    with pytest.raises(_lib.ZkHipError):
        fri_view_shard(b, g["log_n"], g["width"], g["public"], prm)


def test_two_queries_of_the_second_golden_proof_share_a_layer_row():
    """the multiplicities of LAYERS are exercised by a committed fixture"""
    v = golden_view("v8_groups_r0_lookup_8x16")
    tl = A.key_tables(v)[0]
    assert sorted(int(m) for m in tl[:, A.LAY_M] if m) == [1, 1, 1, 1, 2]


# ------------------------------------------------------------------ (c) constraints and buses
@pytest.mark.parametrize("name", FOLD16_GOLDEN)
def test_traces_of_the_golden_views_satisfy_every_constraint_and_balance_every_bus(name):
    main, pre, progs, tabs, pub = A.machine(golden_view(name))
    assert violations(main, pre, progs, tabs, pub) == ([], {})


@pytest.mark.parametrize("R,F,b,Q", RANDOM_SHAPES)
def test_traces_of_random_views_satisfy_every_constraint_and_balance_every_bus(R, F, b, Q):
    v = A.random_view(R, F, b, Q, seed=7 * R + F)
    assert A.consistent(v)
    A.chains(v, check=True)
    tl = A.key_tables(v)[0]
    assert max(int(m) for m in tl[:, A.LAY_M]) >= 2            # at least two queries share a row at some layer
    main, pre, progs, tabs, pub = A.machine(v)
    assert violations(main, pre, progs, tabs, pub) == ([], {})


# ------------------------------------------------------------------ (d) what the constraints catch, one cell at a time
def test_what_single_cells_the_machine_catches():
    R, F, b, Q = 3, 2, 2, 6
    v = A.random_view(R, F, b, Q, seed=3)
    main, pre, progs, tabs, pub = A.machine(v)
    o = A.order(R, F, Q)
    at = {t: i for i, t in enumerate(o)}
    assert violations(main, pre, progs, tabs, pub) == ([], {})

    def caught(table, fn, in_pre=False):
        m, p = [x.copy() for x in main], [None if x is None else x.copy() for x in pre]
        fn((p if in_pre else m)[at[table]])
        bad, net = violations(m, p, progs, tabs, pub)
        return bool(bad) or bool(net)

    def bump(r, c):
        return lambda t: t.__setitem__((r, c), (int(t[r, c]) + 1) % P)
    own0 = v["queries"][0][0] & 15
    sib = (own0 + 1) % 16
    assert caught(A.FOLD16, bump(0, A.E + 4 * sib + 1))                         # a sibling entry (the fold no longer follows; LAYERS lists another)
    assert caught(A.FOLD16, bump(0, A.E + 4 * own0))                            # the own entry
    assert caught(A.FOLD16, bump(1, A.OWN + 2))                                 # ... and its copy on a later row (= the previous row's fold)

    def move_flag(t):
        t[1, A.OF + int(np.argmax(t[1, A.OF:A.OF + 16]))] = 0
        t[1, A.OF + (int(np.argmax(main[at[A.FOLD16]][1, A.OF:A.OF + 16])) + 1) % 16] = 1
    assert caught(A.FOLD16, move_flag)                                          # a one-hot flag moved

    def rotate_x0(t):
        """x0 of a chain's FIRST row times a 16th root of unity, with its inverse and every square kept consistent: the forward recurrence
        x0' = x0^16 w_16^(-..) does not see it (w^16 = 1) -- the backward product does"""
        from pyref import two_adic_generator
        w = two_adic_generator(4)
        x = int(t[0, A.X]) * w % P
        xi = pow(x, P - 2, P)
        for col in (A.X, A.X2, A.X4, A.X8, A.X16):
            t[0, col], x = x, x * x % P
        for col in (A.XI, A.XI2, A.XI4, A.XI8):
            t[0, col], xi = xi, xi * xi % P
        t[0, A.GX16] = t[0, A.X16]
    m = [x.copy() for x in main]
    rotate_x0(m[at[A.FOLD16]])
    failed = {c for i, c, r in violations(m, pre, progs, tabs, pub)[0] if i == at[A.FOLD16]}
    cons = constraints_of(progs[at[A.FOLD16]])
    V = A.V
    backward = cons.index((0, [(1, [V(A.L), V(A.X)]), (P - 1, [V(A.L), V(A.B)])]))
    forward = [i for i, (sel, terms) in enumerate(cons) if terms[0] == (1, [V(A.G), V(A.X, True)])]
    squares = [i for i, (sel, terms) in enumerate(cons) if len(terms) == 2 and terms[0][1] in ([V(c)] for c in (A.X2, A.X4, A.X8, A.X16, A.XI2, A.XI4, A.XI8))]
    inverse = cons.index((0, [(1, [V(A.ACTIVE), V(A.X), V(A.XI)]), (P - 1, [V(A.ACTIVE)])]))
    assert len(forward) == 1 and len(squares) == 7
    assert backward in failed and not (failed & set(forward + squares + [inverse]))      # the backward product sees it; the recurrence, the squarings and X XI = 1 do not
    assert caught(A.FOLD16, rotate_x0)

    def final_index_bit(t):
        r = R - 1                                                                # the last row of chain 0: another nibble flag (one bit of the final index)
        flags = t[r, A.N:A.N + 16]
        j = int(np.argmax(flags))
        t[r, A.N + j], t[r, A.N + (j ^ 1)] = 0, 1
    assert caught(A.FOLD16, final_index_bit)
    assert caught(A.FINAL, bump(1, A.FX - A.FIN_PRE))                           # X changed in the middle of a block
    assert caught(A.FINAL, bump(2, A.FC - A.FIN_PRE + 1))                       # one coefficient in FINAL
    assert caught(A.COEFFS, bump(1, 2), in_pre=True)                            # ... or in COEFFS
    assert caught(A.LAYERS, bump(0, A.LAY_M), in_pre=True)                      # one LAYERS multiplicity
    assert caught(A.QUERIES, bump(0, 5), in_pre=True)                           # one QUERIES multiplicity


# ------------------------------------------------------------------ (e) the key and the machine under the oracle's prover
@pytest.mark.parametrize("name", FOLD16_GOLDEN)
def test_host_key_equals_the_oracles_setup_on_the_restated_tables(oracle, name):
    v = golden_view(name)
    main, pre, progs, tabs, pub = A.machine(v)
    lns = shape_of(main, pre)[0]
    for shape in ((1, 12, 4), (2, 7, 0)):
        assert fri16_key_host(v, Params(*shape)).tolist() == oracle.machine_setup(pre, lns, oracle.default_params(*shape)).tolist()


@pytest.mark.parametrize("which,shape", [("v3_r0_9x8", (1, 12, 4)), ("v8_groups_r0_lookup_8x16", (2, 7, 0)), ((2, 2, 2, 11), (1, 10, 2))])
def test_machine_under_the_oracle_prover_and_three_verifiers(oracle, which, shape):
    O = oracle
    v = golden_view(which) if isinstance(which, str) else A.random_view(*which, seed=5)
    R, F, b, Q = len(v["betas"]), v["F"], v["b"], len(v["queries"])
    main, pre, progs, tabs, pub = A.machine(v)
    lns, ws, pws = shape_of(main, pre)
    oprm, prm = O.default_params(*shape), Params(*shape)
    root = O.machine_setup(pre, lns, oprm)
    assert fri16_key_host(v, prm).tolist() == root.tolist()
    proof = O.prove_machine_keyed(main, pre, progs, tabs, pub, oprm)
    lib = _lib.load()
    assert lib.zkhip_fri16_proof_size(R, F, b, Q, C.byref(prm)) == proof.size

    def three(pub_, root_, Q_=Q):
        """the verdicts of the oracle, the library's fri16 verifier and the Python verifier.  The query count is part of the SHAPE: another count
        means the heights, and with them the order, of another machine"""
        o = A.order(R, F, Q_)
        lr, pg, tb = A.log_rows(R, F, Q_), A.programs(R, F + b), A.interactions(R)
        lns_, ws_, pws_ = [lr[t] for t in o], [[A.width_of(F + b), A.FIN_MAIN, 4, 4, 4][t] for t in o], [[0, A.FIN_PRE, A.LAY_PRE, A.Q_PRE, A.C_PRE][t] for t in o]
        pg, tb = [pg[t] for t in o], [tb[t] for t in o]
        if Q_ == Q:
            assert (lns_, ws_, pws_) == (lns, ws, pws) and all(x.tolist() == y.tolist() for x, y in zip(pg + tb, progs + tabs))
        x = O.verify_machine_keyed(proof, lns_, ws_, pws_, root_, pg, tb, pub_, oprm) == 0
        y = verify_fri16(proof, pub_, R, F, b, Q_, root_, prm)[0] == 0
        try:
            z = pyverify_chips.verify(proof.tobytes(), lns_, ws_, pub_, shape[0], shape[1], shape[2], programs=pg, tables=tb, pre_widths=pws_,
                                      pre_root=[int(c) for c in root_]) is True
        except Exception:
            z = False
        return x, y, z
    assert three(pub, root) == (True, True, True)
    assert verify_machine_keyed(proof, lns, ws, pws, root, progs, tabs, pub, prm) == (0, 0)
    bad_pub = list(pub)
    bad_pub[5 % len(pub)] = (bad_pub[5 % len(pub)] + 1) % P
    assert three(bad_pub, root) == (False, False, False)                         # one beta changed
    bad_root = root.copy()
    bad_root[3] = (int(bad_root[3]) + 1) % P
    assert three(pub, bad_root) == (False, False, False)                         # one key word changed
    assert three(pub, root, Q + 40) == (False, False, False)                     # the query count changed: another machine


def test_entry_point_argument_checks():
    lib = _lib.load()
    u32p = _lib.u32p
    prm = Params(1, 8, 2)
    v = A.random_view(2, 2, 2, 5, seed=1)
    bt, fp, ix, vl, sb = A.view_arrays(v)
    p = lambda a: a.ctypes.data_as(u32p)
    vk = np.zeros(8, dtype=np.uint32)
    ok = lambda: lib.zkhip_fri16_key_host(2, 2, 2, 5, p(bt), p(fp), p(ix), p(vl), p(sb), C.byref(prm), p(vk))
    assert ok() == 0
    b8 = np.zeros(8, dtype=np.uint8).ctypes.data_as(_lib.u8p)
    # shapes outside the list: an error and a message, at key time
    for shape in ((0, 2, 2, 5), (6, 2, 2, 5), (2, 9, 2, 5), (2, 8, 4, 5), (2, 2, 0, 5), (2, 2, 2, 0), (2, 2, 2, 1025), (5, 8, 3, 5)):
        assert lib.zkhip_fri16_key_host(*shape, p(bt), p(fp), p(ix), p(vl), p(sb), C.byref(prm), p(vk)) == -1 and b"fri16" in lib.zkhip_last_error()
        assert lib.zkhip_fri16_proof_size(*shape, C.byref(prm)) == 0
        assert lib.zkhip_fri16_describe(*shape, 0, 0, None, 0, None, None, None, None) == 0
        assert lib.zkhip_verify_fri16(b8, 8, *shape, p(bt), p(vk), C.byref(prm), None) != 0
    # NULLs
    for k in range(5):
        args = [p(bt), p(fp), p(ix), p(vl), p(sb)]
        args[k] = None
        assert lib.zkhip_fri16_key_host(2, 2, 2, 5, *args, C.byref(prm), p(vk)) == -1 and b"null" in lib.zkhip_last_error()
    assert lib.zkhip_fri16_key_host(2, 2, 2, 5, p(bt), p(fp), p(ix), p(vl), p(sb), None, p(vk)) == -1
    assert lib.zkhip_fri16_key_host(2, 2, 2, 5, p(bt), p(fp), p(ix), p(vl), p(sb), C.byref(prm), None) == -1
    assert lib.zkhip_fri16_proof_size(2, 2, 2, 5, None) == 0 and lib.zkhip_fri16_proof_size(2, 2, 2, 5, C.byref(prm)) > 0
    assert lib.zkhip_fri16_describe(2, 2, 2, 5, 5, 0, None, 0, None, None, None, None) == 0 and lib.zkhip_fri16_describe(2, 2, 2, 5, 0, 2, None, 0, None, None, None, None) == 0
    # a non-canonical word, an index with too many bits, a view whose chain does not end in the final polynomial, two queries that disagree
    bad = vl.copy(); bad[0] = P
    assert lib.zkhip_fri16_key_host(2, 2, 2, 5, p(bt), p(fp), p(ix), p(bad), p(sb), C.byref(prm), p(vk)) == -1 and b"canonical" in lib.zkhip_last_error()
    bad = ix.copy(); bad[0] |= 1 << 12
    assert lib.zkhip_fri16_key_host(2, 2, 2, 5, p(bt), p(fp), p(bad), p(vl), p(sb), C.byref(prm), p(vk)) == -1 and b"index" in lib.zkhip_last_error()
    bad = sb.copy(); bad[60 * 2 * 4 + 7] = (int(bad[60 * 2 * 4 + 7]) + 1) % P
    assert lib.zkhip_fri16_key_host(2, 2, 2, 5, p(bt), p(fp), p(ix), p(vl), p(bad), C.byref(prm), p(vk)) == -1 and b"final polynomial" in lib.zkhip_last_error()
    bad = fp.copy(); bad[1] = (int(bad[1]) + 1) % P
    assert lib.zkhip_fri16_key_host(2, 2, 2, 5, p(bt), p(bad), p(ix), p(vl), p(sb), C.byref(prm), p(vk)) == -1
    # the view entry: NULLs, a fold-by-2 proof
    g = GOLDEN["v1_6x8"]
    b = load("v1_6x8")
    pv = np.array(g["public"], dtype=np.uint32)
    gp = Params(*g["shape"])
    big = np.zeros(1 << 16, dtype=np.uint32)
    u8 = b.ctypes.data_as(_lib.u8p)
    assert lib.zkhip_fri16_view_shard(u8, b.size, g["log_n"], g["width"], p(pv), pv.size, C.byref(gp), p(big), p(big), p(big), p(big), p(big), None, None) == -1
    assert b"fold-by-16" in lib.zkhip_last_error()
    assert lib.zkhip_fri16_view_shard(u8, b.size, g["log_n"], g["width"], p(pv), pv.size, C.byref(gp), None, p(big), p(big), p(big), p(big), None, None) == -1
    assert lib.zkhip_fri16_view_path_words(g["log_n"], C.byref(gp)) == 0 and lib.zkhip_fri16_view_path_words(9, None) == 0
    r0 = Params(*GOLDEN["v3_r0_9x8"]["shape"])
    assert lib.zkhip_fri16_view_path_words(9, C.byref(r0)) == 8 * (7 + 3)
    # without a device the provers refuse (no fallback)
    if lib.zkhip_device_count() == 0:
        from zktls_amd.device import Context
        with pytest.raises(_lib.ZkHipError):
            Context(0)
    assert lib.zkhip_fri16_key(None, 2, 2, 2, 5, p(bt), p(fp), p(ix), p(vl), p(sb), C.byref(prm), None, p(vk)) == -1
    assert lib.zkhip_fri16_gen_traces(None, 2, 2, 2, 5, p(bt), p(fp), p(ix), p(vl), p(sb), None, 0, None, 0) == -1
    assert lib.zkhip_prove_fri16(None, None, 2, 2, 2, 5, p(bt), p(fp), p(ix), p(vl), p(sb), C.byref(prm), None, 0, None) == -1
    assert lib.zkhip_verify_fri16(None, 0, 2, 2, 2, 5, p(bt), p(vk), C.byref(prm), None) != 0
