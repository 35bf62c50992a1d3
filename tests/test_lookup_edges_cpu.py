"""The reference side of test_gpu_lookup_edges.py, pinned without a GPU and without the library.

The permutation trace is restated here in plain Python: extension arithmetic from pyref / pyverify (x^4 = 11), inv(0) = 0, the direct
formula 1/ds - 1/dr, a plain running sum.  The oracle (oracle/stark.c orc_perm_trace) must equal it on the steered inputs of
tests/lookup_edges.py and on the edge-challenge runs, so the GPU test can compare against the oracle only.  Every boundary machine of
tests/machines.py is balanced in plain integers (lookup_edges.bus_balance) and proven and verified by the oracle, so a failing GPU
case can only be the device's fault.
"""
import numpy as np
import pytest

import lookup_edges as LE
import machines as M
import pyref
from pyverify import ZERO, ONE, e_add, e_scale, e_sub

P = pyref.P
G, B = 0x1234567, 0x7654321          # base-field gamma and beta of the steered runs


def inv(a):
    """1/a in F_P[x]/(x^4 - 11), inv(0) = 0 (the protocol's convention): with y = x^2, a = A + B x (A = a0 + a2 y, B = a1 + a3 y), so
    a (A - B x) = A^2 - y B^2 = c0 + c1 y and 1/(c0 + c1 y) = (c0 - c1 y) / (c0^2 - 11 c1^2).  Every result is checked by a product."""
    a = [int(x) % P for x in a]
    if a == ZERO:
        return list(ZERO)
    conj = [a[0], -a[1] % P, a[2], -a[3] % P]                        # A - B x
    c = pyref.ext_mul(a, conj)
    assert c[1] == 0 and c[3] == 0
    d = pow((c[0] * c[0] - 11 * c[2] * c[2]) % P, P - 2, P)
    r = pyref.ext_mul(conj, [c[0] * d % P, 0, -c[2] * d % P, 0])
    assert pyref.ext_mul(a, r) == ONE
    return r


def perm_trace_py(trace, pairs, gamma, beta):
    gamma, beta = [int(x) for x in gamma], [int(x) for x in beta]
    out = np.zeros((trace.shape[0], 4 * (pairs + 1)), dtype=np.uint32)
    run = list(ZERO)
    for i, row in enumerate(trace.tolist()):
        for q in range(pairs):
            ds = e_add(e_add(gamma, [row[8 * q], 0, 0, 0]), e_scale(beta, row[8 * q + 1]))
            dr = e_add(e_add(gamma, [row[8 * q + 4], 0, 0, 0]), e_scale(beta, row[8 * q + 5]))
            phi = e_sub(inv(ds), inv(dr))
            out[i, 4 * q:4 * q + 4] = phi
            run = e_add(run, phi)
        out[i, 4 * pairs:] = run
    return out


def test_the_inverse_of_the_restatement_is_pyrefs():
    rng = np.random.default_rng(1)
    for a in [[1, 0, 0, 0], [0, 1, 0, 0], [P - 1, 0, P - 1, 0], [0, 0, 0, P - 1]] + rng.integers(0, P, (4, 4)).tolist():
        assert inv(a) == pyref.ext_inv(a)
    assert inv([0, 0, 0, 0]) == [0, 0, 0, 0]


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("log_n", [0, 5, 8, 9])
def test_oracle_perm_trace_equals_the_restatement_on_steered_rows(oracle, log_n, pairs):
    trace, gamma, beta, cases = LE.steered_logup_trace(log_n, 8 * pairs, pairs, G, B, seed=log_n + pairs)
    exp = perm_trace_py(trace, pairs, gamma, beta)
    got = oracle.perm_trace(trace, pairs, gamma, beta)
    assert LE.first_mismatch(got, exp, cases) is None, LE.first_mismatch(got, exp, cases)
    n = 1 << log_n
    assert {r for r, _, _ in cases} == set(LE.special_rows(n)) and {0, n - 1} <= set(LE.special_rows(n))
    if n >= 6:
        assert all({c for _, q_, c in cases if q_ == q} == set(LE.CASES) for q in range(pairs))
    if n == 512:
        assert {100 + 256, 255, 256} <= set(LE.special_rows(n))
    # each steered pair is the case it says, and its phi what that case demands
    for r, q, case in cases:
        ds, dr = LE.denominators(trace, r, q, G, B)
        phi = exp[r, 4 * q:4 * q + 4].tolist()
        i_s, i_r = pow(ds, P - 2, P), pow(dr, P - 2, P)                 # (pow(0, P - 2, P) = 0)
        assert phi == [(i_s - i_r) % P, 0, 0, 0], (r, q, case)
        if case == "ds0":
            assert ds == 0 and dr != 0 and phi[0] == (P - i_r) % P
        elif case == "dr0":
            assert dr == 0 and ds != 0 and phi[0] == i_s
        elif case == "both0":
            assert ds == 0 and dr == 0 and phi == [0, 0, 0, 0]
        elif case == "eq":
            assert ds == dr != 0 and phi == [0, 0, 0, 0]
        elif case == "neg":
            assert ds != 0 and (ds + dr) % P == 0 and phi[0] == 2 * i_s % P
        else:
            assert ds != 0 and dr != 0 and ds != dr and (ds + dr) % P != 0
    if pairs > 1 and n >= 6:                                            # an ordinary pair beside a zero one in the same row
        kinds = {(r, q): c for r, q, c in cases}
        assert any(c == "ordinary" and any(kinds.get((r, q2)) in ("ds0", "dr0", "both0") for q2 in (q - 1, q + 1)) for (r, q), c in kinds.items())


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("log_n", [0, 5, 8, 9])
def test_oracle_perm_trace_equals_the_restatement_under_edge_challenges(oracle, log_n, pairs):
    rng = np.random.default_rng(100 + log_n + pairs)
    gamma, beta = LE.edge_challenges(rng)
    assert (gamma != beta).any()
    trace = LE.edge_matrix(1 << log_n, 8 * pairs + 4, seed=log_n)       # (a width that is not 8 pairs: the last quad is not read)
    assert (oracle.perm_trace(trace, pairs, gamma, beta) == perm_trace_py(trace, pairs, gamma, beta)).all()


def _columns_read(table):
    t, pos, cols = [int(x) for x in table], 3, set()
    for _ in range(t[1]):
        mult, nv = t[pos + 1], t[pos + 3]
        cols |= set(t[pos + 4:pos + 4 + nv]) | ({mult} if mult != 0xFFFFFFFF else set())
        pos += 4 + nv
    return cols


HEIGHTS = [(8, 5), (9, 5), (9, 8)]


@pytest.mark.parametrize("case", M.BOUNDARY_CASES)
def test_boundary_machines_are_balanced_and_the_oracle_proves_them(oracle, case):
    O = oracle
    prm = O.default_params(1, 8, 4)
    for ls, lr in (HEIGHTS if case == "edge" else HEIGHTS[:1]):
        traces, pre, progs, tables, pub = M.boundary_machine(case, ls, lr, seed=ls + lr)
        lns, ws = [t.shape[0].bit_length() - 1 for t in traces], [t.shape[1] for t in traces]
        assert lns == [ls, lr]
        pres = pre or [None] * len(traces)
        assert LE.bus_balance(traces, pres, tables) == {}
        bent = [t.copy() for t in traces]                               # (the check is not vacuous: one multiplicity off by one)
        mult = int(tables[1][4])
        bent[1][3, mult] = (int(bent[1][3, mult]) + 1) % P
        assert LE.bus_balance(bent, pres, tables) != {}
        wrong = [pub[0], (pub[1] + 1) % P]
        if pre is None:
            proof = O.prove_machine(traces, progs, tables, pub, prm)
            assert O.verify_machine(proof, lns, ws, progs, tables, pub, prm) == 0
            assert O.verify_machine(proof, lns, ws, progs, tables, wrong, prm) != 0
        else:
            pws = [0 if p is None else p.shape[1] for p in pre]
            root = O.machine_setup(pre, lns, prm)
            proof = O.prove_machine_keyed(traces, pre, progs, tables, pub, prm)
            assert O.verify_machine_keyed(proof, lns, ws, pws, root, progs, tables, pub, prm) == 0
            assert O.verify_machine_keyed(proof, lns, ws, pws, root, progs, tables, wrong, prm) != 0


def test_boundary_machines_sit_on_the_limits_they_name(oracle):
    """56 against 57 distinct columns, column 511 against 512, 1 / 63 / 64 interactions, the multiplicities and buses of the edge case"""
    def subject(case):
        traces, pre, progs, tables, pub = M.boundary_machine(case, 8, 5, seed=1)
        rows = traces[0] if pre is None else np.concatenate([pre[0], traces[0]], axis=1)
        return rows, tables[0], (0 if pre is None else pre[0].shape[1])
    for case, used, top in (("used56", 56, 55), ("used57", 57, 56), ("col511", 7, 511), ("col512", 7, 512), ("keyed_used57", 57, None), ("keyed_col512", 15, 512)):
        cols = _columns_read(subject(case)[1])
        assert len(cols) == used and (top is None or max(cols) == top), case
    assert max(_columns_read(M.boundary_machine("col511", 8, 5, seed=1)[3][1])) == 511          # the balancer's tuple ends there too
    assert max(_columns_read(M.boundary_machine("col512", 8, 5, seed=1)[3][1])) == 512
    assert [int(subject(c)[1][1]) for c in ("one", "odd63", "max64")] == [1, 63, 64]
    assert len(_columns_read(subject("max64")[1])) <= 56
    rows, tab, _ = subject("edge")
    assert {int(tab[5]), int(tab[17])} == {0, P - 1}
    for mult in (8, 9, 11, 13):
        assert set(rows[:, mult].tolist()) == set(M.EDGE_MULTS)
    for case, pw in (("keyed4", 4), ("keyed20", 20)):
        rows, tab, got_pw = subject(case)
        t = [int(x) for x in tab]
        assert got_pw == pw and t[7:11] == [pw - 2, pw - 1, pw, pw + 1]                        # a tuple across pre_w
        assert t[12] < pw and min(t[15:18]) >= pw and t[19] >= pw and max(t[22:24]) < pw       # multiplicity / tuple on opposite sides
