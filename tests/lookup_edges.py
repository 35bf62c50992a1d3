"""Inputs that steer the LogUp kernels onto their branches and limits, shared by test_lookup_edges_cpu.py and
test_gpu_lookup_edges.py (no GPU, no library calls here).

The plain LogUp kernel (stark.hip perm_rows_kernel) computes 1/ds - 1/dr as (dr - ds) / (ds dr) and takes the direct formula
only when ds dr = 0 (1/0 = 0).  With gamma, beta and the trace drawn at random that branch has probability
about 2^-124.  With BASE-FIELD challenges gamma = (g, 0, 0, 0), beta = (b, 0, 0, 0) the denominators are base elements,
ds = g + a_s + b b_s, and a row is steered onto a zero by solving for a_s: steered_logup_trace does that per pair for every case
of CASES at the rows where the block-local scan, the scan of the block totals and the fix-up meet.
"""
import numpy as np

from field_edges import edge_ext, edge_matrix
from oracle_lib import P

# per (special row k, pair q) the case CASES[(k + q) % 6]: the neighbours of an "ordinary" pair in its row are "both0" and "ds0",
# so with two or more pairs an ordinary pair sits beside a zero one in the same row
CASES = ("ds0", "dr0", "eq", "neg", "both0", "ordinary")


def special_rows(n):
    """row 0, the last row, the rows on both sides of every multiple of 256 below n, one mid-block row; filled up to six rows
    (as far as n allows) so that every case occurs in every pair"""
    rows = {0, n - 1}
    for m in range(256, n, 256):
        rows |= {m - 1, m}
    rows.add(min(n - 1, 256 * ((n // 256) // 2) + 100) if n > 100 else n // 2)
    r = 1
    while len(rows) < min(n, len(CASES)):
        rows.add(r)
        r += 1
    return sorted(rows)


def steered_logup_trace(log_n, width, pairs, g, b, seed):
    """-> (trace [n][width] canonical u32, gamma, beta, cases): the body is field_edges.edge_matrix (edge words on the device); at
    special_rows(n) the a_s / a_r of every pair are overwritten so that the pair is, by case:
      ds0       ds = 0 only: a_s = -(g + b b_s) mod P
      dr0       dr = 0 only
      both0     ds = dr = 0
      eq        ds == dr != 0 (phi must be four zero WORDS)
      neg       ds == -dr != 0
      ordinary  ds, dr != 0, ds != +-dr
    cases: [(row, pair, case)], so that a failing assert can name the case"""
    n = 1 << log_n
    assert 8 * pairs <= width and 0 < g < P and 0 < b < P
    t = edge_matrix(n, width, seed).astype(np.int64)
    cases = []
    for k, r in enumerate(special_rows(n)):
        for q in range(pairs):
            case = CASES[(k + q) % len(CASES)]
            a_s, b_s, a_r, b_r = (int(t[r, 8 * q + c]) for c in (0, 1, 4, 5))
            zs, zr = -(g + b * b_s) % P, -(g + b * b_r) % P            # the a that makes the denominator zero
            if case in ("ds0", "both0"):
                a_s = zs
            elif a_s == zs:
                a_s = (a_s + 1) % P
            ds = (g + a_s + b * b_s) % P
            if case in ("dr0", "both0"):
                a_r = zr
            elif case == "eq":
                a_r = (ds + zr) % P
            elif case == "neg":
                a_r = (zr - ds) % P
            else:                                                       # ds0 (dr != 0) or ordinary (dr != 0, +-ds)
                while (g + a_r + b * b_r) % P in (0, ds, (P - ds) % P):
                    a_r = (a_r + 1) % P
            t[r, 8 * q], t[r, 8 * q + 4] = a_s, a_r
            cases.append((r, q, case))
    gamma = np.array([g, 0, 0, 0], dtype=np.uint32)
    beta = np.array([b, 0, 0, 0], dtype=np.uint32)
    return t.astype(np.uint32), gamma, beta, cases


def denominators(trace, row, pair, g, b):
    """(ds, dr) of a steered pair in plain integers"""
    a_s, b_s, a_r, b_r = (int(trace[row, 8 * pair + c]) for c in (0, 1, 4, 5))
    return (g + a_s + b * b_s) % P, (g + a_r + b * b_r) % P


def edge_challenges(rng):
    """(gamma, beta): two different field_edges.edge_ext draws, for the runs that steer nothing"""
    pool = edge_ext(rng, 2)
    i, j = rng.choice(len(pool), 2, replace=False)
    return pool[int(i)], pool[int(j)]


def case_at(cases, row, col):
    """the steered case the output word (row, col) of a permutation trace belongs to (the running sum: every case of its row)"""
    here = [(q, c) for r, q, c in cases if r == row]
    if not here:
        return "no steered pair in row %d" % row
    own = [c for q, c in here if q == col // 4]
    return "pair %d: %s" % (col // 4, own[0]) if own else "running sum of a row with %s" % ", ".join("%d:%s" % qc for qc in here)


def first_mismatch(got, exp, cases):
    """None, or a message naming the first differing (row, column) and its steered case"""
    bad = np.argwhere(got != exp)
    if bad.size == 0:
        return None
    r, c = (int(x) for x in bad[0])
    return "first difference at row %d, column %d (%s): got %d, expected %d; %d words differ" % (r, c, case_at(cases, r, c), got[r, c], exp[r, c], len(bad))


def bus_balance(traces, pres, tables):
    """the buses of a machine in plain integers mod P (the constant multiplicity included; in the style of fri16_air.bus_balance):
    -> {(bus, tuple): net multiplicity mod P} of what does not cancel (empty: balanced)"""
    net = {}
    for m, p, tab in zip(traces, pres, tables):
        if tab is None:
            continue
        rows = np.asarray(m, dtype=np.int64) if p is None else np.concatenate([np.asarray(p, dtype=np.int64), np.asarray(m, dtype=np.int64)], axis=1)
        tab = [int(x) for x in tab]
        pos = 3
        for _ in range(tab[1]):
            sign, mult, bus, nv = tab[pos:pos + 4]
            cols = tab[pos + 4:pos + 4 + nv]
            pos += 4 + nv
            ms = np.ones(rows.shape[0], dtype=np.int64) if mult == 0xFFFFFFFF else rows[:, mult]
            for r in np.flatnonzero(ms):
                k = (bus, tuple(int(rows[r, c]) for c in cols))
                net[k] = (net.get(k, 0) + (-int(ms[r]) if sign else int(ms[r]))) % P
    return {k: v for k, v in net.items() if v}
