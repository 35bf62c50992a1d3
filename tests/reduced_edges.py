"""Cases, fills and plain restatements for the stages between the openings and the queries: the reduced opening (FRI input), the
device-challenge fold and the proof-of-work search.  Shared by test_reduced_edges_cpu.py and test_gpu_reduced_edges.py (no GPU and
no library call here).

The reduced opening of one chip (csrc/stark.hip launch_reduced_opening, oracle/stark.c orc_reduced_opening):

  out[p] (+)= off_loc d1 (A_T - y_loc) + off_next d2 (A_T - y_next) + [off_pl d1 (A_P - y_pl) + off_pn d2 (A_P - y_pn)] + off_q d1 (A_Q - y_q)
  A_M = sum_j weights[j] M[p][j],  d1 = dinv[p],  d2 = dinv[rows + p]

launch_rowdot takes one of five kernels for A_T and A_P (rowdot_form below mirrors csrc/stark.hip rowdot_form): with L = lanes_for(width)
lanes per row and nk = ceil(width / 4 / L) column quads per lane, rowdot_regs_kernel<nk> when nk <= 4, rows % (256 / L) == 0 and
rows >= (256 / L) * 16, else rowdot_kernel.  CASES writes the form each case must take as a LITERAL: test_reduced_edges_cpu.py holds the
literals against the mirror, test_gpu_reduced_edges.py holds them against what the library reports it launched.
"""
import numpy as np

import pyref
from field_edges import EDGE_WORDS
from oracle_lib import P, from_monty

ROWDOT_TRIPS = 16
SCALARS = ("y_loc", "y_next", "y_pl", "y_pn", "y_q", "off_next", "off_pl", "off_pn", "off_q", "off_loc")     # the order of the entry's 40 words
FILLS = ("edges", "saturating", "uniform")
TAIL = 64                                   # words kept behind the output, which no launch may touch
TAIL_WORD = 0xA5A5A5A5


def lanes_for(width):
    g, l = width // 4, 1
    while l < g and l < 16:
        l <<= 1
    return l


def rowdot_form(width, rows):
    """0: rowdot_kernel, 1..4: rowdot_regs_kernel<NK>"""
    L = lanes_for(width)
    nk = (width // 4 + L - 1) // L
    return nk if 1 <= nk <= 4 and rows % (256 // L) == 0 and rows >= (256 // L) * ROWDOT_TRIPS else 0


# (id, log_rows, width, padded, p_width, q_width, accumulate, form of the trace block, form of the permutation block or -1)
#   thr / below / twice: the register form at its row threshold (256 / L) * 16 for every L (widths 4, 8, 12 -- three quads on four lanes --, 32, 64), one
#                        step below it (generic) and at twice the threshold (two workgroups)
#   nk:   256 rows, sixteen lanes: every NK with the last k full (64, 128, 192, 256) and holding one lane (68, 132, 196); 260 is nk = 5, generic
#   wide: the widest row, generic;  part: two rows, a wave that is not full
# padded 1: the trace block starts 4 columns into rows of pitch width + 8 (the keyed machine's [pre | main] row), the permutation block has pitch p_width + 4,
# the quotient block q_width + 4.  The switches are spread over the shapes (not a full product): p_width 260 puts a generic permutation block beside a register
# trace block, p_width 8 reaches rowdot_regs_kernel<1> from 2048 rows on.
CASES = (
    ("thr-4x2^12", 12, 4, 0, 0, 0, 0, 1, -1),
    ("below-4x2^11", 11, 4, 1, 8, 8, 0, 0, 1),
    ("twice-4x2^13", 13, 4, 0, 8, 16, 1, 1, 1),
    ("thr-8x2^11", 11, 8, 1, 0, 8, 1, 1, -1),
    ("below-8x2^10", 10, 8, 0, 8, 16, 0, 0, 0),
    ("twice-8x2^12", 12, 8, 1, 8, 0, 0, 1, 1),
    ("thr-12x2^10", 10, 12, 0, 0, 16, 0, 1, -1),
    ("below-12x2^9", 9, 12, 1, 8, 0, 0, 0, 0),
    ("twice-12x2^11", 11, 12, 0, 260, 8, 1, 1, 0),
    ("thr-32x2^9", 9, 32, 1, 0, 0, 1, 1, -1),
    ("below-32x2^8", 8, 32, 0, 8, 8, 0, 0, 0),
    ("twice-32x2^10", 10, 32, 1, 260, 16, 0, 1, 0),
    ("thr-64x2^8", 8, 64, 0, 0, 8, 0, 1, -1),
    ("below-64x2^7", 7, 64, 1, 8, 16, 0, 0, 0),
    ("twice-64x2^9", 9, 64, 0, 260, 0, 1, 1, 0),
    ("nk-64x2^8", 8, 64, 1, 0, 16, 1, 1, -1),
    ("nk-68x2^8", 8, 68, 0, 8, 0, 0, 2, 0),
    ("nk-128x2^8", 8, 128, 1, 260, 8, 0, 2, 0),
    ("nk-132x2^8", 8, 132, 0, 0, 0, 0, 3, -1),
    ("nk-192x2^8", 8, 192, 1, 8, 8, 0, 3, 0),
    ("nk-196x2^8", 8, 196, 0, 260, 16, 1, 4, 0),
    ("nk-256x2^8", 8, 256, 1, 0, 8, 1, 4, -1),
    ("nk-260x2^8", 8, 260, 0, 8, 16, 0, 0, 0),
    ("wide-1024x2^6", 6, 1024, 1, 260, 0, 0, 0, 0),
    ("part-4x2^1", 1, 4, 0, 0, 16, 0, 0, -1),
    ("part-16x2^1", 1, 16, 1, 8, 0, 0, 0, 0),
    ("part-64x2^1", 1, 64, 0, 260, 8, 1, 0, 0),
    ("part-260x2^1", 1, 260, 1, 0, 0, 1, 0, -1),
)

# every switch combination at a height the pure-Python restatement walks (test_reduced_edges_cpu.py): rows 4 and 64
SMALL_CASES = tuple(("small-%dx2^%d-p%d-q%d-a%d-pad%d" % (w, lr, pw, qw, acc, pad), lr, w, pad, pw, qw, acc, 0, 0 if pw else -1)
                    for lr, w in ((2, 12), (6, 20)) for pw in (0, 8) for qw in (0, 8, 16) for acc in (0, 1) for pad in (0, 1))


def _draw(rng, fill, shape):
    """Montgomery WORDS (what the kernels see)"""
    if fill == "edges":
        return rng.choice(EDGE_WORDS, shape).astype(np.uint32)
    if fill == "saturating":
        return np.full(shape, P - 1, dtype=np.uint32)          # the largest word: every dacc2 running sum at its maximum
    assert fill == "uniform"
    return rng.integers(0, P, shape, dtype=np.uint32)


def build(case, fill, seed=0):
    """the words of one case: a dict of
         tbuf / pbuf / qbuf  [rows][pitch] (pbuf, qbuf None when absent), t0 / p0 / q0 the block's first column, weights [n][4], dinv [2][rows][4],
         scalars [10][4], out0 [rows][4] (edge words when the case accumulates, else 0xFFFFFFFF: words that must not be read)
       Padding columns hold words of the same fill, so a kernel that reads them computes something else."""
    name, log_rows, width, padded, p_width, q_width, accumulate, _, _ = case
    rng = np.random.default_rng([seed, log_rows, width, p_width, q_width, FILLS.index(fill)])
    rows = 1 << log_rows
    d = dict(name=name, rows=rows, log_rows=log_rows, width=width, p_width=p_width, q_width=q_width, accumulate=accumulate)
    d["t0"], d["tbuf"] = (4, _draw(rng, fill, (rows, width + 8))) if padded else (0, _draw(rng, fill, (rows, width)))
    d["p0"], d["pbuf"] = (0, _draw(rng, fill, (rows, p_width + (4 if padded else 0)))) if p_width else (0, None)
    d["q0"], d["qbuf"] = (0, _draw(rng, fill, (rows, q_width + (4 if padded else 0)))) if q_width else (0, None)
    d["weights"] = _draw(rng, fill, (max(width, p_width, q_width), 4))
    d["dinv"] = _draw(rng, fill, (2, rows, 4))
    d["scalars"] = _draw(rng, fill, (10, 4))
    d["out0"] = rng.choice(EDGE_WORDS, (rows, 4)).astype(np.uint32) if accumulate else np.full((rows, 4), 0xFFFFFFFF, dtype=np.uint32)
    return d


def block(d, which):
    """the [rows][width] view of a block inside its padded buffer"""
    buf, c0, w = {"t": (d["tbuf"], d["t0"], d["width"]), "p": (d["pbuf"], d["p0"], d["p_width"]), "q": (d["qbuf"], d["q0"], d["q_width"])}[which]
    return None if buf is None else buf[:, c0:c0 + w]


def canonical(words):
    """the field elements the words stand for (the oracle's side)"""
    return None if words is None else from_monty(words)


def oracle_expected(oracle, d):
    """[rows][4] canonical values from orc_reduced_opening on the case's values"""
    cb = {k: canonical(d[k]) for k in ("tbuf", "pbuf", "qbuf")}
    view = lambda k, c0, w: None if cb[k] is None else cb[k][:, c0:c0 + w]
    out0 = canonical(d["out0"]) if d["accumulate"] else None
    return oracle.reduced_opening(view("tbuf", d["t0"], d["width"]), view("pbuf", d["p0"], d["p_width"]), view("qbuf", d["q0"], d["q_width"]),
                                  canonical(d["weights"]), canonical(d["dinv"]), canonical(d["scalars"]), d["accumulate"], out0)


# ---- the same in plain Python integers (pyref.ext_mul)
def _add(a, b):
    return [(x + y) % P for x, y in zip(a, b)]


def _sub(a, b):
    return [(x - y) % P for x, y in zip(a, b)]


def _dot(weights, row):
    acc = [0, 0, 0, 0]
    for w, v in zip(weights, row):
        acc = _add(acc, [c * v % P for c in w])
    return acc


def python_expected(d):
    ints = lambda a: None if a is None else canonical(a).astype(object).tolist()
    t, p, q = (ints(block(d, k)) for k in "tpq")
    wt, dinv, out0 = ints(d["weights"]), ints(d["dinv"]), ints(d["out0"])
    s = dict(zip(SCALARS, ints(d["scalars"])))
    mul = pyref.ext_mul
    out = []
    for r in range(d["rows"]):
        d1, d2 = dinv[0][r], dinv[1][r]
        at = _dot(wt, t[r])
        acc = mul(s["off_loc"], mul(_sub(at, s["y_loc"]), d1))
        acc = _add(acc, mul(s["off_next"], mul(_sub(at, s["y_next"]), d2)))
        if p is not None:
            ap = _dot(wt, p[r])
            acc = _add(acc, mul(s["off_pl"], mul(_sub(ap, s["y_pl"]), d1)))
            acc = _add(acc, mul(s["off_pn"], mul(_sub(ap, s["y_pn"]), d2)))
        aq = _dot(wt, q[r]) if q is not None else [0, 0, 0, 0]
        acc = _add(acc, mul(s["off_q"], mul(_sub(aq, s["y_q"]), d1)))
        if d["accumulate"]:
            acc = _add(acc, out0[r])
        out.append(acc)
    return np.array(out, dtype=np.uint64).astype(np.uint32)


# ---- proof of work: the sponge state the search starts from, and the search itself one candidate at a time
def grind_state(oracle, seed_words, pending):
    """an oracle challenger that absorbed eight seed words (one permutation) and holds `pending` more: -> (challenger, state[16] canonical with the pending
    inputs written to words [0, pending), slot = pending)"""
    ch = oracle.OracleChallenger()
    ch.observe(np.asarray(seed_words, dtype=np.uint32))
    assert ch.c.n_input == 0
    ch.observe(np.array([i * 0x01000193 % P for i in range(1, pending + 1)], dtype=np.uint32))
    assert ch.c.n_input == pending
    state = np.array(ch.c.state, dtype=np.uint32)
    state[:pending] = np.array(ch.c.input, dtype=np.uint32)[:pending]
    return ch, state, pending


def is_witness(oracle, state, slot, bits, w):
    s = np.array(state, dtype=np.uint32)
    s[slot] = w
    return w < P and (int(oracle.poseidon2(s)[7]) & ((1 << bits) - 1)) == 0


def grind_reference(oracle, state, slot, bits, base, count, result=0xFFFFFFFF):
    """min(result, the smallest witness in [base, base + count)): every candidate is tried"""
    for w in range(base, base + count):
        if w >= result:
            break
        if is_witness(oracle, state, slot, bits, w):
            return w
    return result


# a state whose smallest 10-bit witness lies beyond the first two windows of 256 candidates (found with grind_reference, held by test_reduced_edges_cpu.py)
LATE_SEED = (11, 22, 33, 44, 55, 66, 77, 88)
LATE_PENDING = 3
LATE_BITS = 10
LATE_WITNESS = 629
