"""Which quotient kernel a constraint program reaches, and programs built to reach each of them; shared by test_air_forms_cpu.py and
test_gpu_air_forms.py.  No GPU here.

`form()` is a MIRROR of the host's choice (csrc/stark.hip launch_quotient_air, csrc/prover.cpp run_quotient_air, csrc/kernels.h
air_wide_form) and has to be kept in step with them by hand: the GPU tests name the kernel they mean to reach, and
test_air_forms_cpu.py holds every case to this table.

`class_program()` builds FREE programs (no trace satisfies them: the stage-level entry zkhip_quotient_values_air evaluates a program
on any matrix) with a chosen number of distinct monomials per factor count; `derived_program_and_trace()` builds programs that hold
on a trace, for whole proofs, in which every record has a non-zero weight.
"""
import numpy as np

import oracle_lib as O
from field_edges import EDGE_WORDS, edge_canonical

P = O.P
V = O.air_var

# csrc/proof_common.h check_shape (and its restatements in prover.cpp / serialize.cpp): what every public entry takes
MIN_LOG_N, MAX_WIDTH = 5, 1024


# ---------------------------------------------------------------------------------------------- reading a program
def terms_of(prog):
    """(constraint, selector, coefficient, [variables]) of every term, in program order"""
    w = [int(x) for x in prog]
    p = 6
    for k in range(w[3]):
        sel, nt = w[p], w[p + 1]
        p += 2
        for _ in range(nt):
            coeff, d = w[p], w[p + 1]
            yield k, sel, coeff, w[p + 2:p + 2 + d]
            p += 2 + d
    assert p == len(w) == w[5]


def monomial_key(width, sel, variables):
    """csrc/air.h air_term_plan: the slots of a term's factors, sorted -- local column c is slot c, next-row column c slot W + c, the
    selector (one more factor) 2W + sel - 1, public-value factors are dropped (they multiply the coefficient), and a term with no
    factor left reads the constant 1 at slot 2W + 3"""
    key = []
    for v in variables:
        kind, idx = v >> 30, v & 0xFFFF
        if kind == 2:
            continue
        key.append(idx if kind == 0 else width + idx)
    if sel:
        key.append(2 * width + sel - 1)
    if not key:
        key.append(2 * width + 3)
    return tuple(sorted(key))


def class_counts(prog):
    """distinct monomials by their number of factors: [n = 1, .., n = 5]"""
    width = int(prog[2])
    keys = {monomial_key(width, sel, vs) for _, sel, _, vs in terms_of(prog)}
    return [sum(1 for k in keys if len(k) == n) for n in range(1, 6)]


def monomial_count(prog):
    """csrc/air.h air_term_count: the records of the program = its distinct monomials, rounded up to even (records go in pairs)"""
    nm = sum(class_counts(prog))
    return nm + (nm & 1)


def wide_pairs(prog):
    """record pairs per class of the wide form (air_term_records_wide pads every class to an even count)"""
    return [(c + 1) // 2 for c in class_counts(prog)]


def log_quotient_degree(prog):
    return 1 if max(len(vs) + (1 if sel else 0) for _, sel, _, vs in terms_of(prog)) <= 3 else 2


# ---------------------------------------------------------------------------------------------- the launcher's choice
def enterable(width, log_n):
    """check_shape: no public entry, stage level or whole proof, takes another shape -- so the launcher's branches for log_n <= 4 (the
    interpreter at log_n <= 2, terms<64> at log_n 3, a chain of two groups at log_n 4) and for widths that are no multiple of four are
    not live"""
    return log_n >= MIN_LOG_N and 0 < width <= MAX_WIDTH and width % 4 == 0


def form(width, M, log_n, aligned=True, lockstep=False):
    """the kernel launch_quotient_air picks.  M = monomial_count(program); aligned = `ld % 4 == 0` and a 16-byte aligned LDE pointer;
    lockstep = the call is made inside a lock-step batch.  First match wins, in the launcher's order:
      prover.cpp run_quotient_air `wide = !t_batcher && ld % 4 == 0 && aligned pointer && air_wide_form(...)`  (kernels.h air_wide_form)
      stark.hip launch_quotient_air `fits` (width % 4, ld % 4, pointer, m >= 8 << log_qd), `small`
      stark.hip launch_quotient_air `light && chain_len >= 2`, the `nt` loop, launch_chain_nt's `need`
      stark.hip launch_quotient_air launch_terms<64 / 128 / 256> by n_terms"""
    W4 = width // 4
    if M >= 2048 and width % 4 == 0 and 65 * (width + 4) * 4 <= 160 * 1024 and log_n >= 6 and aligned and not lockstep:
        return "wide<16>"
    if width % 4 or not aligned or log_n <= 2 or width > 1024 or (M <= 512 and width <= 16):
        return "interpreter"
    if M <= 512 and log_n >= 4:                          # chain_len = min(32, 2^(log_n - 3)) >= 2
        nt = 64
        while nt < 256 and 8 * W4 > (12 if nt == 64 else 16) * nt:
            nt *= 2
        need = (8 * W4 + nt - 1) // nt
        return "chain<%d,%d>" % (nt, 4 * max(1, (need + 3) // 4))
    if M <= 512:
        return "terms<64>"
    return "terms<128>" if M <= 8192 else "terms<256>"


def chain_len(log_n):
    return min(32, 1 << (log_n - 3))


# the forms a public entry can reach (enterable(): log_n >= 5), each with its lock-step twin except the wide form, which the host
# refuses inside a batch
LIVE_FORMS = ("interpreter", "chain<64,4>", "chain<64,8>", "chain<64,12>", "chain<128,8>", "chain<128,12>", "chain<128,16>",
              "terms<128>", "terms<256>", "wide<16>")
DEAD_FORMS = ("terms<64>",)                              # log_n == 3 only


# ---------------------------------------------------------------------------------------------- free programs
NONZERO_EDGE_WORDS = EDGE_WORDS[EDGE_WORDS != 0]


def _edge_coeffs(rng, k):
    return [int(c) for c in edge_canonical(rng.choice(NONZERO_EDGE_WORDS, k))]


def public_values(n_public, seed):
    """edge-word draws with 1 first, 0 in the middle and P - 1 last (a single value: one draw)"""
    rng = np.random.default_rng(seed)
    v = _edge_coeffs(rng, n_public)
    if n_public >= 2:
        v[0], v[-1] = 1, P - 1
    if n_public >= 3:
        v[n_public // 2] = 0
    return v


def counts_for(M, lqd=1):
    """a class-count vector of M distinct monomials that any width >= 16 can hold"""
    if lqd == 1:
        c2 = min(M // 4, 120)
        return [8, c2, M - 8 - c2, 0, 0]
    c2, c3, c4 = min(M // 8, 60), M // 4, M // 4
    return [8, c2, c3, c4, M - 8 - c2 - c3 - c4]


def class_program(width, counts, seed, n_public=0, max_degree=None):
    """A free program with counts[n - 1] distinct monomials of n factors (the selector counts as a factor, public values do not).
    Every monomial has a coefficient of its own whose Montgomery word is a non-zero edge word; all four selectors occur; about half of
    the factors read the next row; variables repeat (x x x'); columns 0, 3, W - 4, W - 1 and one column of every fourth column group
    occur; the constant monomial occurs (first of the one-factor class); some monomials return in further constraints with other
    coefficients and their factors in another order, so their records merge, and one monomial's two terms sum to zero.  With n_public
    > 0 a third of the terms carry public-value factors as far as the degree allows (up to five: the constant monomial's term is made
    of public values alone).  A term has at most max_degree factors, selector and public values included (default: 3 when the classes
    of four and five factors are empty, else 5), which decides log_quotient_degree.
    Returns (program, public values)."""
    W = width
    counts = list(counts) + [0] * (5 - len(counts))
    if max_degree is None:
        max_degree = 5 if counts[3] or counts[4] else 3
    assert not any(counts[n - 1] for n in range(max_degree + 1, 6))
    rng = np.random.default_rng(seed)
    required = sorted({0, 3, W - 4, W - 1} | {4 * g + (g // 4) % 4 for g in range(0, W // 4, 4)})
    keys, seen, serial = [], set(), 0

    def add(key):
        key = tuple(sorted(key))
        if key in seen:
            return False
        seen.add(key)
        keys.append(key)
        return True

    for n in range(1, 6):
        have = 0
        if n == 1 and counts[0]:
            have += add((2 * W + 3,))                                       # the constant monomial
        if n == 3 and counts[2]:
            have += add((required[1], required[1], W + required[1]))         # x x x'
        tries = 0
        while have < counts[n - 1]:
            tries += 1
            assert tries < 100 * counts[n - 1] + 1000, "width %d cannot hold %d monomials of %d factors" % (W, counts[n - 1], n)
            sel = int(rng.integers(0, 3)) if rng.random() < 0.45 else None
            nc = n - (sel is not None)
            slots = []
            for j in range(nc):
                if j == 0:
                    c = required[serial % len(required)] if serial < 2 * len(required) or rng.random() < 0.25 else int(rng.integers(0, W))
                elif rng.random() < 0.3:
                    c = slots[int(rng.integers(0, j))] % W                   # a repeated variable, on either row
                else:
                    c = int(rng.integers(0, W))
                nxt = (serial // len(required)) & 1 if j == 0 and serial < 2 * len(required) else int(rng.random() < 0.5)
                slots.append(c + W * nxt)
            if sel is not None:
                slots.append(2 * W + sel)
            if add(slots):
                have += 1
                serial += nc > 0
    coeffs = dict(zip(keys, _edge_coeffs(rng, len(keys))))
    order = [keys[i] for i in rng.permutation(len(keys))]
    kind_of = lambda key: key[-1] - 2 * W + 1 if 2 * W <= key[-1] < 2 * W + 3 else 0
    zero_key = next(k for k in order if kind_of(k) == 0 and k != (2 * W + 3,))
    pub_serial = [0]

    def variables(key, with_pub):
        vs = [V(s % W, s >= W) for s in key if s < 2 * W]
        vs = [vs[i] for i in rng.permutation(len(vs))]
        if n_public and with_pub:
            room = max_degree - len(vs) - (1 if kind_of(key) else 0)
            k = room if key == (2 * W + 3,) else min(room, 1 + pub_serial[0] % 5)
            for _ in range(max(k, 0)):
                idx = n_public - 1 if key == (2 * W + 3,) and pub_serial[0] == 0 else pub_serial[0] % n_public
                vs.insert(int(rng.integers(0, len(vs) + 1)), V(idx, public=True))
                pub_serial[0] += 1
        return vs

    cons = []
    by_kind = {s: [k for k in order if kind_of(k) == s] for s in range(4)}
    ti = 0
    for s, ks in by_kind.items():
        i = 0
        while i < len(ks):
            size = int(rng.integers(1, 24))
            terms = []
            for key in ks[i:i + size]:
                with_pub = key == (2 * W + 3,) or (ti % 3 == 0 and key != zero_key)
                vs = variables(key, with_pub)
                terms.append((coeffs[key], vs))
                if key == zero_key:
                    terms.append((P - coeffs[key], vs[::-1]))                # the same monomial again: the record's coefficient is 0
                ti += 1
            cons.append((s, terms))
            i += size
        if ks:                                                              # merging terms: monomials of this kind again, elsewhere
            again = [k for k in ks[:: max(1, len(ks) // 6)] if k != zero_key][:6]
            if again:
                cons.append((s, [(c, variables(k, False)[::-1]) for k, c in zip(again, _edge_coeffs(rng, len(again)))]))
    cons = [cons[i] for i in rng.permutation(len(cons))]
    return O.air_program(W, n_public, cons), public_values(n_public, seed + 1)


def saturated_program(width, n1, n2):
    """ONE constraint on every row (so the only weight is 1 and the records' coefficients are the program's), n1 one-factor and n2
    two-factor monomials, every coefficient the value whose Montgomery word is P - 1: on an LDE of the constant word P - 1 every
    product and every coefficient entering the 64-bit running sums (babybear.cuh dacc2: acc < 2^32 P) is at its maximum"""
    c = int(edge_canonical([P - 1])[0])
    slots = [(s,) for s in range(2 * width)][:n1]
    pairs = [(a, b) for d in range(2 * width) for a in range(2 * width - d) for b in [a + d]]
    assert len(slots) == n1 and len(pairs) >= n2
    terms = [(c, [V(s % width, s >= width) for s in key]) for key in slots + pairs[:n2]]
    return O.air_program(width, 0, [(O.SEL_ALL, terms)])


# ---------------------------------------------------------------------------------------------- programs that hold on a trace
def derived_program_and_trace(log_n, base, derived, terms_per, seed, trace_seed=None):
    """`base` free columns and `derived` columns defined from them: column 0 counts rows (first-row and transition constraints against
    two public values, as airs.counter_program), and derived column j is constrained on every row to be sum_t c_t m_t over terms_per
    monomials m_t of degree <= 3 in the base columns of the row and the next row (the next row of the last row is row 0: the
    constraint holds there too), no monomial used twice in the program, every c_t a non-zero edge value.  So every record of the
    program has a non-zero weight and a kernel that evaluates one monomial wrongly changes the proof.  The trace is computed in exact
    integers.  The program depends on `seed` alone; trace_seed varies the free columns.
    Returns (program, trace, public values); the program has derived (terms_per + 1) + 5 distinct monomials (five in the counter's two constraints)."""
    rng = np.random.default_rng(seed)
    trng = np.random.default_rng(seed if trace_seed is None else trace_seed)
    n, width = 1 << log_n, base + derived
    start, step = int(trng.integers(0, P)), int(trng.integers(1, P))
    t = np.zeros((n, width), dtype=object)
    t[:, 0] = [(start + step * i) % P for i in range(n)]
    for c in range(1, base):
        col = trng.integers(0, P, n)
        if c % 3 == 0:
            col = edge_canonical(trng.choice(EDGE_WORDS, n))
        t[:, c] = [int(x) for x in col]
    nxt = np.roll(t[:, :base], -1, axis=0)
    cons = [(O.SEL_FIRST, [(1, [V(0)]), (P - 1, [V(0, public=True)])]),
            (O.SEL_TRANSITION, [(1, [V(0, True)]), (P - 1, [V(0)]), (P - 1, [V(1, public=True)])])]
    seen = set()
    for j in range(base, width):
        terms, val = [(1, [V(j)])], np.zeros(n, dtype=object)
        for c in _edge_coeffs(rng, terms_per):
            while True:
                d = int(rng.integers(1, 4))
                slots = tuple(sorted(int(rng.integers(1, base)) + base * int(rng.random() < 0.4) for _ in range(d)))
                if slots not in seen:
                    seen.add(slots)
                    break
            prod = np.full(n, c, dtype=object)
            for s in slots:
                prod = prod * (nxt[:, s - base] if s >= base else t[:, s]) % P
            val = (val + prod) % P
            terms.append((P - c, [V(s % base, s >= base) for s in slots]))
        t[:, j] = val
        cons.append((O.SEL_ALL, terms))
    return O.air_program(width, 2, cons), t.astype(np.uint32), [start, step]
