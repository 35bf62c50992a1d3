"""Edge Montgomery words and the inputs built from them, shared by test_field_edges_cpu.py and test_gpu_field_edges.py.

The device keeps field elements as Montgomery words (x R mod P, R = 2^32), and every range argument in the kernels
(babybear.cuh, ntt_bfly.cuh, poseidon2.cuh) is about those WORDS.  DeviceBuffer.upload / Context.from_numpy take canonical
values and convert them, so a canonical edge value such as P-1 reaches a kernel as the word P - R1, not as P-1.  The helpers
here go the other way: pick the words, and hand the tests the canonical values that upload to exactly those words
(edge_canonical), so `ctx.from_numpy(edge_canonical(w))` and `ctx.from_raw(w)` put the same words on the device.

download() reduces mod P on the way back, so it cannot see a non-canonical output word; assert_canonical reads the raw words.
"""
import numpy as np

from oracle_lib import P, from_monty

MONTY_R1 = (1 << 32) % P            # the Montgomery word of 1

# word -> the bound it sits on
EDGE_WORD_REASONS = {
    0: "zero: dcanon / dsub borrow paths, the additive identity in every butterfly",
    1: "smallest non-zero word: dred / monty_reduce of a tiny product",
    2: "small word: dsub(0, x) wraps to P - 2",
    P - 1: "largest canonical word: dadd carries to 2P - 2, dcanon's top case",
    P - 2: "next to the top: dadd of two lands at 2P - 4, one subtraction must still be enough",
    (P - 1) // 2: "centered() boundary from below: the signed Poseidon2 state's largest positive representative",
    (P + 1) // 2: "centered() boundary from above: the signed state's most negative representative",
    P // 2: "P/2: the half-range split of dbfly_mul's (0.26 P, 1.74 P) output window",
    P // 2 + 1: "P/2 + 1: the other side of that split",
    MONTY_R1: "Montgomery one: the multiplicative identity as the device holds it",
    P - MONTY_R1: "Montgomery minus one: the word of P - 1, the common edge input before this module existed",
    (1 << 27) - 1: "2^27 - 1: below the 2^27 factor of P - 1, the lazy stage-4 (LAZY_OUT / SD) slack",
    1 << 27: "2^27: P = 15 * 2^27 + 1, the two-adic limit",
    (1 << 27) + 1: "2^27 + 1: just past it",
    1 << 30: "2^30: dmul_sd's (0.03 P, 1.97 P) window and dacc2's acc < 2^32 P headroom at a large operand",
}
EDGE_WORDS = np.array(sorted(EDGE_WORD_REASONS), dtype=np.uint32)


def edge_canonical(words):
    """canonical values whose Montgomery words are `words` (feed to from_numpy / upload)"""
    return from_monty(np.asarray(words, dtype=np.uint32))


def assert_canonical(buf, nwords=None, offset=0):
    """every word the kernel wrote is < P (download() would reduce a P or a P + 5 and hide it)"""
    w = buf.download_monty(nwords, offset)
    bad = np.flatnonzero(w >= P)
    assert bad.size == 0, "non-canonical words at %s: %s" % (bad[:8].tolist(), w[bad[:8]].tolist())


def assert_canonical_words(words):
    w = np.asarray(words, dtype=np.uint32)
    bad = np.flatnonzero(w.ravel() >= P)
    assert bad.size == 0, "non-canonical words at %s: %s" % (bad[:8].tolist(), w.ravel()[bad[:8]].tolist())


# ---- column patterns.  Each returns n canonical values (the words are the edge words).
def _w(rng):
    return int(rng.choice(EDGE_WORDS))


def col_constant(n, rng):
    return edge_canonical(np.full(n, _w(rng), dtype=np.uint32))


def col_alternating(n, rng):
    a, b = _w(rng), _w(rng)
    return edge_canonical(np.where(np.arange(n) % 2 == 0, a, b).astype(np.uint32))


def col_impulse_first(n, rng):
    c = np.zeros(n, dtype=np.uint32)
    c[0] = _w(rng) or P - MONTY_R1
    return edge_canonical(c)


def col_impulse_last(n, rng):
    c = np.zeros(n, dtype=np.uint32)
    c[-1] = _w(rng) or P - MONTY_R1
    return edge_canonical(c)


def col_random_edges(n, rng):
    return edge_canonical(rng.choice(EDGE_WORDS, n))


def col_uniform(n, rng):
    return rng.integers(0, P, n, dtype=np.uint32)


PATTERNS = (col_constant, col_alternating, col_impulse_first, col_impulse_last, col_random_edges, col_uniform)


def ntt_preimage(oracle, outs):
    """inputs whose forward transform (natural order) is `outs` -- so the transform's OUTPUT words are edge words"""
    return oracle.ntt(outs, inverse=True)


def lde_preimage(oracle, outs, shift=31):
    """inputs whose coset LDE has `outs` ([n][w], canonical) as its first n rows (coset 0, bit-reversed order):
    row r of coset 0 is f(shift w_n^bitrev(r)), so the coefficients are c_j = idft(outs[bitrev])_j / shift^j"""
    n = outs.shape[0]
    log_n = n.bit_length() - 1
    coeffs = oracle.ntt(outs[bitrev_perm(log_n)], inverse=True).astype(np.uint64)
    coeffs = (coeffs * powers(pow(shift, P - 2, P), n)[:, None]) % P
    return oracle.ntt(coeffs.astype(np.uint32))


def bitrev_perm(log_n):
    idx = np.arange(1 << log_n, dtype=np.uint32)
    out = np.zeros_like(idx)
    for b in range(log_n):
        out |= ((idx >> b) & 1) << (log_n - 1 - b)
    return out


def powers(x, n):
    """x^0 .. x^(n-1) mod P as uint64"""
    lo = np.ones(min(n, 1024), dtype=np.uint64)
    for j in range(1, lo.size):
        lo[j] = lo[j - 1] * x % P
    hi = np.ones((n + 1023) // 1024, dtype=np.uint64)
    step = pow(x, 1024, P)
    for j in range(1, hi.size):
        hi[j] = hi[j - 1] * step % P
    return ((hi[:, None] * lo[None, :]) % P).ravel()[:n]


def edge_matrix(n, w, seed, oracle=None, outputs=None, shift=31):
    """[n][w] canonical values, column j on pattern (j + seed) mod the pattern count; with an oracle, every seventh column
    (from column 6 on) is an "edge outputs" column: outputs="ntt" -> its forward transform, outputs="lde" -> coset 0 of its
    LDE (shift `shift`) is a column of random edge words"""
    rng = np.random.default_rng(seed)
    m = np.empty((n, w), dtype=np.uint32)
    pre = []
    for j in range(w):
        if oracle is not None and outputs and j % 7 == 6:
            pre.append(j)
            m[:, j] = col_random_edges(n, rng)
        else:
            m[:, j] = PATTERNS[(j + seed) % len(PATTERNS)](n, rng)
    if pre:
        sub = np.ascontiguousarray(m[:, pre])
        m[:, pre] = ntt_preimage(oracle, sub) if outputs == "ntt" else lde_preimage(oracle, sub, shift)
    return m


def edge_ext(rng, k=0):
    """extension-field challenges (alpha, beta, z, mix): the fixed edge elements, then k random edge-word draws"""
    fixed = [[P - 1] * 4, [0, 0, 0, P - 1], [1, 0, 0, 0], [P - 1, 0, 0, 0], [0, 0, 0, 1],
             edge_canonical([P - 1] * 4).tolist(), edge_canonical([0, 1, P // 2, 1 << 30]).tolist()]
    draws = [edge_canonical(rng.choice(EDGE_WORDS, 4)).tolist() for _ in range(k)]
    return [np.array(e, dtype=np.uint32) for e in fixed + draws]
