"""The oracle against tests/pyref.py on inputs built from edge Montgomery words (tests/field_edges.py).

test_gpu_field_edges.py compares the HIP kernels with the oracle on these inputs; this file is what makes the oracle fit to be
the reference there: each operation agrees with the first-principles restatement at the same edge values.  No GPU needed.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import field_edges as FE
import pyref
from field_edges import EDGE_WORDS, MONTY_R1, P, edge_canonical

HERE = os.path.dirname(os.path.abspath(__file__))


def _cols(m):
    return [[int(x) for x in m[:, j]] for j in range(m.shape[1])]


def test_edge_words_and_their_canonical_preimages(oracle):
    assert MONTY_R1 == 0x0ffffffe and P - MONTY_R1 == 0x68000003
    assert len(set(EDGE_WORDS.tolist())) == len(EDGE_WORDS) and (EDGE_WORDS < P).all()
    for w in (0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, P // 2, P // 2 + 1, MONTY_R1, P - MONTY_R1,
              (1 << 27) - 1, 1 << 27, (1 << 27) + 1, 1 << 30):
        assert w in FE.EDGE_WORD_REASONS
    c = edge_canonical(EDGE_WORDS)
    assert (oracle.to_monty(c) == EDGE_WORDS).all()              # from_numpy(edge_canonical(w)) uploads exactly w
    assert edge_canonical([MONTY_R1])[0] == 1 and edge_canonical([P - MONTY_R1])[0] == P - 1


@pytest.mark.parametrize("log_n", [0, 1, 3, 4])
def test_ntt_forward_and_inverse_on_edge_columns(oracle, log_n):
    n = 1 << log_n
    m = FE.edge_matrix(n, 14, seed=log_n, oracle=oracle, outputs="ntt")
    fwd, inv = oracle.ntt(m), oracle.ntt(m, inverse=True)
    for j, col in enumerate(_cols(m)):
        assert fwd[:, j].tolist() == pyref.dft(col), j
        assert inv[:, j].tolist() == pyref.dft(col, inverse=True), j
    if log_n:
        # the "edge outputs" columns really do transform to edge words
        assert np.isin(oracle.to_monty(fwd[:, 6]), EDGE_WORDS).all() and np.isin(oracle.to_monty(fwd[:, 13]), EDGE_WORDS).all()


@pytest.mark.parametrize("log_n,log_blowup", [(0, 1), (2, 2), (3, 1), (3, 3), (4, 2)])
def test_coset_lde_on_edge_columns(oracle, log_n, log_blowup):
    n = 1 << log_n
    m = FE.edge_matrix(n, 8, seed=10 + log_n, oracle=oracle, outputs="lde")
    got = oracle.coset_lde(m, log_blowup, 31)
    for j, col in enumerate(_cols(m)):
        assert got[:, j].tolist() == pyref.coset_lde_column(col, log_blowup, 31), j
    assert np.isin(oracle.to_monty(got[:n, 6]), EDGE_WORDS).all()     # coset 0 of the edge-outputs column


def _edge_states(width, rng, k):
    rows = [edge_canonical(np.full(width, w, dtype=np.uint32)) for w in EDGE_WORDS]
    rows += [edge_canonical(np.where(np.arange(width) % 2 == 0, a, b)) for a, b in rng.choice(EDGE_WORDS, (k, 2))]
    rows += [edge_canonical(rng.choice(EDGE_WORDS, width)) for _ in range(k)]
    return rows


def test_poseidon2_16_and_24_on_edge_states(oracle):
    rng = np.random.default_rng(16)
    for st in _edge_states(16, rng, 8):
        assert oracle.poseidon2(st).tolist() == pyref.poseidon2([int(x) for x in st])
    for st in _edge_states(24, rng, 4):
        assert oracle.poseidon2_24(st).tolist() == pyref.poseidon2_24([int(x) for x in st])


def test_sponge_and_compress_on_edge_words(oracle):
    rng = np.random.default_rng(17)
    for n in (1, 7, 8, 9, 16, 40):
        v = edge_canonical(rng.choice(EDGE_WORDS, n))
        assert oracle.sponge_hash(v).tolist() == pyref.sponge_hash([int(x) for x in v])
    for _ in range(6):
        l, r = edge_canonical(rng.choice(EDGE_WORDS, 8)), edge_canonical(rng.choice(EDGE_WORDS, 8))
        assert oracle.compress(l, r).tolist() == pyref.compress([int(x) for x in l], [int(x) for x in r])


def _hash_rows_check():
    """hash_rows of edge-word rows (the oracle's eight-lane sponge when it has AVX-512) against pyref's sponge"""
    import oracle_lib as O
    rng = np.random.default_rng(18)
    m = np.stack([edge_canonical(rng.choice(EDGE_WORDS, 13)) for _ in range(24)] +
                 [edge_canonical(np.full(13, w, dtype=np.uint32)) for w in EDGE_WORDS[:8]])
    got = O.hash_rows([m])
    for i in range(m.shape[0]):
        assert got[i].tolist() == pyref.sponge_hash([int(x) for x in m[i]]), i
    tree = O.merkle_tree([m[:16]])
    assert tree[16].tolist() == pyref.compress(tree[0].tolist(), tree[1].tolist())


def test_hash_rows_on_edge_words_both_oracle_forms(oracle):
    _hash_rows_check()
    # the scalar form in a fresh process (the switch is read once per process)
    code = "import sys; sys.path.insert(0, %r); import test_field_edges_cpu as T, oracle_lib as O; " \
           "T._hash_rows_check(); print(int(O.lib().orc_simd_enabled()))" % HERE
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ORC_NO_SIMD="1"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-1] == "0"


def _ext_mul_w(a, b, w):
    t = [0] * 7
    for i in range(4):
        for j in range(4):
            t[i + j] = (t[i + j] + a[i] * b[j]) % P
    return [(t[i] + (w * t[i + 4] if i + 4 < 7 else 0)) % P for i in range(4)]


def test_ext_mul_and_inv_on_edge_elements(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(19)
    es = FE.edge_ext(rng, 6)
    for a in es:
        for b in es:
            out = np.zeros(4, dtype=np.uint32)
            L.orc_bb4_mul(oracle._p(a), oracle._p(b), oracle._p(out))
            assert out.tolist() == pyref.ext_mul(a.tolist(), b.tolist())
            for f in (0, 1):
                assert oracle.hal_ext_mul(a, b, f).tolist() == _ext_mul_w(a.tolist(), b.tolist(), oracle.EXT_W[f])
        out = np.zeros(4, dtype=np.uint32)
        L.orc_bb4_inv(oracle._p(a), oracle._p(out))
        assert out.tolist() == pyref.ext_inv(a.tolist())


def _fold_by_definition(vals, log_h, log_arity, beta):
    """value at beta of the interpolant through the 2^k points of each coset (domain w_h^bitrev(i), bit-reversed order)"""
    h, k = 1 << log_h, 1 << log_arity
    w = pyref.two_adic_generator(log_h)
    out = []
    for i in range(h // k):
        xs = [pow(w, pyref.bitrev(i * k + j, log_h), P) for j in range(k)]
        acc = [0, 0, 0, 0]
        for j in range(k):
            num, den = [1, 0, 0, 0], 1
            for l in range(k):
                if l != j:
                    num = pyref.ext_mul(num, [(beta[0] - xs[l]) % P] + list(beta[1:]))
                    den = den * (xs[j] - xs[l]) % P
            c = pyref.ext_mul([int(x) for x in vals[i * k + j]], [x * pow(den, P - 2, P) % P for x in num])
            acc = [(a + b) % P for a, b in zip(acc, c)]
        out.append(acc)
    return out


@pytest.mark.parametrize("log_h,log_arity", [(1, 1), (4, 1), (4, 2), (5, 3), (5, 4)])
def test_fri_fold_on_edge_words_and_challenges(oracle, log_h, log_arity):
    rng = np.random.default_rng(20 + log_h + log_arity)
    h = 1 << log_h
    vals = np.stack([FE.PATTERNS[j % len(FE.PATTERNS)](h, rng) for j in range(4)], axis=1)
    for beta in FE.edge_ext(rng, 1):
        want = _fold_by_definition(vals, log_h, log_arity, [int(x) for x in beta])
        assert oracle.fri_fold_k(vals, log_arity, beta).tolist() == want
        if log_arity == 1:
            assert oracle.fri_fold(vals, beta).tolist() == want
