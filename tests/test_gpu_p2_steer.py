"""Every device form of the Poseidon2 permutation on states STEERED to edge words inside the rounds (p2_steer: the catalogue the CPU models
are checked on in test_p2_steer_cpu.py): the shipped library's permutation with all 16 words chosen, the other forms through the states mode
of tools/p2mx_bench (built by build()), and the shipped sponge kernels, whose first block leaves the rate words free.  Exact arithmetic:
every word equal to pyref's / the oracle's and every raw device word canonical, no tolerance anywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import p2_steer as S
import pyref
from field_edges import assert_canonical, assert_canonical_words, edge_canonical

P = pyref.P
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOOL = os.path.join(ROOT, "tools", "p2mx_bench")
SMALL_DIAG = [P - 2, 1, 3, 5, 7, 9, 11, 13, 17, 19, 23, 29, 31, 37, 41, 32768]
FORMS16 = ["vec_pair", "mx_pair", "mx5_pair", "mx6_pair", "vec_one", "mx_one", "mx5_one", "mx6_one", "coop"]


def _from_monty(words):
    return (np.asarray(words, dtype=np.uint64) * pow(2**32, -1, P) % P).astype(np.uint32)


@pytest.fixture(scope="module")
def cat16():
    states = np.array([s for _, _, s in S.catalogue(16)], dtype=np.uint32)
    return states, np.array([pyref.poseidon2([int(x) for x in s]) for s in states], dtype=np.uint32)


def _wave_layout(states):
    """the file the tool reads: the states padded to whole waves, then the same waves with their halves swapped -- the matrix-core form is
    wave-cooperative and its constants differ per lane half, so every state sits once in lanes 0..31 and once in lanes 32..63 -- then a partial
    wave.  Returns (file states, index of the catalogue state at each file position)."""
    n = len(states)
    idx = np.concatenate([np.arange(n), np.zeros((-n) % 64, dtype=np.int64)])
    swapped = idx.reshape(-1, 2, 32)[:, ::-1].reshape(-1)
    idx = np.concatenate([idx, swapped, np.arange(37) % n])
    assert len(idx) % 64 == 37
    return states[idx], idx


def _run_tool(tmp_path, states, extra=()):
    src, dst = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    np.ascontiguousarray(states, dtype=np.uint32).tofile(src)
    out = subprocess.run([TOOL, "states", *extra, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["states"] == len(states)
    words = np.fromfile(dst, dtype=np.uint32).reshape(len(r["blocks"]), len(states), states.shape[1])
    return r["blocks"], words


@pytest.fixture(scope="module")
def tool16(cat16, tmp_path_factory):
    states, exp = cat16
    layout, idx = _wave_layout(states)
    blocks, words = _run_tool(tmp_path_factory.mktemp("p2steer16"), layout)
    assert blocks == FORMS16
    return dict(zip(blocks, words)), exp[idx]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS16)
def test_steered_states_every_form(tool16, form):
    words, exp = tool16
    assert_canonical_words(words[form])
    got = _from_monty(words[form])
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, "%s: %d states differ, first at file positions %s" % (form, bad.size, bad[:8].tolist())


@pytest.mark.gpu
def test_steered_states_width24(tmp_path):
    states = np.array([s for _, _, s in S.catalogue(24)], dtype=np.uint32)
    states = np.concatenate([states, states[:(37 - len(states)) % 64]])              # a partial last wave
    assert len(states) % 64 == 37
    exp = np.array([pyref.poseidon2_24([int(x) for x in s]) for s in states], dtype=np.uint32)
    blocks, words = _run_tool(tmp_path, states, ["--w24"])
    assert blocks == ["p24"]
    assert_canonical_words(words[0])
    assert (_from_monty(words[0]) == exp).all()


@pytest.mark.gpu
def test_library_permute_on_steered_states(ctx, cat16):
    # the shipped permute_states_kernel -> p2_permute_dev, paired partial rounds; the state count is no multiple of its 256-lane block
    states, exp = cat16
    assert len(states) % 256
    buf = ctx.from_numpy(states)
    ctx.poseidon2_permute(buf)
    assert_canonical(buf)
    assert (buf.download().reshape(-1, 16) == exp).all()


def _loaded_small_diagonal(tmp_path):
    """child process (the parameter set changes only while no context exists): the small diagonal loaded from a file, which takes the paired
    form, on the catalogue steered FOR THAT diagonal; then the built-in set again"""
    from zktls_amd import _lib
    from zktls_amd.device import Context
    L = _lib.load()
    L.zkhip_release_cached_contexts()
    base = json.load(open(os.path.join(HERE, "golden", "poseidon2_params.json")))

    def run(states):
        c = Context(0)
        buf = c.from_numpy(states)
        c.poseidon2_permute(buf)
        assert_canonical(buf)
        out = buf.download().reshape(-1, 16)
        c.close()
        L.zkhip_release_cached_contexts()
        return out

    states = np.array([s for _, _, s in S.catalogue(16, SMALL_DIAG)], dtype=np.uint32)
    builtin_states = states[::9]                                        # any states do for the built-in words before and after
    builtin = run(builtin_states)
    assert builtin[:8].tolist() == [pyref.poseidon2([int(x) for x in s]) for s in builtin_states[:8]]
    path = os.path.join(str(tmp_path), "small.json")
    json.dump(dict(base, name="test-diag-small-steered", internal_diag=SMALL_DIAG), open(path, "w"))
    assert len(states) % 256
    exp = np.array([S.permute(16, [int(x) for x in s], SMALL_DIAG) for s in states], dtype=np.uint32)
    assert L.zkhip_load_poseidon2_params(path.encode()) == 0, L.zkhip_last_error()
    try:
        got = run(states)
    finally:
        assert L.zkhip_reset_poseidon2_params() == 0
    assert (got == exp).all(), np.flatnonzero((got != exp).any(axis=1))[:8].tolist()
    assert (run(builtin_states) == builtin).all()


@pytest.mark.gpu
def test_library_permute_small_diagonal_steered(tmp_path):
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_p2_steer as t; t._loaded_small_diagonal(%r); print('child ok')"
            % (ROOT, HERE, str(tmp_path)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


# ---- the shipped sponge kernels.  The first block of a leaf has capacity 0, so its rate words (8 at width 16, 16 at width 24) are free: k of
# them reach the first layer's digit words directly, or k chosen S-box inputs of full round 0 through a k x k solve against M_E's columns.
def _solve(width, rows, cols, targets):
    """canonical x (len(cols)) with (M_E x')_rows + rc_0 = targets as Montgomery words, x' = x in `cols`, 0 elsewhere"""
    me, rc0 = S.ME[width], S.params(width)[0][0]
    sub = [[me[i][j] for j in cols] for i in rows]
    rhs = [(t * S.RINV - rc0[i]) % P for t, i in zip(targets, rows)]
    return S.matvec(S.inv_matrix(sub), rhs)


def _rank(m):
    m, rank = [list(r) for r in m], 0
    for c in range(len(m[0])):
        piv = next((r for r in range(rank, len(m)) if m[r][c] % P), None)
        if piv is None:
            continue
        m[rank], m[piv] = m[piv], m[rank]
        inv = pow(m[rank][c], P - 2, P)
        for r in range(rank + 1, len(m)):
            f = m[r][c] * inv % P
            m[r] = [(x - f * y) % P for x, y in zip(m[r], m[rank])]
        rank += 1
    return rank


def _row_sets(width, k):
    """sets of k rows of M_E, independent against the first k columns (rows 8..15 against columns 0..7 are not: rank 4), each grown
    from another start so that between them every row is chosen"""
    sets = []
    for start in sorted(set(range(0, width, width // 4)) | {width - 4}):
        rows = []
        for nxt in range(start, start + width):
            cand = rows + [nxt % width]
            if len(rows) < k and _rank([S.ME[width][i][:k] for i in cand]) == len(cand):
                rows = cand
        assert len(rows) == k
        sets.append(rows)
    return sets


def steered_rows(width, k):
    """canonical rows of k free words for a width-`width` first block: digit words at the first layer (width 16), edge words as the
    first layer's input, and edge words as k S-box inputs of full round 0"""
    ws = S.edge_words()
    rows = []
    if width == 16:
        u0 = [x * S.R % P for x in S.matvec(S.ME_INV[16], S.params(16)[0][0])]
        for _, words in S.digit_patterns():
            lazy = [x + P if x < P // 2 else x for x in words]
            rows.append([(a - b) % P * S.RINV % P for a, b in zip(lazy[:k], u0)])
    for n, w in enumerate(ws):
        rows.append([w * S.RINV % P] * k)
        for rs in _row_sets(width, k):
            rows.append(_solve(width, rs, list(range(k)), [w] * k))
            rows.append(_solve(width, rs, list(range(k)), [w if i % 2 == 0 else (P - w) % P for i in range(k)]))
    return np.array(rows, dtype=np.uint32)


def _sponge_matrix(height, width, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, P, size=(height, width), dtype=np.uint32)
    k = min(width, 8)
    st = steered_rows(16, k)
    assert 2 * len(st) + 32 <= height
    m[:len(st), :k] = st
    m[32 + len(st):32 + 2 * len(st), :k] = st                          # the other lane half of a wave
    m[-len(st):, :k] = st[::-1]                                         # through the partial last wave
    if width > k:
        m[:len(st):3, k:] = edge_canonical(rng.choice(np.array(S.edge_words(), dtype=np.uint32), (len(st[::3]), width - k)))
    return m


# (16384 + 37, 8 / 12): hash_rows_vec_kernel, a full block, a half block, a partial last wave; (1024, 8): hash_rows16_kernel;
# (2^15, [8, 12]): hash_rows_mvec_kernel; (2^15, 5): hash_rows_generic_kernel -- the shapes test_gpu_field_edges.py lists
@pytest.mark.gpu
@pytest.mark.parametrize("height,widths", [(16384 + 37, [8]), (16384 + 37, [12]), (1024, [8]), (1 << 15, [8, 12]), (1 << 15, [5])])
def test_hash_rows_on_steered_first_blocks(ctx, oracle, height, widths):
    mats = [_sponge_matrix(height, w, seed=height % 89 + w + 7 * j) for j, w in enumerate(widths)]
    got = ctx.hash_rows([(ctx.from_numpy(m), m.shape[1]) for m in mats], height)
    assert_canonical(got)
    assert (got.download().reshape(-1, 8) == oracle.hash_rows(mats)).all()


def test_steered_rows_reach_their_targets():
    # CPU: the two constructions, checked against the forward walk (no GPU)
    ws = S.edge_words()
    for width, k in ((16, 8), (16, 5), (24, 16)):
        sets = _row_sets(width, k)
        assert sorted({i for rs in sets for i in rs}) == list(range(width))
        for rs in sets:
            targets = [ws[(i + 3) % len(ws)] for i in range(k)]
            x = _solve(width, rs, list(range(k)), targets)
            got = S.forward_probe(width, ("F", 0), x + [0] * (width - k))
            assert [got[i] for i in rs] == targets
    rows = steered_rows(16, 8)
    u0 = [x * S.R % P for x in S.matvec(S.ME_INV[16], S.params(16)[0][0])]
    lazy = [(int(rows[0][i]) * S.R % P) + u0[i] for i in range(8)]      # the first digit pattern: -128 in planes 0..2, all eight lanes
    assert all(x == P - 128 - 128 * 256 - 128 * 65536 for x in lazy)


@pytest.mark.gpu
def test_merkle_commit_p24_colmajor_on_steered_leaves(ctx, oracle):
    # 16 columns x 2^5 rows: one absorbed block per leaf, 16 of the 24 words free
    st = steered_rows(24, 16)
    idx = np.arange(32) * len(st) // 32
    cm = np.ascontiguousarray(st[idx].T)
    tree = ctx.merkle_commit_p24_colmajor(ctx.from_numpy(cm), 16, 5)
    assert_canonical(tree)
    assert (tree.download().reshape(-1, 8) == oracle.merkle_tree_p24_colmajor(cm)).all()
