"""The width-16 Poseidon2 partial rounds in their paired form (poseidon2.cuh, p2_internal_pair_dev: elements 1..15 updated once per two
rounds) on the device: word for word against the one-round-at-a-time form and the host (tools/p2mx_bench, built by build()), the leaf and
tree kernels that run it against the oracle, and a loaded parameter file whose diagonal is no power of two.  The arithmetic is exact mod P
and every output word canonical: no tolerance anywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pyref

P = 2**31 - 2**27 + 1
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.gpu
def test_paired_words_match_per_round_form_and_host():
    out = subprocess.run([os.path.join(ROOT, "tools", "p2mx_bench"), "12", "2"], capture_output=True, text=True, timeout=120)
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, out.stdout + out.stderr
    assert r["pair_mismatches"] == 0 and r["mismatches"] == 0 and r["host_mismatches"] == 0 and r["checked_words"] > 0


def _edge_rows(m):
    m[0] = 0
    m[1] = P - 1
    m[2] = 0
    m[2, 0] = P - 1                     # one-hot
    m[3, ::2] = 0                       # 0 / P - 1 alternating
    m[3, 1::2] = P - 1
    return m


# (65, 8): one full wave plus one row; (16384 + 37, 12): hash_rows_vec_kernel with a half block and a partial last wave;
# (4096, 256): the cooperative 16-lane leaf kernel
@pytest.mark.gpu
@pytest.mark.parametrize("height,width", [(65, 8), (16384 + 37, 12), (4096, 256)])
def test_hash_rows_matches_oracle(ctx, oracle, height, width):
    rng = np.random.default_rng(1000 * width + height)
    m = _edge_rows(rng.integers(0, P, size=(height, width), dtype=np.uint32))
    got = ctx.hash_rows([(ctx.from_numpy(m), width)], height).download().reshape(-1, 8)
    exp = oracle.hash_rows([m])
    assert got.max() < P and (got == exp).all()


@pytest.mark.gpu
@pytest.mark.parametrize("log_h", [12, 15])
def test_merkle_commit_matches_oracle(ctx, oracle, log_h):
    width = 16
    m = _edge_rows(oracle.fill_uniform(0x50414952 + log_h, log_h, width).copy())
    tree = ctx.merkle_commit([(ctx.from_numpy(m), width)], log_h).download().reshape(-1, 8)
    exp = oracle.merkle_tree([m])
    assert tree.shape == exp.shape and tree.max() < P and (tree == exp).all()


def _loaded_diagonals(tmp_path):
    """child process (the parameter set changes only while no context exists): a small non-power-of-two diagonal, which still takes the
    paired form, and one with a full-size entry, which takes one round at a time; hash_rows against pyref's sponge under the same file
    (the oracle has no parameter loader), then the built-in set again"""
    from zktls_amd import _lib
    from zktls_amd.device import Context
    L = _lib.load()
    L.zkhip_release_cached_contexts()
    base = json.load(open(os.path.join(HERE, "golden", "poseidon2_params.json")))
    rng = np.random.default_rng(77)
    shapes = [(65, 8), (16384 + 37, 12)]
    mats = [_edge_rows(rng.integers(0, P, size=s, dtype=np.uint32)) for s in shapes]
    rows = [0, 1, 2, 3, 63, 64, 16384, 16384 + 36]

    def run():
        c = Context(0)
        out = [c.hash_rows([(c.from_numpy(m), m.shape[1])], m.shape[0]).download().reshape(-1, 8) for m in mats]
        c.close()
        L.zkhip_release_cached_contexts()
        return out

    builtin = run()
    for m, got in zip(mats, builtin):
        for r in (x for x in rows if x < m.shape[0]):
            assert got[r].tolist() == pyref.sponge_hash([int(x) for x in m[r]])
    small = [P - 2, 1, 3, 5, 7, 9, 11, 13, 17, 19, 23, 29, 31, 37, 41, 32768]
    full = list(base["internal_diag"])
    full[7] = 0x3C4F1E2B % P
    old = (pyref.PARAMS, pyref.MI)
    try:
        for name, diag in (("small", small), ("full", full)):
            d = dict(base, name="test-diag-" + name, internal_diag=diag)
            path = os.path.join(str(tmp_path), name + ".json")
            json.dump(d, open(path, "w"))
            assert L.zkhip_load_poseidon2_params(path.encode()) == 0, L.zkhip_last_error()
            pyref.PARAMS = d
            pyref.MI = [[(1 + (diag[i] if i == j else 0)) % P for j in range(16)] for i in range(16)]
            for m, got, was in zip(mats, run(), builtin):
                assert got.max() < P and (got != was).any()
                for r in (x for x in rows if x < m.shape[0]):
                    assert got[r].tolist() == pyref.sponge_hash([int(x) for x in m[r]]), (name, m.shape, r)
    finally:
        pyref.PARAMS, pyref.MI = old
        assert L.zkhip_reset_poseidon2_params() == 0
    for got, was in zip(run(), builtin):
        assert (got == was).all()


@pytest.mark.gpu
def test_loaded_diagonals_follow_the_file(tmp_path):
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_p2_pair as t; t._loaded_diagonals(%r); print('child ok')"
            % (ROOT, HERE, str(tmp_path)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
