"""The width-16 Poseidon2 permutation with its full rounds' external layer on the int8 matrix cores (poseidon2.cuh, p2_permute_mx_dev):
word for word against the all-VALU device form on random and edge states (tools/p2mx_bench, built by build()), and the leaf kernel that
uses it (hash_rows_vec_kernel: one matrix, width a multiple of 4, more rows than the cooperative kernels take) against the oracle."""
import json
import os
import subprocess

import numpy as np
import pytest

P = 2**31 - 2**27 + 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_mx_permutation_matches_valu_form():
    out = subprocess.run([os.path.join(ROOT, "tools", "p2mx_bench"), "16", "2"], capture_output=True, text=True, timeout=300)
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, out.stdout + out.stderr
    assert r["mismatches"] == 0 and r["host_mismatches"] == 0 and r["checked_words"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("height,width", [(16384 + 37, 256), (20000, 12), (65536, 8), (16385, 4)])
def test_hash_rows_vec_matches_oracle(ctx, oracle, height, width):
    # heights past the cooperative kernels' limit (16384 rows) take hash_rows_vec_kernel; the odd heights leave a partial last wave
    rng = np.random.default_rng(height + width)
    m = rng.integers(0, P, size=(height, width), dtype=np.uint32)
    m[:64] = P - 1
    m[64:128] = 0
    got = ctx.hash_rows([(ctx.from_numpy(m), width)], height).download().reshape(-1, 8)
    assert (got == oracle.hash_rows([m])).all()


@pytest.mark.gpu
def test_merkle_commit_2pow21_x256_matches_oracle(ctx, oracle):
    # the headline shard's leaf shape: 2^21 rows of 256 words, every leaf digest and the root
    log_h, width = 21, 256
    m = oracle.fill_uniform(0x4D58, log_h, width)
    d = ctx.from_numpy(m)
    leaves = ctx.hash_rows([(d, width)], 1 << log_h).download().reshape(-1, 8)
    tree = ctx.merkle_commit([(d, width)], log_h).download().reshape(-1, 8)
    exp = oracle.merkle_tree([m])
    assert (leaves == exp[: 1 << log_h]).all()
    assert (tree[-1] == exp[-1]).all()
