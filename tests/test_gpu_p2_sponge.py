"""The leaf kernel's sponge forms (hash.hip hash_rows_sponge_body: ABSORB / ABSORB_RATE / SQUEEZE, poseidon2.cuh p2_permute_mx_form) on the GPU,
word for word: zkhip_hash_rows / zkhip_merkle_commit against the oracle's digests, and the stand-alone sponge kernels of tools/p2mx_bench (built
by build()) against the closed form, the oracle and the CPU model (p2_sponge_model), steered second-block capacity words included."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

P = 2**31 - 2**27 + 1
RINV = pow(2**32 % P, -1, P)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "p2mx_bench")
# a lone lane, a full wave, one lane into the next wave, a partial last workgroup
HEIGHTS = (1, 63, 64, 65, 129, 300)
# rows past this count leave the 16-lanes-per-row kernels for hash_rows_vec_kernel (COOP_MAX_NODES)
COOP_MAX = 16384
# SQUEEZE only; a half block alone after one block; two blocks; two blocks and a half; three; the headline's 32; 32 and a half
WIDTHS = (8, 12, 16, 20, 24, 256, 260)


def _matrix(height, width, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, P, size=(height, width), dtype=np.uint32)
    m[0] = 0
    m[1] = P - 1
    m[2] = (P - 1) * RINV % P                                           # the device's words are x 2^32: these are all P - 1 there
    m[3] = 12345
    m[height - 1] = P - 1
    return m


def _hash_rows(ctx, buf, pitch, width, height):
    out = ctx.alloc(8 * height)
    ptrs, lds, ws = (C.c_void_p * 1)(buf.ptr), (C.c_size_t * 1)(pitch), (C.c_uint32 * 1)(width)
    from zktls_amd.device import check
    check(ctx.lib.zkhip_hash_rows(ctx.handle, ptrs, lds, ws, 1, height, C.c_void_p(out.ptr)))
    return out.download().reshape(-1, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_hash_rows_matches_oracle(ctx, oracle, width):
    """the heights as they are (the 16-lanes-per-row kernel takes them) and past COOP_MAX_NODES, where hash_rows_vec_kernel runs the sponge forms;
    rows of all-zero, all-(P - 1) and uniform words; a row pitch larger than the width"""
    top = COOP_MAX + max(HEIGHTS)
    pitch = width + 12
    m = _matrix(top, width, 0x53504F4E + width)
    exp = oracle.hash_rows([m])
    padded = np.full((top, pitch), 7, dtype=np.uint32)
    padded[:, :width] = m
    tight, wide = ctx.from_numpy(m), ctx.from_numpy(padded)
    for h in HEIGHTS:
        for height in (h, COOP_MAX + h):
            assert (_hash_rows(ctx, tight, width, width, height) == exp[:height]).all(), (width, height)
        assert (_hash_rows(ctx, wide, pitch, width, COOP_MAX + h) == exp[:COOP_MAX + h]).all(), (width, h, "pitch")
    tight.free()
    wide.free()


@pytest.mark.gpu
def test_commitment_root_2pow10_x256(ctx, oracle):
    log_h, width = 10, 256
    m = oracle.fill_uniform(0x53504F4E, log_h, width)
    tree = ctx.merkle_commit([(ctx.from_numpy(m), width)], log_h).download().reshape(-1, 8)
    exp = oracle.merkle_tree([m])
    assert (tree[: 1 << log_h] == exp[: 1 << log_h]).all()
    assert (tree[-1] == exp[-1]).all()


def _sponge_rows(tmp_path, name, cap, rows):
    """tools/p2mx_bench sponge-rows: (closed, forms) digests as canonical field elements"""
    n, width = rows.shape
    src, dst = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    np.concatenate([cap, rows], axis=1).astype("<u4").tofile(src)
    out = subprocess.run([TOOL, "sponge-rows", str(width), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads(out.stdout.strip().splitlines()[-1])["blocks"] == ["closed", "forms"]
    words = np.fromfile(dst, dtype="<u4").astype(np.uint64).reshape(2, n, 8)
    return (words * RINV % P).astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [8, 12, 256])
def test_sponge_kernels_tail(tmp_path, oracle, width):
    """the stand-alone sponge kernels at the heights themselves: lanes past the last row hash it again and store nothing"""
    m = _matrix(max(HEIGHTS), width, 0x7A11 + width)
    exp = oracle.hash_rows([m])
    for h in HEIGHTS:
        closed, forms = _sponge_rows(tmp_path, "tail%d" % h, np.zeros((h, 8), dtype=np.uint32), m[:h])
        assert (forms == exp[:h]).all() and (closed == exp[:h]).all(), (width, h)


@pytest.mark.gpu
def test_steered_second_block(tmp_path):
    """rows whose second block's first layer meets the digit words -128 / 127 / 0 / -1 in all eight capacity lanes (p2_sponge_model.steered_rows),
    of two and of three blocks: both device forms against the CPU model of the forms"""
    import p2_sponge_model as sm
    for n_blocks in (2, 3):
        rows = sm.steered_rows(n_blocks)
        cap = np.array([c for _, c, _ in rows], dtype=np.uint32)
        mat = np.array([r for _, _, r in rows], dtype=np.uint32)
        exp = np.array([sm.sponge_forms(r, c) for _, c, r in rows], dtype=np.uint32)
        closed, forms = _sponge_rows(tmp_path, "steer%d" % n_blocks, cap, mat)
        assert (forms == exp).all() and (closed == exp).all()


@pytest.mark.gpu
def test_sponge_mode_forms_agree():
    """the A/B tool's sponge mode: 2^16 rows of 256 words through both forms, every digest word equal, the first rows against the host form"""
    out = subprocess.run([TOOL, "sponge", "16", "256", "1"], capture_output=True, text=True, timeout=120)
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, out.stdout + out.stderr
    assert r["mismatches"] == 0 and r["host_mismatches"] == 0 and r["checked_words"] == 8 << 16
    assert r["forms_regs"] <= 96                                         # five waves per SIMD
