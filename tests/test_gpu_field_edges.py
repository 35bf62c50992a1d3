"""The HIP kernels on edge Montgomery WORDS (tests/field_edges.py), against the oracle, with every output word required canonical.

The other parity tests upload canonical values through from_numpy, so their "edge" inputs reach the kernels as ordinary words, and
they read results through download(), which reduces mod P and so cannot see a kernel that writes P for 0 or P + 5 for 5.  Here each
case builds its inputs from edge words (constant, alternating, impulse at the first / last row, random edge draws, columns whose
transform OUTPUTS are edge words, a few uniform columns), compares download() with the oracle on the same canonical values, and
calls assert_canonical on the raw words of every output buffer.  test_field_edges_cpu.py pins the oracle against tests/pyref.py
on the same kind of input.

Which kernel each shape reaches (csrc/context.cpp op_dft / op_coset_lde / op_merkle_commit*, and the launchers in ntt.hip,
ntt_small.hip, ntt_fused.hip, hash.hip, stark.hip, hal.hip):

  kernel                                   shape in this file
  ---------------------------------------  ------------------------------------------------------------------------------
  small_eval (by definition, < 32 rows)    dft 2^0 .. 2^4; coset_lde 2^0, 2^3
  ntt_pass_kernel, one pass (2^5..2^10)    dft 2^5 .. 2^10; coset_lde 2^5, 2^8, 2^10
  ntt_pass_kernel, two passes (64..512-    dft 2^11, 2^12, 2^13, 2^14, 2^16, 2^18 x 8 (tile heights 64 .. 512);
    row tiles, 2^11 .. 2^18)               coset_lde 2^11 x 8, 2^12 x 40 (32 + 8 column split), 2^14 x 16, 2^16 x 8
  ntt_pass1024x2_kernel                    dft 2^20 x 32 (forward, bitrev_out, inverse); coset_lde 2^20 x 32 with fusion off
  ntt_combine_kernel (radix-R, > 2^20)     dft 2^21 x 4 and 2^22 x 4 (forward, bitrev_out, inverse)
  lde_small_kernel<1..3>                   coset_lde 2^11 / 2^12 / 2^13 rows x widths 128, 130, 640, blowups 1, 2, 3 (a Latin
                                           square of the three), and 2^12 x 130 with out_ld 136; commit 2^11 x 128
  lde_fused_kernel                         coset_lde 2^20 x 32 and 2^20 x 64, blowups 1 and 2
  (every LDE above)                        again with set_lde_fusion(False) (the pass kernels), required equal
  ntt_colpass_kernel                       batch_interpolate_colmajor / batch_expand_colmajor, 2 x 2^20
  transposing colmajor adapter             the same at 5 x 2^8
  permute_states_kernel                    poseidon2_permute on edge-word states uploaded with from_raw
  hash_rows16_kernel                       hash_rows 1024 x 40 (height <= 16384)
  hash_rows_vec_kernel                     hash_rows 2^15 x 16 (one matrix, width % 4 == 0)
  hash_rows_mvec_kernel                    hash_rows 2^15 x [8, 12]
  hash_rows_generic_kernel                 hash_rows 2^15 x 5
  compress_top16_kernel                    merkle_commit 2^9 (leaves by hash_rows16)
  hash_sub16_kernel + top                  merkle_commit 2^12
  compress_level_kernel, compress_sub16    merkle_commit 2^15 (level 2^15 -> 2^14, then subtrees)
  compress_inject_mvec_kernel              merkle_commit_mixed 2^16 x 8 + 2^15 x 4 (+ 2^9 x 5)
  compress_level16 + hash_rows + inject    merkle_commit_mixed, the 2^9 x 5 injection
  hash_cols24, compress24_level / _top     merkle_commit_p24_colmajor 24 x 2^12 and 7 x 2^5
  hash_rows24 (row-major w24 leaves)       commit(..., hw=24) 2^10 x 16, blowup 2
  quotient_kernel                          quotient_values 2^10 x 16 and 2^12 x 256, edge alphas
  quotient_air_* kernels                   test_gpu_air_forms.py (every live form, with its own kernel / shape table); here the synthetic
                                           program at 2^8 x 8 (the interpreter) and 2^12 x 64 (quotient_air_chain_kernel<64,4>)
  inv_denominators, open_partial*, final   open_at 2^10 x 20 and 2^12 x 64, two edge points
  fri_fold_kernel                          fri_fold 2^1, 2^10, 2^17, edge betas
  fri_fold_k (arities 2 .. 16)             fri_fold_k 2^12 x arities 2, 4, 8, 16 and 2^16 x 16
  rowdot_regs_kernel<1..4>, rowdot_kernel  test_gpu_reduced_edges.py (reduced_opening; its own table of which case takes which form, checked
                                           against the form the library reports)
  reduced_combine_kernel                   test_gpu_reduced_edges.py: every reduced_opening case (p_width 0 / 8 / 260, q_width 0 / 8 / 16,
                                           accumulate 0 / 1, dense and [pre | main] rows)
  fri_fold_dev_kernel, ext_add_kernel      test_gpu_reduced_edges.py: fri_fold_k_dev 2^1, 2^4, 2^9, 2^12 x arities 2 .. 16, edge betas in
                                           device memory, with and without the added vector
  grind_kernel                             test_gpu_reduced_edges.py: grind, slots 0 .. 7, bits 0 .. 10, windows around the witness and up to P
  hal_add / hal_sum_ext                    eltwise_add, eltwise_sum_ext
  hal_zk_shift(_scalar)                    zk_shift with shift P - 1 and edge shifts
  hal_mix_* (plan, sorted, register)       mix_poly_coeffs on the shapes of test_gpu_hal.py that pick each form
  hal_batch_evaluate_any                   batch_evaluate_any, edge points
  hal_scan_*                               prefix_products_ext, both ext_field values, n across the scan block boundaries

A reviewer can confirm one row with `rocprofv3 --kernel-trace --stats -- python -m pytest -m gpu <file>::<test>[<id>]`.
"""
import ctypes as C

import numpy as np
import pytest

import field_edges as FE
from field_edges import EDGE_WORDS, MONTY_R1, P, assert_canonical, assert_canonical_words, bitrev_perm, edge_canonical, edge_matrix, edge_ext
from zktls_amd._lib import check, from_monty, to_monty, u32p
from zktls_amd.device import air_synthetic

pytestmark = pytest.mark.gpu


def _mat(buf, width, ld=None):
    ld = ld or width
    return buf.download().reshape(-1, ld)[:, :width]


# ------------------------------------------------------------------ forward / inverse DFT
@pytest.mark.parametrize("log_n,width", [(0, 8), (1, 8), (2, 8), (3, 8), (4, 8), (5, 8), (6, 7), (8, 8), (10, 8),
                                         (11, 8), (12, 8), (13, 8), (14, 8), (16, 8), (18, 8), (20, 32), (21, 4), (22, 4)])
def test_dft_on_edge_words(ctx, oracle, log_n, width):
    m = edge_matrix(1 << log_n, width, seed=log_n, oracle=oracle, outputs="ntt")
    src = ctx.from_numpy(m)
    exp = oracle.ntt(m)
    nat = ctx.dft(src, log_n, width)
    assert (_mat(nat, width) == exp).all()
    assert_canonical(nat)
    br = ctx.dft(src, log_n, width, bitrev_out=True)
    assert (_mat(br, width)[bitrev_perm(log_n)] == exp).all()
    assert_canonical(br)
    inv = ctx.dft(src, log_n, width, inverse=True)
    assert (_mat(inv, width) == oracle.ntt(m, inverse=True)).all()
    assert_canonical(inv)
    assert (src.download_monty() == to_monty(m).ravel()).all()     # input preserved, word for word


# ------------------------------------------------------------------ coset LDE (every case with fusion on and off)
def _lde_both(ctx, src, log_n, width, log_blowup, out_ld=None):
    ld = out_ld or width
    outs = []
    try:
        for fused in (True, False):
            ctx.set_lde_fusion(fused)
            out = ctx.alloc(ld << (log_n + log_blowup))
            out.upload_monty(np.zeros(out.nwords, dtype=np.uint32))
            ctx.coset_lde(src, log_n, width, log_blowup, out=out, out_ld=ld)
            words = out.download_monty().reshape(-1, ld)
            assert_canonical_words(words[:, :width])
            assert not words[:, width:].any()                         # the padding columns untouched
            outs.append(words[:, :width])
            out.free()
    finally:
        ctx.set_lde_fusion(True)
    assert (outs[0] == outs[1]).all()
    return from_monty(outs[0])


@pytest.mark.parametrize("log_n,width,log_blowup,out_ld", [
    (0, 3, 1, None), (3, 8, 2, None), (5, 7, 1, None), (8, 8, 3, None), (10, 8, 1, None),          # one-pass / by definition
    (11, 8, 1, None), (12, 40, 2, None), (14, 16, 3, None), (16, 8, 1, None),                      # two-pass tiles, 32 + 8 split
    (11, 128, 1, None), (11, 130, 2, None), (11, 640, 3, None),                                    # lde_small_kernel
    (12, 128, 3, None), (12, 130, 1, None), (12, 640, 2, None),
    (13, 128, 2, None), (13, 130, 3, None), (13, 640, 1, None),
    (12, 130, 2, 136),                                                                             # lde_small_kernel, padded out_ld
])
def test_coset_lde_on_edge_words(ctx, oracle, log_n, width, log_blowup, out_ld):
    m = edge_matrix(1 << log_n, width, seed=3 * log_n + width, oracle=oracle, outputs="lde")
    got = _lde_both(ctx, ctx.from_numpy(m), log_n, width, log_blowup, out_ld)
    assert (got == oracle.coset_lde(m, log_blowup, 31)).all()


@pytest.mark.parametrize("width,log_blowup", [(32, 1), (32, 2), (64, 1), (64, 2)])
def test_fused_lde_2pow20_on_edge_words(ctx, oracle, width, log_blowup):
    """lde_fused_kernel at the headline height; the oracle checks the 32-column cases (64 columns: fused against unfused)"""
    log_n = 20
    m = edge_matrix(1 << log_n, width, seed=width + log_blowup, oracle=oracle, outputs="lde")
    got = _lde_both(ctx, ctx.from_numpy(m), log_n, width, log_blowup)
    if width == 32:
        assert (got == oracle.coset_lde(m, log_blowup, 31)).all()


@pytest.mark.parametrize("count,log_size,log_blowup", [(5, 8, 2), (2, 20, 1)])
def test_colmajor_interpolate_and_expand_on_edge_words(ctx, oracle, count, log_size, log_blowup):
    n = 1 << log_size
    evals = edge_matrix(n, count, seed=count, oracle=None)                 # row-major view [n][count]
    coeffs = oracle.ntt(evals, inverse=True)
    d_c = ctx.batch_interpolate_colmajor(ctx.from_numpy(np.ascontiguousarray(evals[bitrev_perm(log_size)].T)), count, log_size)
    assert (d_c.download().reshape(count, n) == coeffs.T).all()
    assert_canonical(d_c)
    # coefficients whose expansion's first coset is made of edge words
    target = edge_matrix(n, count, seed=count + 1, oracle=None)
    cin = oracle.ntt(FE.lde_preimage(oracle, target), inverse=True)
    d_e = ctx.batch_expand_colmajor(ctx.from_numpy(np.ascontiguousarray(cin.T)), count, log_size, log_blowup, 31)
    exp = oracle.coset_lde(oracle.ntt(cin), log_blowup, 31)
    assert (d_e.download().reshape(count, n << log_blowup) == exp.T).all()
    assert_canonical(d_e)


# ------------------------------------------------------------------ Poseidon2 and the Merkle trees
def _edge_word_states(width, rng, k):
    rows = [np.full(width, w, dtype=np.uint32) for w in EDGE_WORDS]
    rows += [np.where(np.arange(width) % 2 == 0, a, b).astype(np.uint32) for a in EDGE_WORDS for b in EDGE_WORDS]
    rows += [rng.choice(EDGE_WORDS, width).astype(np.uint32) for _ in range(k)]
    return np.stack(rows)


def test_poseidon2_permute_on_edge_words(ctx, oracle):
    words = _edge_word_states(16, np.random.default_rng(41), 256)
    buf = ctx.from_raw(words)
    ctx.poseidon2_permute(buf)
    assert_canonical(buf)
    got = buf.download().reshape(-1, 16)
    st = edge_canonical(words)
    for i in range(st.shape[0]):
        assert (got[i] == oracle.poseidon2(st[i])).all(), words[i].tolist()


@pytest.mark.parametrize("height,widths", [(1024, [40]), (1 << 15, [16]), (1 << 15, [8, 12]), (1 << 15, [5])])
def test_hash_rows_on_edge_words(ctx, oracle, height, widths):
    mats = [edge_matrix(height, w, seed=height % 97 + w) for w in widths]
    got = ctx.hash_rows([(ctx.from_numpy(m), m.shape[1]) for m in mats], height)
    assert (got.download().reshape(-1, 8) == oracle.hash_rows(mats)).all()
    assert_canonical(got)


@pytest.mark.parametrize("log_h,width", [(9, 8), (12, 16), (15, 8)])
def test_merkle_commit_on_edge_words(ctx, oracle, log_h, width):
    m = edge_matrix(1 << log_h, width, seed=log_h)
    tree = ctx.merkle_commit([(ctx.from_numpy(m), width)], log_h)
    assert (tree.download().reshape(-1, 8) == oracle.merkle_tree([m])).all()
    assert_canonical(tree)


def test_merkle_commit_mixed_on_edge_words(ctx, oracle):
    shapes = [(16, 8), (15, 4), (9, 5)]
    mats = [edge_matrix(1 << lh, w, seed=lh + w) for lh, w in shapes]
    tree = ctx.merkle_commit_mixed([(ctx.from_numpy(m), m.shape[1], lh) for m, (lh, _) in zip(mats, shapes)])
    assert (tree.download().reshape(-1, 8) == oracle.merkle_tree_mixed(mats)).all()
    assert_canonical(tree)


@pytest.mark.parametrize("cols,log_rows", [(24, 12), (7, 5)])
def test_merkle_commit_p24_colmajor_on_edge_words(ctx, oracle, cols, log_rows):
    cm = np.ascontiguousarray(edge_matrix(1 << log_rows, cols, seed=cols).T)
    tree = ctx.merkle_commit_p24_colmajor(ctx.from_numpy(cm), cols, log_rows)
    assert (tree.download().reshape(-1, 8) == oracle.merkle_tree_p24_colmajor(cm)).all()
    assert_canonical(tree)


@pytest.mark.parametrize("log_n,width,log_blowup,hw", [(11, 128, 1, 16), (10, 16, 2, 24), (9, 8, 1, 24)])
def test_commit_on_edge_words(ctx, oracle, log_n, width, log_blowup, hw):
    m = edge_matrix(1 << log_n, width, seed=log_n + hw, oracle=oracle, outputs="lde")
    lde, tree, root = ctx.commit(ctx.from_numpy(m), log_n, width, log_blowup, hw)
    exp = oracle.coset_lde(m, log_blowup, 31)
    assert (lde.download().reshape(-1, width) == exp).all()
    otree = oracle.merkle_tree_hw(exp, hw)
    assert (tree.download().reshape(-1, 8) == otree).all()
    assert root.tolist() == otree[-1].tolist()
    assert_canonical(lde)
    assert_canonical(tree)


# ------------------------------------------------------------------ STARK stages
@pytest.mark.parametrize("log_n,width", [(10, 16), (12, 256)])
def test_quotient_values_on_edge_words(ctx, oracle, log_n, width):
    lde = edge_matrix(2 << log_n, width, seed=log_n)
    d = ctx.from_numpy(lde)
    for alpha in edge_ext(np.random.default_rng(log_n), 2):
        got = ctx.quotient_values(d, log_n, width, alpha)
        assert (got.download().reshape(-1, 4) == oracle.quotient_values(lde, log_n, alpha)).all(), alpha.tolist()
        assert_canonical(got)


@pytest.mark.parametrize("log_n,width", [(8, 8), (12, 64)])
def test_quotient_values_air_on_edge_words(ctx, oracle, log_n, width):
    prog = air_synthetic(width, 3)
    lde = edge_matrix(2 << log_n, width, seed=log_n + 1)
    d = ctx.from_numpy(lde)
    pub = edge_canonical([P - 1, 0, MONTY_R1]).tolist()
    for alpha in edge_ext(np.random.default_rng(log_n + 1), 1):
        got = ctx.quotient_values_air(prog, d, log_n, width, pub, alpha)
        assert (got.download().reshape(-1, 4) == oracle.quotient_values_air(prog, lde, log_n, pub, alpha)).all(), alpha.tolist()
        assert_canonical(got)


def _open_at_words(ctx, lde, log_n, log_blowup, width, points):
    """Context.open_at, keeping the raw words the kernel wrote"""
    pts = to_monty(np.ascontiguousarray(points, dtype=np.uint32).reshape(-1, 4))
    out = np.empty((pts.shape[0], width, 4), dtype=np.uint32)
    check(ctx.lib.zkhip_open_at(ctx.handle, C.c_void_p(lde.ptr), width, log_n, log_blowup, width,
                                pts.ctypes.data_as(u32p), pts.shape[0], out.ctypes.data_as(u32p)))
    return out


@pytest.mark.parametrize("log_n,width", [(10, 20), (12, 64)])
def test_open_at_on_edge_words(ctx, oracle, log_n, width):
    lde = edge_matrix(2 << log_n, width, seed=log_n + 2)
    d = ctx.from_numpy(lde)
    zs = [z for z in edge_ext(np.random.default_rng(log_n), 2) if z[1:].any()]      # off the (base-field) domain
    for i in range(0, len(zs) - 1):
        words = _open_at_words(ctx, d, log_n, 1, width, np.stack(zs[i:i + 2]))
        assert_canonical_words(words)
        got = from_monty(words)
        for k in range(2):
            assert (got[k] == oracle.open_at(lde, log_n, zs[i + k])).all(), zs[i + k].tolist()


def _edge_ext_rows(n, seed):
    return edge_matrix(n, 4, seed=seed)


@pytest.mark.parametrize("log_h", [1, 10, 17])
def test_fri_fold_on_edge_words(ctx, oracle, log_h):
    v = _edge_ext_rows(1 << log_h, log_h)
    d = ctx.from_numpy(v)
    for beta in edge_ext(np.random.default_rng(log_h), 2):
        got = ctx.fri_fold(d, log_h, beta)
        assert (got.download().reshape(-1, 4) == oracle.fri_fold(v, beta)).all(), beta.tolist()
        assert_canonical(got)


@pytest.mark.parametrize("log_h,log_arity", [(12, 1), (12, 2), (12, 3), (12, 4), (16, 4)])
def test_fri_fold_k_on_edge_words(ctx, oracle, log_h, log_arity):
    v = _edge_ext_rows(1 << log_h, log_h + log_arity)
    d = ctx.from_numpy(v)
    for beta in edge_ext(np.random.default_rng(log_h + log_arity), 1):
        got = ctx.fri_fold_k(d, log_h, log_arity, beta)
        assert (got.download().reshape(-1, 4) == oracle.fri_fold_k(v, log_arity, beta)).all(), beta.tolist()
        assert_canonical(got)


# ------------------------------------------------------------------ RISC Zero Hal operators
def test_eltwise_add_and_sum_ext_on_edge_words(ctx, oracle):
    rng = np.random.default_rng(51)
    pa, pb = np.meshgrid(EDGE_WORDS, EDGE_WORDS)                        # every pair of edge words
    for a, b in ((pa.ravel(), pb.ravel()),
                 (rng.choice(EDGE_WORDS, (1 << 16) + 3), rng.choice(EDGE_WORDS, (1 << 16) + 3))):
        ca, cb = edge_canonical(a), edge_canonical(b)
        got = ctx.eltwise_add(ctx.from_raw(a), ctx.from_raw(b))
        assert (got.download() == oracle.hal_eltwise_add(ca, cb)).all()
        assert_canonical(got)
    for count, to_add in ((33, 5), (4096, 16)):
        e = edge_canonical(rng.choice(EDGE_WORDS, (to_add, count, 4)))
        got = ctx.eltwise_sum_ext(ctx.from_numpy(e), count)
        assert (got.download() == oracle.hal_eltwise_sum_ext(e, count)).all()
        assert_canonical(got)


@pytest.mark.parametrize("count,log_size", [(3, 4), (3, 10), (2, 17)])
def test_zk_shift_on_edge_words(ctx, oracle, count, log_size):
    polys = edge_matrix(1 << log_size, count, seed=log_size).T.copy()
    for shift in [P - 1, 1, 2, P - 2] + [int(x) for x in edge_canonical([MONTY_R1 + 1, 1 << 27, 1 << 30, P // 2])]:
        got = ctx.zk_shift(ctx.from_numpy(polys), count, log_size, shift)
        assert (got.download() == oracle.hal_zk_shift(polys, count, log_size, shift)).all(), shift
        assert_canonical(got)


@pytest.mark.parametrize("ext_field", [0, 1])
def test_mix_poly_coeffs_and_batch_evaluate_any_on_edge_words(ctx, oracle, ext_field):
    rng = np.random.default_rng(60 + ext_field)
    exts = edge_ext(rng, 2)
    # (plan kernel; register form beyond the plan's LDS; 40 combos in runs)
    for k, (count, input_size, ncombo) in enumerate(((6, 5, 3), (1 << 12, 40, 4), (70, 4100, 3), (1 << 12, 333, 40))):
        inp = edge_matrix(count, input_size, seed=k).T.copy()
        combos = rng.integers(0, ncombo, input_size, dtype=np.uint32)
        start, mix = exts[k % len(exts)], exts[(k + 3) % len(exts)]
        out0 = edge_canonical(rng.choice(EDGE_WORDS, (ncombo, count, 4)))
        d_out = ctx.from_numpy(out0)
        ctx.mix_poly_coeffs(d_out, start, mix, ctx.from_numpy(inp), ctx.from_raw(combos), input_size, count, ext_field)
        assert (d_out.download() == oracle.hal_mix_poly_coeffs(out0, start, mix, inp, combos, input_size, count, ext_field)).all()
        assert_canonical(d_out)
    for npoly, log_size in ((3, 4), (5, 11), (2, 16)):
        polys = edge_matrix(1 << log_size, npoly, seed=log_size).T.copy()
        xs = np.stack(exts)
        which = rng.integers(0, npoly, len(xs), dtype=np.uint32)
        got = ctx.batch_evaluate_any(ctx.from_numpy(polys), log_size, ctx.from_raw(which), ctx.from_numpy(xs), ext_field)
        assert (got.download() == oracle.hal_batch_evaluate_any(polys, log_size, which, xs, ext_field)).all()
        assert_canonical(got)


@pytest.mark.parametrize("ext_field", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2048, 2049, 70000])
def test_prefix_products_ext_on_edge_words(ctx, oracle, ext_field, n):
    rng = np.random.default_rng(n + ext_field)
    words = rng.choice(EDGE_WORDS[EDGE_WORDS != 0], (n, 4))            # no zero factor: the products stay non-trivial
    words[::5] = [MONTY_R1, 0, 0, 0]
    words[1::7] = [P - MONTY_R1, 0, 0, 0]
    v = edge_canonical(words)
    got = ctx.prefix_products_ext(ctx.from_numpy(v), ext_field)
    assert (got.download() == oracle.hal_prefix_products_ext(v, ext_field)).all()
    assert_canonical(got)
