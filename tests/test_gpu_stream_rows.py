"""The lane-per-row forms of the quotient and row-sum kernels (csrc/stark.hip quotient_stream_kernel, rowdot_stream_kernel) at their
boundaries, through the entries that reach them, against the oracle.  Cases and the mirrors of the dispatch: stream_rows.py.

  kernel                   case
  -----------------------  -----------------------------------------------------------------------------------------------------
  rowdot_stream_kernel     thr-32 / thr-96 / thr-256 (2048 rows, the threshold: one, three and eight slices), two-256x2^13 (32 workgroups);
                           the permutation block of width 32 / 96 in thr-96, two-256
  rowdot_regs_kernel<NK>   below-* (1024 rows), fall-68 / fall-240 (inside forms 1..4, no whole slices), permutation blocks of width 8, 100, 256
  quotient_stream_kernel   quotient values 2^10 x 32, 2^11 x 96, 2^12 x 256 on edge alphas (both chunks, every row: the last wavefront of a
                           chunk reads the row that wraps to e = parity); whole proofs at 2^10 x 32 with 0 / 2 LogUp pairs, blowup 2 (lde_out) and 4
  quotient_kernel<NG>      quotient values 2^10 x 48 (no whole slices) and 2^9 x 32 (under the threshold)

zkhip_reduced_opening reports the register form (1..4) whichever of the two kernels ran, as before; which kernel a case launched shows in
`rocprofv3 --kernel-trace --stats -- python -m pytest -m gpu <file>::<test>[<id>]`.  The A/B check (tests/checks/stream_rows_ab.py, a child
process on the A/B build) runs every case with the lane-per-row forms and with the 16-lane forms forced and requires equal bytes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import reduced_edges as RE
import stream_rows as SR
from field_edges import assert_canonical, assert_canonical_words, edge_ext, edge_matrix
from test_gpu_reduced_edges import _run_case, _upload_case
from zktls_amd._lib import Params, from_monty
from zktls_amd.device import verify_shard

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5A4B544C53


@pytest.mark.parametrize("fill", RE.FILLS)
@pytest.mark.parametrize("case", [c for c, _, _ in SR.ROWDOT_CASES], ids=[c[0] for c, _, _ in SR.ROWDOT_CASES])
def test_reduced_opening_row_sums(ctx, oracle, case, fill):
    d = RE.build(case, fill)
    dev, out = _upload_case(ctx, d)
    forms = _run_case(ctx, d, dev, out)
    words = out.download_monty()
    n = 4 * d["rows"]
    assert forms == (case[7], case[8]), "register forms reported: %s" % (forms,)
    assert_canonical_words(words[:n])
    exp = RE.oracle_expected(oracle, d)
    bad = np.flatnonzero((from_monty(words[:n]).reshape(-1, 4) != exp).any(axis=1))
    assert bad.size == 0, "%d rows differ, first %s" % (bad.size, bad[:8].tolist())
    assert (words[n:] == RE.TAIL_WORD).all()                                      # nothing written behind the output
    for k, b in dev.items():
        assert (b.download_monty() == d[k].ravel()).all(), k                      # inputs unchanged, word for word
    for b in list(dev.values()) + [out]:
        b.free()


@pytest.mark.parametrize("log_n,width", SR.QUOTIENT_CASES + SR.QUOTIENT_FALLBACK)
def test_quotient_values(ctx, oracle, log_n, width):
    lde = edge_matrix(2 << log_n, width, seed=log_n)
    d = ctx.from_numpy(lde)
    for alpha in edge_ext(np.random.default_rng(log_n), 2):
        got = ctx.quotient_values(d, log_n, width, alpha)
        exp = oracle.quotient_values(lde, log_n, alpha)
        bad = np.flatnonzero((got.download().reshape(-1, 4) != exp).any(axis=1))
        assert bad.size == 0, "alpha %s: %d points differ, first %s" % (alpha.tolist(), bad.size, bad[:8].tolist())
        assert_canonical(got)
    assert (d.download().reshape(-1, width) == lde).all()


@pytest.mark.parametrize("shape", SR.PROOF_CASES)
def test_proofs_with_and_without_lookups_and_lde_out(ctx, oracle, shape):
    log_n, width, pairs = 10, 32, shape[3]
    assert SR.quotient_stream_form(log_n, width) and SR.rowdot_stream_form(width, (1 << shape[0]) << log_n)
    trace = ctx.gen_trace_logup(SEED, 9, log_n, width, pairs) if pairs else ctx.gen_trace(SEED, 9, log_n, width)
    otrace = oracle.gen_trace_logup(SEED, 9, log_n, width, pairs) if pairs else oracle.gen_trace(SEED, 9, log_n, width)
    prm, oprm = Params(*shape), oracle.default_params(*shape)
    proof = ctx.prove_shard(trace, log_n, width, [1, 2], prm)
    assert proof.tobytes() == oracle.prove_shard(otrace, [1, 2], oprm).tobytes()
    assert verify_shard(proof, log_n, width, [1, 2], prm) == (0, 0)


def test_both_forms_give_the_same_bytes():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "stream_rows_ab.py")], cwd=ROOT, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert b"the lane-per-row and the 16-lane forms give the same bytes" in p.stdout
