"""The LogUp kernels (csrc/stark.hip) on zero denominators, staging limits and edge words, word for word against the oracle.

The other lookup tests draw gamma, beta and the trace at random and read results through download(), which reduces mod P: the
zero-denominator branch of perm_rows_kernel (probability about 2^-124 per pair), a phi or a running sum written as P for 0, the
scan of more than 1024 block totals, and the staging limits of lookup_stage_rows are reached by none of them on purpose.  Here the
plain op (ctx.perm_trace) runs on the steered traces of tests/lookup_edges.py -- base-field challenges, so that chosen rows have
ds = 0, dr = 0, both, ds == dr, ds == -dr -- and on edge-word traces under edge challenges; the machine kernels run inside whole
proofs of the boundary machines of tests/machines.py, whose bytes must equal the oracle's.  test_lookup_edges_cpu.py pins the oracle
against a plain-Python restatement on the same inputs and shows every boundary machine balanced in plain integers, so a failure here
is the device's.

  kernel / branch                                   test                       case id
  ------------------------------------------------  -------------------------  ---------------------------------------------
  perm_rows_kernel, ds dr = 0 (direct formula)      test_perm_trace_op         every shape, the "steered" run (ds0, dr0, both0)
  perm_rows_kernel, ds == dr (phi = four 0 words)   test_perm_trace_op         every shape from 2^5 rows up ("eq"; "neg": ds == -dr)
  perm_rows_kernel, partial block                   test_perm_trace_op         0-8-1, 1-8-1, 5-16-2
  perm_rows_kernel, exactly one block               test_perm_trace_op         8-24-3
  perm_rows_kernel, 64 pairs (the entry's maximum)  test_perm_trace_op         8-512-64
  perm_rows_kernel, row pitch > width               test_perm_trace_op         13-40-5-ld48 (the padding holds junk)
  perm_fixup_kernel, first non-zero offset          test_perm_trace_op         9-16-2
  perm_scan_blocks_kernel, per = 1, 1024 lanes      test_perm_trace_op         18-8-1
  perm_scan_blocks_kernel, per = 2 / per = 4        test_perm_trace_op         19-8-1 / 20-8-1
  lookup_stage_rows, 56 columns (pitch 57, the      test_boundary_machine      used56
    largest LDS launch) / 57 (unstaged)                                        used57
  lookup_stage_rows, column 511 (bit 31 of          test_boundary_machine      col511
    chunk_mask) / 512 (unstaged)                                               col512
  one cmap slot, several readers                    test_boundary_machine      reuse
  perm_rows_machine_kernel / lookup_addend_kernel,  test_boundary_machine      one (1 interaction), odd63 (the last column single)
    single-term phi; 64 interactions                                           max64
  lookup_mult, m = 0 / 1 / P - 1 / (P + 1) / 2 on   test_boundary_machine      edge-8-5, edge-9-5, edge-9-8 (32 rows: a partial
    sends and receives; buses 0 and P - 1                                        tile; 2^9: two tiles)
  two sources, quad by quad (col < pre_w);          test_boundary_machine      keyed4, keyed20 (a 16-column chunk from both buffers)
    tuples and multiplicities across pre_w
  the side-by-side copy (prover.cpp, !two)          test_boundary_machine      keyed_col512, keyed_used57
  two sources, main row pitch = width + 4           test_boundary_machine      keyed4-pitch, keyed20-9-8-pitch (the padding holds junk)

The zero-denominator branch of perm_rows_machine_kernel cannot be steered through the ABI: gamma is drawn from the transcript after
the trace is committed.  It stays covered only by its equality in form with the plain kernel's branch, which the steered runs reach.

A reviewer can confirm one row with `rocprofv3 --kernel-trace --stats -- python -m pytest -m gpu <file>::<test>[<id>]`.
"""
import numpy as np
import pytest

import lookup_edges as LE
import machines as M
from field_edges import P, assert_canonical, edge_matrix
from zktls_amd._lib import Params, to_monty
from zktls_amd.device import verify_machine, verify_machine_keyed

pytestmark = pytest.mark.gpu

G, B = 0x1234567, 0x7654321          # base-field gamma and beta of the steered runs (test_lookup_edges_cpu.py uses the same)


def _run_op(ctx, oracle, trace, log_n, width, pairs, ld, gamma, beta, cases, what):
    host = trace
    if ld:                                                              # padded pitch: non-zero junk (non-canonical words too) in the padding
        host = np.full((trace.shape[0], ld), P + 5, dtype=np.uint32)
        host[:, width:] = np.random.default_rng(ld).integers(1, 1 << 32, (trace.shape[0], ld - width), dtype=np.uint64)
        words = host.copy()
        words[:, :width] = to_monty(trace).reshape(trace.shape)
    else:
        words = to_monty(trace).reshape(trace.shape)
    src = ctx.from_raw(words)
    exp = oracle.perm_trace(trace, pairs, gamma, beta)
    out = ctx.perm_trace(src, log_n, width, pairs, gamma, beta, ld=ld)
    got = out.download().reshape(exp.shape)
    bad = LE.first_mismatch(got, exp, cases)
    assert bad is None, "%s: %s" % (what, bad)
    assert_canonical(out)
    assert (src.download_monty() == words.ravel()).all(), "%s: the input changed" % what


OP_SHAPES = [(0, 8, 1, None), (1, 8, 1, None), (5, 16, 2, None), (8, 24, 3, None), (9, 16, 2, None), (8, 512, 64, None),
             (13, 40, 5, 48), (18, 8, 1, None), (19, 8, 1, None), (20, 8, 1, None)]


@pytest.mark.parametrize("log_n,width,pairs,ld", OP_SHAPES, ids=["%d-%d-%d%s" % (ln, w, q, "-ld%d" % ld if ld else "") for ln, w, q, ld in OP_SHAPES])
def test_perm_trace_op(ctx, oracle, log_n, width, pairs, ld):
    """ctx.perm_trace == oracle.perm_trace word for word, raw output words canonical, input unchanged: once steered onto zero and equal
    denominators (base-field gamma, beta), once on edge words under two edge challenges.  (2^20 rows: 32 MB in, 32 MB out.)"""
    trace, gamma, beta, cases = LE.steered_logup_trace(log_n, width, pairs, G, B, seed=log_n + pairs)
    _run_op(ctx, oracle, trace, log_n, width, pairs, ld, gamma, beta, cases, "steered")
    gamma, beta = LE.edge_challenges(np.random.default_rng(log_n + width))
    _run_op(ctx, oracle, edge_matrix(1 << log_n, width, seed=log_n + 1), log_n, width, pairs, ld, gamma, beta, [], "edge challenges")


# ------------------------------------------------------------------ the machine kernels through proofs
HEIGHTS = [(8, 5), (9, 5), (9, 8)]
MACHINES = [(c, 8, 5, False) for c in M.BOUNDARY_CASES if c != "edge"] + [("edge", ls, lr, False) for ls, lr in HEIGHTS] + \
           [("keyed4", 8, 5, True), ("keyed20", 9, 8, True)]


def _padded(ctx, t, pad):
    """(buffer, row pitch) of a matrix uploaded with `pad` words of non-zero junk after every row"""
    host = np.random.default_rng(t.shape[1]).integers(1, P, (t.shape[0], t.shape[1] + pad)).astype(np.uint32)
    host[:, :t.shape[1]] = t
    return ctx.from_numpy(host), t.shape[1] + pad


@pytest.mark.parametrize("case,log_sender,log_receiver,pitch", MACHINES,
                         ids=["%s%s%s" % (c, "" if (ls, lr) == (8, 5) and c != "edge" else "-%d-%d" % (ls, lr), "-pitch" if p else "") for c, ls, lr, p in MACHINES])
def test_boundary_machine(ctx, oracle, case, log_sender, log_receiver, pitch):
    """proof bytes equal the oracle's; both verifiers accept; both reject after one public value is changed"""
    O = oracle
    shape = (1, 8, 4)
    prm, oprm = Params(*shape), O.default_params(*shape)
    traces, pre, progs, tables, pub = M.boundary_machine(case, log_sender, log_receiver, seed=log_sender + log_receiver)
    lns, ws = [t.shape[0].bit_length() - 1 for t in traces], [t.shape[1] for t in traces]
    wrong = [pub[0], (pub[1] + 1) % P]
    if pre is None:
        chips = [(ctx.from_numpy(t), ln, w) for t, ln, w in zip(traces, lns, ws)]
        proof = ctx.prove_machine(chips, progs, tables, pub, prm)
        assert proof.tobytes() == O.prove_machine(traces, progs, tables, pub, oprm).tobytes()
        assert verify_machine(proof, lns, ws, progs, tables, pub, prm) == (0, 0)
        assert O.verify_machine(proof, lns, ws, progs, tables, pub, oprm) == 0
        assert verify_machine(proof, lns, ws, progs, tables, wrong, prm)[0] != 0
        assert O.verify_machine(proof, lns, ws, progs, tables, wrong, oprm) != 0
        return
    pws = [0 if p is None else p.shape[1] for p in pre]
    if pitch:
        chips = [_padded(ctx, t, 4) for t in traces]
        chips = [(buf, ln, w, ld) for (buf, ld), ln, w in zip(chips, lns, ws)]
    else:
        chips = [(ctx.from_numpy(t), ln, w) for t, ln, w in zip(traces, lns, ws)]
    key = ctx.machine_setup([(None if p is None else ctx.from_numpy(p), ln, pw) for p, ln, pw in zip(pre, lns, pws)], prm)
    try:
        assert (key.root == O.machine_setup(pre, lns, oprm)).all()
        proof = ctx.prove_machine_keyed(key, chips, progs, tables, pub, prm)
        assert proof.tobytes() == O.prove_machine_keyed(traces, pre, progs, tables, pub, oprm).tobytes()
        assert verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tables, pub, prm) == (0, 0)
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tables, pub, oprm) == 0
        assert verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tables, wrong, prm)[0] != 0
        assert O.verify_machine_keyed(proof, lns, ws, pws, key.root, progs, tables, wrong, oprm) != 0
    finally:
        key.close()
