"""The JOIN of fold-16 lift proofs on the GPU (zktls_amd/csrc/fri16_chip.hip: zkhip_fri16_join_*; zktls_amd/csrc/machine_verifier.inl: mrec_eval_rows_kernel).
(1) The EVAL row kernel alone against the plain-integer restatement (tests/mrec_eval.py -- which tests/test_fri16_join_cpu.py holds the host's table to), rows and
hand-back word for word, at every term count at which the scan changes path, on random and on edge words.  (2) The same kernel inside the machine: two GPU-made
segment proofs lifted and joined, the bytes against zkhip_prove_machine_verifier on the assembled description and against the host's walk of the witnesses, the one-call
entry, what it refuses.  (3) A machine-mode case outside the lift under both witness settings."""
import numpy as np
import pytest

import machines as M
import mrec_eval
from field_edges import edge_canonical
from zktls_amd._lib import Params, ZkHipError, segment_params
from zktls_amd.device import (InnerMachine, fri16_join_key_host, fri16_join_max_proofs, fri16_lift_inner_machine, machine_verifier_describe, recursion_witnesses_on_host,
                              verify_fri16_join, verify_shard)

pytestmark = pytest.mark.gpu
P = 2013265921
SEED = 0x5A4B544C53
# canonical 0, 1, P - 1 and the values whose Montgomery words are 0, 1, P - 1
EDGES = sorted({0, 1, P - 1} | {int(x) for x in edge_canonical([0, 1, P - 1])})
# one workgroup of 256 lanes per (proof, chip), four wavefronts of 64: a partial wavefront, a full one, one lane into the second; a partial chunk, a full one, a
# carry over one chunk boundary and over two
COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]
KSPAN, N_STREAM = 40, 20                                     # keys 1 .. 20 are read as the opened-value stream, 21 .. 39 from the call's block (public values, selectors)


def draw_terms(rng, counts):
    """chip c has counts[c] terms (0: none).  first flags: random, and SET at a chip's first term, on lane 0 and on the last lane of a wavefront and of a chunk, CLEAR
    next to them; some constraints without a term (coefficient 0, keys 0 0 0, first = 1); keys: random, and the four kinds forced into every chip's head"""
    forced = [0, N_STREAM, N_STREAM + 1, KSPAN - 1]          # the extension one, the last stream value, a public value, a selector
    terms = []
    for c, n in enumerate(counts):
        for i in range(n):
            keys = [int(k) for k in rng.integers(0, KSPAN, 3)]
            if i < len(forced):
                keys[i % 3] = forced[i]
            first = int(rng.integers(0, 4) == 0)
            if i % 64 in (0, 63) or i % 256 == 255:
                first = 1
            if i % 64 in (1, 62):
                first = 0
            coeff = int(rng.choice(EDGES)) if rng.integers(0, 8) == 0 else int(rng.integers(0, P))
            if i % 37 == 5:
                coeff, keys, first = 0, [0, 0, 0], 1          # a constraint of zero terms
            terms.append((c, coeff, keys, first))
    return terms


def draw_values(rng, n_proofs, edge):
    word = (lambda: int(rng.choice(EDGES))) if edge else (lambda: int(rng.integers(0, P)))
    values = [[[word() for _ in range(4)] for _ in range(KSPAN)] for _ in range(n_proofs)]
    alphas = [[word() for _ in range(4)] for _ in range(n_proofs)]
    return values, alphas


def eval_log_rows(im, n_proofs):
    """log2 of the rows of machine mode's EVAL table (the chip of 12 preprocessed and 32 main columns) for n_proofs proofs of the inner machine.  The prover makes the
    rows on the device from 2^15 rows on (csrc/machine_verifier.inl: EVAL_DEVICE_MIN_ROWS) and on the host below"""
    found = [ln for _, ln, mw, pw in (machine_verifier_describe(im, i, 1, n_proofs) for i in range(10)) if (mw, pw) == (32, 12)]
    assert len(found) == 1
    return found[0]


def run_kernel(ctx, terms, n_chips, values, alphas):
    rows, accs = ctx.machine_verifier_gen_eval_rows([t[0] for t in terms], [t[1] for t in terms], [t[2] for t in terms], [t[3] for t in terms], n_chips, values, alphas, N_STREAM)
    assert int(rows.max()) < P and int(accs.max()) < P       # (the entry itself refuses a device word of P or more before it converts)
    return rows, accs


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("edge", [False, True], ids=["random", "edge"])
def test_eval_rows_of_one_chip_equal_the_restatement(ctx, n, edge):
    rng = np.random.default_rng([97, n, int(edge)])
    terms = draw_terms(rng, [n])
    values, alphas = draw_values(rng, 1, edge)
    rows, accs = run_kernel(ctx, terms, 1, values, alphas)
    want, wacc = mrec_eval.table(terms, 1, values, alphas)
    assert np.array_equal(rows, np.array(want, dtype=np.uint32)) and accs.tolist() == wacc
    assert wacc[0] == want[-1][mrec_eval.EV_ACCO:mrec_eval.EV_ACCO + 4]


@pytest.mark.parametrize("n_proofs", [1, 3])
@pytest.mark.parametrize("edge", [False, True], ids=["random", "edge"])
def test_eval_rows_of_several_unequal_chips_in_one_launch(ctx, n_proofs, edge):
    counts = [65, 1, 0, 513, 256, 63, 257, 0, 255, 64]       # (two chips without a term: an empty range, a zero hand-back)
    rng = np.random.default_rng([101, n_proofs, int(edge)])
    terms = draw_terms(rng, counts)
    values, alphas = draw_values(rng, n_proofs, edge)
    rows, accs = run_kernel(ctx, terms, len(counts), values, alphas)
    want, wacc = mrec_eval.table(terms, len(counts), values, alphas)
    assert np.array_equal(rows, np.array(want, dtype=np.uint32)) and accs.tolist() == wacc
    assert all(wacc[p * len(counts) + c] == [0, 0, 0, 0] for p in range(n_proofs) for c in (2, 7))


def test_eval_rows_entry_refuses_what_would_read_out_of_bounds(ctx):
    rng = np.random.default_rng(103)
    values, alphas = draw_values(rng, 1, False)
    ok = [(0, 5, [1, 2, 3], 1), (1, 6, [0, 39, 20], 0)]
    run_kernel(ctx, ok, 2, values, alphas)
    for bad in ([(0, 5, [1, 2, KSPAN], 1)], [(2, 5, [1, 2, 3], 1)], [(1, 5, [1, 2, 3], 1), (0, 5, [1, 2, 3], 1)], [(0, P, [1, 2, 3], 1)], [(0, 5, [1, 2, 3], 2)]):
        with pytest.raises(ZkHipError, match="terms chip by chip"):
            run_kernel(ctx, bad, 2, values, alphas)
    with pytest.raises(ZkHipError, match="canonical"):
        run_kernel(ctx, ok, 2, values, [[P, 0, 0, 0]])


# ------------------------------------------------------------------ (2) inside the machine
def test_two_gpu_segments_lifted_joined_and_the_one_call_entry(ctx, oracle):
    """two GPU-made segment proofs at 2^10 x 16 with 12 queries (tests/test_gpu_fri16_lift.py's shape) -> two lift proofs -> ONE proof"""
    log_n, width, sp = 10, 16, segment_params(12, 0, 2)
    lift, join = Params(1, 12, 4), Params(1, 8, 2)
    pubs = [[7], [8]]
    segs = []
    for pub, shard in zip(pubs, (3, 4)):
        cols = ctx.from_numpy(np.ascontiguousarray(oracle.gen_trace(SEED, shard, log_n, width).T))
        segs.append(ctx.prove_segment(cols, log_n, width, pub, sp))
        cols.free()
    S = ((log_n - int(sp.log_final)) // 4, int(sp.log_final), int(sp.log_blowup), int(sp.num_queries), int(sp.pow_bits), width, 1)      # (R, F, log_blowup, Q, grinding bits, W, NP)
    assert S[:4] == (2, 2, 2, 12)
    assert fri16_join_max_proofs(*S, lift) >= 2
    lkey = ctx.fri16_lift_key(*S, lift)
    jkey = ctx.fri16_join_setup(*S, 2, lift, join)
    im = fri16_lift_inner_machine(*S, lift)
    gkey = ctx.machine_verifier_setup(im, join, 2)
    assert eval_log_rows(im, 2) >= 16                        # more than 2^15 terms: EVAL's rows of this join are the kernel's
    prev = recursion_witnesses_on_host(0)
    try:
        assert jkey.root.tolist() == fri16_join_key_host(*S, 2, lift, join).tolist() == gkey.root.tolist()
        lifted = [ctx.prove_fri16_lift_segment(lkey, s, log_n, width, pub, sp, lift) for s, pub in zip(segs, pubs)]
        joined = ctx.prove_fri16_join(jkey, *S, lifted, pubs, lift, join)
        assert joined.tobytes() == ctx.prove_machine_verifier(gkey, im, lifted, pubs, join).tobytes()      # a shape call, not a second prover
        recursion_witnesses_on_host(1)
        assert ctx.prove_fri16_join(jkey, *S, lifted, pubs, lift, join).tobytes() == joined.tobytes()      # EVAL's rows (and the per-query tables) from the host's walk
        recursion_witnesses_on_host(0)
        assert verify_fri16_join(joined, pubs, *S, 2, jkey.root, lift, join) == (0, 0)
        assert verify_fri16_join(joined, [pubs[1], pubs[0]], *S, 2, jkey.root, lift, join)[0] != 0          # the segments' public values exchanged
        # segment proofs in, one proof out: the step-by-step bytes
        assert ctx.prove_fri16_join_segments(lkey, jkey, segs, log_n, width, pubs, sp, lift, join).tobytes() == joined.tobytes()
        bad = segs[1].copy()
        bad[bad.size // 2] ^= 1
        rc, _ = verify_shard(bad, log_n, width, pubs[1], sp)
        assert rc != 0
        with pytest.raises(ZkHipError, match="prove_fri16_join_segments: segment 1: ") as e:
            ctx.prove_fri16_join_segments(lkey, jkey, [segs[0], bad], log_n, width, pubs, sp, lift, join)
        assert e.value.code == rc
        # what the prover refuses before anything is proven
        with pytest.raises(ZkHipError, match="lift proofs of this shape go into one join, not 0"):
            ctx.prove_fri16_join(jkey, *S, [], [], lift, join)
        with pytest.raises(ZkHipError, match=r"n_proofs x n_inner_public words in proof order \(2 here\), not 3"):
            ctx.prove_fri16_join(jkey, *S, lifted, [[7], [8, 9]], lift, join)
        with pytest.raises(ZkHipError, match="width-24"):
            ctx.prove_fri16_join(jkey, *S, lifted, pubs, lift, join, hash_width=16)
        with pytest.raises(ZkHipError, match="proof 0 rejected: "):      # (the public values move the transcript: whichever check meets the moved challenges first)
            ctx.prove_fri16_join(jkey, *S, lifted, [pubs[1], pubs[0]], lift, join)
    finally:
        recursion_witnesses_on_host(prev)
        lkey.close(), jkey.close(), gkey.close()


# ------------------------------------------------------------------ (3) machine mode outside the lift
def test_a_two_chip_machine_under_device_and_host_witnesses(ctx, oracle):
    """one two-chip keyed machine (tests/machines.py's byte machine, as tests/test_gpu_recursion_machine.py builds it), two proofs, a few thousand terms: below the
    size from which EVAL's rows are the kernel's, so both settings fill them on the host -- device and host witnesses give one outer proof"""
    O = oracle
    q, pb = 3, 1
    proofs, pubs = [], []
    for seed in (1, 2):
        mains, pres, progs, tabs, pub = M.byte_machine(7, 3, seed)
        lns = [m.shape[0].bit_length() - 1 for m in mains]
        vk = [int(x) for x in O.machine_setup(pres, lns, O.default_params(1, q, pb))]
        chips = [dict(ln=lns[c], W=mains[c].shape[1], Pw=0 if pres[c] is None else pres[c].shape[1], prog=progs[c], tab=tabs[c]) for c in range(len(mains))]
        proofs.append(O.prove_machine_keyed(mains, pres, progs, tabs, pub, O.default_params(1, q, pb)))
        pubs.append(pub)
    im = InnerMachine(chips, vk, q, pb, len(pubs[0]))
    prm = Params(1, 20, 8)
    key = ctx.machine_verifier_setup(im, prm, 2)
    assert eval_log_rows(im, 2) < 15
    prev = recursion_witnesses_on_host(0)
    try:
        dev = ctx.prove_machine_verifier(key, im, proofs, pubs, prm).tobytes()
        recursion_witnesses_on_host(1)
        host = ctx.prove_machine_verifier(key, im, proofs, pubs, prm).tobytes()
    finally:
        recursion_witnesses_on_host(prev)
        key.close()
    assert dev == host
