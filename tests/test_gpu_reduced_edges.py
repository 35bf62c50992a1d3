"""The stages between the openings and the queries, each on its own: the reduced opening (FRI input), the device-challenge fold, the
proof-of-work search, and the captured FRI graph against plain launches.  Inside a proof these run at the proof's shapes with challenges
drawn by the transcript; here they run on edge Montgomery words at the shapes where their launchers change kernels.

Which kernel each case reaches (csrc/stark.hip; the reduced-opening cases are reduced_edges.CASES, whose literal forms are compared with
what zkhip_reduced_opening reports it launched -- launch_rowdot switches on the same rowdot_form value):

  kernel                        case
  ----------------------------  ------------------------------------------------------------------------------------------------
  rowdot_regs_kernel<1>         thr-* and twice-* (widths 4, 8, 12, 32, 64 at (256 / L) * 16 rows and twice that), nk-64x2^8;
                                the permutation block of width 8 from 2048 rows on (below-4x2^11, twice-4x2^13, twice-8x2^12)
  rowdot_regs_kernel<2>         nk-68x2^8 (one lane in the last k), nk-128x2^8
  rowdot_regs_kernel<3>         nk-132x2^8 (one lane in the last k), nk-192x2^8
  rowdot_regs_kernel<4>         nk-196x2^8 (one lane in the last k), nk-256x2^8
  rowdot_kernel                 below-* (one step under each threshold), nk-260x2^8 (nk = 5), wide-1024x2^6, part-* (two rows: a partial
                                wave); every permutation block of width 260, and of width 8 under 2048 rows
  reduced_combine_kernel        every case: p_width 0 / 8 / 260, q_width 0 / 8 / 16, accumulate 0 (over 0xFFFFFFFF words) / 1 (over edge
                                words), dense rows and the [pre | main] layout (block 4 columns into rows of pitch width + 8)
  fri_fold_dev_kernel           fri_fold_k_dev 2^1, 2^4, 2^9, 2^12 x arities 2 .. 16 (squarings 0 .. 3), edge betas in device memory
  ext_add_kernel                the same with an added vector of edge words
  grind_kernel                  grind: slots 0 .. 7, bits 0 / 1 / 4 / 8 / 10, windows before, at and past the witness, prefilled results,
                                the window that ends at P
  fri_commit_phase (graph)      prove_shard A B A A and prove_chips between them with the graph on, then off

A reviewer can confirm one row with `rocprofv3 --kernel-trace --stats -- python -m pytest -m gpu <file>::<test>[<id>]`.
"""
import ctypes as C

import numpy as np
import pytest

import reduced_edges as RE
from field_edges import EDGE_WORDS, MONTY_R1, P, assert_canonical_words, edge_ext, edge_matrix
from zktls_amd._lib import Params, ZkHipError, from_monty, to_monty
from zktls_amd.device import DeviceView

pytestmark = pytest.mark.gpu

SEED = 0x5A4B544C53


# ------------------------------------------------------------------ reduced opening
def _upload_case(ctx, d):
    dev = {k: ctx.from_raw(d[k]) for k in ("tbuf", "pbuf", "qbuf", "weights", "dinv") if d[k] is not None}
    out = ctx.alloc(4 * d["rows"] + RE.TAIL)
    out.upload_monty(np.concatenate([d["out0"].ravel(), np.full(RE.TAIL, RE.TAIL_WORD, dtype=np.uint32)]))
    return dev, out


def _run_case(ctx, d, dev, out_buf, **over):
    a = dict(tlde=DeviceView(dev["tbuf"], d["t0"]), t_ld=d["tbuf"].shape[1], width=d["width"], log_rows=d["log_rows"], weights=dev["weights"],
             n_weights=d["weights"].shape[0], dinv=dev["dinv"], scalars=RE.canonical(d["scalars"]), out=out_buf, accumulate=d["accumulate"])
    if d["pbuf"] is not None:
        a.update(plde=DeviceView(dev["pbuf"], d["p0"]), p_ld=d["pbuf"].shape[1], p_width=d["p_width"])
    if d["qbuf"] is not None:
        a.update(qlde=DeviceView(dev["qbuf"], d["q0"]), q_ld=d["qbuf"].shape[1], q_width=d["q_width"])
    a.update(over)
    return ctx.reduced_opening(**a)


@pytest.mark.parametrize("fill", RE.FILLS)
@pytest.mark.parametrize("case", RE.CASES, ids=[c[0] for c in RE.CASES])
def test_reduced_opening_on_edge_words(ctx, oracle, case, fill):
    d = RE.build(case, fill)
    dev, out = _upload_case(ctx, d)
    forms = _run_case(ctx, d, dev, out)
    words = out.download_monty()
    n = 4 * d["rows"]
    assert forms == (case[7], case[8]), "row-sum kernels taken: %s" % (forms,)
    assert_canonical_words(words[:n])
    exp = RE.oracle_expected(oracle, d)
    bad = np.flatnonzero((from_monty(words[:n]).reshape(-1, 4) != exp).any(axis=1))
    assert bad.size == 0, "%d rows differ, first %s" % (bad.size, bad[:8].tolist())
    assert (words[n:] == RE.TAIL_WORD).all()                                      # nothing written behind the output
    for k, b in dev.items():
        assert (b.download_monty() == d[k].ravel()).all(), k                      # inputs unchanged, word for word
    for b in list(dev.values()) + [out]:
        b.free()


def test_reduced_opening_refuses_bad_arguments(ctx):
    d = RE.build(("reject", 4, 12, 1, 8, 8, 0, 0, 0), "uniform")
    dev, out = _upload_case(ctx, d)
    assert _run_case(ctx, d, dev, out) == (0, 0)
    good = out.download_monty()
    out.upload_monty(np.concatenate([d["out0"].ravel(), np.full(RE.TAIL, RE.TAIL_WORD, dtype=np.uint32)]))
    before = out.download_monty()
    bad = [
        dict(width=6), dict(width=10), dict(width=0), dict(t_ld=18), dict(p_width=6), dict(p_ld=10), dict(q_ld=10),        # not multiples of 4
        dict(t_ld=8), dict(p_ld=4), dict(q_ld=4),                                                                         # pitch < width
        dict(tlde=DeviceView(dev["tbuf"], 1)), dict(plde=DeviceView(dev["pbuf"], 2)), dict(qlde=DeviceView(dev["qbuf"], 3)),   # not 16-byte aligned
        dict(weights=DeviceView(dev["weights"], 1)), dict(dinv=DeviceView(dev["dinv"], 2)), dict(out=DeviceView(out, 1)),
        dict(q_width=4), dict(q_width=12), dict(q_width=24),
        dict(n_weights=11), dict(n_weights=7), dict(width=4, p_width=4, n_weights=7),                                       # n < max(width, p_width, q_width)
        dict(log_rows=0), dict(log_rows=-1),
        dict(tlde=None), dict(plde=None), dict(qlde=None), dict(weights=None), dict(dinv=None), dict(out=None),
    ]
    for over in bad:
        with pytest.raises(ZkHipError) as e:
            _run_case(ctx, d, dev, out, **over)
        assert e.value.code == -1, over
    for nulled in (14, 17):                                                        # the scalars, the forms
        args = [ctx.handle, C.c_void_p(dev["tbuf"].ptr), 20, 12, C.c_void_p(dev["pbuf"].ptr), 12, 8, C.c_void_p(dev["qbuf"].ptr), 12, 8, 4,
                C.c_void_p(dev["weights"].ptr), 12, C.c_void_p(dev["dinv"].ptr), np.zeros(40, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)),
                0, C.c_void_p(out.ptr), (C.c_int * 2)()]
        args[nulled] = None
        assert ctx.lib.zkhip_reduced_opening(*args) == -1
    ctx.sync()
    assert (out.download_monty() == before).all()                                  # nothing was launched
    # an absent block's pointer and pitch are not looked at
    d0 = RE.build(("reject0", 4, 12, 1, 0, 0, 0, 0, -1), "uniform")
    dev0, out0 = _upload_case(ctx, d0)
    assert _run_case(ctx, d0, dev0, out0, plde=1, p_ld=3, qlde=2, q_ld=5) == (0, -1)
    assert good.size == before.size and (good[:4 * d["rows"]] != before[:4 * d["rows"]]).any()      # (the accepted call above did write)


# ------------------------------------------------------------------ the fold with its challenge in device memory
SAME_WORD_BETAS = [np.full(4, w, dtype=np.uint32) for w in (0, MONTY_R1, P - 1, P - MONTY_R1)]          # Montgomery words


@pytest.mark.parametrize("log_h,log_arity", [(h, k) for h in (1, 4, 9, 12) for k in (1, 2, 3, 4) if h >= k])
def test_fri_fold_k_dev_on_edge_betas(ctx, oracle, log_h, log_arity):
    rng = np.random.default_rng(100 * log_h + log_arity)
    v = edge_matrix(1 << log_h, 4, seed=log_h + log_arity)
    d_in = ctx.from_numpy(v)
    n_out = 1 << (log_h - log_arity)
    add_words = rng.choice(EDGE_WORDS, (n_out, 4)).astype(np.uint32)
    d_add = ctx.from_raw(add_words)
    betas = SAME_WORD_BETAS + [to_monty(b) for b in edge_ext(rng, 2)]
    for bw in betas:
        beta = from_monty(bw)
        exp = oracle.fri_fold_k(v, log_arity, beta)
        d_beta = ctx.from_raw(bw)
        plain = ctx.fri_fold_k_dev(d_in, log_h, log_arity, d_beta).download_monty()
        added = ctx.fri_fold_k_dev(d_in, log_h, log_arity, d_beta, add=d_add).download_monty()
        host = ctx.fri_fold_k(d_in, log_h, log_arity, beta).download_monty()
        assert_canonical_words(plain)
        assert_canonical_words(added)
        assert (from_monty(plain).reshape(-1, 4) == exp).all(), bw.tolist()
        assert (plain == host).all(), bw.tolist()                                 # the host-challenge entry on the same input, word for word
        exp_added = ((exp.astype(np.uint64) + from_monty(add_words)) % P).astype(np.uint32)
        assert (from_monty(added).reshape(-1, 4) == exp_added).all(), bw.tolist()
        assert (d_beta.download_monty() == bw).all()
    assert (d_in.download_monty() == to_monty(v).ravel()).all() and (d_add.download_monty() == add_words.ravel()).all()


# ------------------------------------------------------------------ proof of work
NONE = 0xFFFFFFFF


@pytest.mark.parametrize("pending", range(8))
def test_grind_returns_the_smallest_witness(ctx, oracle, pending):
    _, state, slot = RE.grind_state(oracle, [100 + pending] * 8, pending)
    assert ctx.grind(state, slot, 0, 12345, 256) == 12345                          # bits 0: the first candidate
    for bits in (1, 4, 8):
        exp = RE.grind_reference(oracle, state, slot, bits, 0, 1 << 12)
        assert exp != NONE
        assert ctx.grind(state, slot, bits, 0, 1 << 12) == exp, bits
    # prefilled results (4 bits): one above the smallest hit is lowered to it; one below every hit of its window is kept, whether the
    # window's workgroups leave early (they start above it) or search and find only larger hits
    w = RE.grind_reference(oracle, state, slot, 4, 0, 1 << 12)
    w2 = RE.grind_reference(oracle, state, slot, 4, w + 1, 1 << 12)
    assert ctx.grind(state, slot, 4, 0, 1 << 12, result=w2 + 1) == w
    assert ctx.grind(state, slot, 4, 0, 1 << 12, result=w2) == w
    assert ctx.grind(state, slot, 4, w + 1, 1 << 12, result=w) == w
    assert ctx.grind(state, slot, 4, w + 1, 1 << 12) == w2
    if w:
        assert ctx.grind(state, slot, 4, 0, 1 << 12, result=w - 1) == w - 1
    # the window that ends at P: candidates >= P are never tried
    assert ctx.grind(state, slot, 0, P - 100, 256) == P - 100
    assert ctx.grind(state, slot, 0, P - 1, 256) == P - 1
    for bits in (4, 8):
        got = ctx.grind(state, slot, bits, P - 100, 256)
        assert got == RE.grind_reference(oracle, state, slot, bits, P - 100, 100) and (got < P or got == NONE)


def test_grind_window_before_the_witness_finds_nothing(ctx, oracle):
    _, state, slot = RE.grind_state(oracle, RE.LATE_SEED, RE.LATE_PENDING)
    result, launches = NONE, 0
    for base in range(0, 1 << 14, 256):
        result = ctx.grind(state, slot, RE.LATE_BITS, base, 256, result=result)
        launches += 1
        if base + 256 <= RE.LATE_WITNESS:
            assert result == NONE, base                                            # the hit lies in a later launch
        if result != NONE:
            break
    assert result == RE.LATE_WITNESS and launches == RE.LATE_WITNESS // 256 + 1 and launches >= 3
    assert ctx.grind(state, slot, RE.LATE_BITS, 0, 256 * launches) == RE.LATE_WITNESS          # one launch over all the windows: several workgroups


def test_grind_refuses_bad_arguments(ctx, oracle):
    _, state, slot = RE.grind_state(oracle, [1] * 8, 2)
    for over in (dict(slot=-1), dict(slot=8), dict(bits=-1), dict(bits=32), dict(count=0), dict(base=0xFFFFFF00, count=257)):
        a = dict(slot=slot, bits=4, base=0, count=256)
        a.update(over)
        with pytest.raises(ZkHipError) as e:
            ctx.grind(state, **a)
        assert e.value.code == -1, over


# ------------------------------------------------------------------ the captured FRI graph against plain launches
@pytest.fixture
def fri_graph():
    from zktls_amd.device import set_fri_graph
    yield set_fri_graph
    set_fri_graph(1)                                             # the library's default


def test_fri_graph_on_and_off_prove_the_same_bytes(ctx, oracle, fri_graph):
    """the graph is keyed on shapes and workspace addresses: alternating shapes on one context rebuild it (A -> B -> A), a repeated shape replays it (A -> A),
    and a two-height machine adds the injected vector's launch; every proof must be the oracle's, with the graph and with plain launches"""
    prm, oprm = Params(1, 10, 4), oracle.default_params(1, 10, 4)
    shards = {"A": (0, 8, 8), "B": (1, 10, 16)}
    chips = [(10, 16), (8, 8)]
    dev = {k: ctx.gen_trace(SEED, s, ln, w) for k, (s, ln, w) in shards.items()}
    mdev = [(ctx.gen_trace(SEED, i, ln, w), ln, w) for i, (ln, w) in enumerate(chips)]
    want = {k: oracle.prove_shard(oracle.gen_trace(SEED, s, ln, w), [1, 2], oprm).tobytes() for k, (s, ln, w) in shards.items()}
    want["M"] = oracle.prove_chips([oracle.gen_trace(SEED, i, ln, w) for i, (ln, w) in enumerate(chips)], [3, 4], oprm).tobytes()

    def prove(k):
        if k == "M":
            return ctx.prove_chips(mdev, [3, 4], prm).tobytes()
        _, ln, w = shards[k]
        return ctx.prove_shard(dev[k], ln, w, [1, 2], prm).tobytes()

    order = ["A", "B", "A", "A", "M", "A", "M", "M", "B"]
    got = {}
    for on in (1, 0):
        fri_graph(on)
        got[on] = [prove(k) for k in order]
    for i, k in enumerate(order):
        assert got[1][i] == got[0][i], "proof %d (%s): graph and plain launches differ" % (i, k)
        assert got[1][i] == want[k], "proof %d (%s) differs from the oracle's" % (i, k)
