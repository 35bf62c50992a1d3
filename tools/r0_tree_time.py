#!/usr/bin/env python3
"""One join against the tree above the join, in full size: N GPU-made 2^20 x 128 segment proofs at ZKHIP_PARAMS_RISC0, lifted ONCE (zkhip_prove_fri16_lift_batch), then
  (A) ONE zkhip_prove_fri16_join of all N (only while one join takes N: skipped with --tree-only, and by itself beyond zkhip_fri16_join_max_proofs),
  (B) zkhip_prove_fri16_tree at join sizes 16 and 32 (--join-sizes), four joins in flight, the last join padded by repeating the last lift proof,
in one process, after one warm-up of each form (allocations, the pooled contexts' keys), alternating A and B for --rounds rounds.  A host clock around calls that end
in a synchronise; prints ms per form and round, then min - max.  Every tree top is checked by zkhip_verify_fri16_tree once.  Not a test.
    python tools/r0_tree_time.py [N = 64] [--join-sizes 16,32] [--rounds 3] [--tree-only] [--log-n 20] [--width 128] [--ab]
Run it once per N, each run under a time limit of its own, e.g. `timeout -k 10 900 python tools/r0_tree_time.py 64`, `... 128 --tree-only`.
ZKHIP_REC_TIMING=1 with --ab prints machine mode's sections for every join and top."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=64)
ap.add_argument("--join-sizes", default="16,32")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tree-only", action="store_true")
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--width", type=int, default=128)
ap.add_argument("--ab", action="store_true")
args = ap.parse_args()
if args.ab:
    import _ab  # noqa: E402,F401
from zktls_amd._lib import Params, segment_params  # noqa: E402
from zktls_amd.device import (Context, fri16_join_max_proofs, fri16_tree_max_join, fri16_tree_max_joins, prove_fri16_lift_batch, verify_fri16_join,  # noqa: E402
                              verify_fri16_tree)

SEED = 0x5A4B544C53
n, log_n, width = args.n, args.log_n, args.width
sp = segment_params()                                       # ZKHIP_PARAMS_RISC0: blowup 4, 50 queries, fold by 16, 2^8 final coefficients, width-24 hash
prm = Params(1, 100, 16)                                    # the lift's, the joins' and the top's outer parameters
NP = 9                                                      # request digest | segment index, as the host mirror's segments carry
S = ((log_n - int(sp.log_final)) // 4, int(sp.log_final), int(sp.log_blowup), int(sp.num_queries), int(sp.pow_bits), width, NP)
ms = lambda t0: (time.perf_counter() - t0) * 1e3
most, most_tree = fri16_join_max_proofs(*S, prm), fri16_tree_max_join(*S, prm, prm)
print("lift shape (R, F, log_blowup, Q, pow_bits, W, NP) = %s, %d segments; one join takes %d, a join under a top %d" % (S, n, most, most_tree), flush=True)
sizes = [int(x) for x in args.join_sizes.split(",") if x]
for J in sizes:
    joins = fri16_tree_max_joins(*S, J, prm, prm)
    print("joins of %d: one top takes %d of them (%d segments)" % (J, joins, J * joins), flush=True)
    assert J <= most_tree and (n + J - 1) // J <= joins, "the tree does not take %d segments in joins of %d" % (n, J)
ctx = Context(0)
pubs = [[1, 2, 3, 4, 5, 6, 7, 8, s] for s in range(n)]
trace = ctx.gen_trace(SEED, 0, log_n, width)
segs = []
t0 = time.perf_counter()
for s in range(n):
    ctx.gen_trace(SEED, s, log_n, width, out=trace)
    segs.append(ctx.prove_shard(trace, log_n, width, pubs[s], sp))
print("core: %d segment proofs %.1f ms" % (n, ms(t0)), flush=True)
trace.free()
t0 = time.perf_counter()
lifted, statuses, _ = prove_fri16_lift_batch([0], segs, log_n, width, pubs, sp, prm, in_flight=4)
assert statuses == [0] * n
print("lift: one batch call %.1f ms (%d bytes per lift proof)" % (ms(t0), lifted[0].size), flush=True)
del segs
one_join = not args.tree_only and n <= most
jkey = ctx.fri16_join_setup(*S, n, prm, prm) if one_join else None
trees = {}
for J in sizes:
    n_joins = (n + J - 1) // J
    jk = ctx.fri16_join_setup(*S, J, prm, prm)              # (the joins' key: the batch's pooled contexts make their own; this one gives the root)
    jvk = jk.root.tolist()
    jk.close()
    pad = n_joins * J - n
    trees[J] = dict(n_joins=n_joins, jvk=jvk, tkey=ctx.fri16_tree_setup(*S, J, jvk, n_joins, prm, prm, prm), lifted=lifted + [lifted[-1]] * pad, pubs=pubs + [pubs[-1]] * pad)


def join():
    return ctx.prove_fri16_join(jkey, *S, lifted, pubs, prm, prm)


def tree(J):
    t = trees[J]
    return ctx.prove_fri16_tree(t["tkey"], *S, t["lifted"], J, t["pubs"], t["jvk"], prm, prm, prm, devices=[0], in_flight=4)[0]


times = {}
if one_join:                                                # warm-up of each form, checked once
    t0 = time.perf_counter()
    ref = join()
    print("warm-up: one join of %d %.1f ms (%d bytes)" % (n, ms(t0), ref.size), flush=True)
    assert verify_fri16_join(ref, pubs, *S, n, jkey.root, prm, prm) == (0, 0)
    times["one join of %d" % n] = []
for J in sizes:
    t0 = time.perf_counter()
    top = tree(J)
    t = trees[J]
    print("warm-up: tree, %d joins of %d %.1f ms (top %d bytes)" % (t["n_joins"], J, ms(t0), top.size), flush=True)
    assert verify_fri16_tree(top, t["pubs"], *S, J, t["jvk"], t["n_joins"], t["tkey"].root, prm, prm, prm) == (0, 0)
    t["top"] = top.tobytes()
    times["tree, joins of %d" % J] = []
for rnd in range(args.rounds):
    line = []
    if one_join:
        t0 = time.perf_counter()
        a = join()
        times["one join of %d" % n].append(ms(t0))
        assert a.tobytes() == ref.tobytes()
        line.append("one join of %d %.1f ms" % (n, times["one join of %d" % n][-1]))
    for J in sizes:
        t0 = time.perf_counter()
        b = tree(J)
        times["tree, joins of %d" % J].append(ms(t0))
        assert b.tobytes() == trees[J]["top"]
        line.append("tree, %d joins of %d, 4 in flight %.1f ms" % (trees[J]["n_joins"], J, times["tree, joins of %d" % J][-1]))
    print("round %d: %s" % (rnd, " | ".join(line)), flush=True)
for k, v in times.items():
    print("N = %d, %-18s: min %.1f  max %.1f  spread %.1f ms" % (n, k, min(v), max(v), max(v) - min(v)), flush=True)
if jkey is not None:
    jkey.close()
for t in trees.values():
    t["tkey"].close()
ctx.close()
