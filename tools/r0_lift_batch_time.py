#!/usr/bin/env python3
"""The lift step of RISC Zero's call in full size, one after the other against one batch call: N GPU-made 2^20 x 128 segment proofs at ZKHIP_PARAMS_RISC0, lifted
  (a) by N calls of zkhip_prove_fri16_lift_segment on one context (what zkhip_prove_fri16_join_segments does),
  (b) by ONE call of zkhip_prove_fri16_lift_batch over the lock-step lanes,
  (c) by ONE call of zkhip_prove_fri16_lift_batch with the lanes off (zkhip_set_lockstep(0, 0): one context per worker, four in flight),
in one process, after a warm-up of each form, alternating (a) (b) (c) for --rounds rounds.  Prints ms per form and round, the batch call's zkhip_lockstep_stats
(merged launches, member requests, mixed rounds) and whether every batch proof is form (a)'s bytes.  Not a test.
    python tools/r0_lift_batch_time.py [N = 4] [--log-n 20] [--width 128] [--rounds 3] [--ab]
Run it once per N (4, 16, 64), each run under a time limit of its own, e.g. `timeout -k 10 600 python tools/r0_lift_batch_time.py 64`."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=4)
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--width", type=int, default=128)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--ab", action="store_true")
args = ap.parse_args()
if args.ab:
    import _ab  # noqa: E402,F401
from zktls_amd._lib import Params, segment_params  # noqa: E402
from zktls_amd.device import Context, lockstep_stats, prove_fri16_lift_batch, set_lockstep  # noqa: E402

SEED = 0x5A4B544C53
n, log_n, width = args.n, args.log_n, args.width
sp = segment_params()                                       # ZKHIP_PARAMS_RISC0: blowup 4, 50 queries, fold by 16, 2^8 final coefficients, width-24 hash
lift = Params(1, 50, 16)
S = ((log_n - int(sp.log_final)) // 4, int(sp.log_final), int(sp.log_blowup), int(sp.num_queries), int(sp.pow_bits), width, 3)
ms = lambda t0: (time.perf_counter() - t0) * 1e3
ctx = Context(0)
print("lift shape (R, F, log_blowup, Q, pow_bits, W, NP) = %s, %d segments" % (S, n), flush=True)
pubs = [[1, 2, 30 + s] for s in range(n)]
trace = ctx.gen_trace(SEED, 0, log_n, width)
segs = []
t0 = time.perf_counter()
for s in range(n):
    ctx.gen_trace(SEED, s, log_n, width, out=trace)
    segs.append(ctx.prove_shard(trace, log_n, width, pubs[s], sp))
print("core: %d segment proofs %.1f ms (%d bytes)" % (n, ms(t0), sum(p.size for p in segs)), flush=True)
trace.free()
lkey = ctx.fri16_lift_key(*S, lift)


def sequential():
    return [ctx.prove_fri16_lift_segment(lkey, p, log_n, width, pv, sp, lift) for p, pv in zip(segs, pubs)]


def batch(lanes_on):
    set_lockstep(16 if lanes_on else 0, 6 if lanes_on else 0)
    try:
        s0 = lockstep_stats()
        proofs, statuses, vk = prove_fri16_lift_batch([0], segs, log_n, width, pubs, sp, lift, in_flight=4)
        s1 = lockstep_stats()
    finally:
        set_lockstep(16, 6)
    assert statuses == [0] * n and vk.tolist() == lkey.root.tolist()
    return proofs, tuple(b - a for a, b in zip(s0, s1))


ref = sequential()                                          # warm-up of each form (allocations, programs, the pooled contexts' keys)
for on in (True, False):
    got, _ = batch(on)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ref, got)), "a batch proof is not the unbatched prover's bytes"
times = {"sequential": [], "lanes": [], "in-flight 4": []}
for rnd in range(args.rounds):
    t0 = time.perf_counter()
    a = sequential()
    times["sequential"].append(ms(t0))
    t0 = time.perf_counter()
    b, st = batch(True)
    times["lanes"].append(ms(t0))
    t0 = time.perf_counter()
    c, _ = batch(False)
    times["in-flight 4"].append(ms(t0))
    same = all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(a, b, c))
    print("round %d: %d lift-segment calls %.1f ms | one batch call, lock-step lanes %.1f ms (%d merged launches, %d member requests, %d mixed rounds) | "
          "one batch call, lanes off, 4 in flight %.1f ms | same bytes: %s"
          % (rnd, n, times["sequential"][-1], times["lanes"][-1], st[0], st[1], st[2], times["in-flight 4"][-1], same), flush=True)
    assert same
for k, v in times.items():
    print("N = %d, %-11s: min %.1f  max %.1f  spread %.1f ms  (%.2f ms per lift at the minimum)" % (n, k, min(v), max(v), max(v) - min(v), min(v) / n), flush=True)
lkey.close()
ctx.close()
