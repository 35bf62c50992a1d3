#!/usr/bin/env python3
"""RISC Zero's call in full size (segments -> lift -> join): n GPU-made 2^20 x 128 segment proofs at ZKHIP_PARAMS_RISC0, each lifted, the lift proofs joined.
Prints ms for the segments (core), the lifts, the join, the one-call entry (zkhip_prove_fri16_join_segments), and the proof bytes in and out.  Not a test.
    python tools/r0_join_time.py [n_segments = 4] [--log-n 20] [--width 128] [--reps 3] [--ab] [--host-witnesses]
--host-witnesses: zkhip_recursion_witnesses_on_host(1) -- the join's witness tables (EVAL's rows among them) from the host's walk, the comparison.
--ab: the A/B build (ZKHIP_REC_SECTIONS=1 then prints the host sections of every inner proof's tables, ZKHIP_REC_TIMING=1 the laps of the machine's proof)."""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ab", action="store_true")
ap.add_argument("--host-witnesses", action="store_true")
args = ap.parse_args()
if args.ab:
    import _ab  # noqa: E402,F401
from zktls_amd._lib import Params, segment_params  # noqa: E402
from zktls_amd.device import Context, fri16_join_max_proofs, recursion_witnesses_on_host, verify_fri16_join  # noqa: E402

SEED = 0x5A4B544C53
n, log_n, width = args.n, args.log_n, args.width
sp = segment_params()                                       # ZKHIP_PARAMS_RISC0: blowup 4, 50 queries, fold by 16, 2^8 final coefficients, width-24 hash
lift = join = Params(1, 50, 16)
S = ((log_n - int(sp.log_final)) // 4, int(sp.log_final), int(sp.log_blowup), int(sp.num_queries), int(sp.pow_bits), width, 3)
ms = lambda t0: (time.perf_counter() - t0) * 1e3
ctx = Context(0)
recursion_witnesses_on_host(1 if args.host_witnesses else 0)
print("lift shape (R, F, log_blowup, Q, pow_bits, W, NP) = %s; one join takes up to %d lift proofs" % (S, fri16_join_max_proofs(*S, lift)), flush=True)
pubs = [[1, 2, 30 + s] for s in range(n)]
trace = ctx.gen_trace(SEED, 0, log_n, width)
lkey, jkey = ctx.fri16_lift_key(*S, lift), ctx.fri16_join_setup(*S, n, lift, join)
for rep in range(args.reps):
    t0 = time.perf_counter()
    segs = []
    for s in range(n):
        ctx.gen_trace(SEED, s, log_n, width, out=trace)
        segs.append(ctx.prove_shard(trace, log_n, width, pubs[s], sp))
    t_core = ms(t0)
    t0 = time.perf_counter()
    lifted = [ctx.prove_fri16_lift_segment(lkey, p, log_n, width, pv, sp, lift) for p, pv in zip(segs, pubs)]
    t_lift = ms(t0)
    t0 = time.perf_counter()
    joined = ctx.prove_fri16_join(jkey, *S, lifted, pubs, lift, join)
    t_join = ms(t0)
    t0 = time.perf_counter()
    one = ctx.prove_fri16_join_segments(lkey, jkey, segs, log_n, width, pubs, sp, lift, join)
    t_one = ms(t0)
    assert one.tobytes() == joined.tobytes() and verify_fri16_join(joined, pubs, *S, n, jkey.root, lift, join) == (0, 0)
    print("rep %d: core %d segments %.1f ms | %d lifts %.1f ms | join %.1f ms | one call (lifts + join) %.1f ms | bytes: segments %d, lift proofs %d, joined %d"
          % (rep, n, t_core, n, t_lift, t_join, t_one, sum(p.size for p in segs), sum(p.size for p in lifted), joined.size), flush=True)
lkey.close(), jkey.close()
ctx.close()
