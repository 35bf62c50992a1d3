"""The lane-per-row forms against the 16-lane forms on one device, byte for byte (GPU box):
    python tests/checks/stream_rows_ab.py
Loads the A/B build (zktls_amd/libzkhip_ab.so, never shipped), whose launchers read ZKHIP_STREAM_OLD at every launch: unset, a shape
takes the form the shipped library gives it; 1, every shape takes quotient_kernel / rowdot_regs_kernel.  Every case of stream_rows.py
runs both ways: reduced openings on the three fills, quotient values on edge alphas, whole proofs with and without lookups and lde_out.
tests/test_gpu_stream_rows.py runs this file in a child process (the suite's own process never loads the A/B build)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), ROOT]
import _ab  # noqa: E402,F401  (before anything loads the library)
import numpy as np  # noqa: E402

import reduced_edges as RE  # noqa: E402
import stream_rows as SR  # noqa: E402
import test_gpu_reduced_edges as TR  # noqa: E402
from field_edges import edge_ext, edge_matrix  # noqa: E402
from zktls_amd._lib import Params  # noqa: E402
from zktls_amd.device import Context  # noqa: E402

SEED = 0x5A4B544C53


def both(fn):
    """fn() with the dispatch as shipped, then with the 16-lane forms forced"""
    os.environ.pop("ZKHIP_STREAM_OLD", None)
    new = fn()
    os.environ["ZKHIP_STREAM_OLD"] = "1"
    try:
        old = fn()
    finally:
        del os.environ["ZKHIP_STREAM_OLD"]
    return new, old


def main():
    ctx = Context(0)
    n = 0
    for case, _, _ in SR.ROWDOT_CASES:
        for fill in RE.FILLS:
            d = RE.build(case, fill)

            def run():
                dev, out = TR._upload_case(ctx, d)
                forms = TR._run_case(ctx, d, dev, out)
                words = out.download_monty()
                for b in list(dev.values()) + [out]:
                    b.free()
                return forms, words

            (fn, wn), (fo, wo) = both(run)
            assert fn == fo == (case[7], case[8]), (case[0], fn, fo)
            assert (wn == wo).all(), "reduced opening %s / %s: the two forms differ" % (case[0], fill)
            n += 1
    for log_n, width in SR.QUOTIENT_CASES + SR.QUOTIENT_FALLBACK:
        d = ctx.from_numpy(edge_matrix(2 << log_n, width, seed=log_n))
        for alpha in edge_ext(np.random.default_rng(log_n), 1):
            new, old = both(lambda: ctx.quotient_values(d, log_n, width, alpha).download_monty())
            assert (new == old).all(), "quotient 2^%d x %d, alpha %s: the two forms differ" % (log_n, width, alpha.tolist())
            n += 1
    for shape in SR.PROOF_CASES:
        log_n, width, pairs = 10, 32, shape[3]
        trace = ctx.gen_trace_logup(SEED, 9, log_n, width, pairs) if pairs else ctx.gen_trace(SEED, 9, log_n, width)
        new, old = both(lambda: ctx.prove_shard(trace, log_n, width, [1, 2], Params(*shape)).tobytes())
        assert new == old, "proof %s: the two forms differ" % (shape,)
        n += 1
    ctx.close()
    print("stream rows A/B: %d comparisons, the lane-per-row and the 16-lane forms give the same bytes" % n)


if __name__ == "__main__":
    main()
