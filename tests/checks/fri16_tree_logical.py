#!/usr/bin/env python3
"""The tree above the fold-16 join over TWO LOGICAL devices of a box with one GPU.

Run as a fresh process (tests/test_gpu_fri16_tree.py does, and so can a person):
    ZKHIP_LOGICAL_DEVICES=2 python tests/checks/fri16_tree_logical.py
It loads the A/B build (see multi_device_logical.py): device ordinals 0 and 1 are two logical devices with their own context pools and workers.  Four GPU-made
segment proofs at 2^10 x 16 are lifted, then joined in twos and put under one top with the joins dealt over [0, 1] and over [0]: the same bytes.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
K = int(os.environ.setdefault("ZKHIP_LOGICAL_DEVICES", "2"))
import _ab  # noqa: E402,F401  (before anything loads the library)
import numpy as np  # noqa: E402
import oracle_lib as O  # noqa: E402
from zktls_amd import _lib  # noqa: E402
from zktls_amd._lib import Params, segment_params  # noqa: E402
from zktls_amd.device import Context, prove_fri16_join_batch, verify_fri16_tree  # noqa: E402

SEED = 0x5A4B544C53


def main():
    O.build()
    out = {"logical_devices": _lib.device_count()}
    assert out["logical_devices"] == K == 2, "the A/B library does not report two logical devices"
    log_n, width, sp = 10, 16, segment_params(12, 0, 2)
    lift, join, top = Params(1, 12, 4), Params(1, 8, 2), Params(1, 8, 2)
    S = ((log_n - int(sp.log_final)) // 4, int(sp.log_final), int(sp.log_blowup), int(sp.num_queries), int(sp.pow_bits), width, 1)
    pubs = [[7], [8], [9], [10]]
    ctx = Context(0)
    lkey = ctx.fri16_lift_key(*S, lift)
    lifted = []
    for pub, shard in zip(pubs, (3, 4, 5, 6)):
        cols = ctx.from_numpy(np.ascontiguousarray(O.gen_trace(SEED, shard, log_n, width).T))
        seg = ctx.prove_segment(cols, log_n, width, pub, sp)
        cols.free()
        lifted.append(ctx.prove_fri16_lift_segment(lkey, seg, log_n, width, pub, sp, lift))
    lkey.close()
    one, vk1 = prove_fri16_join_batch(lifted, 2, pubs, *S, lift, join, devices=[0], in_flight=2)
    two, vk2 = prove_fri16_join_batch(lifted, 2, pubs, *S, lift, join, devices=[0, 1], in_flight=2, verify=True)
    assert vk1.tolist() == vk2.tolist() and [x.tobytes() for x in one] == [x.tobytes() for x in two]
    out["joins_over_two_devices_same_bytes"] = True
    tkey = ctx.fri16_tree_setup(*S, 2, vk1, 2, lift, join, top)
    t1, j1 = ctx.prove_fri16_tree(tkey, *S, lifted, 2, pubs, vk1, lift, join, top, devices=[0])
    t2, j2 = ctx.prove_fri16_tree(tkey, *S, lifted, 2, pubs, vk1, lift, join, top, devices=[0, 1])
    t3, _ = ctx.prove_fri16_tree(tkey, *S, lifted, 2, pubs, vk1, lift, join, top, devices=None)
    assert t1.tobytes() == t2.tobytes() == t3.tobytes() and [x.tobytes() for x in j1] == [x.tobytes() for x in j2] == [x.tobytes() for x in one]
    out["top_over_two_devices_same_bytes"] = True
    out["top_accepted"] = verify_fri16_tree(t2, pubs, *S, 2, vk1, 2, tkey.root, lift, join, top) == (0, 0)
    tkey.close()
    ctx.close()
    _lib.load().zkhip_release_cached_contexts()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
