"""Lock-step batches (csrc/batch.h) of synthetic shards: the choices that exist only INSIDE a batch, restated in plain Python, and the
case table of test_gpu_lockstep_forms.py.  Shared with test_lockstep_forms_cpu.py (no GPU and no library call here).

Inside a batch of `members` provers
  * coop_max_nodes() (batch.cpp) is max(512, 16384 / members) instead of 16384: launch_hash_rows, launch_compress_level, op_merkle_commit and
    compress_inject_ok switch kernels at tree heights of 512 .. 8192 that the unbatched kernel suites only reach at 16384;
  * the FRI commit phase is enqueued launch by launch (no graph replay), the proof-of-work search loops until every member has voted "found";
  * dev_h2d / dev_d2h go through per-member staging rings of 8 MiB / members (up) and 48 MiB / members (down); a copy above half a region is a
    plain hipMemcpyAsync;
  * members whose traces differ in pitch or alignment ask for different NTT pass kernels and are launched group by group ("mixed").

commit_walk() is op_merkle_commit line for line, shard_forms() strings together what one prove_shard launches (pitched.py and reduced_edges.py hold
the launchers' own predicates), stage_fits() is LaunchBatcher::stage, gather_bytes() counts the two large copies of a proof (prover.cpp step 7).
CASES carries the form every case is meant to reach as a LITERAL; test_lockstep_forms_cpu.py holds the literals to these functions.
"""
import collections

import pitched as PT
import reduced_edges as RE

MIB = 1 << 20
UP_BYTES, DOWN_BYTES = 8 * MIB, 48 * MIB     # batch.cpp: the staging areas of one batch, shared out among its members
GRIND_MIN_WINDOW = 1 << 14                   # prover.cpp grind_witness: candidates per launch = max(2^14, 4 << pow_bits), at most 2^20
MIN_LOG_N = 5                                # proof_common.h check_shape: prove_shard takes 2^5 rows or more


# (log_blowup, queries, pow bits, LogUp pairs, log_fold, log_final, hash width, code width): the fields of zkhip_params in order
def params(log_blowup, queries, pow_bits, pairs=0, log_fold=0, log_final=0, hash_width=0, code_width=0):
    return (log_blowup, queries, pow_bits, pairs, log_fold, log_final, hash_width, code_width)


def segment_params(queries=50, pairs=0, log_final=8):
    """zktls_amd._lib.segment_params: blowup 4, fold by 16, Poseidon2 width 24, no proof of work"""
    return params(2, queries, 0, pairs, 4, log_final, 24, 0)


def shape_of(log_n, prm):
    """proof_common.h shape_of -> (b, K, F, hw, R)"""
    b, K, F, hw = prm[0], prm[4] or 1, prm[5], prm[6] or 16
    assert 1 <= b <= 3 and 1 <= K <= 5 and 0 <= F <= min(10, log_n) and (log_n - F) % K == 0 and hw in (16, 24) and prm[7] == 0
    return b, K, F, hw, (log_n - F) // K


def coop_bound(members):
    """batch.cpp coop_max_nodes() for a fiber of a batch of `members` (a batch of one runs without a batcher: the same 16384)"""
    return max(PT.COOP_TOP_NODES, PT.COOP_MAX_NODES // members)


def grind_window(pow_bits):
    return min(max(GRIND_MIN_WINDOW, 4 << pow_bits), 1 << 20)


def commit_walk(log_h, mats, members):
    """context.cpp op_merkle_commit, line for line: the launches of one commitment in order.  mats: (width, ld, off) per matrix"""
    bound = coop_bound(members)
    count = 1 << log_h
    if PT.COOP_TOP_NODES < count <= bound:                       # a medium tree: leaves inside the subtree launch
        rest = 128 if count >= 4096 else 32
        return ["hash_sub16(%d)" % rest, "compress_top16(%d)" % rest]
    out = [PT.hash_rows_form(count, mats, bound)]
    while count > PT.COOP_TOP_NODES:
        if count <= bound:
            rest = 128 if count >= 4096 else 32
            out.append("compress_sub16(%d)" % rest)
            count = rest
            break
        # launch_compress_level(level, next, count / 2)
        out.append(("compress_level16(%d)" if count // 2 <= bound else "compress_level(%d)") % (count // 2))
        count >>= 1
    if count > 1:                                                # launch_compress_top returns at once for a single node
        out.append("compress_top16(%d)" % count)
    return out


def _tree(log_h, width, hw, members):
    """prover.cpp commit_hw of a dense, aligned matrix"""
    return ["p24_rowmajor"] if hw == 24 else commit_walk(log_h, [(width, width, 0)], members)


def shard_forms(log_n, width, ld, off, prm, members):
    """what one prove_shard (prover.cpp prove_shard_impl) launches as a member of a batch of `members`, the trace at pitch ld with its base `off` words
    off 16-byte alignment: a dict.  Everything after the trace's LDE works on the prover's own dense, aligned workspaces."""
    assert log_n >= MIN_LOG_N and width % 4 == 0 and 0 < width <= 1024 and 8 * prm[3] <= width      # proof_common.h check_shape
    b, K, F, hw, R = shape_of(log_n, prm)
    H, pairs = log_n + b, prm[3]
    wp = 4 * (pairs + 1) if pairs else 0
    lde = PT.lde_forms(log_n, width, ld, width, off, 0, log_blowup=b)
    if lde == "lde_small":
        lde = "lde_small<%d>" % (log_n - 10)                      # ntt_small.hip launch_lde_small
    return dict(
        lde=lde,
        trace_tree=_tree(H, width, hw, members),
        perm_tree=_tree(H, wp, hw, members) if pairs else None,
        quotient_tree=_tree(H, 8, hw, members),                   # two chunks of four columns
        fri_trees=[_tree(H - K * (l + 1), 4 << K, hw, members) for l in range(R)],
        quotient=PT.quotient_form(log_n, width),
        logup=bool(pairs),
        open=PT.open_form(width, width, 0),
        rowdot=(RE.rowdot_form(width, 1 << H),) + ((RE.rowdot_form(wp, 1 << H),) if pairs else ()),
        fold=1 << K,
        hash=hw,
    )


def render(f):
    """a dict of shard_forms as the case table carries it: (trace LDE, trace tree, permutation tree, quotient tree, FRI layer trees, the rest)"""
    walk = lambda w: "-" if w is None else "+".join(w)
    fri = [walk(w) for w in f["fri_trees"]]
    small = [w[1][len("compress_top16("):-1] for w in f["fri_trees"] if len(w) == 2 and w[0] == "hash_rows16"]
    if len(small) > 1 and fri[-len(small):] == ["hash_rows16+compress_top16(%s)" % c for c in small]:      # the trees of at most 512 nodes, halving: one entry
        fri[-len(small):] = ["hash_rows16+compress_top16(%s..%s)" % (small[0], small[-1])]
    return (f["lde"], walk(f["trace_tree"]), walk(f["perm_tree"]), walk(f["quotient_tree"]), ", ".join(fri),
            "%s%s | open %s | rowdot %s | fold %d | hash %d" % (f["quotient"], " logup" if f["logup"] else "", f["open"], "/".join(str(r) for r in f["rowdot"]), f["fold"], f["hash"]))


def stage_fits(nbytes, members, direction):
    """batch.cpp LaunchBatcher::stage: does a copy of nbytes go through the member's staging ring (else hipMemcpyAsync and a merged wait)"""
    region = ({"up": UP_BYTES, "down": DOWN_BYTES}[direction] // members) & ~63
    return ((nbytes + 63) & ~63) <= region // 2


def gather_bytes(log_n, width, prm):
    """prover.cpp prove_shard_impl step 7 -> (bytes of the descriptor upload, bytes of the query-section download, bytes of the proof before the queries);
    the last from proof_common.h proof_words, so that the sum of the last two is the length of the proof"""
    b, K, F, hw, R = shape_of(log_n, prm)
    H, Q, pairs = log_n + b, prm[1], prm[3]
    wp = 4 * (pairs + 1) if pairs else 0
    descs = 1 + H + ((1 + H) if pairs else 0) + 1 + H              # a row and a path per committed matrix
    words = width + 8 * H + ((wp + 8 * H) if pairs else 0) + 8 + 8 * H
    for l in range(R):
        lh = H - K * (l + 1)
        descs += ((1 << K) - 1) + lh                               # the row's other entries, one descriptor each, and the path
        words += 4 * ((1 << K) - 1) + 8 * lh
    ext = not (b == 1 and K == 1 and F == 0 and hw == 16)
    head = (12 if ext else (9 if pairs else 8)) + 16 + 8 * width + 4 * 8 + 8 * R + 4 * (1 << F) + 1 + ((8 + 8 * wp) if pairs else 0)
    return 16 * Q * descs, 4 * Q * words, 4 * head


def batches(jobs, max_batch, lanes):
    """jobs.cpp deal_jobs_lockstep: the sizes of the batches one (log_n, width) group of `jobs` jobs is cut into (equal cuts)"""
    cuts = (jobs + max_batch - 1) // max_batch
    if cuts < lanes and jobs >= 2 * lanes:
        cuts = lanes
    return [jobs * (c + 1) // cuts - jobs * c // cuts for c in range(cuts) if jobs * (c + 1) // cuts > jobs * c // cuts]


# ---------------------------------------------------------------------------------------------- the cases
# shards: the shard id of every job (gen_trace(seed, s) per job; distinct over the whole table, so that no context of the pool holds a case's results
# from an earlier case); layouts: (ld, off) of the jobs' traces in turn (None: dense buffers straight from
# ctx.gen_trace; otherwise pitched.embed of the oracle's trace); npub: public values per job (None: [s, 7], else the first j % 4 of PUBLIC);
# host: host traces (zkhip_prove_shard_host: a plain hipMemcpyAsync on the shared stream and launch_convert, not the staging ring);
# form: render(shard_forms) per distinct layout, as members of the batches the jobs are cut into.
Case = collections.namedtuple("Case", "id log_n width prm max_batch lanes shards layouts npub host form")
SEED = 0x10C557E9
PUBLIC = (7, 8, 9)

# n6-grind: 32 jobs = two batches of sixteen (jobs 0 .. 15 and 16 .. 31).  The window is 2^14 candidates at 12 bits; the oracle's witnesses of shards 59 and 28
# (public values [s, 7]) are 18413 and 21293 -- a second window --, every other shard's lies below 2^14 (shard 29: 87): either batch holds a member that is
# done after one launch and goes on launching, and a member that needs the second.  test_lockstep_forms_cpu.py holds this on the oracle's proofs.
GRIND_SHARDS = tuple(59 if s == 5 else s for s in range(32))
GRIND_LATE = (59, 28)

# Shapes moved from the plan, each by a predicate of check_shape (proof_common.h), which every batch entry applies:
#   n5          2^3 rows are refused (log_n >= 5): small_eval_kernel, the LDE by definition, is behind no batch entry -- OUT_OF_SCOPE
#   n10-level   a width of 5 is refused (W % 4 == 0): bound 512 and the plain compress_level_kernel at width 8; `generic` leaves -- OUT_OF_SCOPE
#   n12-small / n13-small   130 -> 132 columns: at 2^12 rows lde_small_kernel<2> takes 8 columns per workgroup, 132 leaves it a half-filled last one
CASES = (
    Case("n5", 5, 8, params(1, 8, 4), 4, 1, tuple(range(100, 104)), None, None, False, (
        ("single-pass:single,single",
         "hash_rows16+compress_top16(64)",
         "-",
         "hash_rows16+compress_top16(64)",
         "hash_rows16+compress_top16(32..2)",
         "quotient_kernel<1> | open generic | rowdot 0 | fold 2 | hash 16"),)),
    Case("n6-grind", 6, 8, params(2, 10, 12, 1), 16, 2, GRIND_SHARDS, None, None, False, (
        ("single-pass:single,single",
         "hash_rows16+compress_top16(256)",
         "hash_rows16+compress_top16(256)",
         "hash_rows16+compress_top16(256)",
         "hash_rows16+compress_top16(128..4)",
         "quotient_kernel<1> logup | open generic | rowdot 0/0 | fold 2 | hash 16"),)),
    Case("n9", 9, 24, params(2, 20, 8, 1), 16, 1, tuple(range(200, 216)), None, None, False, (
        ("single-pass:single,single",
         "vec+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "vec+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "vec+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..4)",
         "quotient_kernel<1> logup | open generic | rowdot 1/1 | fold 2 | hash 16"),)),
    Case("n10-stream", 10, 32, params(1, 20, 8), 16, 1, tuple(range(300, 316)), None, None, False, (
        ("single-pass:pair,pair",
         "vec+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "-",
         "vec+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..2)",
         "stream | open generic | rowdot 1 | fold 2 | hash 16"),)),
    Case("n10-level", 10, 8, params(2, 20, 8), 32, 1, tuple(range(400, 432)), None, None, False, (
        ("single-pass:single,single",
         "vec+compress_level(2048)+compress_level(1024)+compress_level16(512)+compress_top16(512)",
         "-",
         "vec+compress_level(2048)+compress_level(1024)+compress_level16(512)+compress_top16(512)",
         "vec+compress_level(1024)+compress_level16(512)+compress_top16(512), vec+compress_level16(512)+compress_top16(512), hash_rows16+compress_top16(512..4)",
         "quotient_kernel<1> | open generic | rowdot 1 | fold 2 | hash 16"),)),
    Case("n11-eq", 11, 8, params(1, 20, 8), 4, 1, tuple(range(500, 504)), None, None, False, (
        ("I1 single, I2, F1 single, F2 single",
         "hash_sub16(128)+compress_top16(128)",
         "-",
         "hash_sub16(128)+compress_top16(128)",
         "hash_sub16(32)+compress_top16(32), hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..2)",
         "quotient_kernel<1> | open generic | rowdot 1 | fold 2 | hash 16"),)),
    Case("n11-small", 11, 128, params(1, 20, 8), 8, 1, tuple(range(600, 608)), None, None, False, (
        ("lde_small<1>",
         "vec+compress_level16(2048)+compress_sub16(32)+compress_top16(32)",
         "-",
         "vec+compress_level16(2048)+compress_sub16(32)+compress_top16(32)",
         "hash_sub16(32)+compress_top16(32), hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..2)",
         "stream | open quads | rowdot 2 | fold 2 | hash 16"),)),
    Case("n12-b3", 12, 40, params(2, 20, 8, 1), 3, 2, tuple(range(700, 706)), None, None, False, (
        ("I1 pair, I2, F1 pair, F2 pair | I1 single, I2, F1 single, F2 single",
         "vec+compress_level(8192)+compress_level16(4096)+compress_sub16(128)+compress_top16(128)",
         "vec+compress_level(8192)+compress_level16(4096)+compress_sub16(128)+compress_top16(128)",
         "vec+compress_level(8192)+compress_level16(4096)+compress_sub16(128)+compress_top16(128)",
         "vec+compress_level16(4096)+compress_sub16(128)+compress_top16(128), hash_sub16(128)+compress_top16(128), hash_sub16(32)+compress_top16(32), hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..4)",
         "quotient_kernel<1> logup | open generic | rowdot 1/1 | fold 2 | hash 16"),)),
    Case("n12-small", 12, 132, params(2, 20, 8), 16, 1, tuple(range(800, 816)), None, None, False, (
        ("lde_small<2>",
         "vec+compress_level(8192)+compress_level(4096)+compress_level(2048)+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "-",
         "vec+compress_level(8192)+compress_level(4096)+compress_level(2048)+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "vec+compress_level(4096)+compress_level(2048)+compress_level16(1024)+compress_sub16(32)+compress_top16(32), vec+compress_level(2048)+compress_level16(1024)+compress_sub16(32)+compress_top16(32), vec+compress_level16(1024)+compress_sub16(32)+compress_top16(32), hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..4)",
         "quotient_kernel<3> | open quads | rowdot 3 | fold 2 | hash 16"),)),
    Case("n13-small", 13, 132, params(1, 20, 8), 2, 1, tuple(range(900, 902)), None, None, False, (
        ("lde_small<3>",
         "vec+compress_level16(8192)+compress_sub16(128)+compress_top16(128)",
         "-",
         "vec+compress_level16(8192)+compress_sub16(128)+compress_top16(128)",
         "hash_sub16(128)+compress_top16(128), hash_sub16(128)+compress_top16(128), hash_sub16(32)+compress_top16(32), hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..2)",
         "quotient_kernel<3> | open quads | rowdot 3 | fold 2 | hash 16"),)),
    Case("n9-wide", 9, 512, params(1, 100, 8), 64, 1, tuple(range(1000, 1064)), None, None, False, (
        ("single-pass:pair,pair",
         "vec+compress_level16(512)+compress_top16(512)",
         "-",
         "vec+compress_level16(512)+compress_top16(512)",
         "hash_rows16+compress_top16(512..2)",
         "quotient_kernel<8> | open quads | rowdot 0 | fold 2 | hash 16"),)),
    Case("r0", 10, 16, segment_params(50, 0, 2), 8, 1, tuple(range(1100, 1108)), None, None, False, (
        ("single-pass:single,single",
         "p24_rowmajor",
         "-",
         "p24_rowmajor",
         "p24_rowmajor, p24_rowmajor",
         "quotient_kernel<1> | open generic | rowdot 1 | fold 16 | hash 24"),)),
    Case("mixed", 10, 32, params(1, 20, 8), 4, 1, tuple(range(1200, 1204)), ((32, 0), (36, 0), (33, 0), (32, 1)), "cycle", False, (
        ("single-pass:pair,pair",
         "hash_sub16(32)+compress_top16(32)",
         "-",
         "hash_sub16(32)+compress_top16(32)",
         "hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..2)",
         "stream | open generic | rowdot 1 | fold 2 | hash 16"),
        ("single-pass:single,pair",
         "hash_sub16(32)+compress_top16(32)",
         "-",
         "hash_sub16(32)+compress_top16(32)",
         "hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..2)",
         "stream | open generic | rowdot 1 | fold 2 | hash 16"),)),
    Case("cuts-2of3", 6, 8, params(1, 8, 4), 2, 1, tuple(range(1300, 1303)), None, None, False, (
        ("single-pass:single,single",
         "hash_rows16+compress_top16(128)",
         "-",
         "hash_rows16+compress_top16(128)",
         "hash_rows16+compress_top16(64..2)",
         "quotient_kernel<1> | open generic | rowdot 0 | fold 2 | hash 16"),)),
    Case("cuts-4of5", 6, 8, params(1, 8, 4), 4, 1, tuple(range(1400, 1405)), None, None, False, (
        ("single-pass:single,single",
         "hash_rows16+compress_top16(128)",
         "-",
         "hash_rows16+compress_top16(128)",
         "hash_rows16+compress_top16(64..2)",
         "quotient_kernel<1> | open generic | rowdot 0 | fold 2 | hash 16"),)),
    Case("host-n9", 9, 24, params(1, 20, 8), 16, 1, tuple(range(1500, 1516)), None, None, True, (
        ("single-pass:single,single",
         "hash_sub16(32)+compress_top16(32)",
         "-",
         "hash_sub16(32)+compress_top16(32)",
         "hash_rows16+compress_top16(512..2)",
         "quotient_kernel<1> | open generic | rowdot 1 | fold 2 | hash 16"),)),
    Case("host-n11", 11, 128, params(1, 20, 8), 16, 1, tuple(range(1600, 1616)), None, None, True, (
        ("lde_small<1>",
         "vec+compress_level(2048)+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "-",
         "vec+compress_level(2048)+compress_level16(1024)+compress_sub16(32)+compress_top16(32)",
         "vec+compress_level16(1024)+compress_sub16(32)+compress_top16(32), hash_sub16(32)+compress_top16(32), hash_rows16+compress_top16(512..2)",
         "stream | open quads | rowdot 2 | fold 2 | hash 16"),)),
)


def case(id):
    return next(c for c in CASES if c.id == id)


def members_of(c):
    """the sizes of the batches the case's jobs run in"""
    return batches(len(c.shards), c.max_batch, c.lanes)


def layout(c, j):
    """(ld, off) of job j's trace"""
    return c.layouts[j % len(c.layouts)] if c.layouts else (c.width, 0)


def public_values(c, j):
    return list(PUBLIC[:j % 4]) if c.npub else [c.shards[j], 7]


# The two large copies of a proof (gather_bytes) on either side of stage_fits: (case, copy, bytes, members, direction, staged).  Sixty-four members leave a
# member 128 KiB up and 768 KiB down; a copy of more than half of that is hipMemcpyAsync and a merged wait.
STAGING = (
    ("n9-wide", "descriptors", 121600, 64, "up", False),
    ("n9-wide", "queries", 430400, 64, "down", False),
    ("n10-stream", "descriptors", 28480, 16, "up", True),
    ("n10-stream", "queries", 55680, 16, "down", True),
    ("n12-small", "descriptors", 42240, 16, "up", True),
    ("n12-small", "queries", 90560, 16, "down", True),
)
# host traces: 2^9 x 24 words = 48 KiB (within half of a sixteenth of the up ring, 256 KiB) and 2^11 x 128 words = 1 MiB (beyond it).  zkhip_prove_shard_host
# uploads with hipMemcpyAsync on the shared stream whatever the size -- it does not ask the ring --, so both cases run the same copy today; the sizes
# are those at which a staged upload would take either side.
HOST_TRACE_BYTES = {"host-n9": 49152, "host-n11": 1 << 20}

# What a synthetic prove_shards cannot reach under 2^24 cells, with the predicate and the test that runs it:
OUT_OF_SCOPE = {
    "mvec": "launch_hash_rows takes it for two or more matrices; commit_hw commits one -- the machines' op_merkle_commit_mixed in a batch: test_gpu_lockstep.py::test_transcripts_in_lockstep_are_the_same_bytes",
    "compress_inject_mvec": "op_merkle_commit_mixed alone (matrices of several heights): test_gpu_lockstep.py::test_transcripts_in_lockstep_are_the_same_bytes",
    "inject": "op_merkle_commit_mixed alone: test_gpu_lockstep.py::test_transcripts_in_lockstep_are_the_same_bytes",
    "generic": "check_shape requires W % 4 == 0 and every committed matrix is a dense, aligned workspace of width W, 4 (pairs + 1), 8 or 4 * 2^K: no batch entry reaches it; unbatched: test_gpu_pitched.py::test_hash_rows_on_pitched_rows_and_column_slices",
    "small_eval": "check_shape requires log_n >= 5; unbatched: test_gpu_pitched.py::test_dft_on_pitched_rows",
}
