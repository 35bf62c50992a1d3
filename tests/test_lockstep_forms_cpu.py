"""tests/lockstep_forms.py without a GPU: the case table of test_gpu_lockstep_forms.py held to the restated in-batch predicates (a case that
silently stops reaching its kernels shows up here, in review), the proof-of-work condition of n6-grind and the byte counts of the staged
copies held on the oracle's proofs."""
import numpy as np
import pytest

import lockstep_forms as LF
import pitched as PT
import pyverify

ALL = [pytest.param(c, id=c.id) for c in LF.CASES]


def _oparams(oracle, prm):
    return oracle.Params(*prm)


def _forms(c, members):
    seen = []
    for ld, off in (c.layouts or ((c.width, 0),)):
        f = LF.render(LF.shard_forms(c.log_n, c.width, ld, off, c.prm, members))
        if f not in seen:
            seen.append(f)
    return tuple(seen)


@pytest.mark.parametrize("c", ALL)
def test_cases_reach_the_forms_they_name(c):
    sizes = LF.members_of(c)
    assert sum(sizes) == len(c.shards) == len(set(c.shards)) and max(sizes) <= c.max_batch
    assert (c.width << c.log_n) <= 1 << 24 and len(c.shards) >= 2                      # jobs.cpp: small jobs, and at least two of them
    for members in set(sizes):
        assert _forms(c, members) == c.form, (c.id, members)


def test_the_table_holds_every_intent():
    """the union over the table: every in-batch choice the plan names, by the launch that shows it"""
    forms = {c.id: c.form for c in LF.CASES}
    walks = {cid: [w for f in fs for field in f[1:5] for w in field.split(", ")] for cid, fs in forms.items()}
    every = [w for ws in walks.values() for w in ws]
    launches = {l for w in every for l in w.split("+")}
    bound = lambda cid: LF.coop_bound(max(LF.members_of(LF.case(cid))))
    # leaves: the 16-lane kernel, the subtree launch with both values of rest, the vec kernel at 2^10 .. 2^14 rows
    for want in ("hash_rows16", "vec", "hash_sub16(32)", "hash_sub16(128)", "compress_sub16(32)", "compress_sub16(128)", "p24_rowmajor"):
        assert want in launches, want
    assert {"compress_level(%d)" % n for n in (1024, 2048, 4096, 8192)} <= launches       # the plain level kernel below 16384
    assert {"compress_level16(%d)" % n for n in (512, 1024, 2048, 4096, 8192)} <= launches
    assert "compress_top16(512)" in launches and "compress_top16(512..2)" in launches      # one workgroup, from a full top down to two nodes
    # n5: trees of at most 512 nodes only; n9: the LDE is twice the bound, the first height whose leaves leave hash_rows16
    assert all(w.startswith("hash_rows16+compress_top16(") for w in walks["n5"] if w != "-")
    assert bound("n9") == 1024 and forms["n9"][0][1].startswith("vec+compress_level16(1024)") and forms["n9"][0][5].endswith("logup | open generic | rowdot 1/1 | fold 2 | hash 16")
    # bounds: 512 (32 and 64 members), equal to the tree (n11-eq), not a power of two (n12-b3: a level above it and a level below it in one tree), 8192
    assert bound("n10-level") == bound("n9-wide") == 512 and bound("n13-small") == 8192
    assert bound("n11-eq") == 1 << 12 and forms["n11-eq"][0][1] == "hash_sub16(128)+compress_top16(128)"
    assert bound("n12-b3") == 5461 and "compress_level(8192)+compress_level16(4096)+compress_sub16(128)" in forms["n12-b3"][0][1]
    # LDE: one pass single and pair, two passes with one column per lane, the 32 + 8 split, the three small kernels
    ldes = {cid: fs[0][0] for cid, fs in forms.items()}
    assert ldes["n6-grind"] == "single-pass:single,single" and ldes["n10-stream"] == "single-pass:pair,pair"
    assert ldes["n11-eq"] == "I1 single, I2, F1 single, F2 single"
    assert ldes["n12-b3"] == "I1 pair, I2, F1 pair, F2 pair | I1 single, I2, F1 single, F2 single"
    assert (ldes["n11-small"], ldes["n12-small"], ldes["n13-small"]) == ("lde_small<1>", "lde_small<2>", "lde_small<3>")
    assert LF.case("n12-small").prm[0] == 2 and LF.case("n12-small").width % 8 == 4       # four cosets; a half-filled last column group
    # quotient, LogUp, openings, fold, hash
    rest = {cid: fs[0][5] for cid, fs in forms.items()}
    assert rest["n10-stream"].startswith("stream") and 2 << LF.case("n10-stream").log_n == PT.STREAM_MIN_ROWS
    assert rest["n9-wide"].startswith("quotient_kernel<8> | open quads")
    assert "logup" in rest["n6-grind"] and "logup" in rest["n12-b3"] and "logup" not in rest["n10-stream"]
    assert "open quads" in rest["n11-small"] and "open generic" in rest["n9"]
    assert rest["r0"].endswith("fold 16 | hash 24") and forms["r0"][0][4] == "p24_rowmajor, p24_rowmajor"
    assert {r.split("rowdot ")[1].split(" ")[0] for r in rest.values()} >= {"0", "1", "2", "3", "0/0", "1/1"}
    # the largest case: 64 members of 2^18 cells
    assert max(len(c.shards) * (c.width << c.log_n) for c in LF.CASES) == 64 << 18
    # out of scope, named with the tests that run them
    assert set(LF.OUT_OF_SCOPE) == {"mvec", "compress_inject_mvec", "inject", "generic", "small_eval"}
    assert not {"mvec", "generic", "inject", "compress_inject_mvec"} & launches
    with pytest.raises(AssertionError):
        LF.shard_forms(3, 8, 8, 0, LF.params(1, 8, 4), 4)                                  # the plan's 2^3 x 8
    with pytest.raises(AssertionError):
        LF.shard_forms(10, 5, 5, 0, LF.params(2, 20, 8), 32)                               # and its 2^10 x 5


def test_the_cuts_and_the_mixed_layouts():
    ids = [s for c in LF.CASES for s in c.shards]
    assert len(ids) == len(set(ids))                                                       # no case finds another case's results in a pooled context
    assert LF.members_of(LF.case("cuts-2of3")) == [1, 2]                                   # a batch of one (the solo path) beside a merged one
    assert LF.members_of(LF.case("cuts-4of5")) == [2, 3]
    assert LF.members_of(LF.case("n6-grind")) == [16, 16] and LF.members_of(LF.case("n12-b3")) == [3, 3] and LF.members_of(LF.case("n9-wide")) == [64]
    assert LF.batches(64, 16, 6) == [10, 11, 11, 10, 11, 11] and LF.batches(16, 16, 6) == [2, 3, 3, 2, 3, 3] and LF.batches(5, 16, 6) == [5]
    c = LF.case("mixed")
    assert len(LF.members_of(c)) == 1
    # the prover's LDE is dense and aligned: (log_n, W, in_ld, out_ld = W, in_off, out_off = 0)
    ldes = [PT.lde_forms(c.log_n, c.width, LF.layout(c, j)[0], c.width, LF.layout(c, j)[1], 0) for j in range(len(c.shards))]
    assert ldes == ["single-pass:pair,pair", "single-pass:pair,pair", "single-pass:single,pair", "single-pass:single,pair"]
    assert sorted(len(LF.public_values(c, j)) for j in range(4)) == [0, 1, 2, 3]
    assert [LF.layout(c, j) for j in range(4)] == [(32, 0), (36, 0), (33, 0), (32, 1)]


def test_the_restated_predicates_on_their_own_edges():
    assert [LF.coop_bound(m) for m in (1, 2, 3, 4, 5, 6, 8, 16, 32, 33, 64, 256)] == [16384, 8192, 5461, 4096, 3276, 2730, 2048, 1024, 512, 512, 512, 512]
    m8 = [(8, 8, 0)]
    assert LF.commit_walk(9, m8, 16) == ["hash_rows16", "compress_top16(512)"] and LF.commit_walk(0, m8, 16) == ["hash_rows16"]
    assert LF.commit_walk(10, m8, 16) == ["hash_sub16(32)", "compress_top16(32)"] and LF.commit_walk(10, m8, 17) == ["vec", "compress_level16(512)", "compress_top16(512)"]
    assert LF.commit_walk(14, m8, 1) == ["hash_sub16(128)", "compress_top16(128)"]
    assert LF.commit_walk(15, m8, 1) == ["vec", "compress_level16(16384)", "compress_sub16(128)", "compress_top16(128)"]
    assert LF.commit_walk(16, [(6, 6, 0)], 1) == ["generic", "compress_level(32768)", "compress_level16(16384)", "compress_sub16(128)", "compress_top16(128)"]
    assert LF.commit_walk(12, m8, 5) == ["vec", "compress_level16(2048)", "compress_sub16(32)", "compress_top16(32)"]      # bound 3276
    # the defaults of pitched.py's three forms are the unbatched bound
    assert PT.hash_rows_form(1024, m8) == "hash_rows16" and PT.hash_rows_form(1024, m8, 512) == "vec" and PT.hash_rows_form(1024, m8, 1024) == "hash_rows16"
    assert PT.merkle_commit_form(12, m8) == "hash_sub16" and PT.merkle_commit_form(12, m8, 2048) == "vec" and PT.merkle_commit_form(9, m8, 512) == "hash_rows16"
    assert PT.inject_form(2048, m8) == "level+hash_rows16+inject" and PT.inject_form(2048, m8, 1024) == "compress_inject_mvec"
    assert PT.inject_form(2048, [(6, 6, 0)], 1024) == "level+generic+inject"
    # staging: regions of 8 MiB / members up, 48 MiB / members down, rounded down to 64 bytes; a copy fits up to half a region
    assert LF.stage_fits(4 << 20, 1, "up") and not LF.stage_fits((4 << 20) + 1, 1, "up")
    assert LF.stage_fits(65536, 64, "up") and not LF.stage_fits(65537, 64, "up") and LF.stage_fits(393216, 64, "down") and not LF.stage_fits(393217, 64, "down")
    assert LF.stage_fits(1398080, 3, "up") and not LF.stage_fits(1398081, 3, "up")         # (8 MiB / 3) & ~63 = 2796160
    assert LF.grind_window(12) == 1 << 14 and LF.grind_window(13) == 1 << 15 and LF.grind_window(4) == 1 << 14 and LF.grind_window(28) == 1 << 20


def test_the_staging_sides_on_the_oracles_proofs(oracle):
    seen = set()
    for cid, what, nbytes, members, direction, staged in LF.STAGING:
        c = LF.case(cid)
        assert members == max(LF.members_of(c))
        desc, query, head = LF.gather_bytes(c.log_n, c.width, c.prm)
        assert nbytes == {"descriptors": desc, "queries": query}[what] and direction == {"descriptors": "up", "queries": "down"}[what]
        assert LF.stage_fits(nbytes, members, direction) == staged
        seen.add((what, staged))
        proof = oracle.prove_shard(oracle.gen_trace(LF.SEED, c.shards[0], c.log_n, c.width), LF.public_values(c, 0), _oparams(oracle, c.prm))
        assert head + query == len(proof), (cid, head, query, len(proof))
    assert seen == {(w, s) for w in ("descriptors", "queries") for s in (True, False)}
    # every case: the restated counts add up to the oracle's proof length (LogUp, blowup 4, fold by 16 included)
    for c in LF.CASES:
        if c.log_n <= 10 and c.width <= 32:
            make = oracle.gen_trace_logup if c.prm[3] else oracle.gen_trace
            trace = make(LF.SEED, c.shards[0], c.log_n, c.width, *([c.prm[3]] if c.prm[3] else []))
            _, query, head = LF.gather_bytes(c.log_n, c.width, c.prm)
            assert head + query == len(oracle.prove_shard(trace, LF.public_values(c, 0), _oparams(oracle, c.prm))), c.id
    for cid, nbytes in LF.HOST_TRACE_BYTES.items():
        c = LF.case(cid)
        assert c.host and nbytes == 4 * (c.width << c.log_n) and LF.members_of(c) == [16]
    assert LF.stage_fits(LF.HOST_TRACE_BYTES["host-n9"], 16, "up") and not LF.stage_fits(LF.HOST_TRACE_BYTES["host-n11"], 16, "up")


def test_the_grind_shards_need_one_and_two_windows(oracle):
    """the condition is on the reference alone: in either batch of sixteen some witness lies below the window of 2^14 and some at or beyond it"""
    c = LF.case("n6-grind")
    assert c.shards == LF.GRIND_SHARDS and LF.grind_window(c.prm[2]) == 1 << 14
    head = LF.gather_bytes(c.log_n, c.width, c.prm)[2]                                     # the witness is the last word before the queries
    witness = {}
    for j, s in enumerate(c.shards):
        pub = LF.public_values(c, j)
        proof = oracle.prove_shard(oracle.gen_trace_logup(LF.SEED, s, c.log_n, c.width, c.prm[3]), pub, _oparams(oracle, c.prm))
        witness[s] = int(np.frombuffer(proof.tobytes(), dtype=np.uint32)[head // 4 - 1])
        if s in (59, 28, 29):                                                              # ... which the verifier reads as the witness, and accepts
            view = {}
            assert pyverify.verify(proof.tobytes(), c.log_n, c.width, pub, *c.prm, view=view) and view["witness"] == witness[s]
    assert witness[59] == 18413 and witness[28] == 21293 and witness[29] == 87
    assert {s for s, w in witness.items() if w >= 1 << 14} == set(LF.GRIND_LATE)
    at = 0
    for size in LF.members_of(c):
        ws = [witness[s] for s in c.shards[at:at + size]]
        assert min(ws) < 1 << 14 <= max(ws) < 2 << 14
        at += size
