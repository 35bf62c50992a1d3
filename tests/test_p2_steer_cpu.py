"""The steered catalogue (p2_steer) through the exact device models (p2_device_model), on the CPU: every state round-trips, every model of
every form gives pyref's words and the oracle's, no range assertion of a model fires, and -- read from the models' logs, so that the
catalogue cannot silently lose its point -- the catalogue really reaches the boundaries it was built for inside the rounds of each form.
The recorded maxima are printed (DESIGN.md 4.2 quotes them) and must stay inside the bounds the interval passes derive."""
import numpy as np
import pytest

import p2_device_model as M
import p2_steer as S
import pyref

P = pyref.P
SMALL_DIAG = [P - 2, 1, 3, 5, 7, 9, 11, 13, 17, 19, 23, 29, 31, 37, 41, 32768]

# form -> the model run; the partial rounds paired and one at a time, the full rounds all-VALU and on the matrix cores
FORMS16 = {
    "valu_pair": lambda s, log, tr, st: M.permute_valu(s, log=log, track=tr),
    "valu_one": lambda s, log, tr, st: M.permute_valu(s, pair=False, log=log, track=tr),
    "mx_pair": lambda s, log, tr, st: M.permute_mx(s, log=log, track=tr, stats=st),
    "coop": lambda s, log, tr, st: M.permute_coop(s, log=log),
}


class Coverage:
    """what the logs of one form showed: sets of (round, what) and, per lane, the output words 0 and P - 1"""

    def __init__(self):
        self.seen = set()

    def read(self, log):
        seen = self.seen
        for rnd, lane, name, val in log:
            if name == "t":
                if val in (0, 1, -1):
                    seen.add((rnd, "t", val))
            elif name == "u":
                seen.add((rnd, "u", val >= P))
            elif name == "sum":
                if val in (0, 1, -1):
                    seen.add((rnd, "sum", val))
            elif name == "Y":
                if val == 35 * 128:
                    seen.add((rnd, "Y", lane))                          # lane = the plane here
            elif name == "out":
                if val in (0, P - 1):
                    seen.add(("OUT", lane, val))


@pytest.fixture(scope="module")
def cat16():
    return S.catalogue(16)


@pytest.fixture(scope="module")
def cat24():
    return S.catalogue(24)


@pytest.fixture(scope="module")
def run16(cat16):
    """every form's model on the whole width-16 catalogue, once: outputs compared on the way, coverage and maxima kept"""
    cov = {f: Coverage() for f in FORMS16}
    track = {f: {} for f in FORMS16}
    stats = {}
    for label, probe, state in cat16:
        exp = pyref.poseidon2(state)
        for f, run in FORMS16.items():
            log = []
            assert run(state, log, track[f], stats) == exp, (f, label)
            cov[f].read(log)
    return cov, track, stats


@pytest.fixture(scope="module")
def run24(cat24):
    cov, track = Coverage(), {}
    for label, probe, state in cat24:
        log = []
        assert M.permute24(state, log=log, track=track) == pyref.poseidon2_24(state), label
        cov.read(log)
    return cov, track


def test_catalogue_sizes_and_round_trip(cat16, cat24):
    # steer() asserts the round trip of every state it returns; here the independent restatement: pyref's permutation of the steered input,
    # walked forward to the probe by p2_steer, is the target again, and the labels are unique
    print("catalogue: %d states at width 16, %d at width 24" % (len(cat16), len(cat24)))
    assert 1500 <= len(cat16) <= 2500 and 300 <= len(cat24) <= 700
    for w, cat in ((16, cat16), (24, cat24)):
        assert len({c[0] for c in cat}) == len(cat)
        assert {c[1] for c in cat} >= {p for p in S.probes(w) if p[0] != "U" or w == 16}
        for label, probe, state in cat:
            assert len(state) == w and all(0 <= x < P for x in state)
    assert S.catalogue(24) == cat24                                     # deterministic


def test_steps_are_the_permutation(cat16, cat24, oracle):
    for label, probe, state in cat16:
        exp = pyref.poseidon2(state)
        assert S.permute(16, state) == exp and oracle.poseidon2(state).tolist() == exp, label
    for label, probe, state in cat24:
        exp = pyref.poseidon2_24(state)
        assert S.permute(24, state) == exp and oracle.poseidon2_24(state).tolist() == exp, label


def test_probe_words_are_the_targets():
    ws = S.edge_words()
    for w in (16, 24):
        for probe in S.probes(w):
            words = [ws[(3 * i + len(probe)) % len(ws)] for i in range(w)]
            assert S.forward_probe(w, probe, S.steer(w, probe, words)) == words
    # the probes are where the device model holds those words: the S-box inputs of round 5, the state entering partial round 7 (word 0) and
    # the output
    words = [ws[i % len(ws)] for i in range(16)]
    log = []
    M.permute_valu(S.steer(16, ("F", 5), words), log=log)
    assert [v % P for r, _, n, v in log if r == ("F", 5) and n == "t"] == words
    log = []
    M.permute_valu(S.steer(16, ("P", 7), words), log=log)
    assert [v % P for r, _, n, v in log if r == ("P", 7) and n == "t"] == words[:1]
    log = []
    M.permute_mx(S.steer(16, ("U", 2), words), log=log)
    assert [v % P for r, _, n, v in log if r == ("F", 2) and n == "u"] == words
    log = []
    M.permute24(S.steer(24, ("OUT",), words + words[:8]), log=log)
    assert [v for r, _, n, v in log if n == "out"] == words + words[:8]


def test_small_diagonal_catalogue(cat16):
    # a loaded parameter file's diagonal: steered for it, round trip asserted by steer(); the models against the field arithmetic
    rc_i = pyref.PARAMS["internal_rc"]
    k = M.consts_for(SMALL_DIAG, rc_i)
    assert k.pair
    cat = S.catalogue(16, SMALL_DIAG)
    assert len(cat) == len(cat16) and [c[:2] for c in cat] == [c[:2] for c in cat16]
    for label, probe, state in cat[::6]:
        exp = S.permute(16, state, SMALL_DIAG)
        assert M.permute_valu(state, k) == exp and M.permute_valu(state, k, pair=False) == exp, label
        assert M.permute_mx(state, k) == exp and M.permute_coop(state, k) == exp, label
    from test_p2_pair_model import reference
    for label, probe, state in cat[::101]:
        assert S.permute(16, state, SMALL_DIAG) == reference(state, SMALL_DIAG, rc_i)


def test_width16_models_and_coverage(run16):
    cov, track, stats = run16
    full, part = [("F", r) for r in range(8)], [("P", r) for r in range(13)]
    for f, c in cov.items():
        for rnd in full:
            for t in (0, 1, -1):
                assert (rnd, "t", t) in c.seen, "%s: no S-box input %d in full round %d" % (f, t, rnd[1])
            for hi in (False, True):
                assert (rnd, "u", hi) in c.seen, "%s: no lazy output %s P in full round %d" % (f, "at or above" if hi else "below", rnd[1])
        for rnd in part:
            assert (rnd, "t", 0) in c.seen, "%s: no v0 S-box input 0 in partial round %d" % (f, rnd[1])
        for lane in range(16):
            for val in (0, P - 1):
                assert ("OUT", lane, val) in c.seen, "%s: no output word %d in lane %d" % (f, val, lane)
    for f in ("valu_pair", "valu_one", "mx_pair"):
        for rnd in part:
            for t in (0, 1, -1):
                assert (rnd, "sum", t) in cov[f].seen, "%s: no row sum reducing to %d in partial round %d" % (f, t, rnd[1])
    for rnd in ["L0"] + full:
        for plane in range(3):
            assert (rnd, "Y", plane) in cov["mx_pair"].seen, "matrix cores: |Y| = 35 * 128 not reached in plane %d of layer %s" % (plane, rnd)


def test_width16_maxima_inside_the_budgets(run16):
    cov, track, stats = run16
    bounds = {}
    assert M.pair_budget_ok(sum(M.BUILTIN.d[1:]), bounds=bounds)
    one = {}
    assert M.round_budget_ok(16, M.SH_ONE, 13, bounds=one)
    for f in ("valu_pair", "mx_pair"):
        t = track[f]
        print("%s: max |st| = %d (%.4f P, bound %.4f P), |s1| = %d (%.4f P, bound %.4f P), |v| = %d (%.4f P, bound %.4f P)"
              % (f, t["st"], t["st"] / P, bounds["st"] / P, t["s1"], t["s1"] / P, bounds["s1"] / P, t["v"], t["v"] / P, bounds["v"] / P))
        assert t["st"] <= bounds["st"] and t["s1"] <= bounds["s1"] and t["v"] <= bounds["v"] <= P - 1
    t = track["valu_one"]
    print("valu_one: max |sum| = %d (%.4f P, bound %.4f P), |v| = %d (%.4f P, bound %.4f P)"
          % (t["sum"], t["sum"] / P, one["sum"] / P, t["v1"], t["v1"] / P, one["v"] / P))
    assert t["sum"] <= one["sum"] and t["v1"] <= one["v"] <= P - 1
    print("matrix cores: max |Y| = %d (bound %d), top digit %d (bound 120), |w| = %d (%.4f P)" % (stats["Y"], 35 * 128, stats["d3"], stats["w"], stats["w"] / P))
    assert stats["Y"] == 35 * 128 and stats["d3"] <= 120 and stats["w"] < 2**28.2 + P / 2


def test_width24_model_coverage_and_budget(run24):
    cov, track = run24
    for rnd in [("F", r) for r in range(8)]:
        for t in (0, 1, -1):
            assert (rnd, "t", t) in cov.seen, "width 24: no S-box input %d in full round %d" % (t, rnd[1])
        for hi in (False, True):
            assert (rnd, "u", hi) in cov.seen, "width 24: no lazy output %s P in full round %d" % ("at or above" if hi else "below", rnd[1])
    for rnd in [("P", r) for r in range(21)]:
        assert (rnd, "t", 0) in cov.seen, "width 24: no v0 S-box input 0 in partial round %d" % rnd[1]
        for t in (0, 1, -1):
            assert (rnd, "sum", t) in cov.seen, "width 24: no row sum reducing to %d in partial round %d" % (t, rnd[1])
    for lane in range(24):
        for val in (0, P - 1):
            assert ("OUT", lane, val) in cov.seen, "width 24: no output word %d in lane %d" % (val, lane)
    # the interval pass poseidon2.cuh has only as a comment: holds at the 2^26 row-sum scale, fails at 2^27 (24 P 2^27 leaves the 64-bit sum
    # of the reduction no room), and the one-round form of width 16 holds at its 2^27
    bounds = {}
    assert M.round_budget_ok(24, M.SH_24, 21, bounds=bounds) and M.BUILTIN24.ok
    assert not M.round_budget_ok(24, 27, 21)
    assert M.round_budget_ok(16, M.SH_ONE, 13) and not M.round_budget_ok(16, 28, 13)
    assert bounds["sum"] <= 0.875 * P + 2 and bounds["v"] <= P - 1       # the comment's |sum| < 0.875 P
    print("width 24: max |sum| = %d (%.4f P, bound %.4f P), |v| = %d (%.4f P, bound %.4f P)"
          % (track["sum"], track["sum"] / P, bounds["sum"] / P, track["v"], track["v"] / P, bounds["v"] / P))
    assert track["sum"] <= bounds["sum"] and track["v"] <= bounds["v"]


def test_signed_external_layer_hands_over_minus_p():
    # a finding of the steered states: p2_external_linear_signed_dev returns s_i + t - P with s_i and t canonical, which is -P (not inside
    # (-P, P)) where both are 0.  Everything after it takes -P: the S-box (0 comes out), the row sums, dcanon (wraps to 0).  The interval passes
    # therefore start at P, and still hold.
    state = S.steer(16, ("U", 3), [0] * 16)
    log = []
    assert M.permute_valu(state, log=log) == pyref.poseidon2(state)
    assert [v for r, _, n, v in log if r == ("P", 0) and n == "t"] == [-P]
    state = S.steer(16, ("U", 7), [0] * 16)
    assert M.permute_valu(state) == [0] * 16 == pyref.poseidon2(state)
    assert M.dcanon(-P) == 0 and M.dcanon(-1) == P - 1 and M.dcanon(P - 1) == P - 1 and M.dcanon(0) == 0


def test_models_assert_their_ranges():
    # the range assertions are live: a row-sum scale of 2^29 at width 16 overflows the 64-bit accumulator on the largest words
    k = M.BUILTIN
    with pytest.raises(AssertionError):
        T = 0
        for x in [P - 1] * 16:
            T = M.mad(x, 1 << 29, T)
        M.dsmred(T)
    with pytest.raises(AssertionError):
        M.dred(2 * P)
    with pytest.raises(AssertionError):
        M.mx_layer([2 * P] * 16)
    assert k.pair and np.abs(M.ME).max() == 6
