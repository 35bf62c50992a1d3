"""What test_gpu_air_forms.py rests on, checked without a GPU: the oracle's quotient of a constraint program against an evaluation in
Python integers written from docs/PROTOCOL.md (sections 3 and 3b) on the very kind of input the GPU tests use; the GPU file's
parameter lists against the table of kernel forms (tests/air_forms.py); and the programs that hold on a trace."""
import collections

import numpy as np
import pytest

import air_forms as AF
import pyref
from field_edges import edge_ext, edge_matrix

P = pyref.P


# ------------------------------------------------------------------ the oracle against Python integers
def _quotient_in_integers(prog, lde, log_n, pub, alpha):
    """PROTOCOL.md 3 / 3b: the quotient domain is g <w_{2^lqd N}>, point i at row bitrev(i) of the LDE; the next trace row is 2^lqd points
    further; is_first = Z_H(x) / (x - 1), is_last = Z_H(x) / (x - w_N^-1), is_transition = x - w_N^-1; constraints fold as
    acc = acc alpha + selector sum_t coeff_t prod_j var_tj; the value at row bitrev(i) is acc / Z_H(x)"""
    lqd = AF.log_quotient_degree(prog)
    bits = log_n + lqd
    m, n, width = 1 << bits, 1 << log_n, int(prog[2])
    w, wn_inv = pyref.two_adic_generator(bits), pow(pyref.two_adic_generator(log_n), -1, P)
    alpha = [int(a) for a in alpha]
    terms = list(AF.terms_of(prog))
    K = int(prog[3])
    rows = [[int(v) for v in r] for r in lde]
    out = np.zeros((m, 4), dtype=np.uint32)
    for i in range(m):
        x = pyref.GEN * pow(w, i, P) % P
        zh = (pow(x, n, P) - 1) % P
        sel = {0: 1, 1: zh * pow(x - 1, -1, P) % P, 2: zh * pow(x - wn_inv, -1, P) % P, 3: (x - wn_inv) % P}
        local, nxt = rows[pyref.bitrev(i, bits)], rows[pyref.bitrev((i + (1 << lqd)) % m, bits)]
        cvals = [0] * K
        for k, s, coeff, vs in terms:
            prod = coeff
            for v in vs:
                kind, idx = v >> 30, v & 0xFFFF
                prod = prod * (local[idx] if kind == 0 else nxt[idx] if kind == 1 else pub[idx]) % P
            cvals[k] = (cvals[k] + prod * sel[s]) % P
        acc = [0, 0, 0, 0]
        for c in cvals:
            acc = pyref.ext_mul(acc, alpha)
            acc[0] = (acc[0] + c) % P
        izh = pow(zh, -1, P)
        out[pyref.bitrev(i, bits)] = [a * izh % P for a in acc]
    assert width == lde.shape[1]
    return out


@pytest.mark.parametrize("n_public", [0, 7])
@pytest.mark.parametrize("lqd", [1, 2])
@pytest.mark.parametrize("log_n", [3, 5])
@pytest.mark.parametrize("width", [4, 20])
def test_oracle_quotient_of_a_program_equals_the_evaluation_in_integers(oracle, width, log_n, lqd, n_public):
    counts = [6, 10, 14, 0, 0] if lqd == 1 else [6, 8, 10, 9, 7]
    prog, pub = AF.class_program(width, counts, seed=width + log_n + lqd, n_public=n_public)
    assert oracle.air_validate(prog, width, n_public) == 1
    assert oracle.air_log_quotient_degree(prog) == lqd == AF.log_quotient_degree(prog)
    assert AF.class_counts(prog) == counts
    lde = edge_matrix(1 << (log_n + lqd), width, seed=log_n + width)
    for alpha in edge_ext(np.random.default_rng(width), 1)[::3]:
        got = oracle.quotient_values_air(prog, lde, log_n, pub, alpha)
        assert (got == _quotient_in_integers(prog, lde, log_n, pub, alpha)).all(), alpha.tolist()


def test_class_programs_are_what_they_say():
    """the properties class_program promises, read back from a program"""
    W = 48
    prog, pub = AF.class_program(W, [5, 40, 200, 30, 21], seed=9, n_public=65)
    assert AF.class_counts(prog) == [5, 40, 200, 30, 21] and AF.monomial_count(prog) == 296
    terms = list(AF.terms_of(prog))
    assert {s for _, s, _, _ in terms} == {0, 1, 2, 3}
    cols = {(v >> 30, v & 0xFFFF) for _, _, _, vs in terms for v in vs}
    for c in (0, 3, W - 4, W - 1, 16 + 1, 32 + 2):
        assert (0, c) in cols or (1, c) in cols
    nxt = sum(1 for k, c in cols if k == 1)
    assert 0.3 < nxt / sum(1 for k, c in cols if k != 2) < 0.7
    assert {i for k, i in cols if k == 2} == set(range(65)) and pub[0] == 1 and pub[-1] == P - 1 and 0 in pub
    assert any(len(vs) == 5 and all(v >> 30 == 2 for v in vs) for _, _, _, vs in terms)          # five public values and nothing else
    assert any(len(vs) >= 3 and len({v & 0xFFFF for v in vs if v >> 30 != 2}) < sum(1 for v in vs if v >> 30 != 2) for _, _, _, vs in terms)
    per_key = collections.defaultdict(list)
    for k, s, c, vs in terms:
        assert 0 < c < P
        per_key[AF.monomial_key(W, s, vs)].append((k, c, tuple(v for v in vs if v >> 30 == 2)))
    merged = [v for v in per_key.values() if len(v) > 1]
    assert len(merged) >= 4
    zero = [v for v in merged if len(v) == 2 and v[0][0] == v[1][0] and (v[0][1] + v[1][1]) % P == 0 and not v[0][2] and not v[1][2]]
    assert len(zero) == 1                                                                        # one record's coefficient is zero
    low, _ = AF.class_program(W, [5, 40, 200], seed=9, n_public=65)
    assert AF.log_quotient_degree(low) == 1


# ------------------------------------------------------------------ the GPU file's cases against the table of forms
def test_form_table_at_its_thresholds():
    f = AF.form
    assert f(48, 2048, 6) == "wide<16>" and f(48, 2046, 6) == "terms<128>" and f(48, 2048, 5) == "terms<128>"
    assert f(624, 2048, 6) == "wide<16>" and f(628, 2048, 6) == "terms<128>" and f(640, 3366, 12) == "terms<128>"     # the SHA-256 chip
    assert f(48, 2048, 6, lockstep=True) == "terms<128>" and f(48, 2048, 6, aligned=False) == "interpreter"
    assert f(16, 512, 5) == "interpreter" and f(16, 514, 5) == "terms<128>" and f(20, 512, 5) == "chain<64,4>"
    assert f(628, 8192, 6) == "terms<128>" and f(628, 8194, 6) == "terms<256>"
    for lo, hi, name in ((20, 128, "chain<64,4>"), (132, 256, "chain<64,8>"), (260, 384, "chain<64,12>"), (388, 512, "chain<128,8>"),
                         (516, 768, "chain<128,12>"), (772, 1024, "chain<128,16>")):
        assert f(lo, 100, 5) == f(hi, 100, 5) == name
    assert f(64, 100, 3) == "terms<64>" and f(64, 100, 2) == "interpreter" and f(6, 600, 6) == "interpreter"
    assert not AF.enterable(64, 3) and not AF.enterable(64, 4) and not AF.enterable(6, 6) and AF.enterable(1024, 5)
    assert [AF.chain_len(n) for n in (5, 6, 7, 8, 9)] == [4, 8, 16, 32, 32]


def test_gpu_cases_reach_every_live_form_twice():
    """every case of test_gpu_air_forms.py names the kernel it means to reach as its pytest id: the name is what form() says for the
    program the case builds, and every live form occurs at least twice at stage level and once as a lock-step twin"""
    import test_gpu_air_forms as G
    seen = collections.Counter()
    ids, publics, all_public = set(), set(), False
    for param in G.STAGE_CASES:
        case, = param.values
        assert param.id not in ids
        ids.add(param.id)
        assert param.id.split(":")[0] == case.form
        assert AF.enterable(case.width, case.log_n)
        prog, _ = G.build_program(case)
        M = AF.monomial_count(prog)
        if case.M is not None:
            assert M == case.M, (param.id, M)
        assert AF.log_quotient_degree(prog) == case.lqd, param.id
        aligned = case.ld % 4 == 0 and case.ptr_off % 4 == 0
        assert AF.form(case.width, M, case.log_n, aligned=aligned) == case.form, (param.id, M)
        if case.pairs is not None:
            assert AF.wide_pairs(prog) == case.pairs, (param.id, AF.wide_pairs(prog))
        seen[case.form] += 1
        if case.n_public:
            publics.add((case.form.split("<")[0], case.n_public))
            all_public |= any(len(vs) == 5 and all(v >> 30 == 2 for v in vs) for _, _, _, vs in AF.terms_of(prog))
    assert set(seen) == set(AF.LIVE_FORMS), sorted(set(AF.LIVE_FORMS) ^ set(seen))
    assert all(seen[f] >= 2 for f in AF.LIVE_FORMS), seen
    assert publics == {("chain", 1), ("terms", 64), ("terms", 65), ("wide", 300)} and all_public      # public values on every term-parallel form
    # the wide form's deal of record pairs over its 16 wavefronts: every remainder trip, an idle wavefront, the edges of `per`
    pairs = [p for param in G.STAGE_CASES for p in (param.values[0].pairs or [])]
    for want in (0, 1, 2, 3, 7, 64, 65):
        assert want in pairs, want
    trips = set()
    for p in pairs:
        per = (p + 63) // 64 * 4
        for slot in range(16):
            mine = max(0, min(p, slot * per + per) - slot * per)
            trips |= {"idle"} if mine == 0 else ({4} if mine >= 4 else set()) | ({2} if mine & 2 else set()) | ({1} if mine & 1 else set())
    assert trips == {"idle", 4, 2, 1}
    twins = collections.Counter()
    for param in G.TWIN_CASES:
        tw, = param.values
        prog, _, _ = AF.derived_program_and_trace(tw.log_n, tw.base, tw.derived, tw.terms_per, tw.seed)
        M = AF.monomial_count(prog)
        assert AF.form(tw.base + tw.derived, M, tw.log_n, lockstep=True) == param.id == tw.form, (param.id, M)
        assert (AF.form(tw.base + tw.derived, M, tw.log_n) == "wide<16>") == tw.wide_outside
        twins[tw.form] += 1
    assert set(twins) >= {"interpreter", "chain<64,4>", "chain<64,8>", "chain<128,8>", "terms<128>", "terms<256>"}
    assert any(param.values[0].wide_outside for param in G.TWIN_CASES)


# ------------------------------------------------------------------ programs that hold on a trace
@pytest.mark.parametrize("log_n,base,derived,terms_per", [(3, 4, 4, 3), (4, 9, 7, 5)])
def test_derived_trace_satisfies_its_program(oracle, log_n, base, derived, terms_per):
    prog, trace, pub = AF.derived_program_and_trace(log_n, base, derived, terms_per, seed=log_n)
    n, width = trace.shape
    assert width == base + derived and oracle.air_validate(prog, width, 2) == 1
    assert AF.monomial_count(prog) == derived * (terms_per + 1) + 5 + (derived * (terms_per + 1) + 5) % 2
    assert all(c != 0 for _, _, c, _ in AF.terms_of(prog))
    t = [[int(v) for v in r] for r in trace]
    for i in range(n):
        cvals = collections.defaultdict(int)
        sels = {}
        for k, s, coeff, vs in AF.terms_of(prog):
            prod = coeff
            for v in vs:
                kind, idx = v >> 30, v & 0xFFFF
                prod = prod * (t[i][idx] if kind == 0 else t[(i + 1) % n][idx] if kind == 1 else pub[idx]) % P
            cvals[k] = (cvals[k] + prod) % P
            sels[k] = s
        for k, c in cvals.items():
            applies = {0: True, 1: i == 0, 2: i == n - 1, 3: i != n - 1}[sels[k]]
            assert c == 0 or not applies, (i, k)
    # another trace of the same program
    prog2, trace2, _ = AF.derived_program_and_trace(log_n, base, derived, terms_per, seed=log_n, trace_seed=99)
    assert (prog2 == prog).all() and (trace2 != trace).any()
