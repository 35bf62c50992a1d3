"""The JOIN of fold-16 lift proofs (zktls_amd/csrc/fri16_chip.hip: zkhip_fri16_join_*, a shape call over machine mode), CPU side: the join's key against
zkhip_machine_verifier_key_host on the InnerMachine assembled from zkhip_fri16_lift_describe; the key as a function of every shape argument and of n_proofs; the
bound; one join END TO END WITHOUT A GPU -- two oracle lift proofs of one shape, the join's ten main tables from zkhip_machine_verifier_host_tables (the Poseidon2
chip's 360 columns computed here), the oracle's keyed-machine prover, zkhip_verify_fri16_join on (shape, public values, key) --; what a bad lift proof is refused
with; and the host's EVAL table against tests/mrec_eval.py, the comparison tests/test_gpu_fri16_join.py holds the device kernel to."""
import numpy as np
import pytest

import mrec_eval
import poseidon2_air as P2
import pyref
import recursion_machine as RM
import test_fri16_lift_cpu as TL
from zktls_amd import _lib
from zktls_amd._lib import Params
from zktls_amd.device import (InnerMachine, fri16_join_key_host, fri16_join_max_proofs, fri16_join_proof_size, fri16_lift_describe, fri16_lift_inner_machine,
                              fri16_lift_key_host, machine_verifier_describe, machine_verifier_host_tables, machine_verifier_key_host, verify_fri16_join)

P = pyref.P
LIFT, JOIN = (1, 10, 2), (1, 3, 0)                          # the lift proofs' outer parameters (tests/test_fri16_lift_cpu.py's twin proofs), the join's
KEY_SHAPES = [TL.SHAPES[0], TL.SHAPES[1]]                    # (R, F, b, Q, W, NP) = (1,0,1,4,8,1) and (1,1,1,3,40,7), the twin shape
_CASE = {}


def args_of(shape):
    R, F, b, Q, W, NP = shape
    return R, F, b, Q, TL.POW_BITS, W, NP


def last_error():
    return _lib.load().zkhip_last_error().decode()


def assembled(S, lift=LIFT):
    """the InnerMachine put together HERE from the public describe entry (positions 0 .. 12) and the shape's host key: what the join entries build inside"""
    chips = []
    for which in range(13):
        prog, ln, mw, pw, _ = fri16_lift_describe(*S, which, 0)
        chips.append(dict(ln=ln, W=mw, Pw=pw, prog=prog, tab=fri16_lift_describe(*S, which, 1)[0]))
    assert [c["ln"] for c in chips] == sorted((c["ln"] for c in chips), reverse=True) and all(c["W"] % 4 == 0 and c["Pw"] % 4 == 0 for c in chips)
    return InnerMachine(chips, fri16_lift_key_host(*S, Params(*lift)), lift[1], lift[2], S[6])


# ------------------------------------------------------------------ (1) the key
@pytest.mark.parametrize("shape", KEY_SHAPES)
def test_join_key_equals_machine_modes_on_the_assembled_description(shape):
    S = args_of(shape)
    im = assembled(S)
    for n in (1, 2):
        assert fri16_join_key_host(*S, n, Params(*LIFT), Params(*JOIN)).tolist() == machine_verifier_key_host(im, Params(*JOIN), n).tolist()
    assert fri16_join_proof_size(*S, 2, Params(*LIFT), Params(*JOIN)) == _lib.load().zkhip_machine_verifier_proof_size(im.desc, 2, Params(*JOIN)) > 0


def test_join_key_moves_with_every_shape_argument_and_the_bound_is_refused_by_message():
    S = args_of(KEY_SHAPES[0])                               # (the smaller shape: every key below is a host commitment of the join's preprocessed traces)
    lift, join = Params(*LIFT), Params(*JOIN)
    vk = fri16_join_key_host(*S, 2, lift, join).tolist()
    for k in range(7):
        T = list(S)
        T[k] += 8 if k == 5 else 1
        assert fri16_join_key_host(*T, 2, lift, join).tolist() != vk, k
    assert fri16_join_key_host(*S, 1, lift, join).tolist() != vk and fri16_join_key_host(*S, 3, lift, join).tolist() != vk
    assert fri16_join_key_host(*S, 2, Params(1, 11, 2), join).tolist() != vk         # (the lift proofs' queries are part of the inner machine)
    for shape in KEY_SHAPES:
        most = fri16_join_max_proofs(*args_of(shape), lift)
        assert 2 <= most <= 64
        for n in (0, most + 1):
            with pytest.raises(_lib.ZkHipError, match="1 .. %d lift proofs of this shape go into one join, not %d" % (most, n)):
                fri16_join_key_host(*args_of(shape), n, lift, join)
            assert fri16_join_proof_size(*args_of(shape), n, lift, join) == 0
            assert verify_fri16_join(np.zeros(64, dtype=np.uint8), [[0] * shape[5]] * n, *args_of(shape), n, [0] * 8, lift, join)[0] != 0 and "lift proofs of this shape" in last_error()
    with pytest.raises(_lib.ZkHipError, match="width-24"):
        fri16_join_key_host(*S, 2, lift, join, hash_width=16)
    assert fri16_join_max_proofs(*S, lift, hash_width=16) == 0 and "width-24" in last_error()
    assert fri16_join_max_proofs(1, 0, 1, 4, 4, 8, 0, lift) == 0 and "1 .. 30 inner public values" in last_error()      # a shape the lift refuses
    rc, _ = verify_fri16_join(np.zeros(64, dtype=np.uint8), [[0] * 7, [0] * 6], *args_of(TL.TWIN), 2, [0] * 8, lift, join)
    assert rc != 0 and "n_proofs x n_inner_public words in proof order (14 here), not 13" in last_error()


# ------------------------------------------------------------------ (2) end to end without a GPU
def p2r_columns(states, bits, kps, log_rows):
    """the Poseidon2 chip's main trace from (input state [16], direction bit, KP) per used row -- every intermediate of the permutation, tests/poseidon2_air.py's row
    for all rows at once; the rows behind the used ones are the all-zero state's"""
    n = 1 << log_rows
    s = np.zeros((n, 16), dtype=np.uint64)
    s[:len(states)] = states
    t = np.zeros((n, RM.P2_MAIN), dtype=np.uint64)
    ME = np.array(pyref.ME, dtype=np.uint64)
    diag = np.array([pyref.MI[i][i] - 1 for i in range(16)], dtype=np.uint64)
    rc_e, rc_i = np.array(pyref.PARAMS["external_rc"], dtype=np.uint64), [int(x) for x in pyref.PARAMS["internal_rc"]]
    assert int(ME.max()) < 64
    external = lambda v: (v @ ME.T) % P                                           # (entries below 64: sixteen products of 37 bits)
    t[:, P2.IN:P2.IN + 16] = s
    t[:len(states), P2.D:P2.D + 8] = np.where(np.asarray(bits, dtype=np.uint64)[:, None] == 1, states[:, 8:], states[:, :8])
    s = external(s)
    t[:, P2.S0:P2.S0 + 16] = s

    def external_round(r, s):
        y = (s + rc_e[r]) % P
        x3 = y * y % P * y % P
        t[:, P2.X3E(r):P2.X3E(r) + 16] = x3
        s = external(x3 * x3 % P * y % P)
        t[:, P2.OUTE(r):P2.OUTE(r) + 16] = s
        return s
    for r in range(4):
        s = external_round(r, s)
    for r in range(13):
        t[:, P2.S0P(r)] = s[:, 0]
        y = (s[:, 0] + np.uint64(rc_i[r])) % P
        x3 = y * y % P * y % P
        t[:, P2.X3P(r)] = x3
        s[:, 0] = t[:, P2.SBP(r)] = x3 * x3 % P * y % P
        s = (s.sum(axis=1, keepdims=True) + diag * s % P) % P
    t[:, P2.SP:P2.SP + 16] = s
    for r in range(4, 8):
        s = external_round(r, s)
    t[:len(states), P2.BIT] = bits
    t[:len(states), RM.M_KP] = kps
    return t.astype(np.uint32)


def join_case(oracle):
    """two oracle lift proofs of the twin shape (seeds 1 and 2, outer (1, 10, 2)), the join's machine as the library describes it, its ten main tables from the host
    entry, and the oracle's proof of them at join outer (1, 3, 0)"""
    if _CASE:
        return _CASE
    O = oracle
    S = TL.full_shape(TL.view_of(O, TL.TWIN, 1))
    assert S == args_of(TL.TWIN)
    proofs, pubs = [], []
    for seed in (1, 2):
        main, pre, progs, tabs, pub = TL.machine_of(O, TL.TWIN, seed)
        proofs.append(O.prove_machine_keyed(main, pre, progs, tabs, pub, O.default_params(*LIFT)))
        pubs.append([int(x) for x in pub])
    im = fri16_lift_inner_machine(*S, Params(*LIFT))
    mains, pres, progs, tabs, lns = [], [], [], [], []
    for i in range(10):
        prog, ln, mw, pw = machine_verifier_describe(im, i, 0, 2)
        tab = machine_verifier_describe(im, i, 1, 2)[0]
        pre = machine_verifier_describe(im, i, 2, 2)[0]
        got = machine_verifier_host_tables(im, proofs, pubs, i)
        assert got is not None, (i, last_error())
        if mw == RM.P2_MAIN:                                  # the Poseidon2 chip: (input state, bit, KP) per used row
            rows = got.reshape(-1, 18)
            got = p2r_columns(rows[:, :16].astype(np.uint64), rows[:, 16], rows[:, 17], ln)
        mains.append(got.reshape(1 << ln, mw))
        pres.append(pre.reshape(1 << ln, pw) if pw else None)
        progs.append(prog)
        tabs.append(tab)
        lns.append(ln)
    flat = [v for pub in pubs for v in pub]
    joined = O.prove_machine_keyed(mains, pres, progs, tabs, flat, O.default_params(*JOIN))
    vk = O.machine_setup(pres, lns, O.default_params(*JOIN))
    _CASE.update(S=S, proofs=proofs, pubs=pubs, im=im, mains=mains, lns=lns, joined=joined, vk=vk)
    return _CASE


def test_two_oracle_lift_proofs_joined_without_a_gpu(oracle):
    c = join_case(oracle)
    S, pubs, joined = c["S"], c["pubs"], c["joined"]
    lift, join = Params(*LIFT), Params(*JOIN)
    vk = fri16_join_key_host(*S, 2, lift, join)
    assert vk.tolist() == c["vk"].tolist()                                        # the oracle's commitment to the preprocessed traces the library describes
    assert joined.size == fri16_join_proof_size(*S, 2, lift, join)
    assert pubs[0] != pubs[1] and len(pubs[0]) == len(pubs[1]) == 7
    assert verify_fri16_join(joined, pubs, *S, 2, vk, lift, join) == (0, 0)
    assert verify_fri16_join(joined, [pubs[1], pubs[0]], *S, 2, vk, lift, join)[0] != 0                  # the two proofs' public values exchanged
    changed = [list(pubs[0]), list(pubs[1])]
    changed[1][3] = (changed[1][3] + 1) % P
    assert verify_fri16_join(joined, changed, *S, 2, vk, lift, join)[0] != 0                             # one public word
    assert verify_fri16_join(joined, pubs + [pubs[0]], *S, 3, fri16_join_key_host(*S, 3, lift, join), lift, join)[0] != 0      # another n_proofs
    assert verify_fri16_join(joined, pubs[:1], *S, 1, fri16_join_key_host(*S, 1, lift, join), lift, join)[0] != 0
    T = list(S)
    T[3] += 1                                                                     # the key of another shape (one more query), with the shape that made the proof
    assert verify_fri16_join(joined, pubs, *S, 2, fri16_join_key_host(*T, 2, lift, join), lift, join)[0] != 0
    assert verify_fri16_join(joined, pubs, *T, 2, fri16_join_key_host(*T, 2, lift, join), lift, join)[0] != 0


def test_bad_lift_proofs_are_refused_by_name(oracle):
    c = join_case(oracle)
    im, proofs, pubs = c["im"], c["proofs"], c["pubs"]
    bad = proofs[1].copy()
    bad[bad.size // 2] ^= 1
    assert machine_verifier_host_tables(im, [proofs[0], bad], pubs, 0) is None and "proof 1 rejected" in last_error()
    assert machine_verifier_host_tables(im, proofs, [pubs[1], pubs[0]], 0) is None
    assert "proof 0 rejected: a chip's constraints do not match its quotient at zeta" in last_error()


# ------------------------------------------------------------------ (3) the EVAL table
def eval_inputs(sh, c):
    """per proof the value table behind the keys and alpha, read off the proof's words, the public values and the host's SCALARS table"""
    _, m, pre = RM.sc_cols(sh)
    scalars = c["mains"][RM.order(sh).index("SCALARS")]
    o_stream = sh.HL + 2 + 8 + 8 + 4 * sh.C + 8
    values, alphas = [], []
    for p, (proof, pub) in enumerate(zip(c["proofs"], c["pubs"])):
        w = np.frombuffer(proof.tobytes(), dtype=np.uint32)
        tab = [[1, 0, 0, 0]] + w[o_stream:o_stream + 4 * sh.NV].reshape(-1, 4).tolist() + [[v % P, 0, 0, 0] for v in pub]
        for ch in range(sh.C):
            row = scalars[p * sh.C + ch]
            tab += [row[m[name] - pre:m[name] - pre + 4].tolist() for name in ("SELF", "SELL", "SELT")]
        assert len(tab) == sh.KSPAN
        values.append(tab)
        alphas.append(scalars[p * sh.C][m["ALPHA"] - pre:m["ALPHA"] - pre + 4].tolist())
    return values, alphas


def join_shape(c):
    im = c["im"]
    chips = [dict(ln=int(im.log_ns[i]), W=int(im.widths[i]), Pw=int(im.pre_widths[i]), prog=im.keep[i][0], tab=im.keep[i][1]) for i in range(13)]
    sh = RM.MShape(chips, [int(x) for x in im.desc.key_root], LIFT[1], LIFT[2], c["S"][6], 2)
    RM.build_reads(sh)
    return sh


def test_host_eval_table_equals_the_plain_integer_restatement(oracle):
    c = join_case(oracle)
    sh = join_shape(c)
    values, alphas = eval_inputs(sh, c)
    want, accs = mrec_eval.table(sh.terms, sh.C, values, alphas)
    got = c["mains"][RM.order(sh).index("EVAL")]
    assert got.shape[1] == mrec_eval.EV_MAIN and len(want) == 2 * len(sh.terms) <= got.shape[0]
    assert np.array_equal(got[:len(want)], np.array(want, dtype=np.uint32)) and not got[len(want):].any()
    for p in range(2):
        for ch in range(sh.C):
            assert accs[p * sh.C + ch] == want[p * len(sh.terms) + sh.term1[ch]][mrec_eval.EV_ACCO:mrec_eval.EV_ACCO + 4]
