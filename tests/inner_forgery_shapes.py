"""What the two forgery test files (tests/test_inner_forgeries_cpu.py, tests/test_gpu_inner_forgeries.py) share besides the catalogue (tests/inner_forgeries.py, which
calls no library): the cases by name, made once per module, and the fold-16 lift machine of tests/test_gpu_fri16_join.py's shape as the catalogue takes it."""
import inner_forgeries as IF
from zktls_amd._lib import Params, segment_params

LIFT_LOG_N, LIFT_WIDTH, LIFT, JOIN = 10, 16, Params(1, 12, 4), Params(1, 8, 2)
MAKERS = {"byte": IF.byte_case, "mixed": IF.mixed_case, "wide": IF.wide_case, "shard": lambda O: IF.shard_case(O, False), "shard-air": lambda O: IF.shard_case(O, True),
          "shard-5": lambda O: IF.shard_case(O, False, 5)}


def case_factory(oracle):
    """-> get(name): the case of that name, made on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = MAKERS[name](oracle)
        return made[name]
    return get


def lift_shape():
    """(R, F, log_blowup, Q, grinding bits, W, NP) of tests/test_gpu_fri16_join.py's segments: 2^10 x 16, twelve queries"""
    sp = segment_params(12, 0, 2)
    return sp, ((LIFT_LOG_N - int(sp.log_final)) // 4, int(sp.log_final), int(sp.log_blowup), int(sp.num_queries), int(sp.pow_bits), LIFT_WIDTH, 1)


def lift_machine(n_proofs=2):
    """the lift machine of that shape as the catalogue takes it: (chips, key, recursion_machine.MShape over n_proofs lift proofs)"""
    import recursion_machine as RM
    from zktls_amd.device import fri16_lift_describe, fri16_lift_key_host
    _, S = lift_shape()
    chips = []
    for which in range(13):
        prog, ln, mw, pw, _ = fri16_lift_describe(*S, which, 0)
        chips.append(dict(ln=ln, W=mw, Pw=pw, prog=prog, tab=fri16_lift_describe(*S, which, 1)[0]))
    vk = [int(x) for x in fri16_lift_key_host(*S, LIFT)]
    return chips, vk, RM.MShape(chips, vk, int(LIFT.num_queries), int(LIFT.pow_bits), S[6], n_proofs)
