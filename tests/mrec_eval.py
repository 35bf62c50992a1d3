"""Machine mode's EVAL rows (zktls_amd/csrc/machine_verifier.inl: fill_proof's EVAL section on the host, mrec_eval_rows_kernel on the device) once more, in plain
integers: the comparison both are held to.  A term is (chip, coefficient, three keys, first-term-of-its-constraint flag); a key names an extension value of one inner
proof -- 0 the extension one, then the opened-value stream, the public values, three selectors per chip --, here simply an entry of a per-proof table.  Per term one row
of 32 words:

    F0 F1 F2 (the three values) | M = F0 F1 | TV = coeff M F2 | ACCIN | ACCO | ALPHA

with a running value that is zero at a chip's first term: ACCIN = run; run = (first ? run alpha : run) + TV; ACCO = run.  A constraint without a term is the row
(coefficient 0, keys 0 0 0, first = 1): it multiplies the running value by alpha and adds nothing.  Extension arithmetic is tests/pyref.py's (F_p[X] / (X^4 - 11))."""
from pyref import P, ext_mul

EV_F0, EV_M, EV_TV, EV_ACCIN, EV_ACCO, EV_ALPHA, EV_MAIN = 0, 12, 16, 20, 24, 28, 32
ONE = [1, 0, 0, 0]


def rows(terms, n_chips, values, alpha):
    """terms: [(chip, coeff, [k0, k1, k2], first)] chip by chip; values: the proof's table, values[key] = four canonical words (entry 0 is not read); alpha: four words
    -> (rows [len(terms)][32], per chip ACCO of its last term -- [0, 0, 0, 0] for a chip without a term)"""
    out, last = [], [[0] * 4 for _ in range(n_chips)]
    run, chip_before = [0] * 4, None
    for chip, coeff, keys, first in terms:
        assert chip_before is None or chip >= chip_before, "terms stand chip by chip"
        if chip != chip_before:
            run = [0] * 4
        chip_before = chip
        f = [ONE if k == 0 else [int(x) % P for x in values[k]] for k in keys]
        mm = ext_mul(f[0], f[1])
        tv = [x * coeff % P for x in ext_mul(mm, f[2])]
        accin = run
        run = [(a + b) % P for a, b in zip(ext_mul(run, alpha) if first else run, tv)]
        out.append(f[0] + f[1] + f[2] + mm + tv + list(accin) + run + [int(x) % P for x in alpha])
        last[chip] = run
    return out, last


def table(terms, n_chips, values_per_proof, alphas):
    """several proofs over one term list -> (rows [n_proofs len(terms)][32] proof by proof, accumulators [n_proofs n_chips][4])"""
    out, accs = [], []
    for values, alpha in zip(values_per_proof, alphas):
        r, a = rows(terms, n_chips, values, alpha)
        out += r
        accs += a
    return out, accs
