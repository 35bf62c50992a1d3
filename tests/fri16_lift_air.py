"""The fold-by-16 LIFT machine, written a second time -- the first is zktls_amd/csrc/fri16_chip.hip (the machine and its key) and fri16_rows.cuh
(fri16_lift_tables_kernel, the main columns of ROOTS and COEFFS).  It is the identity machine of tests/fri16_identity_air.py with the roots and the final
coefficients OUT of the key.

Statement (the public values are the inner proof's own; the key is a function of the SHAPE and the number of public values alone): "some valid segment proof of
this shape with these public values exists" -- everything the identity machine states about an inner proof, with nothing of that proof in the key.  What pins the
roots and the coefficients is Fiat-Shamir alone: the transcript chain starts from the all-zero state and absorbs every one of them over a bus.  STILL OUTSIDE: the
join of several lift proofs and the r0 host mirror's compress path, lookups, version-7 and version-8 inner proofs, the wiring into the shard verifier, a batch entry.

Thirteen tables, the identity machine's numbers, heights and widths but:
5 ROOTS   main ENDS BETA[4] FOLDROWS 0 0 ROOT[8] (sixteen columns: the root words stood in preprocessed columns 2 .. 9); preprocessed LN DEP ACT 0[7] LISTED HM
          HK[8], ACT = 1 on rows 0 .. R + 1.  The tuples of the path-end buses, the transcript buses and BUS_HR read ROOT from the main columns.  One more
          constraint, ENDS (1 - ACT) = 0: a padding row's digest is free, so it must receive no path end.  The first-row identity names main column 7 (spare)
4 COEFFS  main 0 0 0 0 C[4] (eight columns: c_j stood in preprocessed columns 1 .. 4); preprocessed j 0[4] Q 1 0.  The first-row identity names main column 3
Every other table keeps its program and interaction table word for word."""
import numpy as np

import fri16_air as A
import fri16_head_air as HA
import fri16_identity_air as IA
import fri16_paths_air as PA
import fri16_transcript_air as TA
import oracle_lib as O

P = O.P
V = O.air_var
NAMES = IA.NAMES
COEFFS, ROOTS = HA.COEFFS, HA.ROOTS
CHANGED = [COEFFS, ROOTS]
UNCHANGED = [t for t in range(13) if t not in CHANGED]
ROOTS_MAIN, RL_ROOT, RT_ACT = 16, 8, PA.RT_ROOT                                 # ACT sits where root word 0 stood
COEFFS_MAIN, CL_C = 8, 4
ROOTS_SPARE, COEFFS_SPARE = TA.ROOTS_MAIN - 1, A.TAB_MAIN - 1                   # the main columns the first-row identities name: the ones they named before

log_rows, shape_ok, order = IA.log_rows, IA.shape_ok, IA.order
PRE_WIDTHS = IA.PRE_WIDTHS


def main_widths(lf, n):
    w = IA.main_widths(lf, n)
    w[COEFFS], w[ROOTS] = COEFFS_MAIN, ROOTS_MAIN
    return w


# ---------------------------------------------------------------- programs
def roots_constraints():
    RM = HA.ROOTS_PRE
    return [("row 0: the spare column is zero", O.SEL_FIRST, [(1, [V(RM + ROOTS_SPARE)])]),
            ("FOLDROWS (1 - LISTED) = 0", O.SEL_ALL, [(1, [V(RM + 5)]), (P - 1, [V(RM + 5), V(10)])]),
            ("ENDS (1 - ACT) = 0", O.SEL_ALL, [(1, [V(RM)]), (P - 1, [V(RM), V(RT_ACT)])])]


def coeffs_constraints():
    return [("row 0: the spare column is zero", O.SEL_FIRST, [(1, [V(A.C_PRE + COEFFS_SPARE)])])]


def constraint_names(table, W=0, NP=0, log_n=0, pow_bits=0):
    if table == ROOTS:
        return [n for n, _, _ in roots_constraints()]
    if table == COEFFS:
        return [n for n, _, _ in coeffs_constraints()]
    return IA.constraint_names(table, W, NP, log_n, pow_bits)


def programs(R, F, b, pow_bits, W, NP):
    """by table number"""
    ip = IA.programs(R, F, b, pow_bits, W, NP)
    ip[ROOTS] = O.air_program(HA.ROOTS_PRE + ROOTS_MAIN, NP, [(sel, poly) for _, sel, poly in roots_constraints()])
    ip[COEFFS] = O.air_program(A.C_PRE + COEFFS_MAIN, NP, [(sel, poly) for _, sel, poly in coeffs_constraints()])
    return ip


def interactions(R, lf, n):
    """by table number: the identity machine's, the moved words read from the main columns"""
    it = IA.interactions(R, lf, n)
    ent = lambda tab: [(int(s), int(m), int(bus), [int(c) for c in cols]) for s, m, bus, cols in TA._entries(tab)]
    RM, RT = HA.ROOTS_PRE, PA.RT_ROOT
    root = lambda c: RM + RL_ROOT + c - RT if RT <= c < RT + 8 else c
    roots = [(s, m, bus, [root(c) for c in cols]) for s, m, bus, cols in ent(it[ROOTS])]              # (no key column lies in 2 .. 9: LN 0, DEP 1, HK 12 .. 19)
    coef = lambda c: A.C_PRE + CL_C + c - 1 if 1 <= c <= 4 else c
    coeffs = [(s, m, bus, [coef(c) for c in cols]) for s, m, bus, cols in ent(it[COEFFS])]
    out = list(it)
    out[ROOTS], out[COEFFS] = O.interaction_table(roots), O.interaction_table(coeffs)
    return out


# ---------------------------------------------------------------- tables
def shape_key_tables(R, F, b, Q, pow_bits, W, NP):
    """the key's tables by table number from the SHAPE alone: the identity machine's of a view of that shape whose roots and coefficients are all zero, and ACT"""
    blank = dict(roots=[[0] * 8] * R, queries=[(0, [0] * 4, None)] * Q, F=F, b=b, H=4 * R + F + b, W=W, pubs=[0] * NP, pow_bits=pow_bits, final_poly=[[0] * 4] * (1 << F),
                 troot=[0] * 8, qroot=[0] * 8)
    kt = IA.key_tables(blank)
    kt[ROOTS] = kt[ROOTS].copy()
    kt[ROOTS][:R + 2, RT_ACT] = 1
    return kt


def key_tables(view):
    R, Q, F, b, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"], len(view["pubs"])
    return shape_key_tables(R, F, b, Q, view["pow_bits"], W, NP)


def roots_main(view, base, lr=5):
    """ROOTS' sixteen main columns: the identity machine's eight (base), then the root words of the R layer rows, the trace root's row and the quotient root's"""
    t = np.zeros((1 << lr, ROOTS_MAIN), dtype=np.uint32)
    t[:, :TA.ROOTS_MAIN] = base
    rows = [list(r) for r in view["roots"]] + [list(view["troot"]), list(view["qroot"])]
    t[:len(rows), RL_ROOT:] = np.array(rows, dtype=np.uint64).astype(np.uint32)
    return t


def coeffs_main(view, lr):
    t = np.zeros((1 << lr, COEFFS_MAIN), dtype=np.uint32)
    fp = np.array(view["final_poly"], dtype=np.uint64).astype(np.uint32).reshape(-1, 4)
    t[:fp.shape[0], CL_C:] = fp
    return t


def public_values(view):
    return IA.public_values(view)


def tables(view, p24l=None, honest=True, p24r=None, scalars_acc=None):
    """by table number: (main traces, preprocessed traces)"""
    R, Q, F, b, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"], len(view["pubs"])
    lr = log_rows(R, F, b, Q, W, NP)
    main, _ = IA.tables(view, p24l, honest, p24r, scalars_acc)
    main = list(main)
    main[ROOTS], main[COEFFS] = roots_main(view, main[ROOTS], lr[ROOTS]), coeffs_main(view, lr[COEFFS])
    return main, key_tables(view)


def machine(view, p24l=None, honest=True, p24r=None, scalars_acc=None):
    """-> (main traces, preprocessed traces, programs, interaction tables, public values) in machine order"""
    R, Q, F, b, W, NP = len(view["roots"]), len(view["queries"]), view["F"], view["b"], view["W"], len(view["pubs"])
    assert shape_ok(R, F, b, Q, view["pow_bits"], W, NP)
    main, pre = tables(view, p24l, honest, p24r, scalars_acc)
    progs, tabs = programs(R, F, b, view["pow_bits"], W, NP), interactions(R, F + b, 4 * R + F)
    o = order(R, F, b, Q, W, NP)
    return [main[i] for i in o], [pre[i] for i in o], [progs[i] for i in o], [tabs[i] for i in o], public_values(view)
