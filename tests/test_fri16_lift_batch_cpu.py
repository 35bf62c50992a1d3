"""zkhip_prove_fri16_lift_batch without a GPU: the symbol, its prototype and job struct against the Python binding, and the argument rules -- every refusal
comes before any device is asked for, and a machine without a device gets ZKHIP_ERR_NO_DEVICE on every job (no fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from zktls_amd import _lib
from zktls_amd._lib import Params, u32p, u8p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE = 0, -1, -2
NAME = b"prove_fri16_lift_batch"
INNER = Params(2, 12, 0, 0, 4, 2, 24, 0)           # fold by 16, 2^2 final coefficients: two committed layers at 2^10 rows
OUTER = Params(1, 12, 4)


def header():
    text = open(os.path.join(ROOT, "include", "zkhip_chips.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def jobs_of(n, cap=64):
    """n well-formed jobs over small dummy buffers (nothing reads them before a device is found)"""
    jobs = (_lib.Fri16LiftJob * max(n, 1))()
    keep = []
    for i in range(n):
        seg, pv, out = np.zeros(64, dtype=np.uint8), np.array([i], dtype=np.uint32), np.zeros(cap, dtype=np.uint8)
        keep.append((seg, pv, out))
        jobs[i].segment_proof = seg.ctypes.data_as(u8p); jobs[i].segment_proof_len = seg.size
        jobs[i].public_values = pv.ctypes.data_as(u32p)
        jobs[i].proof = out.ctypes.data_as(u8p); jobs[i].proof_cap = cap
        jobs[i].proof_len = 77; jobs[i].status = 55                      # (the entry must overwrite both)
    return jobs, keep


def call(L, jobs, n, inner=INNER, outer=OUTER, log_n=10, width=16, n_public=1, devices=None, vk=None):
    vk = np.zeros(8, dtype=np.uint32) if vk is None else vk
    devs = (C.c_int * len(devices))(*devices) if devices else None
    return L.zkhip_prove_fri16_lift_batch(devs, len(devices) if devices else 0, jobs, n, log_n, width, n_public, C.byref(inner) if inner is not None else None,
                                          C.byref(outer) if outer is not None else None, 0, 0, vk.ctypes.data_as(u32p))


def test_symbol_prototype_and_struct_match_the_binding():
    L = _lib.load()
    assert hasattr(L, "zkhip_prove_fri16_lift_batch") and "zkhip_prove_fri16_lift_batch" in _lib.EXPORTS
    text = header()
    m = re.search(r"\bint\s+zkhip_prove_fri16_lift_batch\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert m, "include/zkhip_chips.h does not declare zkhip_prove_fri16_lift_batch"
    args = [a.strip() for a in m.group(1).split(",")]
    names = [re.sub(r"\[.*?\]", "", a).split()[-1].lstrip("*") for a in args]
    assert names == ["devices", "n_devices", "jobs", "n_jobs", "log_n", "width", "n_public", "inner_prm", "outer_prm", "in_flight_per_device", "verify", "vk"]
    argtypes = L.zkhip_prove_fri16_lift_batch.argtypes
    assert len(argtypes) == len(args)
    for a, t in zip(args, argtypes):
        assert ("*" in a or "[" in a) == hasattr(t, "contents"), a                 # pointers face pointers, position by position
    assert argtypes[2] == C.POINTER(_lib.Fri16LiftJob) and argtypes[6] == C.c_size_t and argtypes[5] == C.c_uint32
    s = re.search(r"typedef\s+struct\s*(?:\w+\s*)?\{([^}]*)\}\s*zkhip_fri16_lift_job\s*;", text, flags=re.S)
    assert s, "include/zkhip_chips.h does not declare zkhip_fri16_lift_job"
    fields = []
    for decl in s.group(1).split(";"):
        if decl.strip():
            fields.append((decl.split()[-1].lstrip("*"), "*" in decl, "size_t" in decl))
    assert [f[0] for f in fields] == [n for n, _ in _lib.Fri16LiftJob._fields_]
    for (name, ptr, size), (_, t) in zip(fields, _lib.Fri16LiftJob._fields_):
        assert ptr == hasattr(t, "contents"), name
        assert C.sizeof(t) == (8 if ptr or size else 4), name
    assert C.sizeof(_lib.Fri16LiftJob) == 56                                       # five 8-byte words, the length, the status and its padding


def test_an_empty_batch_is_fine():
    L = _lib.load()
    jobs, _ = jobs_of(0)
    assert call(L, jobs, 0) == OK
    L.zkhip_release_cached_contexts()


def test_null_and_negative_arguments_are_refused_in_the_entrys_name():
    L = _lib.load()
    jobs, _ = jobs_of(3)
    for rc in (call(L, None, 3), call(L, jobs, 3, inner=None), call(L, jobs, 3, outer=None), call(L, jobs, -1)):
        assert rc == INVALID
        assert NAME in L.zkhip_last_error()
    assert L.zkhip_prove_fri16_lift_batch(None, 0, jobs, 3, 10, 16, 1, C.byref(INNER), C.byref(OUTER), 0, 0, None) == INVALID and NAME in L.zkhip_last_error()
    assert all(j.status == 55 and j.proof_len == 77 for j in jobs)                 # refused before a job was touched


def test_shape_refusals_come_by_message_before_any_device_is_asked_for():
    L = _lib.load()
    jobs, _ = jobs_of(3)
    # fold by 2: not a segment shape
    assert call(L, jobs, 3, inner=Params(1, 12, 4)) == INVALID
    msg = L.zkhip_last_error()
    assert NAME in msg and b"fold-by-16" in msg and b"no CPU fallback" not in msg
    assert all(j.status == INVALID and j.proof_len == 0 for j in jobs)             # every job's status is set before anything runs
    # fold by 16, but no committed layer at this height (10 - 2 is a multiple of 4; 11 - 2 is not; 2 - 2 leaves none)
    for log_n in (11, 2):
        assert call(L, jobs, 3, log_n=log_n) == INVALID
        assert NAME in L.zkhip_last_error() and b"committed layer" in L.zkhip_last_error()
    # more inner public values than the head of the transcript takes
    assert call(L, jobs, 3, n_public=31) == INVALID
    msg = L.zkhip_last_error()
    assert NAME in msg and b"30 inner public values" in msg and b"no CPU fallback" not in msg
    # a device list that names a device twice is refused like every batch entry's
    assert call(L, jobs, 3, devices=[1, 1]) == INVALID and b"twice" in L.zkhip_last_error()


def test_without_a_device_every_job_is_marked_and_nothing_is_proven():
    L = _lib.load()
    if L.zkhip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    jobs, _ = jobs_of(5)
    vk = np.ones(8, dtype=np.uint32)
    assert call(L, jobs, 5, vk=vk) == NO_DEVICE
    assert b"no CPU fallback" in L.zkhip_last_error()
    assert all(j.status == NO_DEVICE and j.proof_len == 0 for j in jobs)
    assert not vk.any()
    # the Python entry raises with the same code
    from zktls_amd.device import prove_fri16_lift_batch
    with pytest.raises(_lib.ZkHipError) as e:
        prove_fri16_lift_batch(None, [np.zeros(64, dtype=np.uint8)] * 2, 10, 16, [[1], [2]], INNER, OUTER)
    assert e.value.code == NO_DEVICE
    proofs, statuses, _ = prove_fri16_lift_batch(None, [np.zeros(64, dtype=np.uint8)] * 2, 10, 16, [[1], [2]], INNER, OUTER, raise_on_error=False)
    assert statuses == [NO_DEVICE, NO_DEVICE] and all(p.size == 0 for p in proofs)
    L.zkhip_release_cached_contexts()
