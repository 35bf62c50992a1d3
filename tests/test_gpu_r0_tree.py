"""The tree above RISC Zero's join through the C++ mirror (zktls_amd/host/guest_prover_hip.cpp: Risc0HipGuestProver::with_compress -- segments -> lift -> joins -> top):
with zktls_set_compress_join_size(2) a plan of three small segments leaves as ONE blob with ONE proof above two joins (the second repeats the last segment), which the
host checks from (plan, input, ELF, the joins' key) alone, deriving the top's key itself; with the cap back at 0 a two-segment plan is one join as before."""
import ctypes as C
import struct

import pytest

from test_gpu_r0_compress import COMPRESSED, R0_JOINED, SYNTHETIC, Plan, entries, lib, prove  # noqa: F401  (lib: the module's fixture)

pytestmark = pytest.mark.gpu
TREE = 32


def test_three_segments_under_a_join_size_of_two_leave_as_one_tree_proof(lib):
    L = lib
    L.zktls_set_compress_join_size.argtypes = [C.c_uint32]
    L.zktls_set_compress_join_size.restype = None
    cbor, elf = b"\xa2input of the request", b"\x7fELF guest"
    reason = C.c_int(0)
    err = C.create_string_buffer(512)
    try:
        L.zktls_set_compress_join_size(2)
        plan = Plan(10, 16, 3, 12, 0)                        # three segments of 2^10 x 16: two joins of two, the second one repeating the third segment
        blob = prove(L, L.zktls_guest_prove_r0_compressed, plan, cbor, elf)
        flags, ent = entries(blob)
        assert flags == SYNTHETIC | COMPRESSED | R0_JOINED | TREE == L.zktls_batch_flags(blob, len(blob)) and len(ent) == 2 and len(ent[1]) == 36
        key = (C.c_uint32 * 8)()
        assert L.zktls_r0_join_key_host(C.byref(plan), key, err, 512) == 0, err.value.decode()      # the verifier's side: the JOINS' key from the plan, without a GPU
        assert bytes(key) == ent[1][:32] and struct.unpack("<I", ent[1][32:])[0] == 3
        two = Plan(10, 16, 2, 12, 0)
        key2 = (C.c_uint32 * 8)()
        assert L.zktls_r0_join_key_host(C.byref(two), key2, err, 512) == 0 and bytes(key2) == bytes(key)      # (a join of two under either plan: one shape, one key)
        assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(plan), cbor, len(cbor), elf, len(elf), key, C.byref(reason)) == 0
        other = b"\xa2another request's input"
        assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(plan), other, len(other), elf, len(elf), key, C.byref(reason)) == -2      # another input: other public values
        wrong = (C.c_uint32 * 8)(*[(int(v) + 1) % 2013265921 for v in key])
        assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(plan), cbor, len(cbor), elf, len(elf), wrong, C.byref(reason)) == -1
        four = Plan(10, 16, 4, 12, 0)                        # another segment count (the same joins' key: two joins of two)
        assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(four), cbor, len(cbor), elf, len(elf), key, C.byref(reason)) == -1
        L.zktls_set_compress_join_size(0)
        assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(plan), cbor, len(cbor), elf, len(elf), key, C.byref(reason)) == -1      # (the join size is part of the plan)
        # the cap back at 0: two segments are ONE join, the blob tests/test_gpu_r0_compress.py expects
        blob2 = prove(L, L.zktls_guest_prove_r0_compressed, two, cbor, elf)
        flags, ent = entries(blob2)
        assert flags == SYNTHETIC | COMPRESSED | R0_JOINED == L.zktls_batch_flags(blob2, len(blob2)) and len(ent) == 2 and len(ent[1]) == 36
        assert L.zktls_r0_join_key_host(C.byref(two), key2, err, 512) == 0, err.value.decode()
        assert bytes(key2) == ent[1][:32] and struct.unpack("<I", ent[1][32:])[0] == 2
        assert L.zktls_verify_compressed_blob(blob2, len(blob2), C.byref(two), cbor, len(cbor), elf, len(elf), key2, C.byref(reason)) == 0
    finally:
        L.zktls_set_compress_join_size(0)
