"""RISC Zero's compress stage through the C++ mirror (zktls_amd/host/guest_prover_hip.cpp: Risc0HipGuestProver::with_compress -- segments -> lift -> join,
crates/guest-prover-r0/src/prover.rs:88-93): a plan of two small segments leaves as ONE blob with ONE proof, which the host checks from (plan, input, ELF, key) alone;
without compress the blob is the segment proofs as before."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from zktls_amd._lib import Params
from zktls_amd.device import verify_shard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "zktls_amd", "libzktls_guest_prover.so")
SYNTHETIC, COMPRESSED, R0_JOINED = 1, 16, 128


class Plan(C.Structure):
    _fields_ = [("log_n", C.c_int32), ("width", C.c_uint32), ("shards", C.c_uint32), ("num_queries", C.c_int32), ("pow_bits", C.c_int32)]


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(SO)
    u8pp, szp, u32p = C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)
    L.zktls_guest_prove_r0.argtypes = [C.c_int, C.c_int, C.POINTER(Plan), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, u8pp, szp, u8pp, szp, C.c_char_p, C.c_size_t]
    L.zktls_guest_prove_r0_compressed.argtypes = L.zktls_guest_prove_r0.argtypes
    L.zktls_r0_join_key_host.argtypes = [C.POINTER(Plan), u32p, C.c_char_p, C.c_size_t]
    L.zktls_verify_compressed_blob.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Plan), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, u32p, C.POINTER(C.c_int)]
    L.zktls_request_digest.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, u32p]
    L.zktls_batch_flags.argtypes = [C.c_char_p, C.c_size_t]
    L.zktls_free.argtypes = [C.c_void_p]
    L.zktls_release_cached.restype = None
    yield L
    L.zktls_release_cached()


def prove(L, entry, plan, cbor, elf):
    out, outn, pr, prn = C.POINTER(C.c_uint8)(), C.c_size_t(), C.POINTER(C.c_uint8)(), C.c_size_t()
    err = C.create_string_buffer(512)
    rc = entry(0, 2, C.byref(plan), cbor, len(cbor), elf, len(elf), C.byref(out), C.byref(outn), C.byref(pr), C.byref(prn), err, 512)
    assert rc == 0, err.value.decode()
    blob = C.string_at(pr, prn.value)
    L.zktls_free(out), L.zktls_free(pr)
    return blob


def entries(blob):
    magic, version, flags, count = struct.unpack_from("<4sIII", blob, 0)
    assert magic == b"ZKTB"
    out, at = [], 16
    for _ in range(count):
        n, = struct.unpack_from("<I", blob, at)
        out.append(blob[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(blob)
    return flags, out


def test_two_segments_leave_as_one_proof_and_the_host_checks_it(lib):
    L = lib
    plan = Plan(10, 16, 2, 12, 0)                            # two segments of 2^10 x 16: RISC Zero's shape with 12 queries, 2^6 final coefficients, one committed layer
    cbor, elf = b"\xa2input of the request", b"\x7fELF guest"
    blob = prove(L, L.zktls_guest_prove_r0_compressed, plan, cbor, elf)
    flags, ent = entries(blob)
    assert flags == SYNTHETIC | COMPRESSED | R0_JOINED == L.zktls_batch_flags(blob, len(blob)) and len(ent) == 2 and len(ent[1]) == 36
    key = (C.c_uint32 * 8)()
    err = C.create_string_buffer(512)
    assert L.zktls_r0_join_key_host(C.byref(plan), key, err, 512) == 0, err.value.decode()      # the verifier's side: the key from the plan, without a GPU
    assert bytes(key) == ent[1][:32] and struct.unpack("<I", ent[1][32:])[0] == 2
    reason = C.c_int(0)
    assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(plan), cbor, len(cbor), elf, len(elf), key, C.byref(reason)) == 0
    other = b"\xa2another request's input"
    assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(plan), other, len(other), elf, len(elf), key, C.byref(reason)) == -2      # another input: other public values
    wrong = (C.c_uint32 * 8)(*[(int(v) + 1) % 2013265921 for v in key])
    assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(plan), cbor, len(cbor), elf, len(elf), wrong, C.byref(reason)) == -1
    three = Plan(10, 16, 3, 12, 0)
    assert L.zktls_verify_compressed_blob(blob, len(blob), C.byref(three), cbor, len(cbor), elf, len(elf), key, C.byref(reason)) == -1
    # a second request of the same plan takes the parked context with both keys: the same bytes
    assert prove(L, L.zktls_guest_prove_r0_compressed, plan, cbor, elf) == blob
    # without compress the blob is what it was: the two segment proofs, each accepted by the host verifier under (request digest | segment index)
    plain = prove(L, L.zktls_guest_prove_r0, plan, cbor, elf)
    flags, ent = entries(plain)
    assert flags == SYNTHETIC and len(ent) == 2
    digest = (C.c_uint32 * 8)()
    L.zktls_request_digest(cbor, len(cbor), elf, len(elf), digest)
    sp = Params(2, 12, 0, 0, 4, 6, 24, 0)
    for s, proof in enumerate(ent):
        assert verify_shard(np.frombuffer(proof, dtype=np.uint8), 10, 16, list(digest) + [s], sp)[0] == 0
