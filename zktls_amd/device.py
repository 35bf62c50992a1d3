"""Thin object layer over the C ABI: a context bound to one GPU + stream, and device
buffers.  Used by the tests, bench.py and the host-side prover mirror (prover.py).
All numpy arrays crossing this layer are CANONICAL residues unless a name says monty.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import Params, ProveDebug, check, from_monty, to_monty, u32p, u8p


SHA256_WIDTH, SHA256_PUBLIC, SHA256_PADDING_PUBLIC = 640, 91, 75      # include/zkhip.h: ZKHIP_SHA256_*


class DeviceBuffer:
    """A device allocation of uint32 words owned by a Context (or wrapping a torch tensor)."""

    def __init__(self, ctx, nwords, ptr=None, owner=None):
        self.ctx = ctx
        self.nwords = int(nwords)
        self._owned = ptr is None
        self._owner = owner
        if ptr is None:
            p = C.c_void_p()
            check(ctx.lib.zkhip_malloc(ctx.handle, C.c_size_t(self.nwords * 4), C.byref(p)))
            ptr = p.value
            ctx._buffers.add(self)
        self.ptr = ptr

    def offset(self, words):
        return C.c_void_p(self.ptr + 4 * int(words))

    def upload_monty(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        assert arr.size <= self.nwords
        check(self.ctx.lib.zkhip_memcpy_h2d(self.ctx.handle, C.c_void_p(self.ptr), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.size * 4)))

    def upload(self, canonical):
        self.upload_monty(to_monty(canonical))

    def download_monty(self, nwords=None, offset=0):
        n = self.nwords - offset if nwords is None else int(nwords)
        out = np.empty(n, dtype=np.uint32)
        check(self.ctx.lib.zkhip_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), self.offset(offset), C.c_size_t(n * 4)))
        return out

    def download(self, nwords=None, offset=0):
        return from_monty(self.download_monty(nwords, offset))

    def free(self):
        if self._owned and self.ptr and self.ctx.handle:
            self.ctx.lib.zkhip_free(self.ctx.handle, C.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView:
    """words of a DeviceBuffer from an offset on (a column slice of a row-major matrix is a view with the matrix's row pitch)"""

    def __init__(self, buf, words):
        self.base = buf
        self.ptr = buf.ptr + 4 * int(words)
        self.nwords = buf.nwords - int(words)       # to the end of the allocation: the wrappers that size a call by the buffer take a view too


class Context:
    def __init__(self, device=0, stream=None):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.zkhip_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
        self.handle = h
        self.device = device
        self._buffers = weakref.WeakSet()     # allocations made through this context, freed with it

    def close(self):
        if self.handle:
            for b in list(self._buffers):
                b.free()
            self.lib.zkhip_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.zkhip_ctx_sync(self.handle))

    def set_lde_fusion(self, on):
        """fused middle launch of 2^20-row LDEs on (default) / off; returns the previous setting"""
        r = self.lib.zkhip_ctx_set_lde_fusion(self.handle, 1 if on else 0)
        if r < 0:
            check(r)
        return bool(r)

    @property
    def stream(self):
        return self.lib.zkhip_ctx_stream(self.handle)

    def alloc(self, nwords):
        return DeviceBuffer(self, nwords)

    def wrap(self, tensor):
        """wrap a torch CUDA tensor (int32/uint32 storage) without copying"""
        return DeviceBuffer(self, tensor.numel(), ptr=tensor.data_ptr(), owner=tensor)

    def from_numpy(self, canonical):
        a = np.ascontiguousarray(canonical, dtype=np.uint32)
        buf = self.alloc(a.size)
        buf.upload(a)
        return buf

    # ---- synthetic data
    # (ld / in_ld / out_ld below: a matrix's row pitch in words when it exceeds its width; matrices are DeviceBuffers or DeviceViews)
    def fill_uniform(self, seed, log_n, width, out=None, ld=None):
        ld = ld or width
        out = out or self.alloc(ld << log_n)
        check(self.lib.zkhip_fill_uniform(self.handle, seed, log_n, width, C.c_void_p(out.ptr), ld))
        return out

    def gen_trace_logup_cross(self, seed, shard, partner_shard, log_n, width, partner_width, pairs, out=None, ld=None):
        ld = ld or width
        out = out or self.alloc(ld << log_n)
        check(self.lib.zkhip_gen_trace_logup_cross(self.handle, seed, shard, partner_shard, log_n, width, partner_width, pairs, C.c_void_p(out.ptr), ld))
        return out

    def gen_trace(self, seed, shard, log_n, width, out=None, ld=None):
        ld = ld or width
        out = out or self.alloc(ld << log_n)
        check(self.lib.zkhip_gen_trace(self.handle, seed, shard, log_n, width, C.c_void_p(out.ptr), ld))
        return out

    def gen_trace_logup(self, seed, shard, log_n, width, pairs, out=None, ld=None):
        ld = ld or width
        out = out or self.alloc(ld << log_n)
        check(self.lib.zkhip_gen_trace_logup(self.handle, seed, shard, log_n, width, pairs, C.c_void_p(out.ptr), ld))
        return out

    def perm_trace(self, trace, log_n, width, pairs, gamma, beta, out=None, ld=None):
        """ld: the trace's row pitch in words when it exceeds its width"""
        out = out or self.alloc((4 * (pairs + 1)) << log_n)
        g = to_monty(np.asarray(gamma, dtype=np.uint32))
        b = to_monty(np.asarray(beta, dtype=np.uint32))
        check(self.lib.zkhip_perm_trace(self.handle, C.c_void_p(trace.ptr), ld or width, log_n, width, pairs,
                                        g.ctypes.data_as(u32p), b.ctypes.data_as(u32p), C.c_void_p(out.ptr)))
        return out

    # ---- NTT / LDE
    def dft(self, src, log_n, width, inverse=False, bitrev_out=False, out=None, in_ld=None, out_ld=None):
        in_ld, out_ld = in_ld or width, out_ld or width
        out = out or self.alloc(out_ld << log_n)
        check(self.lib.zkhip_dft(self.handle, C.c_void_p(src.ptr), in_ld, C.c_void_p(out.ptr), out_ld, log_n, width,
                                 int(inverse), int(bitrev_out)))
        return out

    def coset_lde(self, src, log_n, width, log_blowup=1, shift=31, out=None, in_ld=None, out_ld=None, out_col=0):
        out_ld = out_ld or width
        in_ld = in_ld or width
        out = out or self.alloc(out_ld << (log_n + log_blowup))
        check(self.lib.zkhip_coset_lde(self.handle, C.c_void_p(src.ptr), in_ld, C.c_void_p(out.ptr + 4 * int(out_col)), out_ld,
                                       log_n, width, log_blowup, shift))
        return out

    def ntt_pass(self, src, dst, log_n, width, which):
        """which 0 / 1: stand-alone passes src -> dst; which 2..5: the LDE launches of a proof on this context's own workspaces (dst unused)"""
        check(self.lib.zkhip_ntt_pass(self.handle, C.c_void_p(src.ptr) if src is not None else None,
                                      C.c_void_p(dst.ptr) if dst is not None else None, width, log_n, width, which))

    # ---- Poseidon2 / Merkle
    def poseidon2_permute(self, states):
        check(self.lib.zkhip_poseidon2_permute(self.handle, C.c_void_p(states.ptr), states.nwords // 16))

    def _mat_args(self, mats, n_fixed=2):
        """mats: tuples of n_fixed entries (buffer or view, width, ...), each optionally followed by the row pitch (default: the width)"""
        n = len(mats)
        ptrs = (C.c_void_p * n)(*[m[0].ptr for m in mats])
        lds = (C.c_size_t * n)(*[m[n_fixed] if len(m) > n_fixed else m[1] for m in mats])
        ws = (C.c_uint32 * n)(*[m[1] for m in mats])
        return ptrs, lds, ws

    def hash_rows(self, mats, height, out=None):
        """mats: list of (buffer or view, width) with contiguous rows, or (buffer or view, width, ld)"""
        out = out or self.alloc(8 * height)
        ptrs, lds, ws = self._mat_args(mats)
        check(self.lib.zkhip_hash_rows(self.handle, ptrs, lds, ws, len(mats), height, C.c_void_p(out.ptr)))
        return out

    def merkle_commit(self, mats, log_h, out=None):
        """mats: as for hash_rows"""
        out = out or self.alloc(8 * ((2 << log_h) - 1))
        ptrs, lds, ws = self._mat_args(mats)
        check(self.lib.zkhip_merkle_commit(self.handle, ptrs, lds, ws, len(mats), log_h, C.c_void_p(out.ptr)))
        return out

    def merkle_commit_mixed(self, mats, out=None):
        """mats: list of (buffer or view, width, log_height) or (buffer or view, width, log_height, ld); tree sized for the tallest"""
        log_h = max(m[2] for m in mats)
        out = out or self.alloc(8 * ((2 << log_h) - 1))
        ptrs, lds, ws = self._mat_args(mats, 3)
        lhs = (C.c_int * len(mats))(*[m[2] for m in mats])
        check(self.lib.zkhip_merkle_commit_mixed(self.handle, ptrs, lds, ws, lhs, len(mats), C.c_void_p(out.ptr)))
        return out

    def merkle_commit_p24_colmajor(self, mat, cols, log_rows, out=None):
        out = out or self.alloc(8 * ((2 << log_rows) - 1))
        check(self.lib.zkhip_merkle_commit_p24_colmajor(self.handle, C.c_void_p(mat.ptr), cols, log_rows, C.c_void_p(out.ptr)))
        return out

    def batch_interpolate_colmajor(self, evals, count, log_size, out=None):
        out = out or self.alloc(count << log_size)
        check(self.lib.zkhip_batch_interpolate_colmajor(self.handle, C.c_void_p(evals.ptr), C.c_void_p(out.ptr), count, log_size))
        return out

    def batch_expand_colmajor(self, coeffs, count, log_size, log_blowup=2, shift=31, out=None):
        out = out or self.alloc(count << (log_size + log_blowup))
        check(self.lib.zkhip_batch_expand_colmajor(self.handle, C.c_void_p(coeffs.ptr), C.c_void_p(out.ptr), count, log_size, log_blowup, shift))
        return out

    # ---- RISC Zero Hal operators (column-major vectors; ext_field 0: x^4 = 11, 1: x^4 = -11)
    def eltwise_add(self, a, b, out=None):
        out = out or self.alloc(a.nwords)
        check(self.lib.zkhip_eltwise_add(self.handle, C.c_void_p(out.ptr), C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.nwords))
        return out

    def eltwise_copy(self, a, out=None):
        out = out or self.alloc(a.nwords)
        check(self.lib.zkhip_eltwise_copy(self.handle, C.c_void_p(out.ptr), C.c_void_p(a.ptr), a.nwords))
        return out

    def eltwise_zeroize(self, io):
        check(self.lib.zkhip_eltwise_zeroize(self.handle, C.c_void_p(io.ptr), io.nwords))
        return io

    def eltwise_sum_ext(self, inp, count, out=None):
        out = out or self.alloc(4 * count)
        check(self.lib.zkhip_eltwise_sum_ext(self.handle, C.c_void_p(out.ptr), C.c_void_p(inp.ptr), count, inp.nwords // (4 * count)))
        return out

    def zk_shift(self, io, count, log_size, shift=3):
        check(self.lib.zkhip_zk_shift(self.handle, C.c_void_p(io.ptr), count, log_size, shift))
        return io

    def mix_poly_coeffs(self, out, mix_start, mix, inp, combos, input_size, count, ext_field=0):
        ms = to_monty(np.asarray(mix_start, dtype=np.uint32))
        mx = to_monty(np.asarray(mix, dtype=np.uint32))
        check(self.lib.zkhip_mix_poly_coeffs(self.handle, C.c_void_p(out.ptr), ms.ctypes.data_as(u32p), mx.ctypes.data_as(u32p),
                                             C.c_void_p(inp.ptr), C.c_void_p(combos.ptr), input_size, count, ext_field))
        return out

    def batch_evaluate_any(self, coeffs, log_size, which, xs, ext_field=0, out=None):
        n = which.nwords
        out = out or self.alloc(4 * n)
        check(self.lib.zkhip_batch_evaluate_any(self.handle, C.c_void_p(coeffs.ptr), log_size, C.c_void_p(which.ptr), C.c_void_p(xs.ptr),
                                                C.c_void_p(out.ptr), n, ext_field))
        return out

    def gather_sample(self, src, idx, size, stride, out=None):
        out = out or self.alloc(size)
        check(self.lib.zkhip_gather_sample(self.handle, C.c_void_p(out.ptr), C.c_void_p(src.ptr), idx, size, stride))
        return out

    def scatter(self, into, index, offsets, values):
        check(self.lib.zkhip_scatter(self.handle, C.c_void_p(into.ptr), C.c_void_p(index.ptr), C.c_void_p(offsets.ptr), C.c_void_p(values.ptr),
                                     index.nwords - 1))
        return into

    def prefix_products_ext(self, io, ext_field=0):
        check(self.lib.zkhip_prefix_products_ext(self.handle, C.c_void_p(io.ptr), io.nwords // 4, ext_field))
        return io

    def hash_rows_sha256(self, mat, cols, rows, out=None):
        out = out or self.alloc(8 * rows)
        check(self.lib.zkhip_hash_rows_sha256(self.handle, C.c_void_p(mat.ptr), cols, rows, C.c_void_p(out.ptr)))
        return out

    def hash_fold_sha256(self, children, count, out=None):
        out = out or self.alloc(8 * count)
        check(self.lib.zkhip_hash_fold_sha256(self.handle, C.c_void_p(children.ptr), C.c_void_p(out.ptr), count))
        return out

    def merkle_commit_sha256_colmajor(self, mat, cols, log_rows, out=None):
        out = out or self.alloc(8 * ((2 << log_rows) - 1))
        check(self.lib.zkhip_merkle_commit_sha256_colmajor(self.handle, C.c_void_p(mat.ptr), cols, log_rows, C.c_void_p(out.ptr)))
        return out

    def from_raw(self, words):
        """upload 32-bit words as they are (indices, digests: no Montgomery conversion)"""
        a = np.ascontiguousarray(words, dtype=np.uint32)
        buf = self.alloc(max(a.size, 1))
        buf.upload_monty(a)
        return buf

    # ---- STARK stages
    def quotient_values(self, lde, log_n, width, alpha, out=None, ld=None):
        out = out or self.alloc(4 << (log_n + 1))
        a = to_monty(np.asarray(alpha, dtype=np.uint32))
        check(self.lib.zkhip_quotient_values(self.handle, C.c_void_p(lde.ptr), ld or width, log_n, width,
                                             a.ctypes.data_as(u32p), C.c_void_p(out.ptr)))
        return out

    def open_at(self, lde, log_n, log_blowup, width, points, ld=None):
        pts = to_monty(np.ascontiguousarray(points, dtype=np.uint32).reshape(-1, 4))
        out = np.empty((pts.shape[0], width, 4), dtype=np.uint32)
        check(self.lib.zkhip_open_at(self.handle, C.c_void_p(lde.ptr), ld or width, log_n, log_blowup, width,
                                     pts.ctypes.data_as(u32p), pts.shape[0], out.ctypes.data_as(u32p)))
        return from_monty(out)

    def fri_fold(self, src, log_h, beta, out=None):
        out = out or self.alloc(4 << (log_h - 1))
        b = to_monty(np.asarray(beta, dtype=np.uint32))
        check(self.lib.zkhip_fri_fold(self.handle, C.c_void_p(src.ptr), log_h, b.ctypes.data_as(u32p), C.c_void_p(out.ptr)))
        return out

    def fri_fold_k(self, src, log_h, log_arity, beta, out=None):
        out = out or self.alloc(4 << (log_h - log_arity))
        b = to_monty(np.asarray(beta, dtype=np.uint32))
        check(self.lib.zkhip_fri_fold_k(self.handle, C.c_void_p(src.ptr), log_h, log_arity, b.ctypes.data_as(u32p), C.c_void_p(out.ptr)))
        return out

    def fri_fold_k_dev(self, src, log_h, log_arity, beta, add=None, out=None):
        """fri_fold_k with the challenge in device memory (beta: a buffer of 4 words), as the prover's commit phase folds; add: a device vector added to the result"""
        out = out or self.alloc(4 << (log_h - log_arity))
        check(self.lib.zkhip_fri_fold_k_dev(self.handle, C.c_void_p(src.ptr), log_h, log_arity, C.c_void_p(beta.ptr),
                                            C.c_void_p(add.ptr) if add is not None else None, C.c_void_p(out.ptr)))
        return out

    def reduced_opening(self, tlde, t_ld, width, log_rows, weights, n_weights, dinv, scalars, out, plde=None, p_ld=0, p_width=0,
                        qlde=None, q_ld=0, q_width=0, accumulate=0):
        """the FRI input of one chip on the caller's device data (zkhip_reduced_opening); scalars: [10][4] canonical, in the header's order; matrices, weights,
        dinv and out are buffers or views (or raw addresses); returns the row-sum forms taken for (trace, permutation) block"""
        def addr(b):
            return None if b is None else C.c_void_p(getattr(b, "ptr", b))
        sc = to_monty(np.ascontiguousarray(scalars, dtype=np.uint32).reshape(40))
        forms = (C.c_int * 2)(-2, -2)
        check(self.lib.zkhip_reduced_opening(self.handle, addr(tlde), t_ld, width, addr(plde), p_ld, p_width, addr(qlde), q_ld, q_width, log_rows,
                                             addr(weights), n_weights, addr(dinv), sc.ctypes.data_as(u32p), int(accumulate), addr(out), forms))
        return forms[0], forms[1]

    def grind(self, state, slot, bits, base, count, result=0xFFFFFFFF):
        """one launch of the proof-of-work search over [base, base + count); state: 16 canonical words of the sponge with the pending inputs in [0, slot);
        returns min(result, the smallest hit), 0xFFFFFFFF for none"""
        st = to_monty(np.ascontiguousarray(state, dtype=np.uint32).reshape(16))
        res = C.c_uint32(result)
        check(self.lib.zkhip_grind(self.handle, st.ctypes.data_as(u32p), int(slot), int(bits), int(base), int(count), C.byref(res)))
        return res.value

    def commit(self, trace, log_n, width, log_blowup=1, hash_width=16, ld=None):
        """coset LDE + Merkle tree + root in one call; returns (lde, tree, root[8] canonical)"""
        h = log_n + log_blowup
        lde, tree = self.alloc(width << h), self.alloc(8 * ((2 << h) - 1))
        root = np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_commit(self.handle, C.c_void_p(trace.ptr), ld or width, log_n, width, log_blowup, hash_width,
                                    C.c_void_p(lde.ptr), C.c_void_p(tree.ptr), root.ctypes.data_as(u32p)))
        return lde, tree, root

    # ---- whole shard
    def prove_shard(self, trace, log_n, width, public_values=(), params=None, ld=None):
        params = params or Params(1, 100, 16, 0)
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        size = self.lib.zkhip_proof_size(log_n, width, C.byref(params), pv.size)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_shard(self.handle, C.c_void_p(trace.ptr), ld or width, log_n, width,
                                         pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                         buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def prove_shard_air(self, program, trace, log_n, width, public_values=(), params=None):
        """prove against a constraint program (the AIR as data: include/zkhip.h); program: numpy u32 words"""
        params = params or Params(1, 100, 16, 0)
        prog = np.ascontiguousarray(program, dtype=np.uint32)
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        size = self.lib.zkhip_proof_size_air(prog.ctypes.data_as(u32p), prog.size, log_n, width, C.byref(params), pv.size)
        if size == 0:
            check(self.lib.zkhip_air_validate(prog.ctypes.data_as(u32p), prog.size, width, pv.size))
            raise _lib.ZkHipError(-1, "prove_shard_air: bad shape (degree 4 / 5 programs need log_blowup >= 2; no logup_pairs)")
        buf = np.empty(max(size, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_shard_air(self.handle, prog.ctypes.data_as(u32p), prog.size, C.c_void_p(trace.ptr), width, log_n, width,
                                             pv.ctypes.data_as(u32p), pv.size, C.byref(params), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    # ---- the SHA-256 compression chip (csrc/sha256_chip.hip)
    def sha256_gen_trace(self, blocks, n_blocks=None, out=None, message_len=None):
        """blocks: the padded message, a multiple of 64 long (sha256_pad / sha256_air.pad remember the message's length; otherwise pass
        message_len) -> (device trace [64 n_blocks][640], public values [91]: 16 digest limbs + the 75 padding values)"""
        if message_len is None:
            message_len = getattr(blocks, "message_len", None)
        if message_len is None:
            raise TypeError("sha256_gen_trace: the message length is part of the statement (pass message_len)")
        b = np.frombuffer(bytes(blocks), dtype=np.uint8)
        active = b.size // 64
        n_blocks = n_blocks or 1 << max(active - 1, 0).bit_length()
        out = out or self.alloc(64 * n_blocks * SHA256_WIDTH)
        limbs = np.zeros(SHA256_PUBLIC, dtype=np.uint32)
        check(self.lib.zkhip_sha256_gen_trace(self.handle, b.ctypes.data_as(u8p), active, n_blocks, message_len, C.c_void_p(out.ptr), SHA256_WIDTH, limbs.ctypes.data_as(u32p)))
        return out, limbs

    def prove_sha256(self, message, params=None):
        """-> (digest bytes, proof bytes): "I know a message with this SHA-256 digest" """
        params = params or Params(1, 100, 16)
        m = np.frombuffer(bytes(message), dtype=np.uint8) if len(message) else np.zeros(1, dtype=np.uint8)
        size = self.lib.zkhip_sha256_proof_size(len(message), C.byref(params))
        if size == 0:
            raise _lib.ZkHipError(-1, "prove_sha256: bad shape or message too long")
        buf = np.empty(size, dtype=np.uint8)
        digest = np.zeros(32, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_sha256(self.handle, m.ctypes.data_as(u8p), len(message), C.byref(params), digest.ctypes.data_as(u8p),
                                          buf.ctypes.data_as(u8p), size, C.byref(got)))
        return digest.tobytes(), buf[: got.value]

    def p2chip_gen_merkle_trace(self, leaves, siblings, indices, log_n=None, hashed_rows=False):
        """the Poseidon2 chip's trace for a set of Merkle paths (numpy arrays of canonical words: leaves [n][8] -- or, with hashed_rows, the
        opened rows [n][8 k], hashed in-circuit --, siblings [n][depth][8], indices [n]) -> (device buffer [2^log_n][360], roots [n][8], log_n)"""
        lv = np.ascontiguousarray(leaves, dtype=np.uint32)
        sb = np.ascontiguousarray(siblings, dtype=np.uint32)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        n, depth = lv.shape[0], sb.shape[1]
        rw = lv.shape[1] if hashed_rows else 0
        if log_n is None:
            log_n = max(5, (n * (depth + rw // 8) - 1).bit_length())
        out = self.alloc(360 << log_n)
        roots = np.zeros((n, 8), dtype=np.uint32)
        check(self.lib.zkhip_p2chip_gen_merkle_trace(self.handle, lv.ctypes.data_as(u32p), rw, sb.ctypes.data_as(u32p), ix.ctypes.data_as(u32p), n, depth, log_n,
                                                     C.c_void_p(out.ptr), 360, roots.ctypes.data_as(u32p)))
        return out, roots, log_n

    def prove_merkle_paths(self, leaves, siblings, indices, root, params=None, hashed_rows=False):
        """-> proof bytes of "I know len(leaves) Merkle paths (with hashed_rows: openings of whole rows) that end in root" (the Poseidon2 chip)"""
        params = params or Params(1, 100, 16)
        lv = np.ascontiguousarray(leaves, dtype=np.uint32)
        sb = np.ascontiguousarray(siblings, dtype=np.uint32)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        rt = np.ascontiguousarray(root, dtype=np.uint32)
        n, depth = lv.shape[0], sb.shape[1]
        rw = lv.shape[1] if hashed_rows else 0
        size = self.lib.zkhip_merkle_paths_proof_size(n, depth, rw, C.byref(params))
        buf = np.empty(max(size, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_merkle_paths(self.handle, lv.ctypes.data_as(u32p), rw, sb.ctypes.data_as(u32p), ix.ctypes.data_as(u32p), n, depth,
                                                rt.ctypes.data_as(u32p), C.byref(params), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def p24chip_gen_merkle_trace(self, leaves, siblings, indices, log_n=None, row_width=0):
        """the width-24 Poseidon2 chip's trace for a set of Merkle paths of a RISC Zero-shape commitment (numpy arrays of canonical words:
        leaves [n][8] digests -- or, with row_width > 0 (a multiple of 4), the opened rows [n][row_width], hashed in-circuit --, siblings
        [n][depth][8], indices [n]) -> (device buffer [2^log_n][540], roots [n][8], log_n)"""
        lv = np.ascontiguousarray(leaves, dtype=np.uint32)
        sb = np.ascontiguousarray(siblings, dtype=np.uint32)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        n, depth = lv.shape[0], sb.shape[1]
        if log_n is None:
            log_n = max(5, (n * (depth + (row_width + 15) // 16) - 1).bit_length())
        out = self.alloc(540 << log_n)
        roots = np.zeros((n, 8), dtype=np.uint32)
        check(self.lib.zkhip_p24chip_gen_merkle_trace(self.handle, lv.ctypes.data_as(u32p), row_width, sb.ctypes.data_as(u32p), ix.ctypes.data_as(u32p), n, depth,
                                                      log_n, C.c_void_p(out.ptr), 540, roots.ctypes.data_as(u32p)))
        return out, roots, log_n

    def prove_merkle_paths_p24(self, leaves, siblings, indices, root, params=None, row_width=0):
        """-> proof bytes of "I know len(leaves) openings of this RISC Zero-shape commitment (row_width > 0: whole opened rows) that end in root"
        (the width-24 Poseidon2 chip)"""
        params = params or Params(1, 100, 16)
        lv = np.ascontiguousarray(leaves, dtype=np.uint32)
        sb = np.ascontiguousarray(siblings, dtype=np.uint32)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        rt = np.ascontiguousarray(root, dtype=np.uint32)
        n, depth = lv.shape[0], sb.shape[1]
        size = self.lib.zkhip_merkle_paths_p24_proof_size(n, depth, row_width, C.byref(params))
        buf = np.empty(max(size, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_merkle_paths_p24(self.handle, lv.ctypes.data_as(u32p), row_width, sb.ctypes.data_as(u32p), ix.ctypes.data_as(u32p), n, depth,
                                                    rt.ctypes.data_as(u32p), C.byref(params), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def sha256_setup(self, params=None):
        """zkhip_sha256_setup: the SHA-256 machine's key (the range table's preprocessed values, committed once) -> MachineKey; .root is the vk"""
        params = params or Params(1, 100, 16)
        handle = C.c_void_p()
        root = np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_sha256_setup(self.handle, C.byref(params), C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, [4])

    def machine_verifier_setup(self, inner, params=None, n_proofs=1):
        """zkhip_machine_verifier_setup: the key of the machine that verifies n_proofs proofs of the inner machine (InnerMachine) in-circuit"""
        params = params or Params()
        handle, root = C.c_void_p(), np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_machine_verifier_setup(self.handle, C.byref(inner.desc), n_proofs, C.byref(params), C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, None)

    def prove_machine_verifier(self, key, inner, proofs, public_values, params=None):
        """zkhip_prove_machine_verifier: proofs = a list of version-11 proofs of the inner machine, public_values one list per proof -> ONE proof"""
        params = params or Params()
        sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in proofs]
        n = len(sps)
        pv = np.ascontiguousarray(np.array([list(v) for v in public_values], dtype=np.uint32).reshape(n, -1)) if inner.n_public else np.zeros((n, 1), dtype=np.uint32)
        size = self.lib.zkhip_machine_verifier_proof_size(C.byref(inner.desc), n, C.byref(params))
        if size == 0:
            check(-1)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        ptrs = (u8p * n)(*[sp.ctypes.data_as(u8p) for sp in sps])
        lens = (C.c_size_t * n)(*[sp.size for sp in sps])
        check(self.lib.zkhip_prove_machine_verifier(self.handle, key.handle, C.byref(inner.desc), ptrs, lens, n, pv.ctypes.data_as(u32p), inner.n_public, C.byref(params),
                                                    buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def sha256_compress_setup(self, message_len, log_blocks_per_shard, inner=None, outer=None):
        """zkhip_sha256_compress_setup -> MachineKey (key.root = vk) for compressed chains of messages with this many shards"""
        inner, outer = inner or Params(1, 100, 16), outer or Params(1, 100, 16)
        handle = C.c_void_p()
        vk = np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_sha256_compress_setup(self.handle, message_len, log_blocks_per_shard, C.byref(inner), C.byref(outer), C.byref(handle), vk.ctypes.data_as(u32p)))
        return MachineKey(self, handle, vk, None)

    def prove_sha256_compressed(self, key, message, log_blocks_per_shard, inner=None, outer=None, devices=None, in_flight=2):
        """zkhip_prove_sha256_compressed: the message as a chain of shards (dealt over `devices`), the shards verified in-circuit on this
        context's device -> (digest bytes, chain [(n_shards + 1) x 8], ONE proof)"""
        inner, outer = inner or Params(1, 100, 16), outer or Params(1, 100, 16)
        m = np.frombuffer(bytes(message), dtype=np.uint8) if len(message) else np.zeros(1, dtype=np.uint8)
        n = self.lib.zkhip_sha256_sharded_count(len(message), log_blocks_per_shard)
        size = self.lib.zkhip_sha256_compressed_proof_size(len(message), log_blocks_per_shard, C.byref(inner), C.byref(outer))
        if n == 0 or size == 0:
            raise _lib.ZkHipError(-1, "prove_sha256_compressed: bad shape")
        chain = np.zeros((n + 1, 8), dtype=np.uint32)
        digest = np.zeros(32, dtype=np.uint8)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        devs = (C.c_int * len(devices))(*devices) if devices else None
        check(self.lib.zkhip_prove_sha256_compressed(self.handle, key.handle, devs, len(devices) if devices else 0, m.ctypes.data_as(u8p), len(message), log_blocks_per_shard,
                                                     C.byref(inner), C.byref(outer), in_flight, digest.ctypes.data_as(u8p), chain.ctypes.data_as(u32p),
                                                     buf.ctypes.data_as(u8p), size, C.byref(got)))
        return digest.tobytes(), chain, buf[: got.value]

    def prove_sha256_machine(self, key, message, params=None):
        """-> (digest bytes, proof bytes): the SHA-256 chip + its range table as a keyed machine (proof version 11)"""
        params = params or Params(1, 100, 16)
        m = np.frombuffer(bytes(message), dtype=np.uint8) if len(message) else np.zeros(1, dtype=np.uint8)
        size = self.lib.zkhip_sha256_machine_proof_size(len(message), C.byref(params))
        if size == 0:
            raise _lib.ZkHipError(-1, "prove_sha256_machine: bad shape or message too long")
        buf = np.empty(size, dtype=np.uint8)
        digest = np.zeros(32, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_sha256_machine(self.handle, key.handle, m.ctypes.data_as(u8p), len(message), C.byref(params), digest.ctypes.data_as(u8p),
                                                  buf.ctypes.data_as(u8p), size, C.byref(got)))
        return digest.tobytes(), buf[: got.value]

    def quotient_values_air(self, program, lde, log_n, width, public_values, alpha, out=None, log_quotient_degree=1):
        out = out or self.alloc(4 << (log_n + log_quotient_degree))
        prog = np.ascontiguousarray(program, dtype=np.uint32)
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        a = to_monty(np.asarray(alpha, dtype=np.uint32))
        check(self.lib.zkhip_quotient_values_air(self.handle, prog.ctypes.data_as(u32p), prog.size, C.c_void_p(lde.ptr), width, log_n, width,
                                                 pv.ctypes.data_as(u32p), pv.size, a.ctypes.data_as(u32p), C.c_void_p(out.ptr)))
        return out

    def prove_shard_host(self, host_trace, public_values=(), params=None, host_ptr=None, log_n=None, width=None):
        """host_trace: numpy [2^log_n][width] canonical words in host memory (or a raw host pointer + shape)"""
        params = params or Params(1, 100, 16, 0)
        if host_ptr is None:
            a = np.ascontiguousarray(host_trace, dtype=np.uint32)
            log_n, width = a.shape[0].bit_length() - 1, a.shape[1]
            host_ptr = a.ctypes.data
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        size = self.lib.zkhip_proof_size(log_n, width, C.byref(params), pv.size)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_shard_host(self.handle, C.c_void_p(host_ptr), log_n, width, pv.ctypes.data_as(u32p), pv.size,
                                              C.byref(params), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def prove_segment(self, cols, log_n, width, public_values=(), params=None):
        """cols: device buffer, column-major [width][2^log_n] (RISC Zero's Hal layout)"""
        params = params or _lib.segment_params()
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        size = self.lib.zkhip_proof_size(log_n, width, C.byref(params), pv.size)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_segment(self.handle, C.c_void_p(cols.ptr), log_n, width,
                                           pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                           buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def prove_chips(self, chips, public_values=(), params=None):
        """chips: [(device buffer, log_n, width[, logup_pairs[, partner]]), ...] tallest first -- one shard of several AIR
        tables (SP1's shard shape); partner = index of the chip this one exchanges lookups with, -1 for none"""
        params = params or Params(1, 100, 16, 0)
        chips = [tuple(c) + ((0,) if len(c) < 4 else ()) for c in chips]
        chips = [tuple(c) + ((-1,) if len(c) < 5 else ()) for c in chips]
        n = len(chips)
        arr = (_lib.Chip * n)(*[_lib.Chip(b.ptr, w, ln, w, pr, pa) for b, ln, w, pr, pa in chips])
        log_ns = (C.c_int32 * n)(*[c[1] for c in chips])
        widths = (C.c_uint32 * n)(*[c[2] for c in chips])
        pairs = (C.c_int32 * n)(*[c[3] for c in chips])
        partners = (C.c_int32 * n)(*[c[4] for c in chips])
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        size = self.lib.zkhip_chips_proof_size(log_ns, widths, pairs, partners, n, C.byref(params), pv.size)
        if size == 0:
            check(-1)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_chips(self.handle, arr, n, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                         buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def prove_chips_air(self, chips, programs, public_values=(), params=None):
        """chips: [(device buffer, log_n, width), ...] tallest first; programs[c]: a constraint program (numpy u32 words; degree 4 / 5 needs log_blowup >= 2)
        or None for the built-in synthetic AIR -- several different AIR tables in one proof (version 9)"""
        params = params or Params(1, 100, 16, 0)
        n = len(chips)
        arr = (_lib.Chip * n)(*[_lib.Chip(b.ptr, w, ln, w, 0, -1) for b, ln, w in chips])
        log_ns = (C.c_int32 * n)(*[c[1] for c in chips])
        widths = (C.c_uint32 * n)(*[c[2] for c in chips])
        keep, pp, pw = _program_table(programs)
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        size = self.lib.zkhip_chips_proof_size_air(log_ns, widths, pp, pw, n, C.byref(params), pv.size)
        if size == 0:
            check(-1)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_chips_air(self.handle, arr, pp, pw, n, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                             buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def range_table(self, trace, ld, rows, columns, log_table, width=4, value_col=0, mult_col=1):
        """a 2^log_table x width range table on the device: value column = row index, multiplicity column = how often the value
        appears in `columns` of `trace` (the other columns zero)"""
        out = self.from_raw(np.zeros(width << log_table, dtype=np.uint32))
        cols = (C.c_uint32 * len(columns))(*[int(c) for c in columns])
        check(self.lib.zkhip_range_table(self.handle, C.c_void_p(trace.ptr), ld, rows, cols, len(columns), log_table, C.c_void_p(out.ptr), width, value_col, mult_col))
        return out

    def prove_machine(self, chips, programs, tables, public_values=(), params=None):
        """chips: [(device buffer, log_n, width), ...] tallest first; programs[c] / tables[c]: the chip's constraint program and its
        interaction table (numpy u32 words) or None -- a machine whose tables look each other up (lookups as data, version 10)"""
        params = params or Params(1, 100, 16, 0)
        n = len(chips)
        arr = (_lib.Chip * n)(*[_lib.Chip(b.ptr, w, ln, w, 0, -1) for b, ln, w in chips])
        log_ns = (C.c_int32 * n)(*[c[1] for c in chips])
        widths = (C.c_uint32 * n)(*[c[2] for c in chips])
        kp, pp, pw = _program_table(programs)
        kt, tp, tw = _program_table(tables)
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        size = self.lib.zkhip_machine_proof_size(log_ns, widths, pp, pw, tp, tw, n, C.byref(params), pv.size)
        if size == 0:
            check(-1)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_machine(self.handle, arr, pp, pw, tp, tw, n, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                           buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def machine_setup(self, pre_chips, params=None):
        """zkhip_machine_setup: pre_chips = [(device buffer or None, log_n, preprocessed width), ...] tallest first -> MachineKey
        (.root: the 8 canonical words a verifier needs; .pre_widths)"""
        params = params or Params(1, 100, 16, 0)
        n = len(pre_chips)
        arr = (_lib.Chip * n)(*[_lib.Chip(c[0].ptr if c[0] is not None else None, c[3] if len(c) > 3 else c[2], c[1], c[2], 0, -1) for c in pre_chips])      # (buffer, log_n, width[, row pitch])
        handle = C.c_void_p()
        root = np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_machine_setup(self.handle, arr, n, C.byref(params), C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, [int(c[2]) for c in pre_chips])

    # ---- the FRI-fold chip (a first recursion step): trace, key, proof
    def fri_indices_key(self, view, inner_pow_bits, params=None):
        """zkhip_fri_indices_key: (query number, reduced opening), the layer roots, the SAMPLES chip's fixed columns -- no index"""
        params = params or Params(1, 100, 16)
        R, Q, betas, idx, vals, sibs, roots, paths = _fri_layers_arrays(view)
        handle, root = C.c_void_p(), np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_fri_indices_key(self.handle, R, Q, inner_pow_bits, vals.ctypes.data_as(u32p), roots.ctypes.data_as(u32p),
                                             C.byref(params), C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, [0, 0, 8, 12, 20])

    def prove_fri_indices(self, key, view, capacity, witness, inner_pow_bits, params=None):
        """zkhip_prove_fri_indices: the transcript machine with the query phase (proof of work, query indices) in-circuit"""
        params = params or Params(1, 100, 16)
        R, Q, betas, idx, vals, sibs, roots, paths = _fri_layers_arrays(view)
        cap8 = np.ascontiguousarray(np.array(capacity, dtype=np.uint32))
        size = self.lib.zkhip_fri_indices_proof_size(R, Q, inner_pow_bits, C.byref(params))
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_fri_indices(self.handle, key.handle, R, Q, inner_pow_bits, betas.ctypes.data_as(u32p), idx.ctypes.data_as(u32p),
                                               vals.ctypes.data_as(u32p), sibs.ctypes.data_as(u32p), roots.ctypes.data_as(u32p), paths.ctypes.data_as(u32p),
                                               cap8.ctypes.data_as(u32p), int(witness), C.byref(params), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    # ---- the fold-by-16 machines: the key and the proof of every kind (_FRI16_KINDS below)
    def _fri16_key(self, kind, view, params):
        params = params or Params(1, 100, 16)
        infix, _, fields, _ = _FRI16_KINDS[kind]
        shape, hw, more, args = _fri16_gather(view, kind, fields)
        handle, root = C.c_void_p(), np.zeros(8, dtype=np.uint32)
        check(getattr(self.lib, "zkhip_fri16%s_key" % infix)(self.handle, *shape, *hw, *more, *args, C.byref(params), C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, None)

    def _prove_fri16(self, kind, key, view, params):
        params = params or Params(1, 100, 16)
        infix, _, _, n = _FRI16_KINDS[kind]
        shape, hw, more, args = _fri16_gather(view, kind, _FRI16_VIEW[:n])
        size = getattr(self.lib, "zkhip_fri16%s_proof_size" % infix)(*shape, *more, C.byref(params))
        buf = np.empty(max(size, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        check(getattr(self.lib, "zkhip_prove_fri16%s" % infix)(self.handle, key.handle, *shape, *hw, *more, *args, C.byref(params), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    # ---- the fold-by-16 FRI machine (FOLD16 + FINAL): key, traces, proof
    def fri16_key(self, view, params=None):
        """zkhip_fri16_key: the LAYERS / QUERIES / COEFFS tables and FINAL's schedule of a fold-16 view, committed on the device -> MachineKey"""
        return self._fri16_key("layers", view, params)

    def fri16_gen_traces(self, view, out=None):
        """zkhip_fri16_gen_traces: the two main traces of a fold-16 view -> (FOLD16 buffer, its log rows, its width, FINAL buffer, its log rows);
        out = (FOLD16 buffer, FINAL buffer) of an earlier call: filled again instead of new ones"""
        shape, arrs = _fri16_arrays(view)
        dims = {}
        for which in range(5):
            _, ln, mw, _, table = fri16_describe(*shape, which, 0)
            dims[table] = (ln, mw)
        (lf, wf), (ln, wn) = dims[0], dims[1]
        fold, final = out if out is not None else (self.alloc(wf << lf), self.alloc(wn << ln))
        check(self.lib.zkhip_fri16_gen_traces(self.handle, *shape, *[a.ctypes.data_as(u32p) for a in arrs], C.c_void_p(fold.ptr), wf, C.c_void_p(final.ptr), wn))
        return fold, lf, wf, final, ln

    def prove_fri16(self, key, view, params=None):
        """zkhip_prove_fri16: "every listed query folds by 16 through the listed rows to the listed final polynomial at its last point"; a view whose
        chains do not end there is refused before anything is proven"""
        return self._prove_fri16("layers", key, view, params)

    # ---- the fold-by-16 PATHS machine (the layer rows' Merkle paths in-circuit: P24L + ROOTS where LAYERS stood)
    def fri16_paths_key(self, view, params=None):
        """zkhip_fri16_paths_key: QUERIES, COEFFS, ROOTS and FINAL's schedule of a fold-16 view, committed on the device -- from the final coefficients,
        the indices, the reduced openings and the layer roots alone -> MachineKey"""
        return self._fri16_key("paths", view, params)

    def fri16_paths_gen_trace(self, view, out=None):
        """zkhip_fri16_paths_gen_trace: the P24L table of a fold-16 view -> (buffer, its log rows, path ends [n][8]); out: a buffer of an earlier call"""
        shape, hw, arrs, _, paths = _fri16_paths_arrays(view)
        ln = [d[1] for d in (fri16_paths_describe(*shape, which, 0) for which in range(6)) if d[4] == 2][0]
        buf = out if out is not None else self.alloc(552 << ln)
        cap = shape[0] * shape[3]
        ends, n = np.zeros(8 * cap, dtype=np.uint32), C.c_size_t(0)
        check(self.lib.zkhip_fri16_paths_gen_trace(self.handle, *shape, hw, *[a.ctypes.data_as(u32p) for a in arrs], paths.ctypes.data_as(u32p), C.c_void_p(buf.ptr), 552,
                                                   ends.ctypes.data_as(u32p), cap, C.byref(n)))
        return buf, ln, ends[:8 * n.value].reshape(-1, 8)

    def prove_fri16_paths(self, key, view, params=None):
        """zkhip_prove_fri16_paths: "every listed query opens the listed layer commitments row by row and folds by 16 through these rows to the listed final
        polynomial at its last point"; refused before anything is proven: a path that does not end in its layer's root, queries that disagree about a
        shared row or its path, a chain that does not end in the final polynomial"""
        return self._prove_fri16("paths", key, view, params)

    def fri16_indices_key(self, view, params=None):
        """zkhip_fri16_indices_key: the key of the fold-16 indices machine, committed on the device -- from the shape, the inner proof's grinding bits, the
        final coefficients, the reduced openings by query number and the layer roots: no index, no challenge -> MachineKey"""
        return self._fri16_key("indices", view, params)

    def fri16_indices_gen_traces(self, R, F, log_blowup, n_queries, pow_bits, capacity, roots, final_poly, witness):
        """zkhip_fri16_indices_gen_traces: the P2T and SAMPLES main traces from the capacity, the layer roots, the final coefficients and the witness alone
        -> (P2T [2^lr][352], SAMPLES [2^lr][288] (canonical words, downloaded), betas [R][4], the Q drawn indices)"""
        u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
        lns = {d[4]: d[1] for d in (fri16_indices_describe(R, F, log_blowup, n_queries, pow_bits, which, 0) for which in range(8))}
        p2t, smp = self.alloc(352 << lns[6]), self.alloc(288 << lns[7])
        cp, rt, fp = u(capacity), u(roots), u(final_poly)
        assert cp.size == 8 and rt.size == 8 * R and fp.size == 4 << F
        betas, idx = np.zeros(4 * R, dtype=np.uint32), np.zeros(n_queries, dtype=np.uint32)
        check(self.lib.zkhip_fri16_indices_gen_traces(self.handle, R, F, log_blowup, n_queries, pow_bits, cp.ctypes.data_as(u32p), rt.ctypes.data_as(u32p), fp.ctypes.data_as(u32p),
                                                      int(witness), C.c_void_p(p2t.ptr), C.c_void_p(smp.ptr), betas.ctypes.data_as(u32p), idx.ctypes.data_as(u32p)))
        return p2t.download().reshape(-1, 352), smp.download().reshape(-1, 288), betas.reshape(R, 4), idx

    def fri16_samples_gen_trace(self, index_bits, n_queries, words):
        """zkhip_fri16_samples_gen_trace: the SAMPLES main trace from given canonical words [ceil((1 + Q) / 8)][8] -> [2^lr][288] (canonical words, downloaded)"""
        w = np.ascontiguousarray(np.array(words, dtype=np.uint32).reshape(-1))
        rows = (1 + n_queries + 7) // 8
        assert w.size == 8 * rows
        lr = 5
        while (1 << lr) < rows:
            lr += 1
        buf = self.alloc(288 << lr)
        check(self.lib.zkhip_fri16_samples_gen_trace(self.handle, index_bits, n_queries, w.ctypes.data_as(u32p), C.c_void_p(buf.ptr)))
        return buf.download().reshape(-1, 288)

    def prove_fri16_indices(self, key, view, params=None):
        """zkhip_prove_fri16_indices: "a sponge chain from this capacity over the listed roots, final coefficients and a witness draws the challenges, a
        proof-of-work word with its low bits zero and the query indices; every query, at the index drawn for it, opens the listed layer commitments and
        folds under the drawn challenges to the listed final polynomial".  view: a paths view with "capacity" [8], "witness" and "pow_bits".  Refused before
        anything is proven: challenges or indices the chain does not draw, a witness that fails the proof of work, and all prove_fri16_paths refuses"""
        return self._prove_fri16("indices", key, view, params)

    # ---- the fold-by-16 OPENINGS machine (the reduced openings in-circuit: ROWSUM16 and QUERY16)
    def fri16_openings_key(self, view, params=None):
        """zkhip_fri16_openings_key: the key of the fold-16 openings machine, committed on the device -- from the shape, the inner proof's grinding bits and trace
        width, the final coefficients, the opened trace and quotient rows by query number and the layer roots: no reduced opening, no index, no challenge -> MachineKey"""
        return self._fri16_key("openings", view, params)

    def fri16_openings_gen_traces(self, R, F, log_blowup, n_queries, pow_bits, W, trows, qrows, consts, indices):
        """zkhip_fri16_openings_gen_traces: the ROWSUM16 and QUERY16 main traces from raw rows [Q][W] and [Q][8], the constants [8][4] and the indices alone
        -> (ROWSUM16 [2^lr][48], QUERY16 [2^lr][72] (canonical words, downloaded), the reduced openings [Q][4])"""
        u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
        lns = {d[4]: d[1] for d in (fri16_openings_describe(R, F, log_blowup, n_queries, pow_bits, W, which, 0) for which in range(10))}
        rs, qm = self.alloc(48 << lns[8]), self.alloc(72 << lns[3])
        tr, qr, cs, ix = u(trows), u(qrows), u(consts), u(indices)
        assert tr.size == n_queries * W and qr.size == 8 * n_queries and cs.size == 32 and ix.size == n_queries
        ros = np.zeros(4 * n_queries, dtype=np.uint32)
        check(self.lib.zkhip_fri16_openings_gen_traces(self.handle, R, F, log_blowup, n_queries, pow_bits, W, tr.ctypes.data_as(u32p), qr.ctypes.data_as(u32p),
                                                       cs.ctypes.data_as(u32p), ix.ctypes.data_as(u32p), C.c_void_p(rs.ptr), C.c_void_p(qm.ptr), ros.ctypes.data_as(u32p)))
        return rs.download().reshape(-1, 48), qm.download().reshape(-1, 72), ros.reshape(-1, 4)

    def prove_fri16_openings(self, key, view, params=None):
        """zkhip_prove_fri16_openings: everything prove_fri16_indices states, and "the value at which query q enters layer 0 is the reduced opening of the trace
        row and the quotient row listed for q, under the public constants, at the index drawn for q".  view: an indices view with "W", "trows" [Q][W], "qrows"
        [Q][8] and "consts" {FA, ZETA, ZNX, YL, YN, YQ, OFFN, OFFQ: [4]}.  Refused before anything is proven, each naming the query: all prove_fri16_indices
        refuses, a reduced opening the rows do not give, a point equal to zeta or zeta g, constants that do not match each other"""
        return self._prove_fri16("openings", key, view, params)

    # ---- the fold-by-16 ROW-PATHS machine (the opened rows' Merkle paths in-circuit: P24R where ROWS stood)
    def fri16_rowpaths_key(self, view, params=None):
        """zkhip_fri16_rowpaths_key: the key of the fold-16 row-paths machine, committed on the device -- from the shape, the inner proof's grinding bits and trace
        width, the final coefficients, the layer roots, the trace root and the quotient root: no row, no index, no value -> MachineKey"""
        return self._fri16_key("rowpaths", view, params)

    def fri16_rowpaths_gen_trace(self, R, F, log_blowup, n_queries, pow_bits, W, trows, qrows, indices, tpaths, qpaths):
        """zkhip_fri16_rowpaths_gen_trace: P24R's main trace from raw rows [Q][W] and [Q][8], the indices and the siblings [Q][H][8] of either tree alone, one launch
        -> (P24R [2^lr][552] (canonical words, downloaded), the path ends [2 Q][8] in tag order: query q's trace path, then its quotient path)"""
        u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
        lns = {d[4]: d[1] for d in (fri16_rowpaths_describe(R, F, log_blowup, n_queries, pow_bits, W, which, 0) for which in range(10))}
        H = 4 * R + F + log_blowup
        tr, qr, ix, tp, qp = u(trows), u(qrows), u(indices), u(tpaths), u(qpaths)
        assert tr.size == n_queries * W and qr.size == 8 * n_queries and ix.size == n_queries and tp.size == qp.size == 8 * H * n_queries
        trace = self.alloc(552 << lns[9])
        ends = np.zeros(16 * n_queries, dtype=np.uint32)
        check(self.lib.zkhip_fri16_rowpaths_gen_trace(self.handle, R, F, log_blowup, n_queries, pow_bits, W, *[a.ctypes.data_as(u32p) for a in (tr, qr, ix, tp, qp)],
                                                      C.c_void_p(trace.ptr), ends.ctypes.data_as(u32p)))
        return trace.download().reshape(-1, 552), ends.reshape(-1, 8)

    def prove_fri16_rowpaths(self, key, view, params=None):
        """zkhip_prove_fri16_rowpaths: everything prove_fri16_openings states, and "the rows from which AT_q and AQ_q are summed are the leaves at the index drawn for
        q of the trees whose roots the key lists as the trace root and the quotient root".  view: an openings view with "tpaths" / "qpaths" [Q][H][8] and "troot" /
        "qroot" [8].  Refused before anything is proven, each naming query and tree: all prove_fri16_openings refuses, a path that does not end in its root,
        path words that are not canonical"""
        return self._prove_fri16("rowpaths", key, view, params)

    # ---- the fold-by-16 HEAD machine (the head of the transcript in-circuit: P2TH, OPENED16, the constants over buses)
    def fri16_head_key(self, view, params=None):
        """zkhip_fri16_head_key: the key of the fold-16 head machine, committed on the device -- from the shape, the inner proof's grinding bits, trace width and
        number of public values, the final coefficients, the layer roots, the trace root and the quotient root: no opened word, no constant, no challenge -> MachineKey"""
        return self._fri16_key("head", view, params)

    def fri16_head_gen_traces(self, R, F, log_blowup, n_queries, pow_bits, W, pubs, troot, qroot, opened, roots, final_poly, witness):
        """zkhip_fri16_head_gen_traces: the P2TH, SAMPLES and OPENED16 main traces from the inner public values, the two roots, the opened values [2 W + 8][4], the layer
        roots, the final coefficients and the witness alone -> (P2TH [2^lr][352], SAMPLES [2^lr][288], OPENED16 [2^lr][36] (canonical words, downloaded), the eight
        derived constants [8][4], the capacity the commit phase finds [8])"""
        u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
        NP = len(pubs)
        lns = {d[4]: d[1] for d in (fri16_head_describe(R, F, log_blowup, n_queries, pow_bits, W, NP, which, 0) for which in range(11))}
        pv, tr, qr, op, rt, fp = u(pubs), u(troot), u(qroot), u(opened), u(roots), u(final_poly)
        assert tr.size == qr.size == 8 and op.size == 8 * (W + 4) and rt.size == 8 * R and fp.size == 4 << F
        p2th, smp, opn = self.alloc(352 << lns[6]), self.alloc(288 << lns[7]), self.alloc(36 << lns[10])
        consts, cap = np.zeros(32, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_fri16_head_gen_traces(self.handle, R, F, log_blowup, n_queries, pow_bits, W, NP, *[a.ctypes.data_as(u32p) for a in (pv, tr, qr, op, rt, fp)],
                                                   int(witness), C.c_void_p(p2th.ptr), C.c_void_p(smp.ptr), C.c_void_p(opn.ptr), consts.ctypes.data_as(u32p),
                                                   cap.ctypes.data_as(u32p)))
        return p2th.download().reshape(-1, 352), smp.download().reshape(-1, 288), opn.download().reshape(-1, 36), consts.reshape(8, 4), cap

    def prove_fri16_head(self, key, view, params=None):
        """zkhip_prove_fri16_head: everything prove_fri16_rowpaths states, and "the transcript starts from the all-zero state, absorbs the header, the trace root, THESE
        public values, the quotient root and the opened values, and the eight constants and the commit phase's capacity are what it gives".  view: a row-paths view with
        "pubs" (the inner proof's public values) and "opened" [2 W + 8][4].  The proof's public values are view["pubs"].  Refused before anything is proven: all
        prove_fri16_rowpaths refuses, a derived constant or capacity that is not the view's, values that are not canonical, more than 30 public values or none"""
        return self._prove_fri16("head", key, view, params)

    # ---- the fold-by-16 IDENTITY machine (the AIR identity at zeta in-circuit: AIR16, SCALARS16)
    def fri16_identity_key(self, view, params=None):
        """zkhip_fri16_identity_key: the key of the fold-16 identity machine, committed on the device -- fri16_head_key's arguments -> MachineKey"""
        return self._fri16_key("identity", view, params)

    def fri16_identity_gen_traces(self, R, F, log_blowup, n_queries, pow_bits, W, NP, alpha, zeta, opened):
        """zkhip_fri16_identity_gen_traces: the AIR16 and SCALARS16 main traces from the shape, alpha, zeta and the opened values [2 W + 8][4] alone -> (AIR16 [2^lr][56],
        SCALARS16 [2^7][4 (17 + log_n)] (canonical words, downloaded), the two accumulators [2][4] (canonical): ACCO of the last group, QUO (zeta^N - 1))"""
        u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
        dims = {d[4]: (d[1], d[2]) for d in (fri16_identity_describe(R, F, log_blowup, n_queries, pow_bits, W, NP, which, 0) for which in range(13))}
        al, ze, op = u(alpha), u(zeta), u(opened)
        assert al.size == ze.size == 4 and op.size == 8 * (W + 4)
        air, sc = self.alloc(dims[11][1] << dims[11][0]), self.alloc(dims[12][1] << dims[12][0])
        accs = np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_fri16_identity_gen_traces(self.handle, R, F, log_blowup, n_queries, pow_bits, W, NP, *[a.ctypes.data_as(u32p) for a in (al, ze, op)],
                                                       C.c_void_p(air.ptr), C.c_void_p(sc.ptr), accs.ctypes.data_as(u32p)))
        return air.download().reshape(-1, dims[11][1]), sc.download().reshape(-1, dims[12][1]), accs.reshape(2, 4)

    def prove_fri16_identity(self, key, view, params=None):
        """zkhip_prove_fri16_identity: everything prove_fri16_head states, and "the synthetic AIR's constraints at zeta, folded with the alpha the transcript draws, equal
        the quotient the opened quotient values give times zeta^N - 1".  view: a head view.  Refused before anything is proven: all prove_fri16_head refuses, zeta = 1, an
        inner proof whose AIR identity at zeta does not hold"""
        return self._prove_fri16("identity", key, view, params)

    # ---- the fold-by-16 LIFT machine (the identity machine with roots and final coefficients out of the key: one key per shape)
    def fri16_lift_key(self, R, F, log_blowup, n_queries, pow_bits, W, NP, params=None, hash_width=24):
        """zkhip_fri16_lift_key: the key of the fold-16 lift machine, committed on the device -- from the SHAPE alone (layers, log_final, log_blowup, queries, the inner
        proof's grinding bits, trace width and number of public values): no root, no coefficient, no proof -> MachineKey"""
        params = params or Params(1, 100, 16)
        handle, root = C.c_void_p(), np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_fri16_lift_key(self.handle, R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(params), C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, None)

    def fri16_lift_gen_tables(self, R, F, log_blowup, n_queries, roots, troot, qroot, final_poly, buffers=False):
        """zkhip_fri16_lift_gen_tables: the main columns of ROOTS and COEFFS of the lift machine from the canonical layer roots [R][8], the trace root, the quotient root
        and the final coefficients [2^F][4] -> (ROOTS [2^5][16] (its first eight columns zero: the transcript launch makes those), COEFFS [max(2^5, 2^F)][8]), canonical
        words, downloaded"""
        u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
        rt, tr, qr, fp = u(roots), u(troot), u(qroot), u(final_poly)
        assert rt.size == 8 * R and tr.size == qr.size == 8 and fp.size == 4 << F
        rm, cm = self.alloc(16 << 5), self.alloc(8 << max(5, F))
        check(self.lib.zkhip_fri16_lift_gen_tables(self.handle, R, F, log_blowup, n_queries, *[a.ctypes.data_as(u32p) for a in (rt, tr, qr, fp)], C.c_void_p(rm.ptr),
                                                   C.c_void_p(cm.ptr)))
        if buffers:                                          # (the device buffers themselves: their raw Montgomery words can be read)
            return rm, cm
        return rm.download().reshape(-1, 16), cm.download().reshape(-1, 8)

    def prove_fri16_lift(self, key, view, params=None):
        """zkhip_prove_fri16_lift: "some valid segment proof of this shape with THESE public values exists" -- everything prove_fri16_identity states, under a key that
        holds no root and no coefficient.  view: a head view.  Refused before anything is proven: all prove_fri16_identity refuses"""
        return self._prove_fri16("lift", key, view, params)

    def prove_fri16_lift_segment(self, key, proof, log_n, width, public_values, inner_params, params=None):
        """zkhip_prove_fri16_lift_segment: segment proof in, lift proof out -- the host verifier once over `proof` with every fold-16 view attached, then prove_fri16_lift.
        Raises with the host verifier's code and message when the inner proof does not verify or is of a form the views do not take"""
        params = params or Params(1, 100, 16)
        pr = np.ascontiguousarray(proof, dtype=np.uint8)
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        sh = _fri16_segment_shape(log_n, inner_params)
        size = self.lib.zkhip_fri16_lift_proof_size(*sh, int(inner_params.pow_bits), width, pv.size, C.byref(params)) if sh else 0
        buf = np.empty(max(size, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        check(self.lib.zkhip_prove_fri16_lift_segment(self.handle, key.handle, pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size,
                                                      C.byref(inner_params), C.byref(params), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    # ---- the JOIN of fold-16 lift proofs (machine mode over the lift machine of a shape): N lift proofs -> one proof
    def fri16_join_setup(self, R, F, log_blowup, n_queries, pow_bits, W, NP, n_proofs, lift_params=None, params=None, hash_width=24):
        """zkhip_fri16_join_setup: the key of the machine that verifies n_proofs lift proofs of this shape (made under lift_params) in-circuit -> MachineKey"""
        lift_params, params = lift_params or Params(1, 100, 16), params or Params(1, 100, 16)
        handle, root = C.c_void_p(), np.zeros(8, dtype=np.uint32)
        check(self.lib.zkhip_fri16_join_setup(self.handle, R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), n_proofs, C.byref(params),
                                              C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, None)

    def prove_fri16_join(self, key, R, F, log_blowup, n_queries, pow_bits, W, NP, lift_proofs, public_values, lift_params=None, params=None, hash_width=24):
        """zkhip_prove_fri16_join: lift_proofs = a list of lift proofs of ONE shape, public_values one list of NP words per proof -> ONE proof, the bytes
        prove_machine_verifier makes from the lift machine's description.  Refused by message: no proof or more than fri16_join_max_proofs, inner hash width 16,
        another number of public values than len(lift_proofs) x NP"""
        lift_params, params = lift_params or Params(1, 100, 16), params or Params(1, 100, 16)
        sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in lift_proofs]
        n = len(sps)
        pv = np.ascontiguousarray(np.array([int(x) for v in public_values for x in v] or [0], dtype=np.uint32))
        n_pub = sum(len(v) for v in public_values)
        shape = (R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params))
        size = self.lib.zkhip_fri16_join_proof_size(*shape, n, C.byref(params))
        buf = np.empty(max(size, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        ptrs = (u8p * max(n, 1))(*[sp.ctypes.data_as(u8p) for sp in sps])
        lens = (C.c_size_t * max(n, 1))(*[sp.size for sp in sps])
        check(self.lib.zkhip_prove_fri16_join(self.handle, key.handle if key is not None else None, *shape, ptrs, lens, n, pv.ctypes.data_as(u32p), n_pub, C.byref(params),
                                              buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def prove_fri16_join_segments(self, lift_key, join_key, segment_proofs, log_n, width, public_values, inner_params, lift_params=None, params=None):
        """zkhip_prove_fri16_join_segments: segment proofs in, ONE proof out -- each segment lifted on this context (prove_fri16_lift_segment under lift_key), then
        prove_fri16_join under join_key.  A segment that does not verify raises with the host verifier's code and a message that names the segment"""
        lift_params, params = lift_params or Params(1, 100, 16), params or Params(1, 100, 16)
        sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in segment_proofs]
        n = len(sps)
        pv = np.ascontiguousarray(np.array([int(x) for v in public_values for x in v] or [0], dtype=np.uint32))
        n_pub = sum(len(v) for v in public_values)
        sh = _fri16_segment_shape(log_n, inner_params)
        size = self.lib.zkhip_fri16_join_proof_size(sh[0], sh[1], sh[2], sh[3], int(inner_params.hash_width), int(inner_params.pow_bits), width, n_pub // max(n, 1),
                                                    C.byref(lift_params), n, C.byref(params)) if sh else 0
        buf = np.empty(max(size, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        ptrs = (u8p * max(n, 1))(*[sp.ctypes.data_as(u8p) for sp in sps])
        lens = (C.c_size_t * max(n, 1))(*[sp.size for sp in sps])
        check(self.lib.zkhip_prove_fri16_join_segments(self.handle, lift_key.handle, join_key.handle, ptrs, lens, n, log_n, width, pv.ctypes.data_as(u32p), n_pub,
                                                       C.byref(inner_params), C.byref(lift_params), C.byref(params), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    # ---- the TREE above the join: more lift proofs than one join takes -> joins -> one proof
    def fri16_tree_setup(self, R, F, log_blowup, n_queries, pow_bits, W, NP, proofs_per_join, join_vk, n_joins, lift_params=None, join_params=None, params=None, hash_width=24):
        """zkhip_fri16_tree_setup: the key of the top that verifies n_joins joins of proofs_per_join lift proofs each; join_vk: fri16_join_key_host's (or
        fri16_join_setup's root) for that join size -> MachineKey"""
        lift_params, join_params, params = lift_params or Params(1, 100, 16), join_params or Params(1, 100, 16), params or Params(1, 100, 16)
        handle, root = C.c_void_p(), np.zeros(8, dtype=np.uint32)
        jvk = np.ascontiguousarray(np.array(join_vk, dtype=np.uint32))
        check(self.lib.zkhip_fri16_tree_setup(self.handle, R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), proofs_per_join, C.byref(join_params),
                                              jvk.ctypes.data_as(u32p), n_joins, C.byref(params), C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, None)

    def prove_fri16_tree(self, top_key, R, F, log_blowup, n_queries, pow_bits, W, NP, lift_proofs, proofs_per_join, public_values, join_vk, lift_params=None, join_params=None,
                         params=None, devices=None, in_flight=4, hash_width=24):
        """zkhip_prove_fri16_tree: lift proofs of ONE shape -> joins of proofs_per_join (in flight, dealt over `devices`) -> ONE proof over the joins on this context
        -> (top proof bytes, [join proof bytes, ...]); public_values: one list of NP words per lift proof.  len(lift_proofs) must be a positive multiple of
        proofs_per_join (the caller pads by repeating the last)"""
        lift_params, join_params, params = lift_params or Params(1, 100, 16), join_params or Params(1, 100, 16), params or Params(1, 100, 16)
        sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in lift_proofs]
        n = len(sps)
        pv = np.ascontiguousarray(np.array([int(x) for v in public_values for x in v] or [0], dtype=np.uint32))
        n_pub = sum(len(v) for v in public_values)
        jvk = np.ascontiguousarray(np.array(join_vk, dtype=np.uint32))
        shape = (R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params))
        n_joins = n // proofs_per_join if proofs_per_join else 0
        jsize = self.lib.zkhip_fri16_join_proof_size(*shape, max(proofs_per_join, 1), C.byref(join_params))
        tsize = self.lib.zkhip_fri16_tree_proof_size(*shape, proofs_per_join, C.byref(join_params), jvk.ctypes.data_as(u32p), max(n_joins, 1), C.byref(params))
        jbuf = np.empty((max(n_joins, 1), max(jsize, 4)), dtype=np.uint8)
        jlens = (C.c_size_t * max(n_joins, 1))()
        ptrs = (u8p * max(n, 1))(*[sp.ctypes.data_as(u8p) for sp in sps])
        lens = (C.c_size_t * max(n, 1))(*[sp.size for sp in sps])
        top = np.empty(max(tsize, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        devs = (C.c_int * len(devices))(*devices) if devices else None
        check(self.lib.zkhip_prove_fri16_tree(self.handle, top_key.handle if top_key is not None else None, *shape, devs, len(devices) if devices else 0, ptrs, lens, n,
                                              proofs_per_join, pv.ctypes.data_as(u32p), n_pub, C.byref(join_params), jvk.ctypes.data_as(u32p), C.byref(params), in_flight,
                                              jbuf.ctypes.data_as(u8p), jbuf.shape[1], jlens, top.ctypes.data_as(u8p), tsize, C.byref(got)))
        return top[: got.value], [jbuf[j, : jlens[j]] for j in range(n_joins)]

    def machine_verifier_gen_eval_rows(self, chips, coeffs, keys, firsts, n_chips, values, alphas, n_stream):
        """zkhip_machine_verifier_gen_eval_rows: machine mode's EVAL row kernel alone, one launch.  chips / coeffs / firsts [n_terms], keys [n_terms][3], values
        [n_proofs][kspan][4] and alphas [n_proofs][4] canonical; keys 1 .. n_stream are read as a proof's opened-value stream, the rest as the call's small block
        -> (rows [n_proofs n_terms][32], accs [n_proofs n_chips][4]), canonical words"""
        u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
        ch, co, ke, fi, al = u(chips), u(coeffs), u(keys), u(firsts), u(alphas)
        vals = np.ascontiguousarray(np.array(values, dtype=np.uint32))
        n_terms, n_proofs, kspan = ch.size, vals.shape[0], vals.shape[1]
        assert co.size == fi.size == n_terms and ke.size == 3 * n_terms and vals.shape[2] == 4 and al.size == 4 * n_proofs
        rows, accs = np.zeros((n_proofs * n_terms, 32), dtype=np.uint32), np.zeros((n_proofs * n_chips, 4), dtype=np.uint32)
        check(self.lib.zkhip_machine_verifier_gen_eval_rows(self.handle, n_terms, *[a.ctypes.data_as(u32p) for a in (ch, co, ke, fi)], n_chips, n_proofs, kspan, n_stream,
                                                            vals.ctypes.data_as(u32p), al.ctypes.data_as(u32p), rows.ctypes.data_as(u32p), accs.ctypes.data_as(u32p)))
        return rows, accs

    def shard_verifier_setup(self, log_n, width, n_queries, inner_pow_bits, n_public, params=None, n_proofs=1, program=None):
        """zkhip_shard_verifier_setup: the key of the shard-verifier machine for n_proofs inner proofs of this SHAPE (no inner proof involved);
        program: the inner proofs are version-7 proofs of that constraint program (zkhip_shard_verifier_setup_air)"""
        params = params or Params(1, 100, 16)
        handle, root = C.c_void_p(), np.zeros(8, dtype=np.uint32)
        if program is None:
            check(self.lib.zkhip_shard_verifier_setup(self.handle, log_n, width, n_queries, inner_pow_bits, n_public, n_proofs, C.byref(params), C.byref(handle), root.ctypes.data_as(u32p)))
        else:
            pg = np.ascontiguousarray(program, dtype=np.uint32)
            check(self.lib.zkhip_shard_verifier_setup_air(self.handle, pg.ctypes.data_as(u32p), pg.size, log_n, width, n_queries, inner_pow_bits, n_public, n_proofs, C.byref(params),
                                                          C.byref(handle), root.ctypes.data_as(u32p)))
        return MachineKey(self, handle, root, None)

    def prove_shard_verifier(self, key, shard_proofs, log_n, width, public_values, inner=None, outer=None, program=None):
        """zkhip_prove_shard_verifier: the WHOLE verification of a shard proof (transcript, AIR identity, openings, FRI) proven in-circuit.
        shard_proofs: one proof (bytes / uint8 array) with its public values, or a LIST of proofs with a list of public-value lists (the join)"""
        inner, outer = inner or Params(1, 100, 16), outer or Params(1, 100, 16)
        if not isinstance(shard_proofs, (list, tuple)):
            shard_proofs, public_values = [shard_proofs], [public_values]
        sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in shard_proofs]
        n = len(sps)
        pv = np.ascontiguousarray(np.array([list(v) for v in public_values], dtype=np.uint32).reshape(n, -1))
        n_public = pv.shape[1]
        pg = None if program is None else np.ascontiguousarray(program, dtype=np.uint32)
        if pg is None:
            size = self.lib.zkhip_shard_verifier_proof_size(log_n, width, inner.num_queries, inner.pow_bits, n_public, n, C.byref(outer))
        else:
            size = self.lib.zkhip_shard_verifier_proof_size_air(pg.ctypes.data_as(u32p), pg.size, log_n, width, inner.num_queries, inner.pow_bits, n_public, n, C.byref(outer))
        if size == 0:
            check(-1)
        buf = np.empty(size, dtype=np.uint8)
        got = C.c_size_t(0)
        ptrs = (u8p * n)(*[sp.ctypes.data_as(u8p) for sp in sps])
        lens = (C.c_size_t * n)(*[sp.size for sp in sps])
        if pg is None:
            check(self.lib.zkhip_prove_shard_verifier(self.handle, key.handle, ptrs, lens, n, log_n, width, pv.ctypes.data_as(u32p), n_public, C.byref(inner),
                                                      C.byref(outer), buf.ctypes.data_as(u8p), size, C.byref(got)))
        else:
            check(self.lib.zkhip_prove_shard_verifier_air(self.handle, key.handle, pg.ctypes.data_as(u32p), pg.size, ptrs, lens, n, log_n, width, pv.ctypes.data_as(u32p), n_public,
                                                          C.byref(inner), C.byref(outer), buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def prove_machine_keyed(self, key, chips, programs, tables, public_values=(), params=None, key_entries=None):
        """a machine with preprocessed columns (proof version 11): `key` from machine_setup; chips as in prove_machine (main columns);
        programs / tables address the combined row [preprocessed | main].  key_entries: per chip the key entry it uses (-1: none) when the
        key holds tables only (zkhip_prove_machine_keyed_at); its preprocessed widths then come from the entries"""
        params = params or Params(1, 100, 16, 0)
        n = len(chips)
        arr = (_lib.Chip * n)(*[_lib.Chip(c[0].ptr, c[3] if len(c) > 3 else c[2], c[1], c[2], 0, -1) for c in chips])      # (buffer, log_n, width[, row pitch])
        log_ns = (C.c_int32 * n)(*[c[1] for c in chips])
        widths = (C.c_uint32 * n)(*[c[2] for c in chips])
        if key_entries is not None:
            per_chip = [key.pre_widths[e] if 0 <= e < len(key.pre_widths) else 0 for e in key_entries]
        else:
            per_chip = (list(key.pre_widths) + [0] * n)[:n]                  # (a key of another shape is the library's to refuse)
        pws = (C.c_uint32 * n)(*per_chip)
        kp, pp, pw = _program_table(programs)
        kt, tp, tw = _program_table(tables)
        pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
        size = self.lib.zkhip_machine_proof_size_keyed(log_ns, widths, pws, pp, pw, tp, tw, n, C.byref(params), pv.size)
        buf = np.empty(max(size, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        if key_entries is not None:
            ke = (C.c_int32 * n)(*[int(e) for e in key_entries])
            check(self.lib.zkhip_prove_machine_keyed_at(self.handle, key.handle, ke, arr, pp, pw, tp, tw, n, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                                        buf.ctypes.data_as(u8p), size, C.byref(got)))
        else:
            check(self.lib.zkhip_prove_machine_keyed(self.handle, key.handle, arr, pp, pw, tp, tw, n, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                                     buf.ctypes.data_as(u8p), size, C.byref(got)))
        return buf[: got.value]

    def prove_debug(self):
        d = ProveDebug()
        check(self.lib.zkhip_last_prove_debug(self.handle, C.byref(d)))
        return {k: (np.array(getattr(d, k), dtype=np.uint32) if k != "pow_witness" else int(d.pow_witness))
                for k, _ in ProveDebug._fields_}


def prove_shards(traces, log_n, width, public_values_list, params=None, device=0, in_flight=4, host=False, lds=None):
    """zkhip_prove_shards: `traces` are DeviceBuffers or DeviceViews (Montgomery; dense, or with lds[i] the row pitch of job i in words)
    or, with host=True, numpy arrays of canonical words (dense).  Returns the list of proofs (numpy uint8 arrays)."""
    lib = _lib.load()
    params = params or Params(1, 100, 16, 0)
    n = len(traces)
    jobs = (_lib.ShardJob * n)()
    pvs, bufs, arrs = [], [], []
    for i, (t, pv) in enumerate(zip(traces, public_values_list)):
        pva = np.ascontiguousarray(np.array(pv, dtype=np.uint32))
        size = lib.zkhip_proof_size(log_n, width, C.byref(params), pva.size)
        buf = np.empty(max(size, 1), dtype=np.uint8)
        if host:
            arr = np.ascontiguousarray(t, dtype=np.uint32)
            arrs.append(arr)
            ptr = arr.ctypes.data
        else:
            ptr = t.ptr
        pvs.append(pva); bufs.append(buf)
        jobs[i].trace = ptr; jobs[i].ld = int(lds[i]) if lds is not None else width; jobs[i].log_n = log_n; jobs[i].width = width
        jobs[i].public_values = pva.ctypes.data_as(u32p); jobs[i].n_public = pva.size
        jobs[i].proof = buf.ctypes.data_as(u8p); jobs[i].proof_cap = size
    check(lib.zkhip_prove_shards(int(device), jobs, n, C.byref(params), int(in_flight), 1 if host else 0))
    return [bufs[i][: jobs[i].proof_len] for i in range(n)]


def prove_shards_multi(traces, log_n, width, public_values_list, params=None, devices=None, in_flight=4, host=False):
    """zkhip_prove_shards_multi: one call, one process, several GPUs; shard s runs on devices[s % len(devices)] (all visible
    devices when `devices` is None).  Device traces must live on that device (see shard_device)."""
    lib = _lib.load()
    params = params or Params(1, 100, 16, 0)
    n = len(traces)
    jobs = (_lib.ShardJob * n)()
    keep = []
    for i, (t, pv) in enumerate(zip(traces, public_values_list)):
        pva = np.ascontiguousarray(np.array(pv, dtype=np.uint32))
        size = lib.zkhip_proof_size(log_n, width, C.byref(params), pva.size)
        buf = np.empty(max(size, 1), dtype=np.uint8)
        arr = np.ascontiguousarray(t, dtype=np.uint32) if host else None
        keep.append((pva, buf, arr))
        jobs[i].trace = arr.ctypes.data if host else t.ptr
        jobs[i].ld = width; jobs[i].log_n = log_n; jobs[i].width = width
        jobs[i].public_values = pva.ctypes.data_as(u32p); jobs[i].n_public = pva.size
        jobs[i].proof = buf.ctypes.data_as(u8p); jobs[i].proof_cap = size
    if devices is None:
        dv, nd = None, 0
    else:
        dv, nd = (C.c_int * len(devices))(*[int(d) for d in devices]), len(devices)
    check(lib.zkhip_prove_shards_multi(dv, nd, jobs, n, C.byref(params), int(in_flight), 1 if host else 0))
    return [keep[i][1][: jobs[i].proof_len] for i in range(n)]


def prove_shards_air_multi(program, traces, log_n, width, public_values_list, params=None, devices=None, in_flight=4):
    """zkhip_prove_shards_air_multi: a batch of device traces of ONE constraint program, dealt over `devices` like prove_shards_multi"""
    lib = _lib.load()
    params = params or Params(1, 100, 16, 0)
    prog = np.ascontiguousarray(program, dtype=np.uint32)
    n = len(traces)
    jobs = (_lib.ShardJob * n)()
    keep = []
    for i, (t, pv) in enumerate(zip(traces, public_values_list)):
        pva = np.ascontiguousarray(np.array(pv, dtype=np.uint32))
        size = lib.zkhip_proof_size_air(prog.ctypes.data_as(u32p), prog.size, log_n, width, C.byref(params), pva.size)
        buf = np.empty(max(size, 1), dtype=np.uint8)
        keep.append((pva, buf))
        jobs[i].trace = t.ptr
        jobs[i].ld = width; jobs[i].log_n = log_n; jobs[i].width = width
        jobs[i].public_values = pva.ctypes.data_as(u32p); jobs[i].n_public = pva.size
        jobs[i].proof = buf.ctypes.data_as(u8p); jobs[i].proof_cap = size
    if devices is None:
        dv, nd = None, 0
    else:
        dv, nd = (C.c_int * len(devices))(*[int(d) for d in devices]), len(devices)
    check(lib.zkhip_prove_shards_air_multi(dv, nd, jobs, n, prog.ctypes.data_as(u32p), prog.size, C.byref(params), int(in_flight)))
    return [keep[i][1][: jobs[i].proof_len] for i in range(n)]


def shard_device(shard_index, devices=None, n_devices=None):
    """the device ordinal zkhip_prove_shards_multi proves shard `shard_index` on"""
    lib = _lib.load()
    if devices is None:
        return lib.zkhip_shard_device(int(shard_index), None, int(n_devices))
    dv = (C.c_int * len(devices))(*[int(d) for d in devices])
    return lib.zkhip_shard_device(int(shard_index), dv, len(devices))


def verify_shard(proof, log_n, width, public_values=(), params=None):
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    reason = C.c_int(0)
    rc = lib.zkhip_verify_shard(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size,
                                C.byref(params), C.byref(reason))
    return rc, reason.value


def verify_shard_air(program, proof, log_n, width, public_values=(), params=None):
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    prog = np.ascontiguousarray(program, dtype=np.uint32)
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    reason = C.c_int(0)
    rc = lib.zkhip_verify_shard_air(prog.ctypes.data_as(u32p), prog.size, pr.ctypes.data_as(u8p), pr.size, log_n, width,
                                    pv.ctypes.data_as(u32p), pv.size, C.byref(params), C.byref(reason))
    return rc, reason.value


def sha256_air_chained():
    """the chip with its initial chaining value public too (32 public values): the program of one shard of a longer message"""
    lib = _lib.load()
    n = lib.zkhip_sha256_air_chained(None, 0)
    out = np.empty(n, dtype=np.uint32)
    assert lib.zkhip_sha256_air_chained(out.ctypes.data_as(u32p), n) == n
    return out


class ShardedSha256:
    """the result of prove_sha256_sharded: digest, chaining values [n + 1][8], the shard proofs"""

    def __init__(self, digest, chain, proofs, stride, lens, log_blocks, message_len):
        self.digest, self.chain, self.buf, self.stride, self.lens, self.log_blocks, self.message_len = digest, chain, proofs, stride, lens, log_blocks, message_len

    @property
    def proofs(self):
        return [self.buf[i * self.stride:i * self.stride + int(n)] for i, n in enumerate(self.lens)]


def prove_sha256_sharded(message, log_blocks_per_shard, params=None, devices=None, in_flight=2):
    """zkhip_prove_sha256_sharded: SHA-256 of a message of any length as a chain of shard proofs dealt over `devices` (None: all visible)"""
    lib = _lib.load()
    params = params or Params(1, 100, 16)
    m = np.frombuffer(bytes(message), dtype=np.uint8) if len(message) else np.zeros(1, dtype=np.uint8)
    n = lib.zkhip_sha256_sharded_count(len(message), log_blocks_per_shard)
    stride = lib.zkhip_sha256_shard_proof_size(log_blocks_per_shard, C.byref(params))
    if n == 0 or stride == 0:
        raise _lib.ZkHipError(-1, "prove_sha256_sharded: bad shape")
    proofs = np.empty(n * stride, dtype=np.uint8)
    lens = (C.c_size_t * n)()
    chain = np.zeros((n + 1, 8), dtype=np.uint32)
    digest = np.zeros(32, dtype=np.uint8)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    check(lib.zkhip_prove_sha256_sharded(devs, len(devices) if devices else 0, m.ctypes.data_as(u8p), len(message), log_blocks_per_shard, C.byref(params), in_flight,
                                         digest.ctypes.data_as(u8p), chain.ctypes.data_as(u32p), proofs.ctypes.data_as(u8p), stride, lens))
    return ShardedSha256(digest.tobytes(), chain, proofs, stride, list(lens), log_blocks_per_shard, len(message))


def verify_sha256_sharded(result, digest=None, params=None, chain=None, proofs=None, message_len=None):
    """-> (rc, failing shard, reason); digest / chain / proofs / message length default to the result's own"""
    lib = _lib.load()
    params = params or Params(1, 100, 16)
    n = len(result.lens)
    lens = (C.c_size_t * n)(*result.lens)
    ch = np.ascontiguousarray(result.chain if chain is None else chain, dtype=np.uint32)
    buf = np.ascontiguousarray(result.buf if proofs is None else proofs, dtype=np.uint8)
    dg = np.frombuffer(bytes(result.digest if digest is None else digest), dtype=np.uint8)
    bad, reason = C.c_size_t(0), C.c_int(0)
    rc = lib.zkhip_verify_sha256_sharded(buf.ctypes.data_as(u8p), result.stride, lens, n, ch.ctypes.data_as(u32p), result.log_blocks, dg.ctypes.data_as(u8p),
                                         result.message_len if message_len is None else message_len, C.byref(params), C.byref(bad), C.byref(reason))
    return rc, bad.value, reason.value


class InnerMachine:
    """zkhip_machine_desc built from Python: chips = [{ln, W, Pw, prog, tab}] tallest first, the machine's key, how its proofs are made"""
    def __init__(self, chips, key_root, n_queries, pow_bits, n_public):
        n = len(chips)
        self.keep = [(np.ascontiguousarray(c["prog"], dtype=np.uint32), np.ascontiguousarray(c["tab"], dtype=np.uint32)) for c in chips]
        self.log_ns = (C.c_int32 * n)(*[int(c["ln"]) for c in chips])
        self.widths = (C.c_uint32 * n)(*[int(c["W"]) for c in chips])
        self.pre_widths = (C.c_uint32 * n)(*[int(c["Pw"]) for c in chips])
        self.progs = (C.POINTER(C.c_uint32) * n)(*[p.ctypes.data_as(u32p) for p, _ in self.keep])
        self.prog_words = (C.c_size_t * n)(*[p.size for p, _ in self.keep])
        self.tabs = (C.POINTER(C.c_uint32) * n)(*[t.ctypes.data_as(u32p) for _, t in self.keep])
        self.tab_words = (C.c_size_t * n)(*[t.size for _, t in self.keep])
        self.desc = _lib.MachineDesc(n, self.log_ns, self.widths, self.pre_widths, self.progs, self.prog_words, self.tabs, self.tab_words,
                                     (C.c_uint32 * 8)(*[int(v) for v in key_root]), int(n_queries), int(pow_bits), int(n_public))
        self.n_public = int(n_public)


def sha256_inner_machine(message_len, key_root, params=None):
    """the keyed SHA-256 machine of messages of this length (zkhip_prove_transcripts' proofs) as an InnerMachine for machine mode"""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    chips = []
    for which in range(2):
        ln, w, pw = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
        parts = []
        for kind in range(2):
            n = lib.zkhip_sha256_machine_describe(message_len, which, kind, None, 0, C.byref(ln), C.byref(w), C.byref(pw))
            out = np.zeros(max(n, 1), dtype=np.uint32)
            assert n and lib.zkhip_sha256_machine_describe(message_len, which, kind, out.ctypes.data_as(u32p), n, C.byref(ln), C.byref(w), C.byref(pw)) == n
            parts.append(out[:n])
        chips.append(dict(ln=ln.value, W=w.value, Pw=pw.value, prog=parts[0], tab=parts[1]))
    return InnerMachine(chips, key_root, params.num_queries, params.pow_bits, SHA256_PUBLIC)


def machine_verifier_describe(inner, which, kind, n_proofs=1):
    """zkhip_machine_verifier_describe -> (words, log_rows, main width, preprocessed width); kind 0 program, 1 interaction table, 2 preprocessed trace"""
    lib = _lib.load()
    ln, mw, pw = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
    n = lib.zkhip_machine_verifier_describe(C.byref(inner.desc), n_proofs, which, kind, None, 0, C.byref(ln), C.byref(mw), C.byref(pw))
    out = np.zeros(max(n, 1), dtype=np.uint32)
    lib.zkhip_machine_verifier_describe(C.byref(inner.desc), n_proofs, which, kind, out.ctypes.data_as(u32p), n, C.byref(ln), C.byref(mw), C.byref(pw))
    return out[:n], ln.value, mw.value, pw.value


def machine_verifier_host_tables(inner, proofs, public_values, which):
    """zkhip_machine_verifier_host_tables: the main trace of the chip at position `which` as the prover fills it on the host (canonical words, flat); None: refused"""
    lib = _lib.load()
    sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in proofs]
    n = len(sps)
    pv = np.ascontiguousarray(np.array([list(v) for v in public_values], dtype=np.uint32).reshape(n, -1)) if inner.n_public else np.zeros((n, 1), dtype=np.uint32)
    ptrs = (u8p * n)(*[sp.ctypes.data_as(u8p) for sp in sps])
    lens = (C.c_size_t * n)(*[sp.size for sp in sps])
    words = lib.zkhip_machine_verifier_host_tables(C.byref(inner.desc), ptrs, lens, n, pv.ctypes.data_as(u32p), inner.n_public, which, None, 0)
    if words == 0:
        return None
    out = np.zeros(words, dtype=np.uint32)
    assert lib.zkhip_machine_verifier_host_tables(C.byref(inner.desc), ptrs, lens, n, pv.ctypes.data_as(u32p), inner.n_public, which, out.ctypes.data_as(u32p), words) == words
    return out


def machine_verifier_key_host(inner, params=None, n_proofs=1):
    params = params or Params()
    vk = np.zeros(8, dtype=np.uint32)
    check(_lib.load().zkhip_machine_verifier_key_host(C.byref(inner.desc), n_proofs, C.byref(params), vk.ctypes.data_as(u32p)))
    return vk


def verify_machine_recursive(inner, proof, public_values, vk, params=None, n_proofs=1):
    """zkhip_verify_machine_recursive: the outer proof against (the inner machine's description, the inner proofs' public values, the key) -> (rc, reason)"""
    params = params or Params()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(list(public_values) or [0], dtype=np.uint32))
    k = np.ascontiguousarray(np.array(vk, dtype=np.uint32))
    reason = C.c_int(0)
    rc = _lib.load().zkhip_verify_machine_recursive(C.byref(inner.desc), pr.ctypes.data_as(u8p), pr.size, pv.ctypes.data_as(u32p), inner.n_public, n_proofs, k.ctypes.data_as(u32p),
                                                    C.byref(params), C.byref(reason))
    return rc, reason.value


def sha256_compress_key_host(message_len, log_blocks_per_shard, inner=None, outer=None):
    """zkhip_sha256_compress_key_host: the key of the compressed chain for a message of this length, without a device -> 8 words"""
    inner, outer = inner or Params(1, 100, 16), outer or Params(1, 100, 16)
    vk = np.zeros(8, dtype=np.uint32)
    check(_lib.load().zkhip_sha256_compress_key_host(message_len, log_blocks_per_shard, C.byref(inner), C.byref(outer), vk.ctypes.data_as(u32p)))
    return vk


def verify_sha256_compressed(proof, digest, message_len, chain, log_blocks_per_shard, vk, inner=None, outer=None):
    """zkhip_verify_sha256_compressed: "digest = SHA-256 of a message of message_len bytes" from ONE proof, the chain and the key -> (rc, reason)"""
    inner, outer = inner or Params(1, 100, 16), outer or Params(1, 100, 16)
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    dg = np.frombuffer(bytes(digest), dtype=np.uint8)
    ch = np.ascontiguousarray(chain, dtype=np.uint32)
    k = np.ascontiguousarray(np.array(vk, dtype=np.uint32))
    reason = C.c_int(0)
    # the C entry reads 8 (n_shards + 1) chain words, n_shards following from the length: another number of shards is another statement
    if ch.size != 8 * (_lib.load().zkhip_sha256_sharded_count(message_len, log_blocks_per_shard) + 1):
        return -6, 1                                               # ZKHIP_ERR_VERIFY
    rc = _lib.load().zkhip_verify_sha256_compressed(pr.ctypes.data_as(u8p), pr.size, dg.ctypes.data_as(u8p), message_len, ch.ctypes.data_as(u32p), log_blocks_per_shard,
                                                    k.ctypes.data_as(u32p), C.byref(inner), C.byref(outer), C.byref(reason))
    return rc, reason.value


def sha256_air():
    """the SHA-256 compression chip's constraint program (u32 words)"""
    lib = _lib.load()
    n = lib.zkhip_sha256_air(None, 0)
    out = np.empty(n, dtype=np.uint32)
    assert lib.zkhip_sha256_air(out.ctypes.data_as(u32p), n) == n
    return out


class PaddedMessage(bytes):
    """padded blocks that remember the message's length (the statement's other half)"""
    message_len = None


def sha256_pad(message):
    lib = _lib.load()
    m = np.frombuffer(bytes(message), dtype=np.uint8) if len(message) else np.zeros(1, dtype=np.uint8)
    n = lib.zkhip_sha256_pad(m.ctypes.data_as(u8p), len(message), None, 0)
    out = np.empty(n, dtype=np.uint8)
    assert lib.zkhip_sha256_pad(m.ctypes.data_as(u8p), len(message), out.ctypes.data_as(u8p), n) == n
    res = PaddedMessage(out.tobytes())
    res.message_len = len(message)
    return res


def sha256_padding_publics(message_len, first_block=0, n_active=None):
    """zkhip_sha256_padding_publics: the 75 public values a verifier derives from the length (whole message: all its blocks)"""
    if n_active is None:
        n_active = (message_len + 8) // 64 + 1 - first_block
    out = np.zeros(SHA256_PADDING_PUBLIC, dtype=np.uint32)
    _lib.load().zkhip_sha256_padding_publics(message_len, first_block, n_active, out.ctypes.data_as(u32p))
    return out


def verify_sha256(proof, digest, params=None, message_len=None):
    """the statement: digest = SHA-256 of a message of message_len bytes"""
    if message_len is None:
        raise TypeError("verify_sha256: the message length is part of the statement")
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    dg = np.frombuffer(bytes(digest), dtype=np.uint8)
    reason = C.c_int(0)
    rc = lib.zkhip_verify_sha256(pr.ctypes.data_as(u8p), pr.size, dg.ctypes.data_as(u8p), message_len, C.byref(params), C.byref(reason))
    return rc, reason.value


def prove_transcripts(messages, params=None, devices=None, in_flight=4, verify=False, keyed=True):
    """zkhip_prove_transcripts: every message proven as the keyed SHA-256 machine in one call, dealt over `devices` (None: all visible);
    verify: each proof is checked against the key inside the call -> (vk, [(digest bytes, proof bytes), ...]).
    keyed=False: zkhip_prove_transcripts_air -- the chip alone (version-7 proofs, what prove_sha256 makes); vk is None"""
    lib = _lib.load()
    params = params or Params(1, 100, 16)
    n = len(messages)
    jobs = (_lib.TranscriptJob * max(n, 1))()
    keep = []
    for i, m in enumerate(messages):
        msg = np.frombuffer(bytes(m), dtype=np.uint8) if len(m) else np.zeros(1, dtype=np.uint8)
        size = lib.zkhip_sha256_machine_proof_size(len(m), C.byref(params)) if keyed else lib.zkhip_sha256_proof_size(len(m), C.byref(params))
        buf = np.empty(max(size, 1), dtype=np.uint8)
        keep.append((msg, buf))
        jobs[i].message = msg.ctypes.data_as(u8p); jobs[i].message_len = len(m)
        jobs[i].proof = buf.ctypes.data_as(u8p); jobs[i].proof_cap = size
    vk = np.zeros(8, dtype=np.uint32)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    if keyed:
        check(lib.zkhip_prove_transcripts(devs, len(devices) if devices else 0, jobs, n, C.byref(params), in_flight, 1 if verify else 0, vk.ctypes.data_as(u32p)))
    else:
        check(lib.zkhip_prove_transcripts_air(devs, len(devices) if devices else 0, jobs, n, C.byref(params), in_flight, 1 if verify else 0))
    return (vk if keyed else None), [(bytes(jobs[i].digest), keep[i][1][: jobs[i].proof_len]) for i in range(n)]


def prove_fri_indices_batch(shard_proofs, log_n, width, public_values, inner=None, outer=None, devices=None, in_flight=4, verify=False):
    """zkhip_prove_fri_indices_batch: the query-phase machine of every shard proof in one call (the compress-like step), dealt over `devices`
    -> [(proof bytes, vk [8], final value [4], capacity [8]), ...]; public_values: one list per shard proof"""
    lib = _lib.load()
    inner, outer = inner or Params(1, 100, 16), outer or Params(1, 100, 16)
    n = len(shard_proofs)
    size = lib.zkhip_fri_indices_proof_size(log_n, inner.num_queries, inner.pow_bits, C.byref(outer))
    jobs = (_lib.FriJob * max(n, 1))()
    keep = []
    for i, sp in enumerate(shard_proofs):
        a = np.ascontiguousarray(sp, dtype=np.uint8)
        pv = np.ascontiguousarray(np.array(public_values[i], dtype=np.uint32))
        buf = np.empty(max(size, 1), dtype=np.uint8)
        keep.append((a, pv, buf))
        jobs[i].shard_proof = a.ctypes.data_as(u8p); jobs[i].shard_proof_len = a.size
        jobs[i].public_values = pv.ctypes.data_as(u32p); jobs[i].n_public = pv.size
        jobs[i].proof = buf.ctypes.data_as(u8p); jobs[i].proof_cap = size
    devs = (C.c_int * len(devices))(*devices) if devices else None
    check(lib.zkhip_prove_fri_indices_batch(devs, len(devices) if devices else 0, jobs, n, log_n, width, C.byref(inner), C.byref(outer), in_flight, 1 if verify else 0))
    return [(keep[i][2][: jobs[i].proof_len], list(jobs[i].vk), list(jobs[i].final_value), list(jobs[i].capacity)) for i in range(n)]


def prove_fri16_lift_batch(devices, segments, log_n, width, public_values, inner, outer=None, in_flight=0, verify=False, raise_on_error=True, proof_caps=None):
    """zkhip_prove_fri16_lift_batch: every segment proof of `segments` (one shape: log_n, width, the length of a public_values entry, inner) lifted in one call, dealt over
    `devices` (None: every visible device) -> ([lift proof bytes, ...], [status, ...], vk [8]); each proof is prove_fri16_lift_segment's bytes.  A job that fails has an
    empty proof and its own status; the call then raises with the lowest failing job's code and message unless raise_on_error is False (then the message is
    zkhip_last_error's).  proof_caps: per job, the room it is given (default: zkhip_fri16_lift_proof_size)"""
    lib = _lib.load()
    outer = outer or Params(1, 100, 16)
    n = len(segments)
    pvs = [np.ascontiguousarray(np.array(v, dtype=np.uint32)) for v in public_values]
    assert len(pvs) == n and all(v.size == pvs[0].size for v in pvs)
    n_public = pvs[0].size if n else 0
    sh = _fri16_segment_shape(log_n, inner)
    size = lib.zkhip_fri16_lift_proof_size(*sh, int(inner.pow_bits), width, n_public, C.byref(outer)) if sh else 0
    jobs = (_lib.Fri16LiftJob * max(n, 1))()
    keep = []
    for i, sp in enumerate(segments):
        a = np.ascontiguousarray(sp, dtype=np.uint8)
        cap = size if proof_caps is None else int(proof_caps[i])
        buf = np.empty(max(cap, 1), dtype=np.uint8)
        keep.append((a, buf))
        jobs[i].segment_proof = a.ctypes.data_as(u8p); jobs[i].segment_proof_len = a.size
        jobs[i].public_values = pvs[i].ctypes.data_as(u32p)
        jobs[i].proof = buf.ctypes.data_as(u8p); jobs[i].proof_cap = cap
    vk = np.zeros(8, dtype=np.uint32)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    rc = lib.zkhip_prove_fri16_lift_batch(devs, len(devices) if devices else 0, jobs, n, log_n, width, n_public, C.byref(inner), C.byref(outer), in_flight, 1 if verify else 0,
                                          vk.ctypes.data_as(u32p))
    if raise_on_error:
        check(rc)
    return [keep[i][1][: jobs[i].proof_len] for i in range(n)], [int(jobs[i].status) for i in range(n)], vk


def prove_shard_verifier_batch(shard_proofs, proofs_per_join, log_n, width, public_values, inner=None, outer=None, devices=None, in_flight=4, verify=False):
    """zkhip_prove_shard_verifier_batch: len(shard_proofs) / proofs_per_join joins of one shape, dealt over `devices`, `in_flight` at a time on each
    -> ([join proof bytes, ...], vk [8]); public_values: one list per shard proof"""
    lib = _lib.load()
    inner, outer = inner or Params(1, 100, 16), outer or Params(1, 100, 16)
    sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in shard_proofs]
    n = len(sps)
    pv = np.ascontiguousarray(np.array([list(v) for v in public_values], dtype=np.uint32).reshape(max(n, 1), -1))
    n_public = pv.shape[1]
    size = lib.zkhip_shard_verifier_proof_size(log_n, width, inner.num_queries, inner.pow_bits, n_public, proofs_per_join, C.byref(outer))
    if size == 0:
        check(-1)
    n_joins = n // proofs_per_join if proofs_per_join else 0
    buf = np.empty((max(n_joins, 1), size), dtype=np.uint8)
    lens = (C.c_size_t * max(n_joins, 1))()
    ptrs = (u8p * max(n, 1))(*[sp.ctypes.data_as(u8p) for sp in sps])
    plens = (C.c_size_t * max(n, 1))(*[sp.size for sp in sps])
    vk = np.zeros(8, dtype=np.uint32)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    check(lib.zkhip_prove_shard_verifier_batch(devs, len(devices) if devices else 0, ptrs, plens, n, proofs_per_join, log_n, width, pv.ctypes.data_as(u32p), n_public,
                                               C.byref(inner), C.byref(outer), in_flight, 1 if verify else 0, buf.ctypes.data_as(u8p), size, lens, vk.ctypes.data_as(u32p)))
    return [buf[j, : lens[j]] for j in range(n_joins)], vk


def prove_shard_tree(ctx, top_key, join_machine, shard_proofs, proofs_per_join, log_n, width, public_values, inner=None, join_outer=None, top_outer=None, devices=None, in_flight=4):
    """zkhip_prove_shard_tree: shard proofs -> joins of proofs_per_join (in flight, dealt over `devices`) -> ONE proof over the joins on `ctx`
    -> (top proof bytes, [join proof bytes, ...], join vk [8]); join_machine: the InnerMachine of the join machine; public_values: one list per shard proof"""
    lib = _lib.load()
    inner, join_outer, top_outer = inner or Params(1, 100, 16), join_outer or Params(1, 100, 16), top_outer or Params(1, 100, 16)
    sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in shard_proofs]
    n = len(sps)
    pv = np.ascontiguousarray(np.array([list(v) for v in public_values], dtype=np.uint32).reshape(max(n, 1), -1))
    n_public = pv.shape[1]
    jsize = lib.zkhip_shard_verifier_proof_size(log_n, width, inner.num_queries, inner.pow_bits, n_public, proofs_per_join, C.byref(join_outer))
    n_joins = n // proofs_per_join if proofs_per_join else 0
    tsize = lib.zkhip_machine_verifier_proof_size(C.byref(join_machine.desc), max(n_joins, 1), C.byref(top_outer))
    if jsize == 0 or tsize == 0:
        check(-1)
    jbuf = np.empty((max(n_joins, 1), jsize), dtype=np.uint8)
    jlens = (C.c_size_t * max(n_joins, 1))()
    ptrs = (u8p * max(n, 1))(*[sp.ctypes.data_as(u8p) for sp in sps])
    plens = (C.c_size_t * max(n, 1))(*[sp.size for sp in sps])
    jvk = np.zeros(8, dtype=np.uint32)
    top = np.empty(tsize, dtype=np.uint8)
    got = C.c_size_t(0)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    check(lib.zkhip_prove_shard_tree(ctx.handle, top_key.handle, C.byref(join_machine.desc), devs, len(devices) if devices else 0, ptrs, plens, n, proofs_per_join, log_n, width,
                                     pv.ctypes.data_as(u32p), n_public, C.byref(inner), C.byref(join_outer), C.byref(top_outer), in_flight, jbuf.ctypes.data_as(u8p), jsize, jlens,
                                     jvk.ctypes.data_as(u32p), top.ctypes.data_as(u8p), tsize, C.byref(got)))
    return top[: got.value], [jbuf[j, : jlens[j]] for j in range(n_joins)], jvk


LKUP_MAGIC, LKUP_SEND, LKUP_RECEIVE = 0x50554B4C, 0, 1


def interaction_table(interactions):
    """[(LKUP_SEND | LKUP_RECEIVE, multiplicity column or None for the constant 1, bus, [value columns]), ...] -> the flat u32 table of include/zkhip.h"""
    body = []
    for sign, mult, bus, cols in interactions:
        body += [sign, 0xFFFFFFFF if mult is None else mult, bus % _lib.P, len(cols)] + list(cols)
    return np.array([LKUP_MAGIC, len(interactions), 3 + len(body)] + body, dtype=np.uint32)


SP1_SHAPED_SPEC = ((20, 96, 3, 1), (20, 32, 3, 0), (19, 64, 2, -1), (18, 128, 4, -1), (16, 256, 8, -1), (14, 40, 1, -1))
SP1_SHAPED_PRE = ((4, 32),)
BUS_SP1 = 300


class Sp1ShapedShard:
    """SP1's shard structure as a KEYED machine (proof version 11; sp1-core-machine's shards, reference Cargo.lock:5822): chips of mixed heights
    (spec: (log_n, width, LogUp pairs, partner) tallest first), each under the synthetic AIR as a constraint program, pair q of a chip sends the
    (a, b) of column group 2q and receives at group 2q + 1 -- in-table (partner -1), or ACROSS two tables of one height that look each other up
    (chip c sends on bus BUS_SP1 + 16 c + q, its partner receives there: the two cumulative sums cancel) --, and preprocessed leading columns
    on the chips of `pre` ((chip, columns), ...: what setup commits once, sp1.rs:113).  Traces are generated on the device
    (zkhip_gen_trace_logup / _cross, stream seed + 100 shard + chip)."""

    def __init__(self, spec=SP1_SHAPED_SPEC, pre=SP1_SHAPED_PRE, n_public=9):
        self.spec, self.pre, self.n_public = [tuple(c) for c in spec], dict(pre), int(n_public)
        self.programs = [air_synthetic(w, n_public) for _, w, _, _ in self.spec]
        self.tables = []
        for c, (ln, w, pairs, partner) in enumerate(self.spec):
            it = []
            for q in range(pairs):
                it.append((LKUP_SEND, None, BUS_SP1 + 16 * c + q, [8 * q, 8 * q + 1]))
                it.append((LKUP_RECEIVE, None, BUS_SP1 + 16 * (c if partner < 0 else partner) + q, [8 * q + 4, 8 * q + 5]))
            self.tables.append(interaction_table(it) if it else None)
        self.log_ns = [c[0] for c in self.spec]
        self.pre_widths = [self.pre.get(c, 0) for c in range(len(self.spec))]
        self.widths = [w - pw for (_, w, _, _), pw in zip(self.spec, self.pre_widths)]                  # main widths
        self.cells = sum(w << ln for ln, w, _, _ in self.spec)

    def gen_traces(self, ctx, seed, shard):
        """-> the full traces [pre | main] of one shard as DeviceBuffers"""
        out = []
        for c, (ln, w, pairs, partner) in enumerate(self.spec):
            if partner < 0:
                out.append(ctx.gen_trace_logup(seed, 100 * shard + c, ln, w, pairs))
            else:
                out.append(ctx.gen_trace_logup_cross(seed, 100 * shard + c, 100 * shard + partner, ln, w, self.spec[partner][1], pairs))
        return out

    def main_chips(self, traces):
        """the chips argument of Context.prove_machine_keyed: the main columns as views of the full traces"""
        return [(DeviceView(t, pw), ln, w, w + pw) for t, ln, w, pw in zip(traces, self.log_ns, self.widths, self.pre_widths)]

    KEY_SHARD = 9999

    def setup(self, ctx, seed, params=None):
        """the key (zkhip_machine_setup) over the preprocessed columns: the leading columns of the chips of `pre`, generated from a stream of their
        own (shard KEY_SHARD) so that every shard of the execution is proven against ONE key, as a program's shards are.  -> (key, the traces it views)"""
        keep = []
        for c, (ln, w, pairs, partner) in enumerate(self.spec):
            keep.append(ctx.gen_trace_logup(seed, 100 * self.KEY_SHARD + c, ln, w, pairs) if self.pre_widths[c] else None)
            assert not (self.pre_widths[c] and (partner >= 0 or self.pre_widths[c] % 8)), "preprocessed columns: whole in-table pairs"
        return ctx.machine_setup([(t, ln, pw, (w + pw) if pw else 0) for t, ln, w, pw in zip(keep, self.log_ns, self.widths, self.pre_widths)], params), keep

    def inner_machine(self, key_root, params=None):
        params = params or Params(1, 100, 16, 0)
        chips = [dict(ln=ln, W=w, Pw=pw, prog=g, tab=t) for ln, w, pw, g, t in zip(self.log_ns, self.widths, self.pre_widths, self.programs, self.tables)]
        return InnerMachine(chips, key_root, params.num_queries, params.pow_bits, self.n_public)


def recursion_witnesses_on_host(enable):
    """zkhip_recursion_witnesses_on_host: 1 = the recursion machines fill their per-query tables on host threads (rounds 4 - 5), 0 = device kernels; returns the previous setting"""
    return int(_lib.load().zkhip_recursion_witnesses_on_host(1 if enable else 0))


def set_lockstep(max_batch, lanes=0):
    """zkhip_set_lockstep: members per lock-step batch of small transcripts (0 / 1 = off), batches in flight per device (0 = keep)"""
    _lib.load().zkhip_set_lockstep(int(max_batch), int(lanes))


def set_fri_graph(on):
    """zkhip_set_fri_graph: 1 (the default) replays the FRI commit phase as one captured graph per proof, 0 enqueues its launches one by one (a debugging switch)"""
    _lib.load().zkhip_set_fri_graph(1 if on else 0)


def lockstep_stats():
    """(merged launches, member launch requests, rendezvous with differing requests, ns waited at rendezvous, ns issuing merged
    launches, ns in votes) since the library was loaded"""
    out = (C.c_uint64 * 6)()
    _lib.load().zkhip_lockstep_stats(out)
    return tuple(int(v) for v in out)


def p2chip_air():
    """the Poseidon2 chip's constraint program for the parameter set in effect"""
    lib = _lib.load()
    n = lib.zkhip_p2chip_air(None, 0)
    out = np.empty(n, dtype=np.uint32)
    assert lib.zkhip_p2chip_air(out.ctypes.data_as(u32p), n) == n
    return out


def verify_merkle_paths(proof, root, n_paths, params=None):
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    rt = np.ascontiguousarray(root, dtype=np.uint32)
    reason = C.c_int(0)
    rc = lib.zkhip_verify_merkle_paths(pr.ctypes.data_as(u8p), pr.size, rt.ctypes.data_as(u32p), n_paths, C.byref(params), C.byref(reason))
    return rc, reason.value


def p24chip_air():
    """the width-24 Poseidon2 chip's constraint program for the parameter set in effect"""
    lib = _lib.load()
    n = lib.zkhip_p24chip_air(None, 0)
    out = np.empty(n, dtype=np.uint32)
    assert lib.zkhip_p24chip_air(out.ctypes.data_as(u32p), n) == n
    return out


def verify_merkle_paths_p24(proof, root, n_paths, params=None):
    """host-only check of a zkhip_prove_merkle_paths_p24 proof -> (rc, reason)"""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    rt = np.ascontiguousarray(root, dtype=np.uint32)
    reason = C.c_int(0)
    rc = lib.zkhip_verify_merkle_paths_p24(pr.ctypes.data_as(u8p), pr.size, rt.ctypes.data_as(u32p), n_paths, C.byref(params), C.byref(reason))
    return rc, reason.value


def verify_sha256_machine(proof, digest, vk, params=None, message_len=None):
    if message_len is None:
        raise TypeError("verify_sha256_machine: the message length is part of the statement")
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    dg = np.frombuffer(bytes(digest), dtype=np.uint8)
    k = np.ascontiguousarray(np.array(vk, dtype=np.uint32))
    reason = C.c_int(0)
    rc = lib.zkhip_verify_sha256_machine(pr.ctypes.data_as(u8p), pr.size, dg.ctypes.data_as(u8p), message_len, k.ctypes.data_as(u32p), C.byref(params), C.byref(reason))
    return rc, reason.value


def air_synthetic(width, n_public):
    lib = _lib.load()
    n = C.c_size_t(0)
    check(lib.zkhip_air_synthetic(width, n_public, None, 0, C.byref(n)))
    out = np.empty(n.value, dtype=np.uint32)
    check(lib.zkhip_air_synthetic(width, n_public, out.ctypes.data_as(u32p), out.size, C.byref(n)))
    return out


def _program_table(programs):
    n = len(programs)
    keep = [(np.ascontiguousarray(p, dtype=np.uint32) if p is not None else None) for p in programs]
    pp = (u32p * n)(*[(p.ctypes.data_as(u32p) if p is not None else None) for p in keep])
    pw = (C.c_size_t * n)(*[(p.size if p is not None else 0) for p in keep])
    return keep, pp, pw


def fri_view_shard(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri_view_shard: what the FRI check of a fold-by-2 shard proof reads -> {"betas": [R][4], "final": [4], "queries": [(index, value[4],
    siblings [R][4])]} (canonical), or raises if the proof is rejected.  Host only."""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    R, Q = log_n, params.num_queries
    betas, final = np.zeros(4 * R, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    idx, vals, sibs = np.zeros(Q, dtype=np.uint32), np.zeros(4 * Q, dtype=np.uint32), np.zeros(4 * Q * R, dtype=np.uint32)
    check(lib.zkhip_fri_view_shard(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                   betas.ctypes.data_as(u32p), final.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), vals.ctypes.data_as(u32p),
                                   sibs.ctypes.data_as(u32p)))
    return {"betas": betas.reshape(R, 4).tolist(), "final": final.tolist(),
            "queries": [(int(idx[q]), vals[4 * q:4 * q + 4].tolist(), sibs[4 * q * R:4 * (q + 1) * R].reshape(R, 4).tolist()) for q in range(Q)]}


def _fri16_arrays(view):
    """a fold-16 view (fri16_view_shard's dict) -> ((R, F, log_blowup, queries), the flat canonical arrays the entries take)"""
    R, Q = len(view["betas"]), len(view["queries"])
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    arrs = (u(view["betas"]), u(view["final_poly"]), u([q[0] for q in view["queries"]]), u([q[1] for q in view["queries"]]), u([q[2] for q in view["queries"]]))
    assert arrs[1].size == 4 << view["F"] and arrs[4].size == 60 * Q * R
    return (R, view["F"], view["b"], Q), arrs


def fri16_view_shard(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri16_view_shard: what the FRI check of a fold-by-16 shard proof reads -> {"betas": [R][4], "final_poly": [2^F][4], "queries": [(index,
    value[4], siblings [R][15][4])], "roots": [R][8], "paths": [query][layer] flat words, "F", "b", "H"} (canonical), or raises if the proof is
    rejected.  Host only."""
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    F, b, Q = params.log_final, params.log_blowup, params.num_queries
    R, H = max((log_n - F) // 4, 0), log_n + b
    pw = lib.zkhip_fri16_view_path_words(log_n, C.byref(params))
    betas, fp, roots = np.zeros(4 * R, dtype=np.uint32), np.zeros(4 << F, dtype=np.uint32), np.zeros(8 * R, dtype=np.uint32)
    idx, vals, sibs, paths = np.zeros(Q, dtype=np.uint32), np.zeros(4 * Q, dtype=np.uint32), np.zeros(60 * Q * R, dtype=np.uint32), np.zeros(max(pw * Q, 1), dtype=np.uint32)
    check(lib.zkhip_fri16_view_shard(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params), betas.ctypes.data_as(u32p),
                                     fp.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), vals.ctypes.data_as(u32p), sibs.ctypes.data_as(u32p), roots.ctypes.data_as(u32p),
                                     paths.ctypes.data_as(u32p)))
    lhs = [H - 4 * (l + 1) for l in range(R)]
    offs = np.concatenate([[0], np.cumsum([8 * lh for lh in lhs])]).astype(int)
    return {"betas": betas.reshape(R, 4).tolist(), "final_poly": fp.reshape(-1, 4).tolist(), "roots": roots.reshape(R, 8).tolist(), "F": F, "b": b, "H": H,
            "hash_width": 24 if params.hash_width == 24 else 16,
            "queries": [(int(idx[q]), vals[4 * q:4 * q + 4].tolist(), sibs[60 * q * R:60 * (q + 1) * R].reshape(R, 15, 4).tolist()) for q in range(Q)],
            "paths": [[paths[q * pw + offs[l]:q * pw + offs[l + 1]].tolist() for l in range(R)] for q in range(Q)]}


def _describe(entry_name, *shape_args, which, kind):
    """zkhip_<entry_name> of a fold-16 machine: the words of the program (kind 0) or interaction table (kind 1) at machine position `which`
    -> (words, log rows, main width, preprocessed width, table number); raises with the library's message for a shape or position it refuses"""
    entry = getattr(_lib.load(), "zkhip_" + entry_name)
    ln, mw, pw, tb = C.c_int(0), C.c_uint32(0), C.c_uint32(0), C.c_int(0)
    refs = (C.byref(ln), C.byref(mw), C.byref(pw), C.byref(tb))
    n = entry(*shape_args, which, kind, None, 0, *refs)
    if n == 0:
        raise _lib.ZkHipError(-1, entry_name + ": " + _lib.load().zkhip_last_error().decode())
    out = np.zeros(n, dtype=np.uint32)
    assert entry(*shape_args, which, kind, out.ctypes.data_as(u32p), n, *refs) == n
    return out, ln.value, mw.value, pw.value, tb.value


def _verify(entry_name, proof, public_values, *shape_args, vk, params, n_public=None):
    """zkhip_<entry_name> of a fold-16 machine: the proof, the shape, the public values, the key -> (rc, reason).  Host only."""
    params = params or Params(1, 100, 16)
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32).reshape(-1))
    assert n_public is None or pv.size == n_public
    k = np.ascontiguousarray(np.array(vk, dtype=np.uint32))
    reason = C.c_int(0)
    rc = getattr(_lib.load(), "zkhip_" + entry_name)(pr.ctypes.data_as(u8p), pr.size, *shape_args, pv.ctypes.data_as(u32p), k.ctypes.data_as(u32p), C.byref(params),
                                                     C.byref(reason))
    return rc, reason.value


def fri16_describe(R, F, log_blowup, n_queries, which, kind):
    """zkhip_fri16_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` of the fold-16 FRI machine
    -> (words, log rows, main width, preprocessed width, table number: 0 FOLD16, 1 FINAL, 2 LAYERS, 3 QUERIES, 4 COEFFS)"""
    return _describe("fri16_describe", R, F, log_blowup, n_queries, which=which, kind=kind)


def fri16_key_host(view, params=None):
    """zkhip_fri16_key_host: the fold-16 FRI machine's key of a view, without a GPU -> 8 canonical words"""
    return _fri16_key_host("layers", view, params)


def verify_fri16(proof, betas, R, F, log_blowup, n_queries, vk, params=None):
    """zkhip_verify_fri16: the challenges, the key, the shape -> (rc, reason).  Host only."""
    return _verify("verify_fri16", proof, betas, R, F, log_blowup, n_queries, vk=vk, params=params)


def _fri16_paths_arrays(view):
    """a fold-16 view with roots and paths -> ((R, F, log_blowup, queries), inner hash width, the arrays of _fri16_arrays, roots [R][8], paths flat).  A view
    that does not say which hash its commitments use ("hash_width") is taken as width-24."""
    shape, arrs = _fri16_arrays(view)
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    roots, paths = u(view["roots"]), u([c for pq in view["paths"] for pl in pq for c in pl])
    H = view["H"]
    assert roots.size == 8 * shape[0] and paths.size == shape[3] * sum(8 * (H - 4 * (l + 1)) for l in range(shape[0]))
    return shape, int(view.get("hash_width", 24)), arrs, roots, paths


def fri16_paths_describe(R, F, log_blowup, n_queries, which, kind):
    """zkhip_fri16_paths_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` (0..5) of the fold-16 paths
    machine -> (words, log rows, main width, preprocessed width, table number: 0 FOLD16, 1 FINAL, 2 P24L, 3 QUERIES, 4 COEFFS, 5 ROOTS)"""
    return _describe("fri16_paths_describe", R, F, log_blowup, n_queries, which=which, kind=kind)


def fri16_paths_key_host(view, params=None):
    """zkhip_fri16_paths_key_host: the fold-16 paths machine's key of a view, without a GPU -> 8 canonical words"""
    return _fri16_key_host("paths", view, params)


def verify_fri16_paths(proof, betas, R, F, log_blowup, n_queries, vk, params=None):
    """zkhip_verify_fri16_paths: the challenges, the key, the shape -> (rc, reason).  Host only."""
    return _verify("verify_fri16_paths", proof, betas, R, F, log_blowup, n_queries, vk=vk, params=params)


def fri16_view_transcript(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri16_view_transcript: the Fiat-Shamir side of a fold-by-16 proof's FRI view -> {"roots": [R][8], "betas": [R][4], "capacity": [8] (the duplex
    challenger's capacity as the commit phase finds it), "pending": inputs pending there (0), "witness": the proof-of-work witness, "pow_bits"}, or raises
    if the proof is rejected.  Host only."""
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    R = max((log_n - params.log_final) // 4, 0)
    roots, betas, tr = np.zeros(8 * max(R, 1), dtype=np.uint32), np.zeros(4 * max(R, 1), dtype=np.uint32), np.zeros(10, dtype=np.uint32)
    check(lib.zkhip_fri16_view_transcript(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params), roots.ctypes.data_as(u32p),
                                          betas.ctypes.data_as(u32p), tr.ctypes.data_as(u32p)))
    return {"roots": roots[:8 * R].reshape(R, 8).tolist(), "betas": betas[:4 * R].reshape(R, 4).tolist(), "capacity": tr[:8].tolist(), "pending": int(tr[8]),
            "witness": int(tr[9]), "pow_bits": int(params.pow_bits)}


def fri16_indices_describe(R, F, log_blowup, n_queries, pow_bits, which, kind):
    """zkhip_fri16_indices_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` (0..7) of the fold-16 indices
    machine -> (words, log rows, main width, preprocessed width, table number: 0 FOLD16B, 1 FINAL, 2 P24L, 3 QUERIES, 4 COEFFS, 5 ROOTS, 6 P2T, 7 SAMPLES)"""
    return _describe("fri16_indices_describe", R, F, log_blowup, n_queries, pow_bits, which=which, kind=kind)


def fri16_indices_key_host(view, params=None):
    """zkhip_fri16_indices_key_host: the fold-16 indices machine's key of a view (with "pow_bits"), without a GPU -> 8 canonical words"""
    return _fri16_key_host("indices", view, params)


def verify_fri16_indices(proof, capacity, R, F, log_blowup, n_queries, pow_bits, vk, params=None):
    """zkhip_verify_fri16_indices: the shape, the inner proof's grinding bits, the capacity, the key -> (rc, reason).  Host only."""
    return _verify("verify_fri16_indices", proof, capacity, R, F, log_blowup, n_queries, pow_bits, vk=vk, params=params, n_public=8)


FRI16_OPENING_CONSTANTS = ("FA", "ZETA", "ZNX", "YL", "YN", "YQ", "OFFN", "OFFQ")          # the order of the openings machine's public values behind the capacity


def _fri16_openings_arrays(view):
    """an openings view -> (trace width, trace rows [Q][W] flat, quotient rows [Q][8] flat, the constants [8][4] flat)"""
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    W, Q = int(view["W"]), len(view["queries"])
    trows, qrows, consts = u(view["trows"]), u(view["qrows"]), u([view["consts"][n] for n in FRI16_OPENING_CONSTANTS])
    assert trows.size == Q * W and qrows.size == 8 * Q and consts.size == 32
    return W, trows, qrows, consts


def fri16_view_openings(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri16_view_openings: what the reduced openings of a fold-by-16 proof are made of -> {"W", "trows": [Q][W], "qrows": [Q][8], "consts": {name: [4]}},
    or raises if the proof is rejected or has lookup pairs.  Host only."""
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    Q = int(params.num_queries)
    trows, qrows, consts = np.zeros(Q * width, dtype=np.uint32), np.zeros(Q * 8, dtype=np.uint32), np.zeros(32, dtype=np.uint32)
    check(lib.zkhip_fri16_view_openings(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params), trows.ctypes.data_as(u32p),
                                        qrows.ctypes.data_as(u32p), consts.ctypes.data_as(u32p)))
    return {"W": int(width), "trows": trows.reshape(Q, width).tolist(), "qrows": qrows.reshape(Q, 8).tolist(),
            "consts": {n: consts[4 * i:4 * i + 4].tolist() for i, n in enumerate(FRI16_OPENING_CONSTANTS)}}


def fri16_openings_describe(R, F, log_blowup, n_queries, pow_bits, W, which, kind):
    """zkhip_fri16_openings_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` (0..9) of the fold-16 openings machine
    -> (words, log rows, main width, preprocessed width, table number: 0 FOLD16C, 1 FINAL, 2 P24L, 3 QUERY16, 4 COEFFS, 5 ROOTS, 6 P2T, 7 SAMPLES, 8 ROWSUM16, 9 ROWS)"""
    return _describe("fri16_openings_describe", R, F, log_blowup, n_queries, pow_bits, W, which=which, kind=kind)


def fri16_openings_key_host(view, params=None):
    """zkhip_fri16_openings_key_host: the fold-16 openings machine's key of a view (with "pow_bits", "W", "trows", "qrows"), without a GPU -> 8 canonical words"""
    return _fri16_key_host("openings", view, params)


def verify_fri16_openings(proof, public_values, R, F, log_blowup, n_queries, pow_bits, W, vk, params=None):
    """zkhip_verify_fri16_openings: the shape, the inner proof's grinding bits and trace width, the 40 public values (capacity, then the eight constants), the key
    -> (rc, reason).  Host only."""
    return _verify("verify_fri16_openings", proof, public_values, R, F, log_blowup, n_queries, pow_bits, W, vk=vk, params=params, n_public=40)


def _fri16_rowpaths_arrays(view):
    """a row-paths view -> (trace paths [Q][H][8] flat, quotient paths [Q][H][8] flat, trace root [8], quotient root [8])"""
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    Q, H = len(view["queries"]), int(view["H"])
    tpaths, qpaths, troot, qroot = u(view["tpaths"]), u(view["qpaths"]), u(view["troot"]), u(view["qroot"])
    assert tpaths.size == qpaths.size == 8 * H * Q and troot.size == qroot.size == 8
    return tpaths, qpaths, troot, qroot


def fri16_view_row_paths(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri16_view_row_paths: the Merkle paths of the rows a fold-by-16 proof opens -> {"tpaths": [Q][H][8], "qpaths": [Q][H][8], "troot": [8], "qroot": [8]},
    or raises if the proof is rejected, has lookup pairs, a preprocessed commitment of its own or the width-16 hash.  Host only."""
    params = params or _lib.segment_params()
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    Q, H = int(params.num_queries), log_n + int(params.log_blowup)
    tp, qp, tr, qr = np.zeros(Q * H * 8, dtype=np.uint32), np.zeros(Q * H * 8, dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    check(lib.zkhip_fri16_view_row_paths(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                         *[a.ctypes.data_as(u32p) for a in (tp, qp, tr, qr)]))
    return {"tpaths": tp.reshape(Q, H, 8).tolist(), "qpaths": qp.reshape(Q, H, 8).tolist(), "troot": tr.tolist(), "qroot": qr.tolist()}


def fri16_rowpaths_describe(R, F, log_blowup, n_queries, pow_bits, W, which, kind):
    """zkhip_fri16_rowpaths_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` (0..9) of the fold-16 row-paths machine
    -> (words, log rows, main width, preprocessed width, table number: the openings machine's with 9 P24R); raises with the library's message for a shape it refuses"""
    return _describe("fri16_rowpaths_describe", R, F, log_blowup, n_queries, pow_bits, W, which=which, kind=kind)


def fri16_rowpaths_key_host(view, params=None):
    """zkhip_fri16_rowpaths_key_host: the fold-16 row-paths machine's key of a view (with "pow_bits", "W", "troot", "qroot"), without a GPU -> 8 canonical words"""
    return _fri16_key_host("rowpaths", view, params)


def verify_fri16_rowpaths(proof, public_values, R, F, log_blowup, n_queries, pow_bits, W, vk, params=None):
    """zkhip_verify_fri16_rowpaths: the shape, the inner proof's grinding bits and trace width, the 40 public values (capacity, then the eight constants), the key
    -> (rc, reason).  Host only."""
    return _verify("verify_fri16_rowpaths", proof, public_values, R, F, log_blowup, n_queries, pow_bits, W, vk=vk, params=params, n_public=40)


def _fri16_head_arrays(view):
    """a head view -> (the inner proof's public values flat, the opened values [2 W + 8][4] flat)"""
    u = lambda a: np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(-1))
    pubs, opened = u(view["pubs"]), u(view["opened"])
    assert opened.size == 8 * (int(view["W"]) + 4)
    return pubs, opened


# the fields of a whole fold-16 view in the order the prove entries take them (the library's fri16::View), and one row per kind of the machine: the entries' infix, the
# shape words behind (R, F, log_blowup, queries[, inner hash width]), the fields the key entries take, and how many of the view's fields the prove entry takes.  The
# lift machine's key takes the shape alone: fri16_lift_key, fri16_lift_key_host
_FRI16_VIEW = ("betas", "final_poly", "indices", "values", "siblings", "roots", "paths", "capacity", "witness", "trows", "qrows", "consts", "tpaths", "qpaths", "troot", "qroot",
               "pubs", "opened")
_FRI16_KINDS = {
    "layers": ("", (), _FRI16_VIEW[:5], 5),
    "paths": ("_paths", (), ("final_poly", "indices", "values", "roots"), 7),
    "indices": ("_indices", ("pow_bits",), ("final_poly", "values", "roots"), 9),
    "openings": ("_openings", ("pow_bits", "W"), ("final_poly", "trows", "qrows", "roots"), 12),
    "rowpaths": ("_rowpaths", ("pow_bits", "W"), ("final_poly", "roots", "troot", "qroot"), 16),
    "head": ("_head", ("pow_bits", "W", "NP"), ("final_poly", "roots", "troot", "qroot"), 18),
    "identity": ("_identity", ("pow_bits", "W", "NP"), ("final_poly", "roots", "troot", "qroot"), 18),
    "lift": ("_lift", ("pow_bits", "W", "NP"), None, 18),
}


def _fri16_gather(view, kind, fields):
    """a view and the fields an entry of this kind takes of it, each from the gatherer that has it (and checks its size) -> ((R, F, log_blowup, queries), (inner hash width,)
    from the paths machine on, the kind's further shape words, the fields as the entry takes them: pointers to flat canonical arrays, the witness a word)"""
    need, f = set(fields), {}
    if kind == "layers":
        shape, arrs = _fri16_arrays(view)
    else:
        shape, f["hash_width"], arrs, f["roots"], f["paths"] = _fri16_paths_arrays(view)
    f.update(zip(_FRI16_VIEW[:5], arrs))
    if need & {"trows", "qrows", "consts"}:
        _, f["trows"], f["qrows"], f["consts"] = _fri16_openings_arrays(view)
    if need & {"tpaths", "qpaths", "troot", "qroot"}:
        f["tpaths"], f["qpaths"], f["troot"], f["qroot"] = _fri16_rowpaths_arrays(view)
    if need & {"pubs", "opened"}:
        f["pubs"], f["opened"] = _fri16_head_arrays(view)
    if "capacity" in need:
        f["capacity"], f["witness"] = np.ascontiguousarray(np.array(view["capacity"], dtype=np.uint32)), int(view["witness"])
        assert f["capacity"].size == 8
    words = {"pow_bits": lambda: int(view["pow_bits"]), "W": lambda: int(view["W"]), "NP": lambda: len(view["pubs"])}
    return (shape, (f["hash_width"],) if kind != "layers" else (), tuple(words[w]() for w in _FRI16_KINDS[kind][1]),
            [f[n] if n == "witness" else f[n].ctypes.data_as(u32p) for n in fields])


def _fri16_key_host(kind, view, params):
    params = params or Params(1, 100, 16)
    infix, _, fields, _ = _FRI16_KINDS[kind]
    shape, hw, more, args = _fri16_gather(view, kind, fields)
    vk = np.zeros(8, dtype=np.uint32)
    check(getattr(_lib.load(), "zkhip_fri16%s_key_host" % infix)(*shape, *hw, *more, *args, C.byref(params), vk.ctypes.data_as(u32p)))
    return vk


def fri16_view_head(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri16_view_head: the head of a fold-by-16 proof's transcript -> {"opened": [2 W + 8][4] in the order the verifier observes them, "alpha": [4],
    "pubs": the public values}, or raises if the proof is rejected, has lookup pairs, a program, a code group or the width-16 hash.  Host only."""
    params = params or _lib.segment_params()
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    opened, alpha = np.zeros(4 * (2 * width + 8), dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    check(lib.zkhip_fri16_view_head(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params), opened.ctypes.data_as(u32p),
                                    alpha.ctypes.data_as(u32p)))
    return {"opened": opened.reshape(-1, 4).tolist(), "alpha": alpha.tolist(), "pubs": [int(x) for x in pv]}


def fri16_head_describe(R, F, log_blowup, n_queries, pow_bits, W, NP, which, kind):
    """zkhip_fri16_head_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` (0..10) of the fold-16 head machine
    -> (words, log rows, main width, preprocessed width, table number: the row-paths machine's with 10 OPENED16); raises with the library's message for a shape it refuses"""
    return _describe("fri16_head_describe", R, F, log_blowup, n_queries, pow_bits, W, NP, which=which, kind=kind)


def fri16_head_key_host(view, params=None):
    """zkhip_fri16_head_key_host: the fold-16 head machine's key of a view (with "pow_bits", "W", "troot", "qroot", "pubs"), without a GPU -> 8 canonical words"""
    return _fri16_key_host("head", view, params)


def fri16_identity_describe(R, F, log_blowup, n_queries, pow_bits, W, NP, which, kind):
    """zkhip_fri16_identity_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` (0..12) of the fold-16 identity machine
    -> (words, log_rows, main_width, pre_width, table number)"""
    return _describe("fri16_identity_describe", R, F, log_blowup, n_queries, pow_bits, W, NP, which=which, kind=kind)


def fri16_identity_key_host(view, params=None):
    """zkhip_fri16_identity_key_host: the fold-16 identity machine's key of a head view, without a GPU -> 8 canonical words"""
    return _fri16_key_host("identity", view, params)


def verify_fri16_identity(proof, inner_public, R, F, log_blowup, n_queries, pow_bits, W, vk, params=None):
    """zkhip_verify_fri16_identity: verify_fri16_head's arguments -> (rc, reason); host only"""
    return _verify("verify_fri16_identity", proof, inner_public, R, F, log_blowup, n_queries, pow_bits, W, len(inner_public), vk=vk, params=params)


def _fri16_segment_shape(log_n, inner_params):
    """(R, F, log_blowup, Q) of a fold-by-16 proof over 2^log_n rows, or None where the parameters are not a fold-by-16 shape with a committed layer"""
    F, b = int(inner_params.log_final), int(inner_params.log_blowup)
    if int(inner_params.log_fold) != 4 or log_n <= F or (log_n - F) % 4:
        return None
    return (log_n - F) // 4, F, b, int(inner_params.num_queries)


def fri16_lift_describe(R, F, log_blowup, n_queries, pow_bits, W, NP, which, kind):
    """zkhip_fri16_lift_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` (0..12) of the fold-16 lift machine
    -> (words, log_rows, main_width, pre_width, table number)"""
    return _describe("fri16_lift_describe", R, F, log_blowup, n_queries, pow_bits, W, NP, which=which, kind=kind)


def fri16_lift_key_host(R, F, log_blowup, n_queries, pow_bits, W, NP, params=None, hash_width=24):
    """zkhip_fri16_lift_key_host: the fold-16 lift machine's key of a SHAPE (no proof data), without a GPU -> 8 canonical words"""
    params = params or Params(1, 100, 16)
    vk = np.zeros(8, dtype=np.uint32)
    check(_lib.load().zkhip_fri16_lift_key_host(R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(params), vk.ctypes.data_as(u32p)))
    return vk


def fri16_lift_inner_machine(R, F, log_blowup, n_queries, pow_bits, W, NP, lift_params=None, hash_width=24):
    """the lift machine of a shape as an InnerMachine for machine mode: fri16_lift_describe's thirteen positions, the shape's key, lift_params' queries and
    proof-of-work bits -- what the fri16_join entries put together inside the library"""
    lift_params = lift_params or Params(1, 100, 16)
    chips = []
    for which in range(13):
        prog, ln, mw, pw, _ = fri16_lift_describe(R, F, log_blowup, n_queries, pow_bits, W, NP, which, 0)
        tab = fri16_lift_describe(R, F, log_blowup, n_queries, pow_bits, W, NP, which, 1)[0]
        chips.append(dict(ln=ln, W=mw, Pw=pw, prog=prog, tab=tab))
    root = fri16_lift_key_host(R, F, log_blowup, n_queries, pow_bits, W, NP, lift_params, hash_width)
    return InnerMachine(chips, root, lift_params.num_queries, lift_params.pow_bits, NP)


def fri16_join_key_host(R, F, log_blowup, n_queries, pow_bits, W, NP, n_proofs, lift_params=None, params=None, hash_width=24):
    """zkhip_fri16_join_key_host: the join's key of (lift shape, lift parameters, n_proofs, join parameters), without a GPU -> 8 canonical words"""
    lift_params, params = lift_params or Params(1, 100, 16), params or Params(1, 100, 16)
    vk = np.zeros(8, dtype=np.uint32)
    check(_lib.load().zkhip_fri16_join_key_host(R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), n_proofs, C.byref(params), vk.ctypes.data_as(u32p)))
    return vk


def fri16_join_max_proofs(R, F, log_blowup, n_queries, pow_bits, W, NP, lift_params=None, hash_width=24):
    """zkhip_fri16_join_max_proofs: the most lift proofs of this shape one join takes; 0 for a shape the lift refuses (last_error says why)"""
    lift_params = lift_params or Params(1, 100, 16)
    return int(_lib.load().zkhip_fri16_join_max_proofs(R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params)))


def fri16_join_proof_size(R, F, log_blowup, n_queries, pow_bits, W, NP, n_proofs, lift_params=None, params=None, hash_width=24):
    lift_params, params = lift_params or Params(1, 100, 16), params or Params(1, 100, 16)
    return int(_lib.load().zkhip_fri16_join_proof_size(R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), n_proofs, C.byref(params)))


def verify_fri16_join(proof, public_values, R, F, log_blowup, n_queries, pow_bits, W, NP, n_proofs, vk, lift_params=None, params=None, hash_width=24):
    """zkhip_verify_fri16_join: the joined proof against (lift shape, the segments' public values in proof order -- one list per proof --, the join's key) -> (rc, reason);
    host only, no byte of a lift or segment proof"""
    lift_params, params = lift_params or Params(1, 100, 16), params or Params(1, 100, 16)
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    flat = [int(x) for v in public_values for x in v]
    pv = np.ascontiguousarray(np.array(flat or [0], dtype=np.uint32))
    k = np.ascontiguousarray(np.array(vk, dtype=np.uint32))
    reason = C.c_int(0)
    rc = _lib.load().zkhip_verify_fri16_join(R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), pr.ctypes.data_as(u8p), pr.size,
                                             pv.ctypes.data_as(u32p), len(flat), n_proofs, k.ctypes.data_as(u32p), C.byref(params), C.byref(reason))
    return rc, reason.value


def prove_fri16_join_batch(lift_proofs, proofs_per_join, public_values, R, F, log_blowup, n_queries, pow_bits, W, NP, lift_params=None, params=None, devices=None, in_flight=4,
                           verify=False, hash_width=24):
    """zkhip_prove_fri16_join_batch: len(lift_proofs) / proofs_per_join joins of one shape, dealt over `devices`, `in_flight` at a time on each
    -> ([join proof bytes, ...], vk [8]); public_values: one list of NP words per lift proof.  Every join is prove_fri16_join's bytes on the same inputs"""
    lib = _lib.load()
    lift_params, params = lift_params or Params(1, 100, 16), params or Params(1, 100, 16)
    sps = [np.ascontiguousarray(sp, dtype=np.uint8) for sp in lift_proofs]
    n = len(sps)
    pv = np.ascontiguousarray(np.array([int(x) for v in public_values for x in v] or [0], dtype=np.uint32))
    n_pub = sum(len(v) for v in public_values)
    shape = (R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params))
    size = lib.zkhip_fri16_join_proof_size(*shape, max(proofs_per_join, 1), C.byref(params))
    n_joins = n // proofs_per_join if proofs_per_join else 0
    buf = np.empty((max(n_joins, 1), max(size, 4)), dtype=np.uint8)
    lens = (C.c_size_t * max(n_joins, 1))()
    ptrs = (u8p * max(n, 1))(*[sp.ctypes.data_as(u8p) for sp in sps])
    plens = (C.c_size_t * max(n, 1))(*[sp.size for sp in sps])
    vk = np.zeros(8, dtype=np.uint32)
    devs = (C.c_int * len(devices))(*devices) if devices else None
    check(lib.zkhip_prove_fri16_join_batch(devs, len(devices) if devices else 0, *shape, ptrs, plens, n, proofs_per_join, pv.ctypes.data_as(u32p), n_pub, C.byref(params), in_flight,
                                           1 if verify else 0, buf.ctypes.data_as(u8p), buf.shape[1], lens, vk.ctypes.data_as(u32p)))
    return [buf[j, : lens[j]] for j in range(n_joins)], vk


def fri16_tree_max_join(R, F, log_blowup, n_queries, pow_bits, W, NP, lift_params=None, join_params=None, hash_width=24):
    """zkhip_fri16_tree_max_join: the largest join size whose join machine a top takes; 0 if none (last_error says why)"""
    lift_params, join_params = lift_params or Params(1, 100, 16), join_params or Params(1, 100, 16)
    return int(_lib.load().zkhip_fri16_tree_max_join(R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), C.byref(join_params)))


def fri16_tree_max_joins(R, F, log_blowup, n_queries, pow_bits, W, NP, proofs_per_join, lift_params=None, join_params=None, hash_width=24):
    """zkhip_fri16_tree_max_joins: the most joins of proofs_per_join lift proofs one top takes; 0 if none (last_error says why)"""
    lift_params, join_params = lift_params or Params(1, 100, 16), join_params or Params(1, 100, 16)
    return int(_lib.load().zkhip_fri16_tree_max_joins(R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), proofs_per_join, C.byref(join_params)))


def _fri16_tree_shape(R, F, log_blowup, n_queries, pow_bits, W, NP, proofs_per_join, join_vk, n_joins, lift_params, join_params, params, hash_width):
    jvk = np.ascontiguousarray(np.array(join_vk, dtype=np.uint32))
    return jvk, (R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), proofs_per_join, C.byref(join_params), jvk.ctypes.data_as(u32p), n_joins,
                 C.byref(params))


def fri16_tree_key_host(R, F, log_blowup, n_queries, pow_bits, W, NP, proofs_per_join, join_vk, n_joins, lift_params=None, join_params=None, params=None, hash_width=24):
    """zkhip_fri16_tree_key_host: the top's key of (lift shape, lift parameters, join size, join parameters, the joins' key, n_joins, top parameters), without a GPU"""
    lift_params, join_params, params = lift_params or Params(1, 100, 16), join_params or Params(1, 100, 16), params or Params(1, 100, 16)
    _, shape = _fri16_tree_shape(R, F, log_blowup, n_queries, pow_bits, W, NP, proofs_per_join, join_vk, n_joins, lift_params, join_params, params, hash_width)
    vk = np.zeros(8, dtype=np.uint32)
    check(_lib.load().zkhip_fri16_tree_key_host(*shape, vk.ctypes.data_as(u32p)))
    return vk


def fri16_tree_proof_size(R, F, log_blowup, n_queries, pow_bits, W, NP, proofs_per_join, join_vk, n_joins, lift_params=None, join_params=None, params=None, hash_width=24):
    lift_params, join_params, params = lift_params or Params(1, 100, 16), join_params or Params(1, 100, 16), params or Params(1, 100, 16)
    _, shape = _fri16_tree_shape(R, F, log_blowup, n_queries, pow_bits, W, NP, proofs_per_join, join_vk, n_joins, lift_params, join_params, params, hash_width)
    return int(_lib.load().zkhip_fri16_tree_proof_size(*shape))


def verify_fri16_tree(proof, public_values, R, F, log_blowup, n_queries, pow_bits, W, NP, proofs_per_join, join_vk, n_joins, top_vk, lift_params=None, join_params=None,
                      params=None, hash_width=24):
    """zkhip_verify_fri16_tree: the top proof against (lift shape, join size, the joins' key, n_joins, every segment's public values in order -- one list per segment --,
    the top's key) -> (rc, reason); host only, no byte of a segment, lift or join proof"""
    lift_params, join_params, params = lift_params or Params(1, 100, 16), join_params or Params(1, 100, 16), params or Params(1, 100, 16)
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    flat = [int(x) for v in public_values for x in v]
    pv = np.ascontiguousarray(np.array(flat or [0], dtype=np.uint32))
    jvk = np.ascontiguousarray(np.array(join_vk, dtype=np.uint32))
    k = np.ascontiguousarray(np.array(top_vk, dtype=np.uint32))
    reason = C.c_int(0)
    rc = _lib.load().zkhip_verify_fri16_tree(R, F, log_blowup, n_queries, hash_width, pow_bits, W, NP, C.byref(lift_params), proofs_per_join, C.byref(join_params),
                                             jvk.ctypes.data_as(u32p), n_joins, pr.ctypes.data_as(u8p), pr.size, pv.ctypes.data_as(u32p), len(flat), k.ctypes.data_as(u32p),
                                             C.byref(params), C.byref(reason))
    return rc, reason.value


def verify_fri16_lift(proof, inner_public, R, F, log_blowup, n_queries, pow_bits, W, vk, params=None):
    """zkhip_verify_fri16_lift: verify_fri16_head's arguments, vk the SHAPE's key -> (rc, reason); host only"""
    return _verify("verify_fri16_lift", proof, inner_public, R, F, log_blowup, n_queries, pow_bits, W, len(inner_public), vk=vk, params=params)


def verify_fri16_head(proof, inner_public, R, F, log_blowup, n_queries, pow_bits, W, vk, params=None):
    """zkhip_verify_fri16_head: the shape, the inner proof's grinding bits and trace width, the inner proof's public values (the machine's own), the key
    -> (rc, reason).  Host only."""
    return _verify("verify_fri16_head", proof, inner_public, R, F, log_blowup, n_queries, pow_bits, W, len(inner_public), vk=vk, params=params)


def fri_view_transcript(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri_view_transcript -> (roots [R][8], betas [R][4], capacity [8], pending inputs): the Fiat-Shamir side of the FRI view
    (fri_view_witness: the proof-of-work witness, the transcript array's last word)"""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    R = log_n
    roots, betas, tr = np.zeros(8 * R, dtype=np.uint32), np.zeros(4 * R, dtype=np.uint32), np.zeros(10, dtype=np.uint32)
    check(lib.zkhip_fri_view_transcript(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                        roots.ctypes.data_as(u32p), betas.ctypes.data_as(u32p), tr.ctypes.data_as(u32p)))
    return roots.reshape(R, 8).tolist(), betas.reshape(R, 4).tolist(), tr[:8].tolist(), int(tr[8])


def fri_view_witness(proof, log_n, width, public_values=(), params=None):
    """the proof-of-work witness of a shard proof (zkhip_fri_view_transcript's transcript[9])"""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    roots, betas, tr = np.zeros(8 * log_n, dtype=np.uint32), np.zeros(4 * log_n, dtype=np.uint32), np.zeros(10, dtype=np.uint32)
    check(lib.zkhip_fri_view_transcript(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                        roots.ctypes.data_as(u32p), betas.ctypes.data_as(u32p), tr.ctypes.data_as(u32p)))
    return int(tr[9])


def fri_view_all(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri_view_all: the view of fri_view_shard_paths, the challenger's capacity and the proof-of-work witness from ONE pass over the proof
    -> (view, capacity [8], witness)"""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    R, Q = log_n, params.num_queries
    pw = lib.zkhip_fri_view_path_words(R)
    betas, final, idx, vals, sibs = (np.zeros(n, dtype=np.uint32) for n in (4 * R, 4, Q, 4 * Q, 4 * Q * R))
    roots, paths, tr = np.zeros(8 * R, dtype=np.uint32), np.zeros(pw * Q, dtype=np.uint32), np.zeros(10, dtype=np.uint32)
    check(lib.zkhip_fri_view_all(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                 *[a.ctypes.data_as(u32p) for a in (betas, final, idx, vals, sibs, roots, paths, tr)]))
    view = {"betas": betas.reshape(R, 4).tolist(), "final": final.tolist(),
            "queries": [(int(idx[q]), vals[4 * q:4 * q + 4].tolist(), sibs[4 * q * R:4 * (q + 1) * R].reshape(R, 4).tolist()) for q in range(Q)],
            "roots": roots.reshape(R, 8).tolist(), "paths": []}
    per_q = paths.reshape(Q, pw) if Q else paths
    for q in range(Q):
        off, pq = 0, []
        for l in range(R):
            pq.append(per_q[q, off:off + 8 * (R - l)].reshape(R - l, 8).tolist())
            off += 8 * (R - l)
        view["paths"].append(pq)
    return view, tr[:8].tolist(), int(tr[9])


def fri_view_shard_paths(proof, log_n, width, public_values=(), params=None):
    """zkhip_fri_view_shard_paths: the view of fri_view_shard plus "roots": [R][8] and, per query, "paths": [R] lists of (R - l) digests"""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    R, Q = log_n, params.num_queries
    per = int(lib.zkhip_fri_view_path_words(R))
    betas, final = np.zeros(4 * R, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    idx, vals, sibs = np.zeros(Q, dtype=np.uint32), np.zeros(4 * Q, dtype=np.uint32), np.zeros(4 * Q * R, dtype=np.uint32)
    roots, paths = np.zeros(8 * R, dtype=np.uint32), np.zeros(per * Q, dtype=np.uint32)
    check(lib.zkhip_fri_view_shard_paths(pr.ctypes.data_as(u8p), pr.size, log_n, width, pv.ctypes.data_as(u32p), pv.size, C.byref(params),
                                         betas.ctypes.data_as(u32p), final.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), vals.ctypes.data_as(u32p),
                                         sibs.ctypes.data_as(u32p), roots.ctypes.data_as(u32p), paths.ctypes.data_as(u32p)))
    view = {"betas": betas.reshape(R, 4).tolist(), "final": final.tolist(), "roots": roots.reshape(R, 8).tolist(),
            "queries": [(int(idx[q]), vals[4 * q:4 * q + 4].tolist(), sibs[4 * q * R:4 * (q + 1) * R].reshape(R, 4).tolist()) for q in range(Q)], "paths": []}
    for q in range(Q):
        off, pq = q * per, []
        for l in range(R):
            n = 8 * (R - l)
            pq.append(paths[off:off + n].reshape(R - l, 8).tolist())
            off += n
        view["paths"].append(pq)
    return view


def _fri_layers_arrays(view):
    R, Q, betas, idx, vals, sibs = _fri_view_arrays(view)
    roots = np.ascontiguousarray(np.array(view["roots"], dtype=np.uint32).reshape(-1))
    paths = np.ascontiguousarray(np.array([w for pq in view["paths"] for layer in pq for dg in layer for w in dg], dtype=np.uint32))
    return R, Q, betas, idx, vals, sibs, roots, paths


def fri_layers_programs(layers):
    """-> (the Poseidon2 chip's FRI-layers variant, the fold chip's wired form) as the library builds them"""
    lib = _lib.load()
    out = []
    for f in (lib.zkhip_p2chip_air_fri_layers, lib.zkhip_fri_layers_chip_air):
        n = f(layers, None, 0)
        buf = np.zeros(n, dtype=np.uint32)
        assert n and f(layers, buf.ctypes.data_as(u32p), n) == n
        out.append(buf)
    return out


def fri_transcript_programs(layers):
    """-> (the Poseidon2 chip's transcript variant, the fold chip's wired form with the transcript machine's public values)"""
    lib = _lib.load()
    out = []
    for f in (lib.zkhip_p2chip_air_fri_transcript, lib.zkhip_fri_transcript_chip_air):
        n = f(layers, None, 0)
        buf = np.zeros(n, dtype=np.uint32)
        assert n and f(layers, buf.ctypes.data_as(u32p), n) == n
        out.append(buf)
    return out


def fri_indices_programs(layers, inner_pow_bits):
    """-> (the Poseidon2 chip with query-phase rows, the SAMPLES chip): what the query-phase machine adds to the transcript machine"""
    lib = _lib.load()
    out = []
    for which in (0, 1):
        n = lib.zkhip_fri_indices_program(which, layers, inner_pow_bits, None, 0)
        buf = np.zeros(n, dtype=np.uint32)
        assert n and lib.zkhip_fri_indices_program(which, layers, inner_pow_bits, buf.ctypes.data_as(u32p), n) == n
        out.append(buf)
    return out


def verify_shard_recursive(proof, log_n, width, n_queries, inner_pow_bits, public_values, vk, params=None, n_proofs=1, program=None):
    """zkhip_verify_shard_recursive (host): the inner proofs' shape and public values (a flat list: proof 0's, then proof 1's, ...) and the shape's key --
    no byte of an inner proof"""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32).ravel())
    k = np.ascontiguousarray(np.array(vk, dtype=np.uint32))
    reason = C.c_int(0)
    if program is None:
        rc = lib.zkhip_verify_shard_recursive(pr.ctypes.data_as(u8p), pr.size, log_n, width, n_queries, inner_pow_bits, pv.ctypes.data_as(u32p), pv.size // max(n_proofs, 1), n_proofs,
                                              k.ctypes.data_as(u32p), C.byref(params), C.byref(reason))
    else:
        pg = np.ascontiguousarray(program, dtype=np.uint32)
        rc = lib.zkhip_verify_shard_recursive_air(pg.ctypes.data_as(u32p), pg.size, pr.ctypes.data_as(u8p), pr.size, log_n, width, n_queries, inner_pow_bits, pv.ctypes.data_as(u32p),
                                                  pv.size // max(n_proofs, 1), n_proofs, k.ctypes.data_as(u32p), C.byref(params), C.byref(reason))
    return rc, reason.value


def shard_verifier_key_host(log_n, width, n_queries, inner_pow_bits, n_public, params=None, n_proofs=1, program=None):
    """zkhip_shard_verifier_key_host[_air]: the key of the shape (and program) computed on the HOST (no context, no device) -> 8 canonical words"""
    params = params or Params()
    vk = np.zeros(8, dtype=np.uint32)
    if program is None:
        check(_lib.load().zkhip_shard_verifier_key_host(log_n, width, n_queries, inner_pow_bits, n_public, n_proofs, C.byref(params), vk.ctypes.data_as(u32p)))
    else:
        pg = np.ascontiguousarray(program, dtype=np.uint32)
        check(_lib.load().zkhip_shard_verifier_key_host_air(pg.ctypes.data_as(u32p), pg.size, log_n, width, n_queries, inner_pow_bits, n_public, n_proofs, C.byref(params), vk.ctypes.data_as(u32p)))
    return vk


def machine_key_host(traces, log_ns, params=None):
    """zkhip_machine_key_host: traces[c] = None or a [2^log_n][pre_width] array of MONTGOMERY words (host) -> the key's 8 canonical words"""
    params = params or Params()
    arrs = [None if t is None else np.ascontiguousarray(t, dtype=np.uint32) for t in traces]
    ptrs = (u32p * len(arrs))(*[None if a is None else a.ctypes.data_as(u32p) for a in arrs])
    lns = (C.c_int32 * len(arrs))(*[int(x) for x in log_ns])
    pws = np.array([0 if a is None else a.shape[1] for a in arrs], dtype=np.uint32)
    root = np.zeros(8, dtype=np.uint32)
    check(_lib.load().zkhip_machine_key_host(ptrs, lns, pws.ctypes.data_as(u32p), len(arrs), C.byref(params), root.ctypes.data_as(u32p)))
    return root


def shard_verifier_max_proofs(log_n, width, n_queries, inner_pow_bits, n_public, outer=None, program=None):
    """zkhip_shard_verifier_max_proofs[_air] (host): how many shard proofs of this shape ONE join takes (outer: the outer proof's params; None = blowup 2)"""
    o = C.byref(outer) if outer is not None else None
    if program is None:
        return int(_lib.load().zkhip_shard_verifier_max_proofs(log_n, width, n_queries, inner_pow_bits, n_public, o))
    pg = np.ascontiguousarray(program, dtype=np.uint32)
    return int(_lib.load().zkhip_shard_verifier_max_proofs_air(pg.ctypes.data_as(u32p), pg.size, log_n, width, n_queries, inner_pow_bits, n_public, o))


def shard_verifier_describe(log_n, width, n_queries, inner_pow_bits, n_public, which, kind, n_proofs=1, program=None):
    """zkhip_shard_verifier_describe[_air] -> (words, log_rows, main width, preprocessed width); kind 0 program, 1 interaction table, 2 preprocessed trace"""
    lib = _lib.load()
    ln, mw, pw = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
    shape = (log_n, width, n_queries, inner_pow_bits, n_public, n_proofs)
    if program is None:
        fn = lambda *a: lib.zkhip_shard_verifier_describe(*shape, *a)
    else:
        pg = np.ascontiguousarray(program, dtype=np.uint32)
        fn = lambda *a: lib.zkhip_shard_verifier_describe_air(pg.ctypes.data_as(u32p), pg.size, *shape, *a)
    n = fn(which, kind, None, 0, C.byref(ln), C.byref(mw), C.byref(pw))
    out = np.zeros(max(n, 1), dtype=np.uint32)
    fn(which, kind, out.ctypes.data_as(u32p), n, C.byref(ln), C.byref(mw), C.byref(pw))
    return out[:n], ln.value, mw.value, pw.value


def verify_fri_indices(proof, final, capacity, layers, n_queries, inner_pow_bits, vk, params=None):
    """zkhip_verify_fri_indices: the final value, the challenger's capacity, the key -- no challenge, no index"""
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    f = np.ascontiguousarray(np.array(final, dtype=np.uint32))
    c8 = np.ascontiguousarray(np.array(capacity, dtype=np.uint32))
    k = np.ascontiguousarray(np.array(vk, dtype=np.uint32))
    reason = C.c_int(0)
    rc = lib.zkhip_verify_fri_indices(pr.ctypes.data_as(u8p), pr.size, layers, n_queries, inner_pow_bits, f.ctypes.data_as(u32p), c8.ctypes.data_as(u32p),
                                      k.ctypes.data_as(u32p), C.byref(params), C.byref(reason))
    return rc, reason.value






def _fri_view_arrays(view):
    R, Q = len(view["betas"]), len(view["queries"])
    betas = np.ascontiguousarray(np.array(view["betas"], dtype=np.uint32).reshape(-1))
    idx = np.ascontiguousarray(np.array([q[0] for q in view["queries"]], dtype=np.uint32))
    vals = np.ascontiguousarray(np.array([q[1] for q in view["queries"]], dtype=np.uint32).reshape(-1))
    sibs = np.ascontiguousarray(np.array([q[2] for q in view["queries"]], dtype=np.uint32).reshape(-1))
    return R, Q, betas, idx, vals, sibs


def fri_chip_air(layers):
    lib = _lib.load()
    n = lib.zkhip_fri_chip_air(layers, None, 0)
    out = np.zeros(n, dtype=np.uint32)
    assert n and lib.zkhip_fri_chip_air(layers, out.ctypes.data_as(u32p), n) == n
    return out




class MachineKey:
    """the proving key of a keyed machine (device-resident preprocessed traces, LDEs and tree) + what the verifier needs of it"""

    def __init__(self, ctx, handle, root, pre_widths):
        self.ctx, self.handle, self.root, self.pre_widths = ctx, handle, root, pre_widths

    def close(self):
        if self.handle:
            self.ctx.lib.zkhip_machine_key_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_machine_keyed(proof, log_ns, widths, pre_widths, root, programs, tables, public_values=(), params=None):
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    rt = np.ascontiguousarray(np.array(root, dtype=np.uint32))
    n = len(log_ns)
    ln = (C.c_int32 * n)(*[int(x) for x in log_ns])
    ws = (C.c_uint32 * n)(*[int(x) for x in widths])
    pws = (C.c_uint32 * n)(*[int(x) for x in pre_widths])
    kp, pp, pw = _program_table(programs)
    kt, tp, tw = _program_table(tables)
    reason = C.c_int(0)
    rc = lib.zkhip_verify_machine_keyed(pr.ctypes.data_as(u8p), pr.size, ln, ws, pws, rt.ctypes.data_as(u32p), pp, pw, tp, tw, n,
                                        pv.ctypes.data_as(u32p), pv.size, C.byref(params), C.byref(reason))
    return rc, reason.value


def verify_machine(proof, log_ns, widths, programs, tables, public_values=(), params=None):
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    n = len(log_ns)
    ln = (C.c_int32 * n)(*[int(x) for x in log_ns])
    ws = (C.c_uint32 * n)(*[int(x) for x in widths])
    kp, pp, pw = _program_table(programs)
    kt, tp, tw = _program_table(tables)
    reason = C.c_int(0)
    rc = lib.zkhip_verify_machine(pr.ctypes.data_as(u8p), pr.size, ln, ws, pp, pw, tp, tw, n, pv.ctypes.data_as(u32p), pv.size, C.byref(params), C.byref(reason))
    return rc, reason.value


def verify_chips_air(proof, log_ns, widths, programs, public_values=(), params=None):
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    n = len(log_ns)
    ln = (C.c_int32 * n)(*[int(x) for x in log_ns])
    ws = (C.c_uint32 * n)(*[int(x) for x in widths])
    keep, pp, pw = _program_table(programs)
    reason = C.c_int(0)
    rc = lib.zkhip_verify_chips_air(pr.ctypes.data_as(u8p), pr.size, ln, ws, pp, pw, n, pv.ctypes.data_as(u32p), pv.size, C.byref(params), C.byref(reason))
    return rc, reason.value


def verify_chips(proof, log_ns, widths, public_values=(), params=None, pairs=None, partners=None):
    params = params or Params(1, 100, 16)
    lib = _lib.load()
    pr = np.ascontiguousarray(proof, dtype=np.uint8)
    pv = np.ascontiguousarray(np.array(public_values, dtype=np.uint32))
    n = len(log_ns)
    ln = (C.c_int32 * n)(*[int(x) for x in log_ns])
    ws = (C.c_uint32 * n)(*[int(x) for x in widths])
    prs = (C.c_int32 * n)(*[int(x) for x in pairs]) if pairs is not None else None
    pas = (C.c_int32 * n)(*[int(x) for x in partners]) if partners is not None else None
    reason = C.c_int(0)
    rc = lib.zkhip_verify_chips(pr.ctypes.data_as(u8p), pr.size, ln, ws, prs, pas, n, pv.ctypes.data_as(u32p), pv.size, C.byref(params), C.byref(reason))
    return rc, reason.value
