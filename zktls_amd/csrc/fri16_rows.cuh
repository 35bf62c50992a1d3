// fri16_rows.cuh -- column layout of the fold-by-16 FRI machine's two main tables and the gfx950 kernels that fill them from a view's arrays
// (fri16_chip.hip: the constraint programs over these columns, the preprocessed tables and the C entries; tests/fri16_air.py: the same
// rows written a second time).  Every column section starts on a 16-byte boundary, so a lane writes its row with 16-byte stores.
#pragma once
#include <hip/hip_runtime.h>

#include "babybear.cuh"

namespace zk {
namespace fri16 {

// FOLD16, one row per (query, layer)
constexpr uint32_t E = 0, F1 = 64, F2 = 96, F3 = 112, FOLD = 120, OWN = 124, BETA = 128, B2 = 132, B4 = 136, B8 = 140;
constexpr uint32_t X = 144, X2 = 145, X4 = 146, X8 = 147, X16 = 148, XI = 149, XI2 = 150, XI4 = 151, XI8 = 152, ROW = 153, IDX = 154, LN = 155,
                   ACTIVE = 156, G = 157, GX16 = 158, GT = 159, T = 160, B = 161, U = 162, TL = 163;
constexpr uint32_t OF = 164, KJ = 180, L = 196, N = 204;
// FINAL, main columns (the preprocessed schedule J FIRST LAST ACT NL 0 0 0 sits in front of them in the combined row)
constexpr uint32_t FIN_PRE = 8, FIN_MAIN = 16, FC = 0, FACC = 4, FAX = 8, FX = 12;
constexpr int MAX_R = 5, MAX_F = 8, MAX_LF = 11;
constexpr size_t MAX_Q = 1024;

// the lf bits left of ROW on a chain's last row, as up to three nibbles, lowest first
ZK_HD constexpr uint32_t nibble_bits(uint32_t lf, uint32_t k) { return lf > 4 * k ? (lf - 4 * k < 4 ? lf - 4 * k : 4u) : 0u; }
ZK_HD constexpr uint32_t fold16_width(uint32_t lf) {
    uint32_t flags = 0;
    for (uint32_t k = 0; k < 3; k++) if (nibble_bits(lf, k)) flags += 1u << nibble_bits(lf, k);
    return (N + flags + 3u) & ~3u;
}
// prod_i w_{2^(first_bit + i + 5)}^{bit_i(j)}, i < nbits: what bits first_bit .. first_bit + nbits - 1 of a layer-0 row index, holding j, contribute to
// that row's x0 = w_{2^(lh+4)}^bitrev(row, lh)
ZK_HD constexpr uint32_t nibble_factor(uint32_t first_bit, uint32_t nbits, uint32_t j) {
    return fpow(two_adic_generator((int)(first_bit + nbits + 4u)), reverse_bits(j, (int)nbits));
}
// w_16^(-e) = w_16^(16 - e), Montgomery: the constant parts of the fold points' inverses and of the step from x0^16 to the next row's x0
struct W16Inv { uint32_t v[16]; };
ZK_HD constexpr W16Inv w16_inverse_powers() {
    W16Inv t{};
    const uint32_t w = two_adic_generator(4);
    for (uint32_t e = 0; e < 16; e++) t.v[e] = fpow(w, (16u - e) & 15u);
    return t;
}
// step s (0..3), pair t: 1 / w_{2^(4-s)}^bitrev(t, 3-s) = w_16^(-(bitrev(t, 3-s) << s))
ZK_HD constexpr uint32_t step_exponent(uint32_t s, uint32_t t) { return reverse_bits(t, (int)(3u - s)) << s; }

struct ViewArgs {
    const uint32_t *betas, *final_poly, *indices, *values, *siblings;   // canonical words on the device, each array 16-byte aligned: [R][4], [2^F][4], [Q], [Q][4], [Q][R][15][4]
    uint32_t n_queries, R, F, lf, H;
};
struct FoldRowsArgs {
    ViewArgs v;
    uint32_t width; uint64_t rows;      // fold16_width(lf); 2^log_rows >= Q R
    uint32_t* trace; uint64_t ld;       // Montgomery; 16-byte aligned, ld % 4 == 0
    uint32_t* ends;                     // [Q][8] Montgomery: (x0^16, fold[4], 0, 0, 0) of every chain's last row
};
struct FinalRowsArgs {
    ViewArgs v;
    uint64_t rows;                      // 2^log_rows >= Q 2^F
    uint32_t* trace; uint64_t ld;
    uint32_t* ends;                     // [Q][8] Montgomery: (x, acc[4], 0, 0, 0) of every block's last row
};

#if defined(__HIPCC__)
__device__ __forceinline__ Ext ld_ext(const uint32_t* p) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    return Ext{{dmul(v.x, MONTY_R2), dmul(v.y, MONTY_R2), dmul(v.z, MONTY_R2), dmul(v.w, MONTY_R2)}};
}
__device__ __forceinline__ void st_ext(uint32_t* p, const Ext& e) { *reinterpret_cast<uint4*>(p) = make_uint4(e.c[0], e.c[1], e.c[2], e.c[3]); }
__device__ __forceinline__ void st4(uint32_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { *reinterpret_cast<uint4*>(p) = make_uint4(a, b, c, d); }
__device__ __forceinline__ Ext ext_add_dev(const Ext& a, const Ext& b) { return Ext{{dadd(a.c[0], b.c[0]), dadd(a.c[1], b.c[1]), dadd(a.c[2], b.c[2]), dadd(a.c[3], b.c[3])}}; }
__device__ __forceinline__ Ext ext_sub_dev(const Ext& a, const Ext& b) { return Ext{{dsub(a.c[0], b.c[0]), dsub(a.c[1], b.c[1]), dsub(a.c[2], b.c[2]), dsub(a.c[3], b.c[3])}}; }
__device__ __forceinline__ uint32_t fpow_dev(uint32_t a, uint32_t e) {
    uint32_t r = MONTY_R1;
#pragma unroll 1
    while (e) { if (e & 1u) r = dmul(r, a); a = dmul(a, a); e >>= 1; }
    return r;
}
__device__ __forceinline__ uint32_t root_dev(uint32_t bits) {          // w_{2^bits}
    uint32_t g = to_monty(TWO_ADIC_GEN);
#pragma unroll 1
    for (uint32_t i = bits; i < (uint32_t)TWO_ADICITY; i++) g = dmul(g, g);
    return g;
}
// one fold step: n pairs of `in` at the points x0^(2^s) w_{2^(4-s)}^bitrev(t, 3-s); half_xi = 1 / (2 x0^(2^s))
template <int S>
__device__ __forceinline__ void fold_step(const Ext* in, Ext* out, const Ext& beta, uint32_t half_xi) {
    constexpr W16Inv w = w16_inverse_powers();
#pragma unroll
    for (int t = 0; t < (8 >> S); t++) {
        const Ext even = ext_mul_base_dev(ext_add_dev(in[2 * t], in[2 * t + 1]), MONTY_INV2);
        const Ext odd = ext_mul_base_dev(ext_sub_dev(in[2 * t], in[2 * t + 1]), dmul(half_xi, w.v[step_exponent(S, t)]));
        out[t] = ext_add_dev(even, ext_mul_dev(beta, odd));
    }
}
// the 16 entries of the row query q reads at layer l: the 15 of the proof with `own` put at the own position
__device__ __forceinline__ void load_row(const uint32_t* sib, uint32_t own_pos, const Ext& own, Ext* e) {
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        uint32_t k = j - (j > own_pos ? 1u : 0u);
        k = k < 14u ? k : 14u;                                  // (j = own_pos = 15 would read past the 15 entries; its load is not used)
        const Ext s = ld_ext(sib + 4u * k);
#pragma unroll
        for (int c = 0; c < 4; c++) e[j].c[c] = j == own_pos ? own.c[c] : s.c[c];
    }
}

// FOLD16: a lane per (query, layer).  A row needs its chain's earlier folds; the lane refolds that prefix (at most R - 1 = 4 rows of 15 pair folds, no
// stores) instead of one lane per query walking its R rows: with 50 queries that walk keeps one wave busy and puts R row writes (61 16-byte stores each)
// on its critical path, here Q R lanes each write one row.  Lanes past the chains zero the padding rows.
__device__ __forceinline__ uint32_t brev_dev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32u - bits) : 0u; }
__device__ __forceinline__ void fri16_fold_rows_body(const FoldRowsArgs& a) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t R = a.v.R, Q = a.v.n_queries, W = a.width, used = Q * R, H = a.v.H, lf = a.v.lf;
    if (g >= used) {
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x - used;
        for (uint64_t r = (uint64_t)g; r < a.rows; r += stride) {
            uint32_t* row = a.trace + r * a.ld;
            for (uint32_t c = 0; c < W; c += 4) st4(row + c, 0u, 0u, 0u, 0u);
        }
        return;
    }
    const uint32_t q = g / R, l = g % R, index = a.v.indices[q];
    uint32_t idx = index, row = 0, own = 0, x0 = 0, xi = 0, xi2 = 0, xi4 = 0, xi8 = 0;
    Ext val = ld_ext(a.v.values + 4u * q);
    Ext e[16], f1[8], f2[4], f3[2], fold[1], beta, b2, b4, b8;
#pragma unroll 1
    for (uint32_t m = 0;; m++) {
        row = idx >> 4; own = idx & 15u;
        const uint32_t lh = H - 4u * (m + 1u), w = root_dev(lh + 4u), br = brev_dev(row, lh), mask = (1u << (lh + 4u)) - 1u;
        x0 = fpow_dev(w, br);
        xi = fpow_dev(w, (mask + 1u - br) & mask);
        xi2 = dmul(xi, xi); xi4 = dmul(xi2, xi2); xi8 = dmul(xi4, xi4);
        beta = ld_ext(a.v.betas + 4u * m);
        b2 = ext_mul_dev(beta, beta); b4 = ext_mul_dev(b2, b2); b8 = ext_mul_dev(b4, b4);
        load_row(a.v.siblings + 60u * ((size_t)q * R + m), own, val, e);
        fold_step<0>(e, f1, beta, dmul(xi, MONTY_INV2));
        fold_step<1>(f1, f2, b2, dmul(xi2, MONTY_INV2));
        fold_step<2>(f2, f3, b4, dmul(xi4, MONTY_INV2));
        fold_step<3>(f3, fold, b8, dmul(xi8, MONTY_INV2));
        if (m == l) break;
        val = fold[0];
        idx = row;
    }
    uint32_t* t = a.trace + (uint64_t)g * a.ld;
#pragma unroll
    for (int j = 0; j < 16; j++) st_ext(t + E + 4 * j, e[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) st_ext(t + F1 + 4 * j, f1[j]);
#pragma unroll
    for (int j = 0; j < 4; j++) st_ext(t + F2 + 4 * j, f2[j]);
    st_ext(t + F3, f3[0]); st_ext(t + F3 + 4, f3[1]); st_ext(t + FOLD, fold[0]);
    st_ext(t + OWN, val); st_ext(t + BETA, beta); st_ext(t + B2, b2); st_ext(t + B4, b4); st_ext(t + B8, b8);
    // the backward product: this row's factor T, the chain's last factor TL (the lf bits left of its last ROW), B = T_l ... T_{R-1} TL
    const bool end = l + 1u == R;
    const uint32_t last_row = index >> (4u * R);
    uint32_t form[3], flag_pos[3], off = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        const uint32_t nb = nibble_bits(lf, k), nk = (last_row >> (4u * k)) & ((1u << nb) - 1u);
        form[k] = nb ? fpow_dev(root_dev(4u * (R - 1u) + 4u * k + nb + 4u), brev_dev(nk, nb)) : MONTY_R1;
        flag_pos[k] = nb && end ? off + nk : 0xFFFFFFFFu;
        off += nb ? 1u << nb : 0u;
    }
    const uint32_t u = dmul(form[0], form[1]), tl = dmul(u, form[2]);
    uint32_t bacc = tl, tcol = MONTY_R1;
#pragma unroll 1
    for (uint32_t m = R; m-- > l;) {
        const uint32_t tm = m ? fpow_dev(root_dev(4u * m + 4u), brev_dev((index >> (4u * m)) & 15u, 4u)) : MONTY_R1;
        if (m == l) tcol = tm;
        bacc = dmul(bacc, tm);
    }
    const uint32_t x2 = dmul(x0, x0), x4 = dmul(x2, x2), x8 = dmul(x4, x4), x16 = dmul(x8, x8), gate = end ? 0u : MONTY_R1;
    st4(t + X, x0, x2, x4, x8);
    st4(t + X16, x16, xi, xi2, xi4);
    st4(t + XI8, xi8, dmul(row, MONTY_R2), dmul(idx, MONTY_R2), dmul(l, MONTY_R2));
    st4(t + ACTIVE, MONTY_R1, gate, end ? 0u : x16, end ? 0u : tcol);
    st4(t + T, tcol, bacc, end ? u : 0u, end ? tl : 0u);
#pragma unroll
    for (uint32_t j = 0; j < 16; j += 4)
        st4(t + OF + j, own == j ? MONTY_R1 : 0u, own == j + 1 ? MONTY_R1 : 0u, own == j + 2 ? MONTY_R1 : 0u, own == j + 3 ? MONTY_R1 : 0u);
#pragma unroll
    for (uint32_t j = 0; j < 16; j += 4)
        st4(t + KJ + j, dmul(16u * row + j, MONTY_R2), dmul(16u * row + j + 1, MONTY_R2), dmul(16u * row + j + 2, MONTY_R2), dmul(16u * row + j + 3, MONTY_R2));
    st4(t + L, l == 0 ? MONTY_R1 : 0u, l == 1 ? MONTY_R1 : 0u, l == 2 ? MONTY_R1 : 0u, l == 3 ? MONTY_R1 : 0u);
    st4(t + L + 4, l == 4 ? MONTY_R1 : 0u, 0u, 0u, 0u);
    for (uint32_t c = N; c < W; c += 4) {
        uint32_t f[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) { const uint32_t r = c - N + i; f[i] = r == flag_pos[0] || r == flag_pos[1] || r == flag_pos[2] ? MONTY_R1 : 0u; }
        st4(t + c, f[0], f[1], f[2], f[3]);
    }
    if (end) { st4(a.ends + 8u * q, x16, fold[0].c[0], fold[0].c[1], fold[0].c[2]); st4(a.ends + 8u * q + 4, fold[0].c[3], 0u, 0u, 0u); }
}
__global__ void __launch_bounds__(64) fri16_fold_rows_kernel(FoldRowsArgs a) { fri16_fold_rows_body(a); }

// FINAL: per query a block of n = 2^F rows, acc <- acc x + c from the top coefficient down.  The step is an affine map with one x per block, so a block
// is a scan: min(n, 64) lanes per block (a wave per block at n >= 64, several blocks per wave below), each lane Horner over its n / 64 (at most 4)
// coefficients from zero, a log2(lanes)-step cross-lane scan of the partial values (the span's power of x is the same in every lane: squared per step),
// then each lane redoes its rows from the value that reaches it and writes them.  Lanes past the blocks zero the padding rows.
__device__ __forceinline__ Ext shfl_up_ext(const Ext& v, uint32_t d, int width) {
    return Ext{{(uint32_t)__shfl_up((int)v.c[0], d, width), (uint32_t)__shfl_up((int)v.c[1], d, width), (uint32_t)__shfl_up((int)v.c[2], d, width),
                (uint32_t)__shfl_up((int)v.c[3], d, width)}};
}
__device__ __forceinline__ void fri16_final_rows_body(const FinalRowsArgs& a) {
    const uint32_t F = a.v.F, n = 1u << F, per = n > 64u ? n >> 6 : 1u, lanes = n / per;
    const uint64_t r0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * per;       // this lane's rows: r0 .. r0 + per - 1
    const uint32_t blk = (uint32_t)(r0 >> F), first = (uint32_t)r0 & (n - 1u), lam = first / per;
    const bool in_trace = r0 < a.rows, active = in_trace && blk < a.v.n_queries;
    uint32_t x = 0;
    if (active) x = fpow_dev(root_dev(a.v.lf), brev_dev(a.v.indices[blk] >> (4u * a.v.R), a.v.lf));
    Ext p = ext_zero();
    if (active) {
#pragma unroll 1
        for (uint32_t i = 0; i < per; i++) p = ext_add_dev(ext_mul_base_dev(p, x), ld_ext(a.v.final_poly + 4u * (n - 1u - first - i)));
    }
    uint32_t span = x;                                      // x^(rows of the span that ends in this lane)
    for (uint32_t k = per; k > 1u; k >>= 1) span = dmul(span, span);
    for (uint32_t d = 1; d < lanes; d <<= 1) {
        const Ext o = shfl_up_ext(p, d, (int)lanes);
        if (lam >= d) p = ext_add_dev(ext_mul_base_dev(o, span), p);
        span = dmul(span, span);
    }
    Ext acc = shfl_up_ext(p, 1u, (int)lanes);
    if (lam == 0) acc = ext_zero();
    if (!in_trace) return;
#pragma unroll 1
    for (uint32_t i = 0; i < per; i++) {
        uint32_t* t = a.trace + (r0 + i) * a.ld;
        if (!active) { st4(t + FC, 0u, 0u, 0u, 0u); st4(t + FACC, 0u, 0u, 0u, 0u); st4(t + FAX, 0u, 0u, 0u, 0u); st4(t + FX, 0u, 0u, 0u, 0u); continue; }
        const Ext c = ld_ext(a.v.final_poly + 4u * (n - 1u - first - i));
        acc = ext_add_dev(ext_mul_base_dev(acc, x), c);
        st_ext(t + FC, c); st_ext(t + FACC, acc); st_ext(t + FAX, ext_mul_base_dev(acc, x)); st4(t + FX, x, 0u, 0u, 0u);
    }
    if (active && first + per == n) { st4(a.ends + 8u * blk, x, acc.c[0], acc.c[1], acc.c[2]); st4(a.ends + 8u * blk + 4, acc.c[3], 0u, 0u, 0u); }
}
__global__ void __launch_bounds__(64) fri16_final_rows_kernel(FinalRowsArgs a) { fri16_final_rows_body(a); }
#endif

}  // namespace fri16
}  // namespace zk
