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
// the openings machine: ROWSUM16 (V[8] ACCIN[4] T[8][4] FA[4]) and QUERY16 (IDX XQ, then RO AT AQ I1 I2 P1 P2 P2O P3 P3O ZETA ZNX YL YN YQ OFFN OFFQ, four words
// each, two unused), both dense
constexpr uint32_t RS_V = 0, RS_ACCIN = 8, RS_T = 12, RS_FA = 44, RS_MAIN16 = 48;
constexpr uint32_t QM_IDX = 0, QM_XQ = 1, QM_RO = 2, QM_ZETA = 42, Q16_MAIN = 72;
constexpr uint32_t MAX_OPEN_W = 1024;
struct OpeningsRowsArgs {
    const uint32_t *trows, *qrows, *consts, *indices;   // canonical words on the device, each array 16-byte aligned: [Q][W], [Q][8], fa zeta zeta g YL YN YQ OFFN OFFQ [8][4], [Q]
    const uint32_t* view_values;                        // [Q][4] canonical, or null: what every reduced opening is compared with
    uint32_t Q, W, H;
    uint64_t rowsum_rows, query_rows;                   // the tables' heights
    uint32_t *rowsum, *query;                           // Montgomery, dense, 16-byte aligned
    uint32_t* openings;                                 // [Q][4] CANONICAL: the reduced openings, where the fold kernel reads its chains' first values
    uint32_t* status;                                   // [4], 0xFFFFFFFF before the launch: the least query whose opening differs from the view's; the least whose point has no inverse
};
struct XqColsArgs {
    const uint32_t* indices; uint32_t Q, R, H;
    uint64_t rows; uint32_t* trace; uint64_t ld; uint32_t col;
};
// the head machine: OPENED16 (V[8] FA[4] FA2[4] PW[4] T[4] PT[4] Y[4] PWN[4]), dense.  One row per 8 opened words (two extension values) in transcript order:
// W / 2 rows of values at zeta, W / 2 of values at zeta g, 4 of quotient values -- three segments, each summed in fa from its own first row
constexpr uint32_t OP_V = 0, OP_FA = 8, OP_FA2 = 12, OP_PW = 16, OP_T = 20, OP_PT = 24, OP_Y = 28, OP_PWN = 32, OP_MAIN16 = 36, OPENED_LANES = 256;
struct OpenedRowsArgs {
    const uint32_t* opened;             // canonical words on the device, 16-byte aligned: [W + 4][8]
    const uint32_t* fa;                 // canonical [4]
    uint32_t W; uint64_t rows;          // the table's height, >= W + 4
    uint32_t* trace;                    // Montgomery, dense, 16-byte aligned
    uint32_t* sums;                     // [4][4] CANONICAL: YL, YN, YQ, OFFN = fa^W, written by the lanes at the segment ends
};
// the identity machine: AIR16 (A B C D DN ALPHA SELT SELF A2 AB ACCIN U1 U2 ACCO, four words each, one row per group of four trace columns) and SCALARS16
// (ALPHA ZETA ZP_1 .. ZP_n INVF SELF SELT QZ_0 .. QZ_7 QK0 QK1 QUO ACC, four words each, ONE row repeated down the table), both dense
constexpr uint32_t AI_A = 0, AI_B = 4, AI_C = 8, AI_D = 12, AI_DN = 16, AI_ALPHA = 20, AI_SELT = 24, AI_SELF = 28, AI_A2 = 32, AI_AB = 36, AI_ACCIN = 40, AI_U1 = 44, AI_U2 = 48,
                   AI_ACCO = 52, AIR_MAIN16 = 56, IDENTITY_LANES = 256;
constexpr uint32_t SC_ALPHA = 0, SC_ZETA = 4, SC_ZP = 8, SC16_LOG_ROWS = 7, SC16_MAX_N = 26;
ZK_HD constexpr uint32_t sc16_invf(uint32_t n) { return SC_ZP + 4u * n; }          // then SELF SELT QZ[8] QK0 QK1 QUO ACC
ZK_HD constexpr uint32_t sc16_width(uint32_t n) { return sc16_invf(n) + 4u * 15u; }
struct IdentityRowsArgs {
    const uint32_t* opened;             // canonical words on the device, 16-byte aligned: [2 W + 8][4], loc, nxt, quotient values
    const uint32_t *alpha, *zeta;       // canonical [4] each
    uint32_t W, n;                      // the trace width (G = W / 4 <= 256 groups); zeta^N takes n squarings
    uint32_t gn_inv, za[2], zb[2];      // Montgomery: 1 / g_N; zps_k = za_k zeta^N + zb_k
    uint64_t air_rows;                  // AIR16's height, G <= air_rows <= 256
    uint32_t *air, *scalars;            // Montgomery, dense, 16-byte aligned; SCALARS16 has 2^7 rows of sc16_width(n) words
    uint32_t* accs;                     // [2][4] CANONICAL: ACCO of the last group, QUO (zeta^N - 1)
};
// the lift machine: the main columns of ROOTS (ENDS BETA[4] FOLDROWS 0 0 ROOT[8]) and COEFFS (0 0 0 0 C[4]), both dense.  The root and coefficient words are read where
// the transcript stage left them on the device: the chain's input states ([rows][16] canonical), in which row `row_layers` + l holds layer root l in its rate half, the
// rows behind the R root rows the final coefficients two a row (F = 0: c_0 in the first four words of the witness row), row `row_quotient` the quotient root, and the
// stream words 10 .. 17 of rows 1 and 2 the trace root
constexpr uint32_t ROOTS_MAIN_L = 16, RL_ROOT = 8, COEFFS_MAIN_L = 8, CL_C = 4, LIFT_STREAM_ROOT = 10;
struct LiftTablesArgs {
    const uint32_t* chain;              // canonical words on the device, 16-byte aligned: [rows][16]
    const uint32_t* roots_base;         // Montgomery [roots_rows][8]: ROOTS' first eight main columns as the transcript launch wrote them, or null: zero
    uint32_t R, F, row_quotient, row_layers;
    uint64_t roots_rows, coeffs_rows;   // the tables' heights: >= R + 2, >= 2^F
    uint32_t *roots_main, *coeffs_main; // Montgomery, dense, 16-byte aligned: [roots_rows][16], [coeffs_rows][8]
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

// ---- the openings machine's rows
__device__ __forceinline__ uint32_t canon_dev(uint32_t m) { return dmul(m, 1u); }          // Montgomery -> canonical
__device__ __forceinline__ Ext ext_sub_from_base(uint32_t x, const Ext& z) { return Ext{{dsub(x, z.c[0]), dsub(0u, z.c[1]), dsub(0u, z.c[2]), dsub(0u, z.c[3])}}; }
__device__ __forceinline__ bool ext_is_zero(const Ext& e) { return (e.c[0] | e.c[1] | e.c[2] | e.c[3]) == 0u; }
// one QUERY16 row from the query's two sums: x = g XQ, I1 = 1 / (x - zeta), I2 = 1 / (x - zeta g), RO = (AT - YL) I1 + OFFN (AT - YN) I2 + OFFQ (AQ - YQ) I1
__device__ __forceinline__ void query16_row(const OpeningsRowsArgs& a, uint32_t q, const Ext& at, const Ext& aq) {
    Ext k[7];                                                          // ZETA ZNX YL YN YQ OFFN OFFQ
#pragma unroll
    for (int i = 0; i < 7; i++) k[i] = ld_ext(a.consts + 4 + 4 * i);
    const uint32_t index = a.indices[q], xq = fpow_dev(root_dev(a.H), brev_dev(index, a.H)), x = dmul(xq, MONTY_GEN);
    const Ext d1 = ext_sub_from_base(x, k[0]), d2 = ext_sub_from_base(x, k[1]);
    const Ext i1 = ext_inv_dev(d1), i2 = ext_inv_dev(d2);
    const Ext p1 = ext_mul_dev(ext_sub_dev(at, k[2]), i1), p2 = ext_mul_dev(ext_sub_dev(at, k[3]), i2), p2o = ext_mul_dev(k[5], p2);
    const Ext p3 = ext_mul_dev(ext_sub_dev(aq, k[4]), i1), p3o = ext_mul_dev(k[6], p3), ro = ext_add_dev(ext_add_dev(p1, p2o), p3o);
    uint32_t w[Q16_MAIN];
    w[QM_IDX] = dmul(index, MONTY_R2); w[QM_XQ] = xq; w[Q16_MAIN - 2] = 0u; w[Q16_MAIN - 1] = 0u;
    auto put = [&](uint32_t col, const Ext& e) { w[col] = e.c[0]; w[col + 1] = e.c[1]; w[col + 2] = e.c[2]; w[col + 3] = e.c[3]; };
    put(QM_RO, ro); put(QM_RO + 4, at); put(QM_RO + 8, aq); put(QM_RO + 12, i1); put(QM_RO + 16, i2);
    put(QM_RO + 20, p1); put(QM_RO + 24, p2); put(QM_RO + 28, p2o); put(QM_RO + 32, p3); put(QM_RO + 36, p3o);
#pragma unroll
    for (int i = 0; i < 7; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) w[QM_ZETA + 4 * i + c] = k[i].c[c];
    uint32_t* t = a.query + (uint64_t)q * Q16_MAIN;
#pragma unroll
    for (uint32_t c = 0; c < Q16_MAIN; c += 4) st4(t + c, w[c], w[c + 1], w[c + 2], w[c + 3]);
    const uint32_t r0 = canon_dev(ro.c[0]), r1 = canon_dev(ro.c[1]), r2 = canon_dev(ro.c[2]), r3 = canon_dev(ro.c[3]);
    st4(a.openings + 4u * q, r0, r1, r2, r3);
    if (a.view_values) {
        const uint4 want = *reinterpret_cast<const uint4*>(a.view_values + 4u * q);
        if (want.x != r0 || want.y != r1 || want.z != r2 || want.w != r3) atomicMin(a.status, q);
    }
    if (ext_is_zero(d1) || ext_is_zero(d2)) atomicMin(a.status + 1, q);
}
// the padding rows of both tables, shared among `lanes` lanes: the constants in the constant columns, zero elsewhere
__device__ __forceinline__ void openings_padding_rows(const OpeningsRowsArgs& a, uint64_t g, uint64_t lanes) {
    const uint4 fa = make_uint4(dmul(a.consts[0], MONTY_R2), dmul(a.consts[1], MONTY_R2), dmul(a.consts[2], MONTY_R2), dmul(a.consts[3], MONTY_R2));
    for (uint64_t r = (uint64_t)a.Q * ((a.W >> 3) + 1u) + g; r < a.rowsum_rows; r += lanes) {
        uint32_t* t = a.rowsum + r * RS_MAIN16;
#pragma unroll
        for (uint32_t c = 0; c < RS_FA; c += 4) st4(t + c, 0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4*>(t + RS_FA) = fa;
    }
    for (uint64_t r = (uint64_t)a.Q + g; r < a.query_rows; r += lanes) {
        uint32_t* t = a.query + r * Q16_MAIN;
        uint32_t w[Q16_MAIN];
#pragma unroll
        for (uint32_t c = 0; c < Q16_MAIN; c++) w[c] = c >= QM_ZETA && c < QM_ZETA + 28u ? dmul(a.consts[4u + c - QM_ZETA], MONTY_R2) : 0u;
#pragma unroll
        for (uint32_t c = 0; c < Q16_MAIN; c += 4) st4(t + c, w[c], w[c + 1], w[c + 2], w[c + 3]);
    }
}

// ROWSUM16 and QUERY16 (the openings machine), one launch.  ROWSUM16 has one row per 8 words of an opened row, per query the trace blocks from the last to the
// first and then the quotient block; a query's trace blocks are one Horner chain in fa (T_s = T_{s+1} fa + V_s down the eight words, ACCIN = the block before's
// T_0), its quotient block a chain of one row.  A lane per ROW: Horner over its own eight words from zero, a segmented cross-lane scan of the blocks' partial sums
// (fri16_final_rows_body's scan with an extension multiplier, fa^8, squared per step; a lane takes from lane - d only while its position in its segment is >= d),
// then each lane redoes its eight steps from the ACCIN that reaches it and writes its row with twelve 16-byte stores.  A segment never straddles a wave without a
// carry: while W / 8 + 1 <= 64 whole queries are packed into a wave (64 / (W / 8 + 1) of them), a taller query has a wave of its own and takes rounds of 64 blocks
// from the top, the running value carried from round to round.  The quotient lane has the trace's sum in the lane before it (or in the carry) and its own in
// hand: it computes the query's QUERY16 row -- the point, the two inversions, the five products -- writes the reduced opening where the fold kernel reads its
// chains' first values and compares it with the view's.  Then all lanes share the padding rows of both tables.
template <bool TALL>
__device__ __forceinline__ void fri16_openings_rows_body(const OpeningsRowsArgs& a) {
    const uint32_t lane = threadIdx.x, WB = a.W >> 3, per = WB + 1u, Q = a.Q;
    const uint32_t qpw = TALL ? 1u : 64u / per, sub = TALL ? 0u : lane / per, q = blockIdx.x * qpw + sub;
    const uint32_t rounds = TALL ? (per + 63u) >> 6 : 1u, reach = TALL ? 64u : per;
    const Ext fa = ld_ext(a.consts), fa2 = ext_mul_dev(fa, fa), fa4 = ext_mul_dev(fa2, fa2), fa8 = ext_mul_dev(fa4, fa4);
    Ext carry = ext_zero();
#pragma unroll 1
    for (uint32_t rd = 0; rd < rounds; rd++) {
        const uint32_t pos = TALL ? rd * 64u + lane : lane - sub * per;
        const bool act = q < Q && sub < qpw && pos < per, quot = pos == WB;
        const uint32_t seg = quot ? 0u : (TALL ? lane : pos);          // position in the segment (TALL: counted from this round's first lane, which starts from the carry)
        uint32_t v[8];
#pragma unroll
        for (int s = 0; s < 8; s++) v[s] = 0u;
        if (act) {
            const uint32_t* src = quot ? a.qrows + 8u * (size_t)q : a.trows + (size_t)q * a.W + 8u * (WB - 1u - pos);
            const uint4 lo = *reinterpret_cast<const uint4*>(src), hi = *reinterpret_cast<const uint4*>(src + 4);
            v[0] = dmul(lo.x, MONTY_R2); v[1] = dmul(lo.y, MONTY_R2); v[2] = dmul(lo.z, MONTY_R2); v[3] = dmul(lo.w, MONTY_R2);
            v[4] = dmul(hi.x, MONTY_R2); v[5] = dmul(hi.y, MONTY_R2); v[6] = dmul(hi.z, MONTY_R2); v[7] = dmul(hi.w, MONTY_R2);
        }
        Ext p = seg == 0u && !quot ? carry : ext_zero();
#pragma unroll
        for (int s = 7; s >= 0; s--) { p = ext_mul_dev(p, fa); p.c[0] = dadd(p.c[0], v[s]); }
        Ext m = fa8;
#pragma unroll 1
        for (uint32_t d = 1; d < reach; d <<= 1) {
            const Ext o = shfl_up_ext(p, d, 64);
            if (seg >= d) p = ext_add_dev(ext_mul_dev(o, m), p);
            m = ext_mul_dev(m, m);
        }
        Ext prev = shfl_up_ext(p, 1u, 64);                             // T_0 of the row before
        if (TALL && lane == 0u) prev = carry;
        const Ext accin = quot ? ext_zero() : (seg == 0u ? carry : prev);
        if (TALL) carry = Ext{{(uint32_t)__shfl((int)p.c[0], 63, 64), (uint32_t)__shfl((int)p.c[1], 63, 64), (uint32_t)__shfl((int)p.c[2], 63, 64), (uint32_t)__shfl((int)p.c[3], 63, 64)}};
        if (!act) continue;
        uint32_t* t = a.rowsum + ((uint64_t)q * per + pos) * RS_MAIN16;
        st4(t + RS_V, v[0], v[1], v[2], v[3]); st4(t + RS_V + 4, v[4], v[5], v[6], v[7]);
        st_ext(t + RS_ACCIN, accin);
        Ext acc = accin;
#pragma unroll
        for (int s = 7; s >= 0; s--) { acc = ext_mul_dev(acc, fa); acc.c[0] = dadd(acc.c[0], v[s]); st_ext(t + RS_T + 4 * s, acc); }
        st_ext(t + RS_FA, fa);
        if (quot) query16_row(a, q, prev, acc);
    }
    openings_padding_rows(a, blockIdx.x * 64u + lane, gridDim.x * 64u);
}
// (the plain form -- a lane per query walking its blocks -- that this one was checked against and timed beside: tools/fri16_openings_forms.hip)
__global__ void __launch_bounds__(64) fri16_openings_rows_kernel(OpeningsRowsArgs a) { fri16_openings_rows_body<false>(a); }
__global__ void __launch_bounds__(64) fri16_openings_rows_tall_kernel(OpeningsRowsArgs a) { fri16_openings_rows_body<true>(a); }

// FOLD16C's column XQ = X sum_j O_j w_16^bitrev(j, 4) = w_{2^(H - 4 l)}^bitrev(index >> 4 l, H - 4 l) on the row of (query, layer l), and the three unused cells
// beside it; zero on the padding rows.  The fold kernel above writes the columns in front of it.
__device__ __forceinline__ void fri16_xq_cols_body(const XqColsArgs& a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.rows) return;
    uint32_t xq = 0u;
    if (r < (uint64_t)a.Q * a.R) {
        const uint32_t q = (uint32_t)(r / a.R), l = (uint32_t)(r % a.R), bits = a.H - 4u * l;
        xq = fpow_dev(root_dev(bits), brev_dev(a.indices[q] >> (4u * l), bits));
    }
    st4(a.trace + r * a.ld + a.col, xq, 0u, 0u, 0u);
}
__global__ void __launch_bounds__(64) fri16_xq_cols_kernel(XqColsArgs a) { fri16_xq_cols_body(a); }

// ---- the head machine's OPENED16 rows.  Row r holds two opened extension values V0, V1; with p its position in its segment (values at zeta, values at zeta g,
// quotient values): PW = fa^(2 p), T = V0 + fa V1, PT = PW T, Y = the segment's sum of PT up to this row, PWN = PW fa^2.  Y at a segment's end is the sum of
// fa^j value_j over the segment; PWN at the end of the first one is fa^W.
__device__ __forceinline__ Ext ext_pow_dev(Ext a, uint32_t e) {
    Ext r = Ext{{MONTY_R1, 0u, 0u, 0u}};
#pragma unroll 1
    while (e) { if (e & 1u) r = ext_mul_dev(r, a); a = ext_mul_dev(a, a); e >>= 1; }
    return r;
}
__device__ __forceinline__ void opened_load(const OpenedRowsArgs& a, uint32_t r, uint32_t v[8]) {
    const uint4 lo = *reinterpret_cast<const uint4*>(a.opened + 8u * (size_t)r), hi = *reinterpret_cast<const uint4*>(a.opened + 8u * (size_t)r + 4);
    v[0] = dmul(lo.x, MONTY_R2); v[1] = dmul(lo.y, MONTY_R2); v[2] = dmul(lo.z, MONTY_R2); v[3] = dmul(lo.w, MONTY_R2);
    v[4] = dmul(hi.x, MONTY_R2); v[5] = dmul(hi.y, MONTY_R2); v[6] = dmul(hi.z, MONTY_R2); v[7] = dmul(hi.w, MONTY_R2);
}
__device__ __forceinline__ void opened_store(const OpenedRowsArgs& a, uint32_t r, const uint32_t v[8], const Ext& fa, const Ext& fa2, const Ext& pw, const Ext& t, const Ext& pt,
                                             const Ext& y, const Ext& pwn) {
    uint32_t* row = a.trace + (uint64_t)r * OP_MAIN16;
    st4(row + OP_V, v[0], v[1], v[2], v[3]); st4(row + OP_V + 4, v[4], v[5], v[6], v[7]);
    st_ext(row + OP_FA, fa); st_ext(row + OP_FA2, fa2); st_ext(row + OP_PW, pw); st_ext(row + OP_T, t); st_ext(row + OP_PT, pt); st_ext(row + OP_Y, y); st_ext(row + OP_PWN, pwn);
    const uint32_t half = a.W >> 1;
    auto canon4 = [&](uint32_t* dst, const Ext& e) { st4(dst, canon_dev(e.c[0]), canon_dev(e.c[1]), canon_dev(e.c[2]), canon_dev(e.c[3])); };
    if (r + 1u == half) { canon4(a.sums, y); canon4(a.sums + 12, pwn); }
    if (r + 1u == a.W) canon4(a.sums + 4, y);
    if (r == a.W + 3u) canon4(a.sums + 8, y);
}
// the padding rows, shared among `lanes` lanes: FA and FA2 in their columns (FA' = FA holds on every transition), zero elsewhere
__device__ __forceinline__ void opened_padding_rows(const OpenedRowsArgs& a, uint32_t g, uint32_t lanes, const Ext& fa, const Ext& fa2) {
    for (uint64_t r = (uint64_t)a.W + 4u + g; r < a.rows; r += lanes) {
        uint32_t* row = a.trace + r * OP_MAIN16;
        st4(row + OP_V, 0u, 0u, 0u, 0u); st4(row + OP_V + 4, 0u, 0u, 0u, 0u);
        st_ext(row + OP_FA, fa); st_ext(row + OP_FA2, fa2);
#pragma unroll
        for (uint32_t c = OP_PW; c < OP_MAIN16; c += 4) st4(row + c, 0u, 0u, 0u, 0u);
    }
}
// The scan form, ONE workgroup of OPENED_LANES lanes: a lane per row computes T and fa^(2 p) from its position (square-and-multiply, at most 9 steps), the lanes of a
// wave take an inclusive segmented sum of PW T with a cross-lane scan (a lane takes from lane - d only while both its position in its segment and its lane number
// are >= d), the waves' last values go through LDS and every lane adds what reaches its wave from the waves before; with more than OPENED_LANES rows (W > 504) the
// workgroup takes rounds, the running value carried in a register every lane computes alike.  No second workgroup, nothing to wait for.
__device__ __forceinline__ void fri16_opened_rows_body(const OpenedRowsArgs& a) {
    constexpr uint32_t WAVES = OPENED_LANES / 64u;
    __shared__ uint32_t tot[WAVES][4];
    __shared__ uint32_t reaches_back[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, half = a.W >> 1, active = a.W + 4u;
    const Ext fa = ld_ext(a.fa), fa2 = ext_mul_dev(fa, fa);
    Ext run = ext_zero();                                              // the sum that reaches the round's first row from the rounds before
#pragma unroll 1
    for (uint32_t base = 0; base < active; base += OPENED_LANES) {
        const uint32_t r = base + tid;
        const bool act = r < active;
        const uint32_t first = r < half ? 0u : (r < a.W ? half : a.W), p = act ? r - first : 0u, reach = p < lane ? p : lane;
        uint32_t v[8];
#pragma unroll
        for (int s = 0; s < 8; s++) v[s] = 0u;
        if (act) opened_load(a, r, v);
        const Ext t = ext_add_dev(Ext{{v[0], v[1], v[2], v[3]}}, ext_mul_dev(fa, Ext{{v[4], v[5], v[6], v[7]}}));
        const Ext pw = ext_pow_dev(fa2, p), pt = act ? ext_mul_dev(pw, t) : ext_zero();
        Ext y = pt;
#pragma unroll 1
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const Ext o = shfl_up_ext(y, d, 64);
            if (reach >= d) y = ext_add_dev(y, o);
        }
        if (lane == 63u) { tot[wave][0] = y.c[0]; tot[wave][1] = y.c[1]; tot[wave][2] = y.c[2]; tot[wave][3] = y.c[3]; reaches_back[wave] = p > 63u ? 1u : 0u; }
        __syncthreads();
        Ext c = run, mine = ext_zero();
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) {
            if (w == wave) mine = c;
            Ext full = Ext{{tot[w][0], tot[w][1], tot[w][2], tot[w][3]}};
            if (reaches_back[w]) full = ext_add_dev(full, c);
            c = full;
        }
        run = c;
        if (p > lane) y = ext_add_dev(y, mine);
        __syncthreads();                                               // (the next round writes tot again)
        if (act) opened_store(a, r, v, fa, fa2, pw, t, pt, y, ext_mul_dev(pw, fa2));
    }
    opened_padding_rows(a, tid, OPENED_LANES, fa, fa2);
}
// The plain form: one lane walks all rows, the others wait for the padding rows (tools/fri16_head_forms.hip checks the scan form against it and times both)
__device__ __forceinline__ void fri16_opened_rows_plain_body(const OpenedRowsArgs& a) {
    const uint32_t tid = threadIdx.x, half = a.W >> 1, active = a.W + 4u;
    const Ext fa = ld_ext(a.fa), fa2 = ext_mul_dev(fa, fa);
    if (tid == 0u) {
        Ext pw = ext_zero(), y = ext_zero();
#pragma unroll 1
        for (uint32_t r = 0; r < active; r++) {
            if (r == 0u || r == half || r == a.W) { pw = Ext{{MONTY_R1, 0u, 0u, 0u}}; y = ext_zero(); }
            uint32_t v[8];
            opened_load(a, r, v);
            const Ext t = ext_add_dev(Ext{{v[0], v[1], v[2], v[3]}}, ext_mul_dev(fa, Ext{{v[4], v[5], v[6], v[7]}})), pt = ext_mul_dev(pw, t), pwn = ext_mul_dev(pw, fa2);
            y = ext_add_dev(y, pt);
            opened_store(a, r, v, fa, fa2, pw, t, pt, y, pwn);
            pw = pwn;
        }
    }
    opened_padding_rows(a, tid, blockDim.x, fa, fa2);
}
__global__ void __launch_bounds__(OPENED_LANES) fri16_opened_rows_kernel(OpenedRowsArgs a) { fri16_opened_rows_body(a); }

// ---- the identity machine's AIR16 and SCALARS16 rows.  Group g holds a, b, c, d = loc[4 g .. 4 g + 3] and dn = nxt[4 g + 3]; with c1 = c - a^2 b - (g + 1),
// c2 = SELT (dn - a b - c - (2 g + 3)), c3 = SELF (d - (5 g + 7)):  U1 = ACCIN alpha + c1, U2 = U1 alpha + c2, ACCO = U2 alpha + c3, ACCIN = the ACCO of the group before.
struct IdentityScalars { Ext alpha, zeta, znn, invf, self, selt; };
__device__ __forceinline__ Ext ext_sub_base_dev(const Ext& e, uint32_t x) { return Ext{{dsub(e.c[0], x), e.c[1], e.c[2], e.c[3]}}; }
__device__ __forceinline__ void identity_scalars(const IdentityRowsArgs& a, IdentityScalars& k) {      // every lane alike: n squarings, one inversion
    k.alpha = ld_ext(a.alpha); k.zeta = ld_ext(a.zeta);
    k.znn = k.zeta;
#pragma unroll 1
    for (uint32_t i = 0; i < a.n; i++) k.znn = ext_mul_dev(k.znn, k.znn);
    k.invf = ext_inv_dev(ext_sub_base_dev(k.zeta, MONTY_R1));
    k.self = ext_mul_dev(ext_sub_base_dev(k.znn, MONTY_R1), k.invf);
    k.selt = ext_sub_base_dev(k.zeta, a.gn_inv);
}
// SCALARS16's one row into `row` (LDS, sc16_width(n) words) and QUO (zeta^N - 1), canonical, where the host reads it: one lane
__device__ __forceinline__ void identity_scalars_row(const IdentityRowsArgs& a, const IdentityScalars& k, uint32_t* row) {
    auto put = [&](uint32_t col, const Ext& e) { row[col] = e.c[0]; row[col + 1] = e.c[1]; row[col + 2] = e.c[2]; row[col + 3] = e.c[3]; };
    put(SC_ALPHA, k.alpha); put(SC_ZETA, k.zeta);
    Ext z = k.zeta;
#pragma unroll 1
    for (uint32_t i = 0; i < a.n; i++) { z = ext_mul_dev(z, z); put(SC_ZP + 4u * i, z); }
    const uint32_t c = sc16_invf(a.n);
    put(c, k.invf); put(c + 4, k.self); put(c + 8, k.selt);
    Ext qk[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
        qk[h] = ext_zero();
#pragma unroll
        for (uint32_t t = 0; t < 4; t++) {
            const Ext q = ld_ext(a.opened + 4u * (2u * (size_t)a.W + 4u * h + t));
            put(c + 12 + 4u * (4u * h + t), q);
            Ext basis = ext_zero();
            basis.c[t] = MONTY_R1;
            qk[h] = ext_add_dev(qk[h], ext_mul_dev(basis, q));
        }
        put(c + 44 + 4u * h, qk[h]);
    }
    Ext z0 = ext_mul_base_dev(k.znn, a.za[0]), z1 = ext_mul_base_dev(k.znn, a.za[1]);
    z0.c[0] = dadd(z0.c[0], a.zb[0]); z1.c[0] = dadd(z1.c[0], a.zb[1]);
    const Ext quo = ext_add_dev(ext_mul_dev(z0, qk[0]), ext_mul_dev(z1, qk[1])), acc = ext_mul_dev(quo, ext_sub_base_dev(k.znn, MONTY_R1));
    put(c + 52, quo); put(c + 56, acc);
    st4(a.accs + 4, canon_dev(acc.c[0]), canon_dev(acc.c[1]), canon_dev(acc.c[2]), canon_dev(acc.c[3]));
}
// the row repeated down SCALARS16, all lanes, adjacent lanes writing adjacent 16 bytes
__device__ __forceinline__ void identity_scalars_rows(const IdentityRowsArgs& a, const uint32_t* row, uint32_t tid, uint32_t lanes) {
    const uint32_t w4 = sc16_width(a.n) >> 2, total = w4 << SC16_LOG_ROWS;
    for (uint32_t i = tid; i < total; i += lanes) {
        const uint32_t c = 4u * (i % w4);
        st4(a.scalars + 4u * (size_t)i, row[c], row[c + 1], row[c + 2], row[c + 3]);
    }
}
struct IdentityGroup { Ext a, b, c, d, dn, a2, ab, c1, c2, c3; };
__device__ __forceinline__ void identity_group(const IdentityRowsArgs& a, const IdentityScalars& k, uint32_t g, IdentityGroup& r) {
    const uint32_t* loc = a.opened + 16u * (size_t)g;
    r.a = ld_ext(loc); r.b = ld_ext(loc + 4); r.c = ld_ext(loc + 8); r.d = ld_ext(loc + 12);
    r.dn = ld_ext(a.opened + 4u * ((size_t)a.W + 4u * g + 3u));
    r.a2 = ext_mul_dev(r.a, r.a); r.ab = ext_mul_dev(r.a, r.b);
    r.c1 = ext_sub_base_dev(ext_sub_dev(r.c, ext_mul_dev(r.a2, r.b)), dmul(g + 1u, MONTY_R2));
    r.c2 = ext_mul_dev(k.selt, ext_sub_base_dev(ext_sub_dev(ext_sub_dev(r.dn, r.ab), r.c), dmul(2u * g + 3u, MONTY_R2)));
    r.c3 = ext_mul_dev(k.self, ext_sub_base_dev(r.d, dmul(5u * g + 7u, MONTY_R2)));
}
// one AIR16 row from the ACCIN that reaches it; returns its ACCO
__device__ __forceinline__ Ext identity_store(const IdentityRowsArgs& a, const IdentityScalars& k, uint32_t g, const IdentityGroup& r, const Ext& accin) {
    const Ext u1 = ext_add_dev(ext_mul_dev(accin, k.alpha), r.c1), u2 = ext_add_dev(ext_mul_dev(u1, k.alpha), r.c2), acco = ext_add_dev(ext_mul_dev(u2, k.alpha), r.c3);
    uint32_t* t = a.air + (uint64_t)g * AIR_MAIN16;
    st_ext(t + AI_A, r.a); st_ext(t + AI_B, r.b); st_ext(t + AI_C, r.c); st_ext(t + AI_D, r.d); st_ext(t + AI_DN, r.dn);
    st_ext(t + AI_ALPHA, k.alpha); st_ext(t + AI_SELT, k.selt); st_ext(t + AI_SELF, k.self); st_ext(t + AI_A2, r.a2); st_ext(t + AI_AB, r.ab);
    st_ext(t + AI_ACCIN, accin); st_ext(t + AI_U1, u1); st_ext(t + AI_U2, u2); st_ext(t + AI_ACCO, acco);
    if (g + 1u == (a.W >> 2)) st4(a.accs, canon_dev(acco.c[0]), canon_dev(acco.c[1]), canon_dev(acco.c[2]), canon_dev(acco.c[3]));
    return acco;
}
__device__ __forceinline__ void identity_zero_row(const IdentityRowsArgs& a, uint32_t g) {
    uint32_t* t = a.air + (uint64_t)g * AIR_MAIN16;
#pragma unroll
    for (uint32_t c = 0; c < AIR_MAIN16; c += 4) st4(t + c, 0u, 0u, 0u, 0u);
}
// The scan form, ONE workgroup of IDENTITY_LANES lanes, a lane per AIR16 row (G <= 256: one round).  ACCO_g = alpha^3 ACCO_(g-1) + t_g with t_g = c1 alpha^2 + c2 alpha
// + c3 is an affine recurrence with one multiplier: an inclusive cross-lane scan in which step d adds alpha^(3 d) times lane - d's value (the power squared per step,
// the same in every lane), the waves' last values joined through LDS as fri16_opened_rows_body does -- wave w starts from c_w = tot_(w-1) + alpha^(3 64) c_(w-1), lane l
// adds alpha^(3 (l + 1)) c_w.  Each lane then redoes its three steps from the ACCIN that reaches it and writes its row.  Lane 0 computes SCALARS16's row into LDS; all
// lanes write it down the table.  No second workgroup, nothing to wait for.
__device__ __forceinline__ void fri16_identity_rows_body(const IdentityRowsArgs& a) {
    __shared__ uint32_t sc_row[sc16_width(SC16_MAX_N)];
    __shared__ uint32_t tot[IDENTITY_LANES / 64u][4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, G = a.W >> 2;
    IdentityScalars k;
    identity_scalars(a, k);
    if (tid == 0u) identity_scalars_row(a, k, sc_row);
    const bool act = tid < G;
    IdentityGroup r;
    Ext p = ext_zero();
    const Ext al2 = ext_mul_dev(k.alpha, k.alpha), al3 = ext_mul_dev(al2, k.alpha);
    if (act) {
        identity_group(a, k, tid, r);
        p = ext_add_dev(ext_add_dev(ext_mul_dev(r.c1, al2), ext_mul_dev(r.c2, k.alpha)), r.c3);
    }
    Ext m = al3;
#pragma unroll 1
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const Ext o = shfl_up_ext(p, d, 64);
        if (lane >= d) p = ext_add_dev(p, ext_mul_dev(o, m));
        m = ext_mul_dev(m, m);
    }
    if (lane == 63u) { tot[wave][0] = p.c[0]; tot[wave][1] = p.c[1]; tot[wave][2] = p.c[2]; tot[wave][3] = p.c[3]; }
    __syncthreads();
    Ext cin = ext_zero();                                              // ACCO of the last lane of the wave before
#pragma unroll 1
    for (uint32_t w = 0; w < wave; w++) cin = ext_add_dev(Ext{{tot[w][0], tot[w][1], tot[w][2], tot[w][3]}}, ext_mul_dev(m, cin));
    p = ext_add_dev(p, ext_mul_dev(ext_pow_dev(al3, lane + 1u), cin));
    Ext accin = shfl_up_ext(p, 1u, 64);
    if (lane == 0u) accin = cin;
    if (act) identity_store(a, k, tid, r, accin);
    else if (tid < a.air_rows) identity_zero_row(a, tid);
    identity_scalars_rows(a, sc_row, tid, IDENTITY_LANES);
}
// The plain form: one lane walks all groups, the others zero the padding rows (tools/fri16_identity_forms.hip checks the scan form against it and times both)
__device__ __forceinline__ void fri16_identity_rows_plain_body(const IdentityRowsArgs& a) {
    __shared__ uint32_t sc_row[sc16_width(SC16_MAX_N)];
    const uint32_t tid = threadIdx.x, G = a.W >> 2;
    IdentityScalars k;
    identity_scalars(a, k);
    if (tid == 0u) {
        identity_scalars_row(a, k, sc_row);
        Ext acc = ext_zero();
#pragma unroll 1
        for (uint32_t g = 0; g < G; g++) {
            IdentityGroup r;
            identity_group(a, k, g, r);
            acc = identity_store(a, k, g, r, acc);
        }
    } else if (tid >= G && tid < a.air_rows) identity_zero_row(a, tid);
    __syncthreads();
    identity_scalars_rows(a, sc_row, tid, blockDim.x);
}
__global__ void __launch_bounds__(IDENTITY_LANES) fri16_identity_rows_kernel(IdentityRowsArgs a) { fri16_identity_rows_body(a); }

// ROOTS' and COEFFS' main columns of the lift machine in one launch: a lane per 16-byte group of a row, adjacent lanes on adjacent addresses -- four groups per ROOTS
// row (two copied from roots_base, two the root's halves), then two per COEFFS row (the unused columns, c_j).  Rows past the active ones are written as zero; the
// words go to Montgomery form here.  Every store is a 16-byte vector store.
__device__ __forceinline__ void fri16_lift_tables_body(const LiftTablesArgs& a) {
    uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t root_groups = 4 * a.roots_rows;
    if (g < root_groups) {
        const uint64_t row = g >> 2;
        const uint32_t grp = (uint32_t)g & 3u, h = grp & 1u;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (grp < 2u) { if (a.roots_base) v = *reinterpret_cast<const uint4*>(a.roots_base + 4 * g - 8 * row); }
        else if (row < a.R) v = *reinterpret_cast<const uint4*>(a.chain + 16 * ((uint64_t)a.row_layers + row) + 4u * h);
        else if (row == a.R) {                                         // the trace root: stream words 10 .. 17, which straddle two rows
            uint32_t w[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) { const uint32_t pos = LIFT_STREAM_ROOT + 4u * h + i; w[i] = a.chain[16u * (pos >> 3) + (pos & 7u)]; }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        } else if (row == (uint64_t)a.R + 1) v = *reinterpret_cast<const uint4*>(a.chain + 16 * (uint64_t)a.row_quotient + 4u * h);
        if (grp >= 2u) v = make_uint4(dmul(v.x, MONTY_R2), dmul(v.y, MONTY_R2), dmul(v.z, MONTY_R2), dmul(v.w, MONTY_R2));
        *reinterpret_cast<uint4*>(a.roots_main + 4 * g) = v;
        return;
    }
    g -= root_groups;
    if (g >= 2 * a.coeffs_rows) return;
    const uint64_t j = g >> 1;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((g & 1u) && j < ((uint64_t)1 << a.F)) {
        const uint64_t row = (uint64_t)a.row_layers + a.R + (a.F ? j >> 1 : 0);
        v = *reinterpret_cast<const uint4*>(a.chain + 16 * row + (a.F ? 4u * ((uint32_t)j & 1u) : 0u));
        v = make_uint4(dmul(v.x, MONTY_R2), dmul(v.y, MONTY_R2), dmul(v.z, MONTY_R2), dmul(v.w, MONTY_R2));
    }
    *reinterpret_cast<uint4*>(a.coeffs_main + 4 * g) = v;
}
__global__ void __launch_bounds__(64) fri16_lift_tables_kernel(LiftTablesArgs a) { fri16_lift_tables_body(a); }
#endif

}  // namespace fri16
}  // namespace zk
