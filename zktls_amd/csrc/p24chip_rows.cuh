// p24chip_rows.cuh -- the device code that writes rows of the width-24 Poseidon2 chip's tables (p24chip.h): the lane-per-path row writer and the Merkle-paths body,
// the cooperative wave-per-path row writer, the layer-paths body (P24L) and the row-paths body (P24R).  A header so that hash.hip (the library's kernels and their
// launchers) and tools/fri16_rowpaths_forms.hip (the two forms of P24R's kernel, checked against each other and timed stand-alone) compile the same text.
#pragma once
#include "poseidon2.cuh"
#include "p24chip.h"

namespace zk {

// ------------------------------------------------------------------ trace of the width-24 Poseidon2 chip (p24chip.h)
// One row = one width-24 permutation with every intermediate the chip's constraints name (poseidon2_chip.cpp), on the width-24 constants of
// the tables in effect (P24K: the constants behind zkhip_merkle_commit_p24_colmajor).  The columns are laid out in the order they are
// produced, each section on a 16-byte boundary: a lane writes its row front to back with 16-byte stores (135 per row).
__device__ __forceinline__ void p24chip_store4(uint32_t* t, uint32_t col, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    *reinterpret_cast<uint4*>(t + col) = make_uint4(a, b, c, d);
}
__device__ __forceinline__ void p24chip_store24(uint32_t* t, uint32_t col, const uint32_t v[24]) {
#pragma unroll
    for (int i = 0; i < 24; i += 4) p24chip_store4(t, col + i, v[i], v[i + 1], v[i + 2], v[i + 3]);
}
// groups: rate-word groups 4..8, 8..12, 12..16 absorbed by a sponge row (0..3; 0 on every other row)
__device__ void p24chip_fill_row(uint32_t* t, const uint32_t in[24], uint32_t bit, uint32_t ch, uint32_t end, uint32_t cnt, uint32_t spg, uint32_t ss,
                                 uint32_t groups, uint32_t out[24]) {
    using namespace p24chip;
    uint32_t s[24];
#pragma unroll
    for (int i = 0; i < 24; i++) s[i] = in[i];
    p24chip_store24(t, IN, s);
    p24_external_linear_dev(s);
    p24chip_store24(t, S0, s);
    auto external_round = [&](uint32_t r) {
        uint32_t x3[24];
#pragma unroll
        for (int i = 0; i < 24; i++) {
            const uint32_t y = fadd(s[i], P24K.ext_rc[r][i]);
            x3[i] = fmul(fmul(y, y), y);
            s[i] = fmul(fmul(x3[i], x3[i]), y);
        }
        p24chip_store24(t, x3e(r), x3);
        p24_external_linear_dev(s);
        p24chip_store24(t, oute(r), s);
    };
#pragma unroll 1
    for (uint32_t r = 0; r < 4; r++) external_round(r);
    // internal rounds: three columns each (63, then the unused column 303), flushed four at a time
    uint32_t w[4];
#pragma unroll
    for (int r = 0; r < 21; r++) {
        const uint32_t y = fadd(s[0], P24K.int_rc[r]);
        const uint32_t x3 = fmul(fmul(y, y), y);
        w[(3 * r) & 3] = s[0];
        if (((3 * r) & 3) == 3) p24chip_store4(t, s0p(0) + 3 * r - 3, w[0], w[1], w[2], w[3]);
        w[(3 * r + 1) & 3] = x3;
        if (((3 * r + 1) & 3) == 3) p24chip_store4(t, s0p(0) + 3 * r + 1 - 3, w[0], w[1], w[2], w[3]);
        s[0] = fmul(fmul(x3, x3), y);
        w[(3 * r + 2) & 3] = s[0];
        if (((3 * r + 2) & 3) == 3) p24chip_store4(t, s0p(0) + 3 * r + 2 - 3, w[0], w[1], w[2], w[3]);
        uint32_t sum = 0u;
#pragma unroll
        for (int i = 0; i < 24; i++) sum = fadd(sum, s[i]);
#pragma unroll
        for (int i = 0; i < 24; i++) s[i] = fadd(fmul(s[i], P24K.diag[i]), sum);
    }
    p24chip_store4(t, SPARE - 3, w[0], w[1], w[2], 0u);
    p24chip_store24(t, SP, s);
#pragma unroll 1
    for (uint32_t r = 4; r < 8; r++) external_round(r);
#pragma unroll
    for (int j = 0; j < 8; j += 4)
        p24chip_store4(t, D + j, bit ? in[8 + j] : in[j], bit ? in[9 + j] : in[1 + j], bit ? in[10 + j] : in[2 + j], bit ? in[11 + j] : in[3 + j]);
    const uint32_t one = MONTY_R1;
    p24chip_store4(t, BIT, bit ? one : 0u, ch ? one : 0u, end ? one : 0u, to_monty(cnt));
    p24chip_store4(t, SPG, spg ? one : 0u, ss ? one : 0u, groups >= 1 ? one : 0u, groups >= 2 ? one : 0u);
    p24chip_store4(t, G(3), groups >= 3 ? one : 0u, spg && groups < 1 ? one : 0u, spg && groups < 2 ? one : 0u, spg && groups < 3 ? one : 0u);
#pragma unroll
    for (int j = 0; j < 24; j++) out[j] = s[j];
}
static_assert(p24chip::BIT % 4 == 0 && p24chip::SPG == p24chip::BIT + 4 && p24chip::G(3) == p24chip::SPG + 4 && p24chip::C(1) == p24chip::G(3) + 1,
              "p24chip_fill_row writes the flag columns four at a time");
static_assert(p24chip::s0p(0) % 4 == 0 && p24chip::SPARE % 4 == 3 && p24chip::SP % 4 == 0 && p24chip::D % 4 == 0, "p24chip_fill_row: 16-byte sections");
// one lane per path (its rows are a serial chain): the sponge rows over the opened row (16 values a row, the last block 4, 8, 12 or 16), then
// one compression row per level; the lanes behind the paths fill the padding rows (permutations of the zero state, no flags) side by side
__device__ __forceinline__ void p24chip_merkle_kernel_body(const p24chip::MerkleTraceArgs& a) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t sponge_rows = (a.row_width + 15) / 16;
    const uint64_t per_path = (uint64_t)sponge_rows + a.depth, path_rows = a.n_paths * per_path;
    uint32_t out[24], in[24];
    if (p < a.n_paths) {
        uint32_t* t = a.trace + p * per_path * a.ld;
#pragma unroll
        for (int j = 0; j < 24; j++) out[j] = 0u;
        if (sponge_rows) {                                       // the leaf: overwrite-mode sponge from the zero state
            const uint32_t* vals = a.leaves + p * a.row_width;
            for (uint32_t k = 0; k < sponge_rows; k++, t += a.ld) {
                const uint32_t n = a.row_width - 16 * k < 16 ? a.row_width - 16 * k : 16u;
#pragma unroll
                for (int j = 0; j < 24; j++) in[j] = (uint32_t)j < n ? to_monty(vals[16 * k + j]) : out[j];
                p24chip_fill_row(t, in, 0u, 0u, 0u, (uint32_t)p, k ? 1u : 0u, k ? 0u : 1u, n / 4 - 1, out);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) out[j] = to_monty(a.leaves[8 * p + j]);
        }
        const uint32_t index = a.indices[p];
        for (uint32_t lvl = 0; lvl < a.depth; lvl++, t += a.ld) {
            const uint32_t bit = (index >> lvl) & 1u;
            const uint32_t* sib = a.siblings + 8 * (p * a.depth + lvl);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t sv = to_monty(sib[j]);
                in[j] = bit ? sv : out[j];
                in[8 + j] = bit ? out[j] : sv;
                in[16 + j] = 0u;
            }
            const uint32_t end = lvl + 1 == a.depth ? 1u : 0u;
            p24chip_fill_row(t, in, bit, (lvl || sponge_rows) ? 1u : 0u, end, (uint32_t)p + end, 0u, 0u, 0u, out);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) a.roots[8 * p + j] = from_monty(out[j]);
        return;
    }
    const uint64_t row = path_rows + (p - a.n_paths);
    if (row >= a.rows) return;
#pragma unroll
    for (int j = 0; j < 24; j++) in[j] = 0u;
    p24chip_fill_row(a.trace + row * a.ld, in, 0u, 0u, 0u, (uint32_t)a.n_paths, 0u, 0u, 0u, out);
}

// the LAYER-PATHS variant (p24chip.h, LayerPathsArgs): the P24L table of the fold-16 paths machine, all layers in ONE launch.  A WAVE per path: lane i < 24 holds
// state word i.  A path is 14 - 27 dependent permutations, so a lane per path (the form above) is bound by one lane's arithmetic; here the S-boxes of an
// external round run side by side, the 4 x 4 blocks and the column sums of the external layer and the internal layer's sum go over cross-lane moves (no LDS),
// and the internal rounds' S-box is computed from lane 0's word.  Every 24-column section is stored by 24 adjacent lanes (96 contiguous bytes), the 64 columns of
// the internal rounds by the whole wave.  The leaf's 64 words are read from the first reader's row of the FOLD16 trace -- already Montgomery, where
// fri16_fold_rows_kernel put the query's own value or the previous layer's fold among the 15 siblings -- and compared, a word per lane, with the other readers'.
// A wave past the paths computes the padding row once and stores it 16 times.  (Timed against the lane-per-path form: DESIGN.md section 3c.)
__device__ __forceinline__ uint32_t p24l_coop_ext_linear(uint32_t x, int lane) {
    const int base = lane & ~3, k = lane & 3;
    uint32_t b0 = (uint32_t)__shfl((int)x, base), b1 = (uint32_t)__shfl((int)x, base + 1), b2 = (uint32_t)__shfl((int)x, base + 2), b3 = (uint32_t)__shfl((int)x, base + 3);
    p2_m4_hl_dev(b0, b1, b2, b3);
    const uint32_t y = k == 0 ? b0 : k == 1 ? b1 : k == 2 ? b2 : b3;
    uint32_t t = 0u;
#pragma unroll
    for (int j = 0; j < 6; j++) t = dadd(t, (uint32_t)__shfl((int)y, k + 4 * j));
    return dadd(y, t);
}
// one row: `in` = this lane's input word (lanes < 24), `ft` = this lane's word of the 24 columns BIT .. K3; the row goes to t, t + ld, ... (nrep times)
__device__ __forceinline__ uint32_t p24l_coop_row(uint32_t* t, uint64_t ld, uint32_t nrep, uint32_t in, uint32_t ft, uint32_t bit) {
    using namespace p24chip;
    const int lane = (int)threadIdx.x, li = lane < 24 ? lane : 0;
    const bool act = lane < 24;
    auto put = [&](uint32_t col, uint32_t v, int n) {
        if (lane < n) for (uint32_t r = 0; r < nrep; r++) t[(uint64_t)r * ld + col + lane] = v;
    };
    uint32_t s = act ? in : 0u;
    put(IN, s, 24);
    s = p24l_coop_ext_linear(s, lane);
    put(S0, s, 24);
    auto external_round = [&](uint32_t r) {
        const uint32_t y = fadd(s, P24K.ext_rc[r][li]), x3 = fmul(fmul(y, y), y);
        put(x3e(r), x3, 24);
        s = p24l_coop_ext_linear(fmul(fmul(x3, x3), y), lane);
        put(oute(r), s, 24);
    };
#pragma unroll 1
    for (uint32_t r = 0; r < 4; r++) external_round(r);
    uint32_t w = 0u;                                            // column s0p(0) + lane of the internal rounds' section
    const uint32_t dg = P24K.diag[li];
#pragma unroll 1
    for (int r = 0; r < 21; r++) {
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s), y = fadd(s0, P24K.int_rc[r]), x3 = fmul(fmul(y, y), y), s7 = fmul(fmul(x3, x3), y);
        w = lane == 3 * r ? s0 : lane == 3 * r + 1 ? x3 : lane == 3 * r + 2 ? s7 : w;
        if (lane == 0) s = s7;
        uint32_t sum = act ? s : 0u;
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) sum = dadd(sum, (uint32_t)__shfl_xor((int)sum, d));
        s = fadd(fmul(s, dg), sum);
    }
    for (uint32_t r = 0; r < nrep; r++) t[(uint64_t)r * ld + s0p(0) + lane] = w;
    put(SP, s, 24);
#pragma unroll 1
    for (uint32_t r = 4; r < 8; r++) external_round(r);
    const uint32_t hi = (uint32_t)__shfl((int)in, (lane + 8) & 63);
    put(D, bit ? hi : in, 8);
    put(BIT, ft, 24);
    return s;
}
static_assert(p24chip::WIDTH_L == p24chip::BIT + 24 && p24chip::s0p(0) + 64 == p24chip::SP, "p24l_coop_row: the flag and tail columns are 24 words, the internal rounds' section 64");
__device__ __forceinline__ void p24chip_layer_paths_kernel_body(const p24chip::LayerPathsArgs& a) {
    using namespace p24chip;
    const uint64_t p = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const uint32_t one = MONTY_R1;
    auto pick = [&](const uint32_t (&v)[24]) {
        uint32_t x = 0u;
#pragma unroll
        for (int j = 0; j < 24; j++) x = lane == j ? v[j] : x;
        return x;
    };
    if (p < a.n_paths) {
        const uint4 d0 = reinterpret_cast<const uint4*>(a.desc)[2 * p], d1 = reinterpret_cast<const uint4*>(a.desc)[2 * p + 1];
        const uint32_t layer = d0.x, row = d0.y, depth = d0.z, mult = d0.w, first = d1.x, rd = d1.y, sib_off = d1.z;
        const uint32_t* leaf = a.fold + (uint64_t)a.readers[rd] * a.fold_ld;
        const uint32_t mine = leaf[lane];
        uint32_t differs = 0u;
        for (uint32_t r = 1; r < mult; r++) {
            const uint32_t theirs = (a.fold + (uint64_t)a.readers[rd + r] * a.fold_ld)[lane];
            if (__ballot(mine != theirs) != 0ull && !differs) differs = r + 1u;
        }
        if (lane == 0) a.differs[p] = differs;
        uint32_t* t = a.trace + (uint64_t)first * a.ld;
        const uint32_t ln = to_monty(layer), kp2 = to_monty(2u * row), m = to_monty(mult), cnt = to_monty((uint32_t)p);
        uint32_t out = 0u;
        for (uint32_t k = 0; k < LEAF_ROWS; k++, t += a.ld) {
            const uint32_t key = 16u * row + 4u * k;
            const uint32_t ft[24] = {0u, 0u, 0u, cnt, k ? one : 0u, k ? 0u : one, one, one, one, 0u, 0u, 0u, ln, kp2, m, 0u,
                                     k == 0 ? one : 0u, k == 1 ? one : 0u, k == 2 ? one : 0u, k == 3 ? one : 0u, to_monty(key), to_monty(key + 1u), to_monty(key + 2u), to_monty(key + 3u)};
            out = p24l_coop_row(t, a.ld, 1u, lane < 16 ? leaf[16u * k + (uint32_t)(lane & 15)] : out, pick(ft), 0u);
        }
        const uint32_t* sib = a.siblings + sib_off;
        for (uint32_t lvl = 0; lvl < depth; lvl++, t += a.ld) {
            const uint32_t bit = (row >> lvl) & 1u, end = lvl + 1 == depth ? 1u : 0u;
            const uint32_t sv = to_monty(sib[8u * lvl + (uint32_t)(lane & 7)]), lo = (uint32_t)__shfl((int)out, lane & 7);
            const uint32_t in = lane < 8 ? (bit ? sv : lo) : lane < 16 ? (bit ? lo : sv) : 0u;
            const uint32_t ft[24] = {bit ? one : 0u, one, end ? one : 0u, to_monty((uint32_t)p + end), 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, ln, to_monty(row >> lvl), 0u, to_monty(lvl + 1u),
                                     0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            out = p24l_coop_row(t, a.ld, 1u, in, pick(ft), bit);
        }
        if (lane < 8) a.ends[8 * p + lane] = from_monty(out);
        return;
    }
    const uint64_t r0 = a.used_rows + (p - a.n_paths) * 16u;
    if (r0 >= a.rows) return;
    const uint32_t n = a.rows - r0 < 16u ? (uint32_t)(a.rows - r0) : 16u;
    p24l_coop_row(a.trace + r0 * a.ld, a.ld, n, 0u, lane == 3 ? to_monty((uint32_t)a.n_paths) : 0u, 0u);
}

// the ROW-PATHS variant (p24chip.h, RowPathsArgs): the P24R table of the fold-16 row-paths machine, the trace tree's and the quotient tree's paths in ONE launch.  A wave
// per path through the cooperative row writer above.  The leaf is read from the RAW opened rows the openings kernel's staging block already holds (canonical words,
// converted here); its length floats: ceil(width / 16) sponge rows, the last one partial when width mod 16 = 8.  On a partial block the lanes at or past the words
// absorbed keep the previous row's output (overwrite mode) -- zero on the first row --, and so do the capacity lanes.  No sharing: two queries that draw one index have
// a path each.  A wave past the paths computes the padding row once and stores it 16 times.  (Timed against the lane-per-path form: DESIGN.md section 3c.)
__device__ __forceinline__ void p24chip_row_paths_kernel_body(const p24chip::RowPathsArgs& a) {
    using namespace p24chip;
    const uint64_t p = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const uint32_t one = MONTY_R1;
    auto pick = [&](const uint32_t (&v)[24]) {
        uint32_t x = 0u;
#pragma unroll
        for (int j = 0; j < 24; j++) x = lane == j ? v[j] : x;
        return x;
    };
    if (p < a.n_paths) {
        const uint4 d0 = reinterpret_cast<const uint4*>(a.desc)[2 * p], d1 = reinterpret_cast<const uint4*>(a.desc)[2 * p + 1];
        const uint32_t tag = d0.x, tree = d0.y, index = d0.z, width = d0.w, first = d1.x, leaf_off = d1.y, sib_off = d1.z;
        const uint32_t* leaf = a.rows + leaf_off;
        uint32_t* t = a.trace + (uint64_t)first * a.ld;
        const uint32_t tg = to_monty(tag), ln = to_monty(tree), kp2 = to_monty(2u * index), ix = to_monty(index), cnt = to_monty((uint32_t)p);
        const uint32_t blocks = (width + 15u) / 16u;
        uint32_t out = 0u;
        for (uint32_t k = 0; k < blocks; k++, t += a.ld) {
            const uint32_t n = width - 16u * k < 16u ? width - 16u * k : 16u, groups = n / 4u - 1u, spg = k ? one : 0u;
            const uint32_t ft[24] = {0u, 0u, 0u, cnt, spg, k ? 0u : one, groups >= 1u ? one : 0u, groups >= 2u ? one : 0u,
                                     groups >= 3u ? one : 0u, k && groups < 1u ? one : 0u, k && groups < 2u ? one : 0u, k && groups < 3u ? one : 0u, tg, ln, kp2, 0u,
                                     ix, to_monty(k), k + 1u == blocks ? one : 0u, one, to_monty(4u * k), to_monty(4u * k + 1u), to_monty(4u * k + 2u), to_monty(4u * k + 3u)};
            uint32_t in = k ? out : 0u;                          // the lanes past the words absorbed, the capacity lanes among them
            if ((uint32_t)lane < n) in = to_monty(leaf[16u * k + (uint32_t)lane]);
            out = p24l_coop_row(t, a.ld, 1u, in, pick(ft), 0u);
        }
        const uint32_t* sib = a.siblings + sib_off;
        for (uint32_t lvl = 0; lvl < a.depth; lvl++, t += a.ld) {
            const uint32_t bit = (index >> lvl) & 1u, end = lvl + 1 == a.depth ? 1u : 0u;
            const uint32_t sv = to_monty(sib[8u * lvl + (uint32_t)(lane & 7)]), lo = (uint32_t)__shfl((int)out, lane & 7);
            const uint32_t in = lane < 8 ? (bit ? sv : lo) : lane < 16 ? (bit ? lo : sv) : 0u;
            const uint32_t ft[24] = {bit ? one : 0u, one, end ? one : 0u, to_monty((uint32_t)p + end), 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, tg, ln, to_monty(index >> lvl), to_monty(lvl + 1u),
                                     0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            out = p24l_coop_row(t, a.ld, 1u, in, pick(ft), bit);
        }
        if (lane < 8) a.ends[8 * p + lane] = from_monty(out);
        return;
    }
    const uint64_t r0 = a.used_rows + (p - a.n_paths) * 16u;
    if (r0 >= a.trace_rows) return;
    const uint32_t n = a.trace_rows - r0 < 16u ? (uint32_t)(a.trace_rows - r0) : 16u;
    p24l_coop_row(a.trace + r0 * a.ld, a.ld, n, 0u, lane == 3 ? to_monty((uint32_t)a.n_paths) : 0u, 0u);
}
static_assert(p24chip::R_TAG == p24chip::BIT + 12 && p24chip::R_K + 4 == p24chip::WIDTH_R, "p24chip_row_paths_kernel: the 24 flag and tail words of a row");

}  // namespace zk
