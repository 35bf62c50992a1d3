// fri16_rowpaths_forms.hip -- the two forms of the kernel that fills P24R (the fold-16 row-paths machine, zktls_amd/csrc/p24chip_rows.cuh), stand-alone: the WAVE
// form (a wave per path through the cooperative row writer, both trees in one launch; the library's p24chip_row_paths_kernel) and the LANE form (a lane per path:
// the existing p24chip_merkle_kernel run once per tree, which writes the same first 540 columns).  First both forms on the same random rows, siblings and indices
// at shapes on both sides of the partial-block cases, the first 540 columns of every path's rows and every path's end compared word for word; then both timed at
// the full-size shape (Q = 50, W = 128, H = 22: 100 paths, 2 650 rows in 2^12): one process, after a warm-up, alternating, HIP events around the launch (the lane
// form's two launches inside one pair of events), means of 25 launches each.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I zktls_amd/csrc -o tools/fri16_rowpaths_forms tools/fri16_rowpaths_forms.hip && tools/fri16_rowpaths_forms
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "p24chip_rows.cuh"

namespace zk { P2Tables g_p2_tables = P2_BUILTIN; }
using namespace zk;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

__global__ void __launch_bounds__(64) row_paths_wave_kernel(p24chip::RowPathsArgs a) { p24chip_row_paths_kernel_body(a); }
__global__ void __launch_bounds__(64) row_paths_lane_kernel(p24chip::MerkleTraceArgs a) { p24chip_merkle_kernel_body(a); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % P); }

struct Case {
    uint32_t Q, W, H;
    size_t blocks, wave_rows, lane_rows[2], in_words;
    size_t o_trows, o_qrows, o_idx, o_sib[2], o_desc;      // word offsets into d_in; the wave form's siblings are [path][H][8], the lane form's [tree][query][H][8]
    uint32_t *d_in = nullptr, *d_wave = nullptr, *d_lane[2] = {nullptr, nullptr}, *d_ends[2] = {nullptr, nullptr};     // d_ends[0]: wave [2 Q][8]; [1]: lane [tree][Q][8]
    size_t wave_words() const { return wave_rows * p24chip::WIDTH_R; }
    size_t lane_words(int tree) const { return lane_rows[tree] * p24chip::WIDTH; }
};
static size_t pow2_rows(size_t n, int lo) { int l = lo; while (((size_t)1 << l) < n) l++; return (size_t)1 << l; }
static int make_case(Case& c, uint32_t Q, uint32_t W, uint32_t H) {
    c.Q = Q; c.W = W; c.H = H; c.blocks = (W + 15) / 16;
    c.wave_rows = pow2_rows((size_t)Q * (c.blocks + 1 + 2 * H), 6);
    c.lane_rows[0] = pow2_rows((size_t)Q * (c.blocks + H), 5); c.lane_rows[1] = pow2_rows((size_t)Q * (1 + H), 5);
    const size_t nt = (size_t)Q * W, nq = 8 * (size_t)Q, ni = (Q + 3) & ~3u, ns = 8 * (size_t)H * Q;
    c.o_trows = 0; c.o_qrows = nt; c.o_idx = nt + nq; c.o_sib[0] = c.o_idx + ni; c.o_sib[1] = c.o_sib[0] + ns; c.o_desc = c.o_sib[1] + ns;
    const size_t o_wsib = c.o_desc + 16 * (size_t)Q;
    c.in_words = o_wsib + 2 * ns;
    std::vector<uint32_t> in(c.in_words, 0u);
    for (size_t i = 0; i < nt + nq; i++) in[i] = rnd();
    for (uint32_t q = 0; q < Q; q++) in[c.o_idx + q] = q == 0 ? 0u : q == 1 ? (1u << H) - 1u : rnd() & ((1u << H) - 1u);
    for (size_t i = c.o_sib[0]; i < c.o_desc; i++) in[i] = rnd();
    size_t used = 0;
    for (uint32_t q = 0; q < Q; q++)
        for (uint32_t tree = 0; tree < 2; tree++) {
            const size_t p = 2 * (size_t)q + tree;
            const uint32_t d[8] = {(uint32_t)p, 2u + tree, in[c.o_idx + q], tree ? 8u : W, (uint32_t)used, (uint32_t)(tree ? nt + 8 * (size_t)q : (size_t)W * q), (uint32_t)(8 * (size_t)H * p), 0u};
            std::memcpy(in.data() + c.o_desc + 8 * p, d, 32);
            std::memcpy(in.data() + o_wsib + 8 * (size_t)H * p, in.data() + c.o_sib[tree] + 8 * (size_t)H * q, 32 * (size_t)H);
            used += (tree ? 1 : c.blocks) + H;
        }
    CK(hipMalloc((void**)&c.d_in, c.in_words * 4));
    CK(hipMemcpy(c.d_in, in.data(), c.in_words * 4, hipMemcpyHostToDevice));
    CK(hipMalloc((void**)&c.d_wave, c.wave_words() * 4));
    for (int t = 0; t < 2; t++) { CK(hipMalloc((void**)&c.d_lane[t], c.lane_words(t) * 4)); CK(hipMalloc((void**)&c.d_ends[t], 16 * (size_t)Q * 4)); }
    return 0;
}
static void free_case(Case& c) { (void)hipFree(c.d_in); (void)hipFree(c.d_wave); for (int t = 0; t < 2; t++) { (void)hipFree(c.d_lane[t]); (void)hipFree(c.d_ends[t]); } }
static void launch(const Case& c, int form, hipStream_t s) {
    const size_t per_query = c.blocks + 1 + 2 * (size_t)c.H;
    if (form == 0) {
        p24chip::RowPathsArgs a{};
        a.desc = c.d_in + c.o_desc; a.rows = c.d_in; a.siblings = c.d_in + c.o_desc + 16 * (size_t)c.Q; a.n_paths = 2 * (uint64_t)c.Q; a.trace_rows = c.wave_rows;
        a.used_rows = (uint64_t)c.Q * per_query; a.depth = c.H; a.trace = c.d_wave; a.ld = p24chip::WIDTH_R; a.ends = c.d_ends[0];
        hipLaunchKernelGGL(row_paths_wave_kernel, dim3((unsigned)(a.n_paths + (a.trace_rows - a.used_rows + 15) / 16)), dim3(64), 0, s, a);
        return;
    }
    for (int tree = 0; tree < 2; tree++) {
        p24chip::MerkleTraceArgs a{};
        a.leaves = c.d_in + (tree ? c.o_qrows : c.o_trows); a.row_width = tree ? 8u : c.W; a.siblings = c.d_in + c.o_sib[tree]; a.indices = c.d_in + c.o_idx;
        a.n_paths = c.Q; a.rows = c.lane_rows[tree]; a.depth = c.H; a.trace = c.d_lane[tree]; a.ld = p24chip::WIDTH; a.roots = c.d_ends[1] + 8 * (size_t)c.Q * tree;
        const uint64_t lanes = a.n_paths + (a.rows - a.n_paths * (((uint64_t)a.row_width + 15) / 16 + a.depth));
        hipLaunchKernelGGL(row_paths_lane_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, a);
    }
}
// the first 540 columns but CNT (each form counts its own table's path ends) of every path's rows, and every path's end
static int compare(const Case& c) {
    std::vector<uint32_t> w(c.wave_words()), l[2], ew(16 * (size_t)c.Q), el(16 * (size_t)c.Q);
    CK(hipMemcpy(w.data(), c.d_wave, w.size() * 4, hipMemcpyDeviceToHost));
    for (int t = 0; t < 2; t++) { l[t].resize(c.lane_words(t)); CK(hipMemcpy(l[t].data(), c.d_lane[t], l[t].size() * 4, hipMemcpyDeviceToHost)); }
    CK(hipMemcpy(ew.data(), c.d_ends[0], ew.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(el.data(), c.d_ends[1], el.size() * 4, hipMemcpyDeviceToHost));
    size_t bad = 0, words = 0, wrow = 0;
    for (uint32_t q = 0; q < c.Q; q++)
        for (int tree = 0; tree < 2; tree++) {
            const size_t n = (tree ? 1 : c.blocks) + c.H;
            for (size_t r = 0; r < n; r++, wrow++)
                for (uint32_t col = 0; col < p24chip::WIDTH; col++) {
                    if (col == p24chip::CNT) continue;
                    words++;
                    if (w[wrow * p24chip::WIDTH_R + col] != l[tree][((size_t)q * n + r) * p24chip::WIDTH + col]) {
                        if (!bad) std::printf("  first difference: query %u tree %d row %zu column %u\n", q, tree, r, col);
                        bad++;
                    }
                }
            words += 8;
            if (std::memcmp(ew.data() + 8 * (2 * (size_t)q + tree), el.data() + 8 * ((size_t)c.Q * tree + q), 32) != 0) bad++;
        }
    std::printf("Q %u W %u H %u: %zu words, %zu differ%s\n", c.Q, c.W, c.H, words, bad, bad ? "" : " (the forms agree)");
    return bad ? 1 : 0;
}

int main() {
    const uint32_t shapes[][3] = {{1, 8, 5}, {3, 16, 9}, {33, 24, 9}, {5, 40, 9}, {3, 128, 12}, {2, 1016, 9}, {2, 1024, 27}, {50, 128, 22}};
    for (const auto& sh : shapes) {
        Case c;
        if (make_case(c, sh[0], sh[1], sh[2])) return 2;
        launch(c, 0, 0);
        CK(hipGetLastError());
        launch(c, 1, 0);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        const int rc = compare(c);
        free_case(c);
        if (rc) return rc;
    }
    Case c;
    if (make_case(c, 50, 128, 22)) return 2;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 10; i++) { launch(c, 0, 0); launch(c, 1, 0); }
    CK(hipDeviceSynchronize());
    double sum[2] = {0, 0};
    const int N = 25;
    for (int i = 0; i < N; i++)
        for (int f = 0; f < 2; f++) {
            CK(hipEventRecord(e0, 0));
            launch(c, f, 0);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            sum[f] += ms;
        }
    std::printf("Q 50 W 128 H 22 (100 paths, 2650 rows), means of %d launches, alternating: wave per path %.2f us, lane per path (two launches) %.2f us\n", N,
                1e3 * sum[0] / N, 1e3 * sum[1] / N);
    free_case(c);
    return 0;
}
