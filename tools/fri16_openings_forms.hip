// fri16_openings_forms.hip -- the two forms of the kernel that fills ROWSUM16 and QUERY16 (the fold-16 openings machine, zktls_amd/csrc/fri16_rows.cuh), stand-alone:
// the PLAIN form (a lane per query walks its blocks, as sv_rowsum_query_kernel does for the shard verifier; kept here, not in the library) and the SCAN form (a lane
// per row, segmented cross-lane scan; the library's).  First both forms on the same random inputs at shapes on both sides of every packing threshold, outputs
// compared word for word; then both timed at the full-size shape (Q = 50, W = 128, H = 22): one process, after a warm-up, alternating, HIP events around each
// launch, means of 25 launches each.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I zktls_amd/csrc -o tools/fri16_openings_forms tools/fri16_openings_forms.hip && tools/fri16_openings_forms
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fri16_rows.cuh"

using namespace zk;
using namespace zk::fri16;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

// THE PLAIN FORM: a lane per query walks its blocks from the last to the first, then its quotient block, and computes its QUERY16 row; lanes past the queries
// share the padding rows
__global__ void __launch_bounds__(64) openings_rows_plain_kernel(OpeningsRowsArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t WB = a.W >> 3, per = WB + 1u;
    if (g >= a.Q) { openings_padding_rows(a, g - a.Q, lanes - a.Q); return; }
    const uint32_t q = (uint32_t)g;
    const Ext fa = ld_ext(a.consts);
    Ext acc = ext_zero(), at = ext_zero();
#pragma unroll 1
    for (uint32_t pos = 0; pos < per; pos++) {
        const bool quot = pos == WB;
        if (quot) { at = acc; acc = ext_zero(); }
        const uint32_t* src = quot ? a.qrows + 8u * (size_t)q : a.trows + (size_t)q * a.W + 8u * (WB - 1u - pos);
        const uint4 lo = *reinterpret_cast<const uint4*>(src), hi = *reinterpret_cast<const uint4*>(src + 4);
        const uint32_t v[8] = {dmul(lo.x, MONTY_R2), dmul(lo.y, MONTY_R2), dmul(lo.z, MONTY_R2), dmul(lo.w, MONTY_R2),
                               dmul(hi.x, MONTY_R2), dmul(hi.y, MONTY_R2), dmul(hi.z, MONTY_R2), dmul(hi.w, MONTY_R2)};
        uint32_t* t = a.rowsum + ((uint64_t)q * per + pos) * RS_MAIN16;
        st4(t + RS_V, v[0], v[1], v[2], v[3]); st4(t + RS_V + 4, v[4], v[5], v[6], v[7]);
        st_ext(t + RS_ACCIN, acc);
#pragma unroll
        for (int s = 7; s >= 0; s--) { acc = ext_mul_dev(acc, fa); acc.c[0] = dadd(acc.c[0], v[s]); st_ext(t + RS_T + 4 * s, acc); }
        st_ext(t + RS_FA, fa);
    }
    query16_row(a, q, at, acc);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % P); }
static size_t lg_rows(size_t n, int lo) { int l = lo; while (((size_t)1 << l) < n) l++; return (size_t)1 << l; }

struct Case {
    uint32_t Q, W, H;
    size_t rs_rows, q_rows, in_words;
    uint32_t *d_in = nullptr, *d_out[2] = {nullptr, nullptr};          // inputs; per form: rowsum | query | openings | status
    size_t out_words() const { return rs_rows * RS_MAIN16 + q_rows * Q16_MAIN + 4 * (size_t)Q + 4; }
    OpeningsRowsArgs args(int form) const {
        const size_t nt = (size_t)Q * W, nq = 8 * (size_t)Q;
        OpeningsRowsArgs a{};
        a.trows = d_in; a.qrows = d_in + nt; a.consts = d_in + nt + nq; a.indices = d_in + nt + nq + 32; a.view_values = nullptr;
        a.Q = Q; a.W = W; a.H = H; a.rowsum_rows = rs_rows; a.query_rows = q_rows;
        a.rowsum = d_out[form]; a.query = a.rowsum + rs_rows * RS_MAIN16; a.openings = a.query + q_rows * Q16_MAIN; a.status = a.openings + 4 * (size_t)Q;
        return a;
    }
};
static int make_case(Case& c, uint32_t Q, uint32_t W, uint32_t H) {
    c.Q = Q; c.W = W; c.H = H;
    c.rs_rows = lg_rows((size_t)Q * (W / 8 + 1), 6); c.q_rows = lg_rows(Q, 5);
    const size_t nt = (size_t)Q * W, nq = 8 * (size_t)Q;
    c.in_words = nt + nq + 32 + ((Q + 3) & ~3u);
    std::vector<uint32_t> in(c.in_words, 0u);
    for (size_t i = 0; i < nt + nq + 32; i++) in[i] = rnd();
    for (uint32_t q = 0; q < Q; q++) in[nt + nq + 32 + q] = rnd() & ((1u << H) - 1u);
    CK(hipMalloc((void**)&c.d_in, c.in_words * 4));
    CK(hipMemcpy(c.d_in, in.data(), c.in_words * 4, hipMemcpyHostToDevice));
    for (int f = 0; f < 2; f++) { CK(hipMalloc((void**)&c.d_out[f], c.out_words() * 4)); CK(hipMemset(c.d_out[f], 0xFF, c.out_words() * 4)); }
    return 0;
}
static void free_case(Case& c) { (void)hipFree(c.d_in); (void)hipFree(c.d_out[0]); (void)hipFree(c.d_out[1]); }
static void launch(const Case& c, int form, hipStream_t s) {
    const OpeningsRowsArgs a = c.args(form);
    const uint32_t per = c.W / 8 + 1;
    if (form == 0) {
        const size_t pad = (c.rs_rows - (size_t)c.Q * per) + (c.q_rows - c.Q), extra = pad < 4096 ? (pad ? pad : 1) : 4096;
        hipLaunchKernelGGL(openings_rows_plain_kernel, dim3((unsigned)((c.Q + extra + 63) / 64)), dim3(64), 0, s, a);
    } else if (per <= 64) {
        const uint32_t qpw = 64 / per;
        hipLaunchKernelGGL(fri16_openings_rows_kernel, dim3((c.Q + qpw - 1) / qpw), dim3(64), 0, s, a);
    } else
        hipLaunchKernelGGL(fri16_openings_rows_tall_kernel, dim3(c.Q), dim3(64), 0, s, a);
}

int main() {
    const uint32_t shapes[][3] = {{1, 8, 9}, {33, 8, 9}, {3, 24, 9}, {65, 128, 12}, {5, 496, 9}, {4, 504, 9}, {3, 512, 9}, {2, 520, 9}, {2, 1024, 27}, {50, 128, 22}};
    for (const auto& sh : shapes) {
        Case c;
        if (make_case(c, sh[0], sh[1], sh[2])) return 2;
        launch(c, 0, 0);
        CK(hipGetLastError());
        launch(c, 1, 0);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        std::vector<uint32_t> a(c.out_words()), b(c.out_words());
        CK(hipMemcpy(a.data(), c.d_out[0], a.size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(b.data(), c.d_out[1], b.size() * 4, hipMemcpyDeviceToHost));
        size_t bad = 0, first = 0;
        for (size_t i = 0; i < a.size(); i++) if (a[i] != b[i]) { if (!bad) first = i; bad++; }
        std::printf("Q %u W %u H %u: %zu words, %zu differ%s\n", sh[0], sh[1], sh[2], a.size(), bad, bad ? "" : " (the forms agree)");
        if (bad) { std::printf("  first difference at word %zu: plain %u scan %u\n", first, a[first], b[first]); return 1; }
        free_case(c);
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
    std::printf("Q 50 W 128 H 22, means of %d launches, alternating: plain form %.2f us, scan form %.2f us\n", N, 1e3 * sum[0] / N, 1e3 * sum[1] / N);
    free_case(c);
    return 0;
}
