// fri16_identity_forms.hip -- the two forms of the kernel that fills AIR16 and SCALARS16 (the fold-16 identity machine, zktls_amd/csrc/fri16_rows.cuh), stand-alone:
// the PLAIN form (one lane walks all groups, the others zero the padding rows) and the SCAN form (a lane per group, an inclusive cross-lane scan of the affine
// recurrence ACCO_g = alpha^3 ACCO_(g-1) + t_g with the power squared per step, the waves' last values through LDS; the library's).  Both bodies are the header's
// text; SCALARS16's row is the same code in both.  First both forms on the same random inputs at the widths of tests/test_gpu_fri16_identity.py -- inside, filling
// and straddling a wave of 64 groups, two waves, and the full workgroup of 256 -- outputs (both tables and the two accumulators) compared word for word; then both
// timed at W = 128 and W = 1024: one process, after a warm-up, alternating, HIP events around each launch, means of 25 launches each.  (1 / g_N and the zps constants
// are random words here: the forms are compared, not the identity.)
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I zktls_amd/csrc -o tools/fri16_identity_forms tools/fri16_identity_forms.hip && tools/fri16_identity_forms
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fri16_rows.cuh"

using namespace zk;
using namespace zk::fri16;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

__global__ void __launch_bounds__(IDENTITY_LANES) identity_rows_plain_kernel(IdentityRowsArgs a) { fri16_identity_rows_plain_body(a); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % P); }
static size_t lg_rows(size_t n, int lo) { int l = lo; while (((size_t)1 << l) < n) l++; return (size_t)1 << l; }

struct Case {
    uint32_t W, n, consts[5];
    size_t rows, in_words;
    uint32_t *d_in = nullptr, *d_out[2] = {nullptr, nullptr};          // inputs (opened values, alpha, zeta); per form: AIR16 | SCALARS16 | the two accumulators
    size_t air_words() const { return rows * AIR_MAIN16; }
    size_t sc_words() const { return (size_t)sc16_width(n) << SC16_LOG_ROWS; }
    size_t out_words() const { return air_words() + sc_words() + 8; }
    IdentityRowsArgs args(int form) const {
        IdentityRowsArgs a{};
        a.opened = d_in; a.alpha = d_in + 8 * ((size_t)W + 4); a.zeta = a.alpha + 4; a.W = W; a.n = n;
        a.gn_inv = consts[0]; a.za[0] = consts[1]; a.za[1] = consts[2]; a.zb[0] = consts[3]; a.zb[1] = consts[4];
        a.air_rows = rows; a.air = d_out[form]; a.scalars = d_out[form] + air_words(); a.accs = a.scalars + sc_words();
        return a;
    }
};
static int make_case(Case& c, uint32_t W, uint32_t n) {
    c.W = W; c.n = n;
    c.rows = lg_rows((size_t)W / 4, 6);
    c.in_words = 8 * ((size_t)W + 4) + 8;
    std::vector<uint32_t> in(c.in_words);
    for (auto& w : in) w = rnd();
    for (auto& w : c.consts) w = rnd();
    CK(hipMalloc((void**)&c.d_in, c.in_words * 4));
    CK(hipMemcpy(c.d_in, in.data(), c.in_words * 4, hipMemcpyHostToDevice));
    for (int f = 0; f < 2; f++) { CK(hipMalloc((void**)&c.d_out[f], c.out_words() * 4)); CK(hipMemset(c.d_out[f], 0xFF, c.out_words() * 4)); }
    return 0;
}
static void free_case(Case& c) { (void)hipFree(c.d_in); (void)hipFree(c.d_out[0]); (void)hipFree(c.d_out[1]); }
static void launch(const Case& c, int form, hipStream_t s) {
    if (form == 0) hipLaunchKernelGGL(identity_rows_plain_kernel, dim3(1), dim3(IDENTITY_LANES), 0, s, c.args(0));
    else hipLaunchKernelGGL(fri16_identity_rows_kernel, dim3(1), dim3(IDENTITY_LANES), 0, s, c.args(1));
}

int main() {
    const uint32_t widths[][2] = {{8, 8}, {16, 8}, {248, 8}, {256, 8}, {264, 8}, {504, 8}, {512, 8}, {520, 8}, {1016, 8}, {1024, 8}, {8, 26}, {1024, 20}};
    for (const auto& wn : widths) {
        Case c;
        if (make_case(c, wn[0], wn[1])) return 2;
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
        std::printf("W %u, n %u (%u groups of %zu rows): %zu words, %zu differ%s\n", wn[0], wn[1], wn[0] / 4, c.rows, a.size(), bad, bad ? "" : " (the forms agree)");
        if (bad) { std::printf("  first difference at word %zu: plain %u scan %u\n", first, a[first], b[first]); return 1; }
        free_case(c);
    }
    const uint32_t timed[] = {128, 1024};
    for (uint32_t W : timed) {
        Case c;
        if (make_case(c, W, 20)) return 2;
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
        std::printf("W %u, n 20, means of %d launches, alternating: plain form %.2f us, scan form %.2f us\n", W, N, 1e3 * sum[0] / N, 1e3 * sum[1] / N);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        free_case(c);
    }
    return 0;
}
