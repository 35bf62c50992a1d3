// tools/p2mx_bench.hip -- the width-16 Poseidon2 permutation with its full rounds' external layer on the int8 matrix cores
// (p2_permute_mx_dev) against the all-VALU device form (p2_permute_dev), stand-alone, at the same states and the same wave count.
//   ./tools/p2mx_bench [log_states] [chain]   log_states default 21 (states = lanes), chain = permutations per lane (default 32,
//                                              the 256-wide leaf row of the headline shard)
// Prints one JSON line: word-for-word mismatches of the two device forms (random states plus edge words, chains of 1 and 3, and the first
// 256 states against the host's portable form), each kernel's resources, and min / median milliseconds of alternating timed launches.
// The width-16 partial rounds run paired (elements 1..15 updated once per two rounds, p2_internal_pair_dev) or one at a time by a flag of
// the constant tables: the correctness pass also runs every form with the flag cleared ("pair_mismatches": against the paired all-VALU
// words), and the throughput pass times both settings of both permutations ("*_pr_ms_*": one round at a time).
//   ./tools/p2mx_bench states [--w24] <in.bin> <out.bin>
//       no timing: reads N states of 16 canonical u32 words (24 with --w24), permutes them with every device form and writes the raw device
//       words (Montgomery form) of each form, N states per block, in the order the JSON line names: p2_permute_dev, p2_permute_mx_dev at the
//       compiler's register budget, at 5 and at 6 waves, each with the paired partial rounds and with the flag cleared, then coop_permute
//       (poseidon2_coop.cuh, 16 lanes per state); with --w24 one block from p24_permute_dev.  tests/test_gpu_p2_steer.py feeds it states
//       steered to edge words inside the rounds.
//   ./tools/p2mx_bench sponge [log_rows] [width] [reps]
//       the leaf sponge of hash.hip's single-matrix kernel (overwrite mode, rate 8, 5 waves per SIMD) over log_rows rows (default 21) of
//       width words (default 256, a multiple of 4) in two forms: the closed permutation per block, and the sponge forms ABSORB / ABSORB_RATE /
//       SQUEEZE (p2_permute_mx_form), which leave out what the next block overwrites.  Digests compared word for word over all rows (and the
//       first 64 rows against the host's portable form), then reps (default 3) alternating timed launches of each.  One JSON line.
//   ./tools/p2mx_bench sponge-rows <width> <in.bin> <out.bin>
//       no timing: reads N rows of 8 + width canonical u32 words, the sponge's initial capacity words 8..15 and then the row, runs both sponge
//       kernels on them and writes the raw digest words (Montgomery form), N x 8 per form: closed, forms.  tests/test_gpu_p2_sponge.py feeds
//       it first blocks run backwards from capacity words that are edge digit words in the second block's first layer.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/p2mx_bench tools/p2mx_bench.hip   (__graft_entry__.build() does)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string.h>

#include <algorithm>
#include <vector>

#include "../zktls_amd/csrc/poseidon2.cuh"
#include "../zktls_amd/csrc/poseidon2_coop.cuh"

namespace zk { P2Tables g_p2_tables = P2_BUILTIN; }
using namespace zk;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("{\"error\": \"%s at line %d\"}\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

__device__ __forceinline__ void load_state(const uint32_t* st, uint64_t i, uint32_t s[16]) {
    const uint4* p = reinterpret_cast<const uint4*>(st + 16 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint4 v = p[k]; s[4 * k] = v.x; s[4 * k + 1] = v.y; s[4 * k + 2] = v.z; s[4 * k + 3] = v.w; }
}
__device__ __forceinline__ void store_state(uint32_t* st, uint64_t i, const uint32_t s[16]) {
    uint4* p = reinterpret_cast<uint4*>(st + 16 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = make_uint4(s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
}

__global__ void __launch_bounds__(256) perm_vec_kernel(uint32_t* st, uint64_t n, int chain) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[16];
    load_state(st, i, s);
    for (int c = 0; c < chain; c++) p2_permute_dev(s);
    store_state(st, i, s);
}
// wave-cooperative: every lane runs the permutation; lanes past n work on state n - 1 and store nothing.  WPE = the register budget in
// waves per SIMD (0: the compiler's own choice, 4 waves; 5 and 6 spill a few values outside the rounds' inner work)
template <int WPE>
__device__ __forceinline__ void perm_mx_body(uint32_t* st, uint64_t n, int chain) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s[16];
    load_state(st, i < n ? i : n - 1, s);
    for (int c = 0; c < chain; c++) p2_permute_mx_dev(s);
    if (i < n) store_state(st, i, s);
}
__global__ void __launch_bounds__(256) perm_mx_kernel(uint32_t* st, uint64_t n, int chain) { perm_mx_body<0>(st, n, chain); }
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) perm_mx5_kernel(uint32_t* st, uint64_t n, int chain) {
    perm_mx_body<5>(st, n, chain);
}
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) perm_mx6_kernel(uint32_t* st, uint64_t n, int chain) {
    perm_mx_body<6>(st, n, chain);
}

// one state over the 16 lanes of a DPP row, as the cooperative leaf and tree kernels of hash.hip run it; whole rows leave together
__global__ void __launch_bounds__(256) perm_coop_kernel(uint32_t* st, uint64_t n) {
    const uint64_t node = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int lane16 = threadIdx.x & 15;
    if (node >= n) return;
    const CoopConsts k = coop_load_consts(lane16);
    st[16 * node + lane16] = coop_permute(st[16 * node + lane16], lane16, k);
}
__global__ void __launch_bounds__(256) perm24_kernel(uint32_t* st, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[24];
#pragma unroll
    for (int k = 0; k < 24; k++) s[k] = st[24 * i + k];
    p24_permute_dev(s);
#pragma unroll
    for (int k = 0; k < 24; k++) st[24 * i + k] = s[k];
}

// the leaf sponge in both forms, as hash.hip's hash_rows_vec_body<true> and hash_rows_sponge_body; the row pitch is the width
__global__ void sponge_fill_kernel(uint32_t* m, uint64_t words) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        m[i] = (uint32_t)((z ^ (z >> 31)) % P);
    }
}
__device__ __forceinline__ void sponge_load(const uint4* rp, uint32_t q, bool both, uint32_t s[16]) {
    const uint4 v0 = rp[2 * q];
    s[0] = v0.x; s[1] = v0.y; s[2] = v0.z; s[3] = v0.w;
    if (both) { const uint4 v1 = rp[2 * q + 1]; s[4] = v1.x; s[5] = v1.y; s[6] = v1.z; s[7] = v1.w; }
}
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) sponge_closed_kernel(const uint32_t* __restrict__ mat, uint32_t width, uint64_t height, uint32_t* __restrict__ digests, const uint32_t* __restrict__ cap) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row - __lane_id() >= height) return;
    const uint64_t rr = row < height ? row : height - 1;
    const uint4* rp = reinterpret_cast<const uint4*>(mat + rr * width);
    uint32_t s[16];
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = 0u;
    if (cap) {
#pragma unroll
        for (int i = 0; i < 8; i++) s[8 + i] = cap[8 * rr + i];
    }
    for (uint32_t q = 0; q < width / 8; q++) { sponge_load(rp, q, true, s); p2_permute_mx_dev(s); }
    if (width & 4u) { sponge_load(rp, width / 8, false, s); p2_permute_mx_dev(s); }
    if (row >= height) return;
    uint4* d = reinterpret_cast<uint4*>(digests + row * 8);
    d[0] = make_uint4(s[0], s[1], s[2], s[3]);
    d[1] = make_uint4(s[4], s[5], s[6], s[7]);
}
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) sponge_forms_kernel(const uint32_t* __restrict__ mat, uint32_t width, uint64_t height, uint32_t* __restrict__ digests, const uint32_t* __restrict__ cap) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row - __lane_id() >= height) return;
    const uint64_t rr = row < height ? row : height - 1;
    const uint4* rp = reinterpret_cast<const uint4*>(mat + rr * width);
    uint32_t s[16];
#pragma unroll
    for (int i = 0; i < 8; i++) { s[i] = 0u; s[8 + i] = (uint32_t)P2T.mx16.cap0[i]; }
    if (cap) {                                                                    // a given canonical capacity in the forms' signed form: centred(c + M_E^-1 ext_rc[0])
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t t = dadd(cap[8 * rr + i], P2T.mx16.in0[i >> 2][4 + (i & 3)] - MX_BIAS);
            s[8 + i] = t > P / 2 ? t - P : t;
        }
    }
    const uint32_t nb = width / 8, half = width & 4u;
    uint32_t q = 0;
    for (; q + 1 < nb; q++) { sponge_load(rp, q, true, s); p2_permute_mx_form<P2MxForm::ABSORB>(s); }
    if (half && nb) { sponge_load(rp, q, true, s); p2_permute_mx_form<P2MxForm::ABSORB_RATE>(s); q++; }
    if (width) { sponge_load(rp, q, !half, s); p2_permute_mx_form<P2MxForm::SQUEEZE>(s); }
    if (row >= height) return;
    uint4* d = reinterpret_cast<uint4*>(digests + row * 8);
    d[0] = make_uint4(s[0], s[1], s[2], s[3]);
    d[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

static uint64_t splitmix(uint64_t& x) {
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// random canonical words; the first states are edge words: all 0, all P - 1, all 1, all R mod P, 0 / P - 1 alternating both ways,
// P - 1 in one position, and P / 2, P / 2 + 1 patterns
static void fill_states(std::vector<uint32_t>& h, uint64_t n, uint64_t seed) {
    for (uint64_t k = 0; k < 16 * n; k++) h[k] = (uint32_t)(splitmix(seed) % P);
    const uint32_t edge[8] = {0u, P - 1, 1u, MONTY_R1, P / 2, P / 2 + 1, P - 2, 2u};
    uint64_t e = 0;
    for (int a = 0; a < 8 && e < n; a++, e++) for (int k = 0; k < 16; k++) h[16 * e + k] = edge[a];
    for (int a = 0; a < 8 && e < n; a++, e++) for (int k = 0; k < 16; k++) h[16 * e + k] = ((k ^ a) & 1) ? edge[a] : edge[(a + 1) & 7];
    for (int k = 0; k < 16 && e < n; k++, e++) for (int j = 0; j < 16; j++) h[16 * e + j] = j == k ? P - 1 : 0u;
}

static void launch(int form, uint32_t* d, uint64_t n, int chain) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (form == 3) perm_mx6_kernel<<<blocks, 256>>>(d, n, chain);
    else if (form == 2) perm_mx5_kernel<<<blocks, 256>>>(d, n, chain);
    else if (form == 1) perm_mx_kernel<<<blocks, 256>>>(d, n, chain);
    else perm_vec_kernel<<<blocks, 256>>>(d, n, chain);
    CK(hipGetLastError());
}

// the "states" mode: every device form on the states of a file
static int run_states(int argc, char** argv) {
    bool w24 = false;
    const char* path[2] = {nullptr, nullptr};
    int np = 0;
    for (int a = 2; a < argc; a++) {
        if (!strcmp(argv[a], "--w24")) w24 = true;
        else if (np < 2) path[np++] = argv[a];
        else np = 3;
    }
    if (np != 2) { printf("{\"error\": \"usage: states [--w24] <in.bin> <out.bin>\"}\n"); return 2; }
    const size_t W = w24 ? 24 : 16;
    FILE* f = fopen(path[0], "rb");
    if (!f) { printf("{\"error\": \"cannot open the input file\"}\n"); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (long)(4 * W) || (size_t)bytes / (4 * W) > (1u << 20)) { fclose(f); printf("{\"error\": \"bad input size\"}\n"); return 2; }
    const uint64_t n = (uint64_t)bytes / (4 * W);
    std::vector<uint32_t> h(W * n), out(W * n);
    const size_t got = fread(h.data(), 4, W * n, f);
    fclose(f);
    if (got != W * n) { printf("{\"error\": \"short read\"}\n"); return 2; }
    for (auto& x : h) {
        if (x >= P) { printf("{\"error\": \"input word not canonical\"}\n"); return 2; }
        x = to_monty(x);
    }
    FILE* o = fopen(path[1], "wb");
    if (!o) { printf("{\"error\": \"cannot open the output file\"}\n"); return 2; }
    uint32_t* d;
    CK(hipMalloc(&d, W * n * 4));
    const auto run = [&](int form) {                                             // 0..3 as launch(); 4 coop_permute; 5 width 24
        CK(hipMemcpy(d, h.data(), W * n * 4, hipMemcpyHostToDevice));
        if (form == 5) perm24_kernel<<<(unsigned)((n + 255) / 256), 256>>>(d, n);
        else if (form == 4) perm_coop_kernel<<<(unsigned)((16 * n + 255) / 256), 256>>>(d, n);
        else launch(form, d, n, 1);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(out.data(), d, W * n * 4, hipMemcpyDeviceToHost));
        if (fwrite(out.data(), 4, W * n, o) != W * n) { printf("{\"error\": \"short write\"}\n"); exit(1); }
    };
    if (w24) {
        run(5);
        printf("{\"states\": %llu, \"width\": 24, \"blocks\": [\"p24\"]}\n", (unsigned long long)n);
    } else {
        P2Tables per_round = P2_BUILTIN;
        per_round.pk16.pair = 0;
        for (int pair : {1, 0}) {
            CK(p2_upload_tables(pair ? g_p2_tables : per_round, 0));
            CK(hipDeviceSynchronize());
            for (int form = 0; form < 4; form++) run(form);
        }
        CK(p2_upload_tables(g_p2_tables, 0));
        CK(hipDeviceSynchronize());
        run(4);
        printf("{\"states\": %llu, \"width\": 16, \"blocks\": [\"vec_pair\", \"mx_pair\", \"mx5_pair\", \"mx6_pair\", "
               "\"vec_one\", \"mx_one\", \"mx5_one\", \"mx6_one\", \"coop\"]}\n", (unsigned long long)n);
    }
    fclose(o);
    CK(hipFree(d));
    return 0;
}

// the "sponge-rows" mode: both sponge kernels on the rows of a file, each row with its own initial capacity
static int run_sponge_rows(int argc, char** argv) {
    const int width = argc == 5 ? atoi(argv[2]) : 0;
    if (width < 4 || width > 1024 || width % 4) { printf("{\"error\": \"usage: sponge-rows <width> <in.bin> <out.bin>\"}\n"); return 2; }
    const size_t W = 8 + (size_t)width;
    FILE* f = fopen(argv[3], "rb");
    if (!f) { printf("{\"error\": \"cannot open the input file\"}\n"); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (long)(4 * W) || (size_t)bytes / (4 * W) > (1u << 20)) { fclose(f); printf("{\"error\": \"bad input size\"}\n"); return 2; }
    const uint64_t n = (uint64_t)bytes / (4 * W);
    std::vector<uint32_t> h(W * n), hc(8 * n), hm((size_t)width * n), out(8 * n);
    const size_t got = fread(h.data(), 4, W * n, f);
    fclose(f);
    if (got != W * n) { printf("{\"error\": \"short read\"}\n"); return 2; }
    for (uint64_t i = 0; i < n; i++)
        for (size_t k = 0; k < W; k++) {
            const uint32_t x = h[W * i + k];
            if (x >= P) { printf("{\"error\": \"input word not canonical\"}\n"); return 2; }
            (k < 8 ? hc[8 * i + k] : hm[(size_t)width * i + (k - 8)]) = to_monty(x);
        }
    FILE* o = fopen(argv[4], "wb");
    if (!o) { printf("{\"error\": \"cannot open the output file\"}\n"); return 2; }
    uint32_t *m, *c, *d;
    CK(hipMalloc(&m, hm.size() * 4));
    CK(hipMalloc(&c, hc.size() * 4));
    CK(hipMalloc(&d, out.size() * 4));
    CK(hipMemcpy(m, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(c, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((n + 255) / 256);
    for (int form = 0; form < 2; form++) {
        CK(hipMemset(d, 0xFF, out.size() * 4));
        if (form) sponge_forms_kernel<<<blocks, 256>>>(m, (uint32_t)width, n, d, c);
        else sponge_closed_kernel<<<blocks, 256>>>(m, (uint32_t)width, n, d, c);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(out.data(), d, out.size() * 4, hipMemcpyDeviceToHost));
        if (fwrite(out.data(), 4, out.size(), o) != out.size()) { printf("{\"error\": \"short write\"}\n"); return 1; }
    }
    fclose(o);
    printf("{\"rows\": %llu, \"width\": %d, \"blocks\": [\"closed\", \"forms\"]}\n", (unsigned long long)n, width);
    CK(hipFree(m));
    CK(hipFree(c));
    CK(hipFree(d));
    return 0;
}

// the "sponge" mode: the leaf sponge with the closed permutation per block against the sponge forms
static int run_sponge(int argc, char** argv) {
    const int log_n = argc > 2 ? atoi(argv[2]) : 21;
    const int width = argc > 3 ? atoi(argv[3]) : 256;
    const int reps = argc > 4 ? atoi(argv[4]) : 3;
    if (log_n < 0 || log_n > 22 || width < 4 || width > 1024 || width % 4 || reps < 1 || reps > 64) { printf("{\"error\": \"bad arguments\"}\n"); return 2; }
    const uint64_t n = 1ull << log_n, words = n * (uint64_t)width;
    uint32_t *m, *da, *db;
    CK(hipMalloc(&m, words * 4));
    CK(hipMalloc(&da, n * 8 * 4));
    CK(hipMalloc(&db, n * 8 * 4));
    sponge_fill_kernel<<<4096, 256>>>(m, words);
    CK(hipGetLastError());
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const auto run = [&](int form) {
        if (form) sponge_forms_kernel<<<blocks, 256>>>(m, (uint32_t)width, n, db, nullptr);
        else sponge_closed_kernel<<<blocks, 256>>>(m, (uint32_t)width, n, da, nullptr);
        CK(hipGetLastError());
    };
    CK(hipMemset(da, 0xFF, n * 8 * 4));
    CK(hipMemset(db, 0xEE, n * 8 * 4));
    run(0); run(1);                                                               // (the warm-up launches too)
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> ha(8 * n), hb(8 * n);
    CK(hipMemcpy(ha.data(), da, n * 8 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), db, n * 8 * 4, hipMemcpyDeviceToHost));
    uint64_t mism = 0, host_mism = 0;
    for (uint64_t k = 0; k < 8 * n; k++) mism += ha[k] != hb[k];
    const uint64_t nhost = std::min<uint64_t>(n, 64);
    std::vector<uint32_t> hm(nhost * width);
    CK(hipMemcpy(hm.data(), m, nhost * width * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < nhost; i++) {
        uint32_t s[16] = {};
        for (int q = 0; q < width; q += 8) {
            for (int k = 0; k < 8 && q + k < width; k++) s[k] = hm[i * width + q + k];
            p2_permute_scalar(s);
        }
        for (int k = 0; k < 8; k++) host_mism += s[k] != hb[8 * i + k];
    }
    hipFuncAttributes fa, fb;
    CK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(sponge_closed_kernel)));
    CK(hipFuncGetAttributes(&fb, reinterpret_cast<const void*>(sponge_forms_kernel)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float> t[2];
    for (int r = 0; r < 2 * reps; r++) {
        CK(hipEventRecord(e0));
        run(r & 1);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        t[r & 1].push_back(ms);
    }
    printf("{\"mode\": \"sponge\", \"rows\": %llu, \"width\": %d, \"mismatches\": %llu, \"checked_words\": %llu, \"host_mismatches\": %llu, "
           "\"closed_regs\": %d, \"closed_scratch\": %d, \"forms_regs\": %d, \"forms_scratch\": %d, \"closed_ms\": [",
           (unsigned long long)n, width, (unsigned long long)mism, (unsigned long long)(8 * n), (unsigned long long)host_mism,
           fa.numRegs, (int)fa.localSizeBytes, fb.numRegs, (int)fb.localSizeBytes);
    for (int r = 0; r < reps; r++) printf("%s%.4f", r ? ", " : "", t[0][r]);
    printf("], \"forms_ms\": [");
    for (int r = 0; r < reps; r++) printf("%s%.4f", r ? ", " : "", t[1][r]);
    for (auto& v : t) std::sort(v.begin(), v.end());
    printf("], \"closed_ms_med\": %.4f, \"forms_ms_med\": %.4f, \"forms_over_closed_med\": %.4f}\n", t[0][reps / 2], t[1][reps / 2], t[1][reps / 2] / t[0][reps / 2]);
    CK(hipFree(m));
    CK(hipFree(da));
    CK(hipFree(db));
    return mism || host_mism ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "states")) return run_states(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "sponge")) return run_sponge(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "sponge-rows")) return run_sponge_rows(argc, argv);
    const int log_n = argc > 1 ? atoi(argv[1]) : 21;
    const int chain = argc > 2 ? atoi(argv[2]) : 32;
    if (log_n < 6 || log_n > 24 || chain < 1 || chain > 256) { printf("{\"error\": \"bad arguments\"}\n"); return 2; }
    const uint64_t n = 1ull << log_n;
    std::vector<uint32_t> h0(16 * n), ha(16 * n), hb(16 * n);
    fill_states(h0, n, 0x5A4B544C53ull);
    uint32_t *d0, *d1;
    CK(hipMalloc(&d0, 16 * n * 4));
    CK(hipMalloc(&d1, 16 * n * 4));

    // correctness: both device forms, chains of 1 and 3, word for word; the first 256 states of chain 1 against the host form.
    // A state count that is not a multiple of 64 exercises the partial last wave.
    uint64_t mism = 0, host_mism = 0;
    const uint64_t nchk = std::min<uint64_t>(n, 1u << 16) - 5;
    for (int c : {1, 3})
    for (int form : {1, 2, 3}) {
        CK(hipMemcpy(d0, h0.data(), 16 * nchk * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d1, h0.data(), 16 * nchk * 4, hipMemcpyHostToDevice));
        launch(0, d0, nchk, c);
        launch(form, d1, nchk, c);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(ha.data(), d0, 16 * nchk * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hb.data(), d1, 16 * nchk * 4, hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < 16 * nchk; k++) mism += ha[k] != hb[k];
        if (c == 1 && form == 1)
            for (uint64_t i = 0; i < 256; i++) {
                uint32_t s[16];
                for (int k = 0; k < 16; k++) s[k] = h0[16 * i + k];
                p2_permute_scalar(s);
                for (int k = 0; k < 16; k++) host_mism += s[k] != hb[16 * i + k];
            }
    }

    // the partial rounds one at a time (the flag cleared in this program's constant tables) against the paired words, every form
    uint64_t pair_mism = 0;
    P2Tables per_round = P2_BUILTIN;
    per_round.pk16.pair = 0;
    for (int c : {1, 3})
    for (int form : {0, 1, 2, 3}) {
        CK(hipMemcpy(d0, h0.data(), 16 * nchk * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d1, h0.data(), 16 * nchk * 4, hipMemcpyHostToDevice));
        CK(p2_upload_tables(g_p2_tables, 0));
        launch(0, d0, nchk, c);
        CK(hipDeviceSynchronize());
        CK(p2_upload_tables(per_round, 0));
        launch(form, d1, nchk, c);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(ha.data(), d0, 16 * nchk * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hb.data(), d1, 16 * nchk * 4, hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < 16 * nchk; k++) pair_mism += ha[k] != hb[k];
    }
    CK(p2_upload_tables(g_p2_tables, 0));
    CK(hipDeviceSynchronize());

    hipFuncAttributes fa, fb, fc, fd;
    CK(hipFuncGetAttributes(&fd, reinterpret_cast<const void*>(perm_mx6_kernel)));
    CK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(perm_vec_kernel)));
    CK(hipFuncGetAttributes(&fb, reinterpret_cast<const void*>(perm_mx_kernel)));
    CK(hipFuncGetAttributes(&fc, reinterpret_cast<const void*>(perm_mx5_kernel)));

    // throughput: alternating launches on the same buffer contents, after one warm-up launch of each
    CK(hipMemcpy(d0, h0.data(), 16 * n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d1, h0.data(), 16 * n * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int form = 0; form < 4; form++) launch(form, form ? d1 : d0, n, chain);
    CK(hipDeviceSynchronize());
    const int reps = 7;
    std::vector<float> t[4];
    for (int r = 0; r < 4 * reps; r++) {
        const int form = r % 4;
        CK(hipEventRecord(e0));
        launch(form, form ? d1 : d0, n, chain);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        t[form].push_back(ms);
    }
    for (auto& v : t) std::sort(v.begin(), v.end());
    // paired against one round at a time: the all-VALU form and the 5-wave matrix-core form (the leaf kernel's), settings alternating
    std::vector<float> tp[4];                                                     // vec paired, vec per-round, mx5 paired, mx5 per-round
    for (int r = 0; r < 4 * reps; r++) {
        const int k = r % 4, form = k < 2 ? 0 : 2;
        CK(p2_upload_tables(k & 1 ? per_round : g_p2_tables, 0));
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0));
        launch(form, form ? d1 : d0, n, chain);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        tp[k].push_back(ms);
    }
    CK(p2_upload_tables(g_p2_tables, 0));
    CK(hipDeviceSynchronize());
    for (auto& v : tp) std::sort(v.begin(), v.end());
    printf("{\"states\": %llu, \"chain\": %d, \"mismatches\": %llu, \"checked_words\": %llu, \"host_mismatches\": %llu, "
           "\"vec_regs\": %d, \"mx_regs\": %d, \"mx5_regs\": %d, \"vec_scratch\": %d, \"mx_scratch\": %d, \"mx5_scratch\": %d, "
           "\"vec_ms_min\": %.4f, \"vec_ms_med\": %.4f, \"mx_ms_min\": %.4f, \"mx_ms_med\": %.4f, \"mx5_ms_min\": %.4f, \"mx5_ms_med\": %.4f, "
           "\"mx6_ms_min\": %.4f, \"mx6_ms_med\": %.4f, \"mx6_regs\": %d, \"mx6_scratch\": %d, "
           "\"mx_over_vec_med\": %.4f, \"mx5_over_vec_med\": %.4f, \"mx6_over_vec_med\": %.4f, "
           "\"pair_mismatches\": %llu, \"vec_pair_ms_min\": %.4f, \"vec_pair_ms_med\": %.4f, \"vec_pr_ms_min\": %.4f, \"vec_pr_ms_med\": %.4f, "
           "\"mx5_pair_ms_min\": %.4f, \"mx5_pair_ms_med\": %.4f, \"mx5_pr_ms_min\": %.4f, \"mx5_pr_ms_med\": %.4f, "
           "\"vec_pair_over_pr_med\": %.4f, \"mx5_pair_over_pr_med\": %.4f}\n",
           (unsigned long long)n, chain, (unsigned long long)mism, (unsigned long long)(4 * 16 * nchk), (unsigned long long)host_mism,
           fa.numRegs, fb.numRegs, fc.numRegs, (int)fa.localSizeBytes, (int)fb.localSizeBytes, (int)fc.localSizeBytes,
           t[0][0], t[0][reps / 2], t[1][0], t[1][reps / 2], t[2][0], t[2][reps / 2], t[3][0], t[3][reps / 2],
           fd.numRegs, (int)fd.localSizeBytes, t[1][reps / 2] / t[0][reps / 2], t[2][reps / 2] / t[0][reps / 2], t[3][reps / 2] / t[0][reps / 2],
           (unsigned long long)pair_mism, tp[0][0], tp[0][reps / 2], tp[1][0], tp[1][reps / 2], tp[2][0], tp[2][reps / 2], tp[3][0], tp[3][reps / 2],
           tp[0][reps / 2] / tp[1][reps / 2], tp[2][reps / 2] / tp[3][reps / 2]);
    CK(hipFree(d0));
    CK(hipFree(d1));
    return mism || host_mism || pair_mism ? 1 : 0;
}
