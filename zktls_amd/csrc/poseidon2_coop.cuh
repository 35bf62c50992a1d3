// poseidon2_coop.cuh -- the width-16 Poseidon2 permutation spread over the 16 lanes of a DPP row (device only).  The cooperative leaf,
// tree and challenger kernels of hash.hip run it; tools/p2mx_bench includes it to run the same code on chosen states.
#pragma once
#include "poseidon2.cuh"

#if defined(__HIPCC__)
namespace zk {

// ------------------------------------------------------------------ latency-optimised form
// One permutation spread over the 16 lanes of a DPP row (state word i in lane i): an
// external round is 4 dependent products + ~13 dependent additions, an internal round one
// S-box + a 4-step rotate-and-add + one product, instead of ~10 k serial instructions.  A
// permutation finishes in ~3 us instead of ~19 us, which is what bounds the SMALL levels of
// every Merkle tree (a proof walks ~250 such levels one after the other).  Throughput per
// wave is worse (4 permutations instead of 64), so the wide levels keep the lane-per-state form.
template <int CTRL>
ZK_D uint32_t dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false); }

struct CoopConsts { uint32_t rc_ext[8]; uint32_t diag; };
ZK_D CoopConsts coop_load_consts(int lane16) {
    CoopConsts k;
#pragma unroll
    for (int r = 0; r < 8; r++) k.rc_ext[r] = P2K.ext_rcm[r][lane16];      // rc - P, see p2_sbox_rc_dev
    k.diag = P2K.diag[lane16];
    return k;
}
ZK_D uint32_t coop_external_linear(uint32_t x) {
    // M4 = circ(2,3,1,1) inside each quad: y_i = 2 x_i + 3 x_{i+1} + x_{i+2} + x_{i+3} = (quad sum) + x_i + 2 x_{i+1};
    // quad_perm [1,2,3,0] [2,3,0,1] [3,0,1,2] are the three rotations
    const uint32_t r1 = dpp<0x39>(x), r2 = dpp<0x4E>(x), r3 = dpp<0x93>(x);
    const uint32_t sum = dadd(dadd(x, r1), dadd(r2, r3));
    const uint32_t y = dadd(dadd(sum, x), ddbl(r1));
    uint32_t t = dadd(y, dpp<0x124>(y));                                  // row_ror:4
    t = dadd(t, dpp<0x128>(t));                                           // row_ror:8
    return dadd(y, t);
}
ZK_D uint32_t coop_permute(uint32_t x, int lane16, const CoopConsts& k) {
    x = coop_external_linear(x);
#pragma unroll 1
    for (int r = 0; r < 4; r++) x = coop_external_linear(p2_sbox_rc_dev(x, k.rc_ext[r]));
#pragma unroll 1
    for (int r = 0; r < 13; r++) {
        const uint32_t sb = p2_sbox_rc_dev(x, P2K.int_rcm[r]);
        x = lane16 == 0 ? sb : x;
        uint32_t t = dadd(x, dpp<0x128>(x));
        t = dadd(t, dpp<0x124>(t));
        t = dadd(t, dpp<0x122>(t));
        t = dadd(t, dpp<0x121>(t));                                       // every lane holds the sum
        x = dadd(dmul(x, k.diag), t);
    }
#pragma unroll 1
    for (int r = 4; r < 8; r++) x = coop_external_linear(p2_sbox_rc_dev(x, k.rc_ext[r]));
    return x;
}

}  // namespace zk
#endif
