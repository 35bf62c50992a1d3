// p24chip.h -- column layout of the width-24 Poseidon2 permutation chip (poseidon2_chip.cpp, its width-24 part: the constraint program and
// the C entries; hash.hip: the on-device trace generator).  One row = one width-24 permutation (RISC Zero's shape: 8 full + 21 partial
// rounds); the columns are laid out in the order the permutation produces them, and every section starts on a 16-byte boundary, so that a
// lane writes its row with 16-byte stores of consecutive columns.
#pragma once
#include <cstdint>

namespace zk {
namespace p24chip {

constexpr uint32_t IN = 0, S0 = 24, SPARE = 303, SP = 304, D = 520, BIT = 528, CH = 529, END = 530, CNT = 531, SPG = 532, SS = 533,
                   WIDTH = 540, N_PUBLIC = 9;
// external round r: cubes of the round's input + constant, then the state after the round; rounds 0..3 sit before the internal rounds,
// rounds 4..7 after SP
constexpr uint32_t x3e(uint32_t r) { return r < 4 ? 48 + 48 * r : 328 + 48 * (r - 4); }
constexpr uint32_t oute(uint32_t r) { return x3e(r) + 24; }
constexpr uint32_t s0p(uint32_t r) { return 240 + 3 * r; }      // internal round r: element 0 before the S-box,
constexpr uint32_t x3p(uint32_t r) { return 241 + 3 * r; }      // its cube,
constexpr uint32_t sbp(uint32_t r) { return 242 + 3 * r; }      // its seventh power (column 303 after the 21st round is unused)
constexpr uint32_t ext_input(uint32_t r) { return r == 0 ? S0 : (r == 4 ? SP : oute(r - 1)); }
// partial blocks: G(k), k = 1..3, = rate words 4k .. 4k + 4 are absorbed (words 0..4 always are); C(k) = SPG (1 - G(k)) = those words
// carry over from the previous row's output
constexpr uint32_t G(uint32_t k) { return 533 + k; }
constexpr uint32_t C(uint32_t k) { return 536 + k; }
static_assert(C(3) + 1 == WIDTH && WIDTH % 4 == 0, "p24chip layout");
static_assert(oute(7) + 24 == D && sbp(20) + 1 == SPARE, "p24chip layout");

// path p = rows [p (ceil(row_width / 16) + depth), ...): the sponge rows over its opened row (none when row_width = 0: the leaf digest is
// given), then depth compression rows; leaves / siblings / indices are canonical words already on the device
struct MerkleTraceArgs {
    const uint32_t* leaves;      // [n_paths][8] digests, or [n_paths][row_width] opened rows
    uint32_t row_width;          // 0, or a multiple of 4
    const uint32_t* siblings;    // [n_paths][depth][8]
    const uint32_t* indices;     // [n_paths]: bit l = the node is a right child at level l
    uint64_t n_paths, rows;
    uint32_t depth;
    uint32_t* trace; uint64_t ld;   // [rows][ld], Montgomery; 16-byte aligned, ld % 4 == 0
    uint32_t* roots;             // [n_paths][8], canonical
};

// The LAYER-PATHS variant (the fold-16 paths machine, fri16_chip.hip: P24L stands where the LAYERS table stood).  The 540 columns above keep their
// positions; a tail section follows: LN layer | KP index walk | M receive multiplicity | DEP compression rows so far | Z0..Z3 one-hot number of a
// leaf's sponge row | K0..K3 the bus keys of the four entries a sponge row absorbs.  A path = four sponge rows over the 64 words of a layer row
// (KP = 2 row, BIT = 0, DEP = 0, K_i = 16 row + 4 k + i on sponge row k, M = readers on all four), then `depth` compression rows (KP = row >> level,
// DEP = level + 1, M = K = Z = 0).  Padding rows: the permutation of the zero state, every flag and the tail zero.
constexpr uint32_t L_LN = 540, L_KP = 541, L_M = 542, L_DEP = 543, L_Z = 544, L_K = 548, WIDTH_L = 552, LEAF_ROWS = 4, LEAF_WORDS = 64;
static_assert(L_LN == WIDTH && L_Z % 4 == 0 && L_K % 4 == 0 && WIDTH_L % 4 == 0, "p24chip layer-paths tail: 16-byte sections");
struct LayerPathsArgs {
    const uint32_t* desc;        // [n_paths][8]: layer, row index, depth, readers, first trace row, offset into `readers`, word offset into `siblings`, 0
    const uint32_t* readers;     // per path its readers' rows of the FOLD16 trace; the first one's E columns are the leaf
    const uint32_t* fold;        // the FOLD16 trace (Montgomery; fri16_rows.cuh: E = columns 0..64), leading dimension fold_ld
    uint64_t fold_ld;
    const uint32_t* siblings;    // canonical digests, `depth` of them per path from its offset
    uint64_t n_paths, rows, used_rows;
    uint32_t* trace; uint64_t ld;   // [rows][ld], Montgomery; 16-byte aligned, ld % 4 == 0
    uint32_t* ends;              // [n_paths][8] canonical: where each path ends
    uint32_t* differs;           // [n_paths]: 0, or 1 + the number (within the path's readers) of the first reader whose 64 words are not the first reader's
};

// The ROW-PATHS variant (the fold-16 row-paths machine, fri16_chip.hip: P24R stands where the ROWS table stood).  The 540 columns keep their positions; the tail:
// TAG 2 query + tree | LNR the tree's number in ROOTS | KP index walk | DEP compression rows so far | IX the index | BL block number | LSP last sponge row | M0 sponge
// row | K0..K3 = 4 BL + i the bus keys of the row's four groups.  A path = ceil(width / 16) sponge rows over the opened row (the last one absorbs 2 groups when
// width mod 16 = 8; KP = 2 index, DEP = 0), then `depth` compression rows (KP = index >> level, DEP = level + 1, the other tail cells but TAG and LNR zero).
constexpr uint32_t R_TAG = 540, R_LNR = 541, R_KP = 542, R_DEP = 543, R_IX = 544, R_BL = 545, R_LSP = 546, R_M0 = 547, R_K = 548, WIDTH_R = 552;
static_assert(R_TAG == WIDTH && WIDTH_R == WIDTH_L, "p24chip row-paths tail: the layer-paths variant's width, so that its row writer serves both");
struct RowPathsArgs {
    const uint32_t* desc;        // [n_paths][8]: tag, tree number, index, leaf width, first trace row, word offset of the leaf in `rows`, word offset into `siblings`, 0
    const uint32_t* rows;        // the raw opened rows (canonical words) already on the device
    const uint32_t* siblings;    // canonical digests, `depth` of them per path from its offset
    uint64_t n_paths, trace_rows, used_rows;
    uint32_t depth;
    uint32_t* trace; uint64_t ld;   // [trace_rows][ld], Montgomery; 16-byte aligned, ld % 4 == 0
    uint32_t* ends;              // [n_paths][8] canonical: where each path ends
};

}  // namespace p24chip
}  // namespace zk
