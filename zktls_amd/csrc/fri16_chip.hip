// fri16_chip.hip -- the FRI check of a FOLD-BY-16 proof (the RISC Zero shape: zkhip_prove_segment, log_fold = 4) inside a proof: the FOLD16 and FINAL chips.
//
// The RISC Zero side's lift -> join (prover.rs:90) needs, beside the width-24 Poseidon2 chip (poseidon2_chip.cpp), a chip that folds rows of 16 entries and
// one that evaluates the final polynomial at every query's last point.  This file is those two as a keyed machine of its own, the way fri_chip.hip's first
// generation was for the SP1 shape.  With H = log_n + log_blowup, R = (log_n - F) / 4 committed layers, lf = F + log_blowup: layer l is a matrix of 2^lh
// rows, lh = H - 4 (l + 1), of 16 adjacent extension entries; a query (idx, val) reads row idx >> 4, puts val at position idx & 15, folds the row four times
// by 2 with beta, beta^2, beta^4, beta^8 and goes on with (idx >> 4, folded); after R layers the value must be sum_j c_j xf^j, xf = w_{2^lf}^bitrev(idx, lf).
// With row = idx >> 4 and x0 = w_{2^(lh+4)}^bitrev(row, lh): fold step s folds pair t at x0^(2^s) w_{2^(4-s)}^bitrev(t, 3-s); x0 = prod_i w_{2^(i+5)}^bit_i(row);
// the next row's x0' = x0^16 w_16^(-bitrev(row & 15, 4)); after the last layer x0^16 = xf.
//
// Statement (public values: beta_0 .. beta_{R-1}; the key commits LAYERS, QUERIES, COEFFS):
//     "every query listed in QUERIES, taken as entry index & 15 of row index >> 4 of layer 0, folds through rows listed in LAYERS -- each listed row read
//      exactly as often as listed -- at the points its index fixes, to the value at its last point of the polynomial whose coefficients are listed in COEFFS"
// Five tables (machine order: tallest first, equal heights by the numbers below):
//   0 FOLD16   main, one row per (query, layer): the 16 entries, the 8 + 4 + 2 + 1 folds, beta and its squarings, x0, 1 / x0 and their squarings, the row
//              index, the own position as sixteen one-hot flags, layer selectors, and the BACKWARD product B = T B' (T: the factor of the own position's
//              nibble in the chain's FIRST x0; on the last row times TL, the factor of the lf bits left of ROW, held as up to three one-hot nibbles) with
//              X = B on a chain's first row: the forward recurrence alone fixes x0 only up to a 16^R-th root of unity.  Columns: fri16_rows.cuh.
//              Sends the 16 entries (LN, 16 ROW + j, E_j) to LAYERS, (IDX, OWN) on a chain's first row to QUERIES, (X16, FOLD) on its last row to FINAL.
//   1 FINAL    one block of 2^F rows per query, Horner from the top coefficient down.  Preprocessed schedule J FIRST LAST ACT NL; main C ACC AX = ACC X, X.
//              Receives (J, C) from COEFFS on every row and (X, ACC) from FOLD16 on a block's last row: the multiset of chain ends = that of block ends.
//   2 LAYERS   preprocessed: per distinct (layer, row), ascending: LN, the 16 keys, the number of queries reading it, the 16 entries.  THE TABLE A
//              WIDTH-24 POSEIDON2 CHIP ON THE SAME BUS REPLACES (its leaf rows then receive these tuples): until then the rows' Merkle paths are NOT proven.
//   3 QUERIES  preprocessed: distinct (index, reduced opening) with multiplicity.       4 COEFFS  preprocessed: (j, c_j, queries).
// NOT in this machine: the Merkle paths of the layer rows, the transcript (challenges, query indices), the reduced openings.  tests/fri16_air.py writes
// the programs, tables and traces independently; the words must be equal.
// SEVEN machines are kept here as ONE description read at seven kinds (enum Kind), each kind the one before it with a step more of the inner verifier inside:
//   LAYERS   (zkhip_prove_fri16)           the five tables above
//   PATHS    (zkhip_prove_fri16_paths)     P24L, the width-24 Poseidon2 chip's layer-paths variant, where LAYERS stands, and a preprocessed ROOTS table: the layer rows' Merkle
//                                          paths ARE proven and the key holds the layer roots and no layer value (tests/fri16_paths_air.py)
//   INDICES  (zkhip_prove_fri16_indices)   the Fiat-Shamir transcript inside: a transcript-only width-16 Poseidon2 table (P2T) walks the duplex challenger from the commit phase
//                                          on, the SAMPLES chip of fri_chip.hip takes the bits of the words it hands out; the challenges reach FOLD16 over a bus and the key
//                                          holds neither a challenge nor an index (tests/fri16_transcript_air.py)
//   OPENINGS (zkhip_prove_fri16_openings)  the reduced openings computed in-circuit: ROWSUM16 sums the opened trace row and quotient row in fa, QUERY16 puts the three quotients
//                                          together at the point FOLD16C hands it; the key holds the opened rows and no reduced opening; the eight constants of the formula are
//                                          PUBLIC VALUES in this step -- the step that brings them in over buses is a later one (tests/fri16_openings_air.py)
//   ROWPATHS (zkhip_prove_fri16_rowpaths)  the Merkle paths of the opened trace row and quotient row proven: P24R, a second layer-paths-style variant of the width-24 chip,
//                                          stands where the preprocessed ROWS table stood; the key holds roots and final coefficients only, no opened word
//                                          (tests/fri16_rowpaths_air.py)
//   HEAD     (zkhip_prove_fri16_head)      the head of the transcript inside: P2TH walks the duplex challenger from the all-zero state -- the header, the trace root, the inner
//                                          proof's public values, alpha, the quotient root, zeta, the opened values, fa -- into the commit phase; OPENED16 sums the opened
//                                          values in fa; the eight constants reach ROWSUM16H and QUERY16H over buses.  The public values are the INNER PROOF'S public values
//                                          and nothing else.  alpha is drawn and used by nothing here: the AIR identity at zeta is the step that consumes it
//                                          (tests/fri16_head_air.py)
//   IDENTITY (zkhip_prove_fri16_identity)  the AIR identity at zeta inside: AIR16 folds the synthetic AIR's constraints over the opened values (which OPENED16 sends on
//                                          two more buses) with the alpha P2TH now sends; SCALARS16 squares zeta up to zeta^N, derives the two selectors, puts the quotient
//                                          together from the eight opened quotient values and ties the two: acc = quot (zeta^N - 1).  With it the proof says that the inner
//                                          statement holds, not only that its columns were opened consistently (tests/fri16_identity_air.py)
//   LIFT     (zkhip_prove_fri16_lift)      the roots and the final coefficients OUT of the key: they are main columns of ROOTS and COEFFS, made on the device
//                                          (fri16_lift_tables_kernel) and pinned by the transcript chain alone.  The key is a function of the shape and the public-value
//                                          count: ONE key per shape states "some valid segment proof of this shape with these public values exists" -- RISC Zero's lift.
//                                          zkhip_prove_fri16_lift_segment is the call from segment proof to lift proof (tests/fri16_lift_air.py);
//                                          zkhip_prove_fri16_lift_batch is many of them in one call, side by side on the lock-step lanes (batch.h)
//   JOIN     (zkhip_prove_fri16_join)      no machine of this file: N lift proofs of one shape are N proofs of ONE keyed machine, which machine mode
//                                          (machine_verifier.inl) verifies in-circuit.  The entries at the end of the file describe the lift machine to it
//   TREE     (zkhip_prove_fri16_tree)      no machine of this file either: a join is a machine-mode proof, and machine mode verifies its own proofs.  More lift
//                                          proofs than one join takes go into several joins of one shape (zkhip_prove_fri16_join_batch: side by side, dealt over the
//                                          devices) and ONE proof over the joins; the entries describe the JOIN machine of (shape, join size) to machine mode
// The file in order: the chips' programs and each kind's key tables, section by section as the kinds came; then the one description -- Shape (flat: kind, the numbers, per
// table number the height and widths), shape_of (every kind's validity checks), program_of and interactions_of (per TABLE, what each kind adds
// to or changes in the kind before it), Machine and machine_of (one cache keyed by kind and shape; the machine order and the arrays by position are keyed_machine.h's) --
// and what every entry does with it (describe, key_upload, proof_size, verify, and keyed_machine.h's key_host and prove directly); then the kernels' launchers, the provers' stages (transcript, openings, layer paths) and the extern "C" entries, which are a shape call,
// their own argument checks and those helpers.  The builders of constraint programs and interaction tables and the expression algebra are air_builder.h's, shared with the other chips.
// ADDING A KIND: a value of Kind and its table count in N_TABLES; its new or replaced tables in shape_of (with its checks), program_of and interactions_of -- one `if` on
// the kind in the case of every table it touches; its public values in n_public_of; a builder of its key tables beside the others; a stage for what its prover launches;
// its entries.  Machine, machine_of and the helpers take no new case.
#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "air.h"
#include "air_builder.h"
#include "context.h"
#include "batch.h"
#include "fri16_rows.cuh"
#include "keyed_machine.h"
#include "kernels.h"
#include "p24chip.h"
#include "p2chip.h"

namespace zk {
extern std::atomic<uint64_t> g_p2_generation;      // params.cpp
namespace p24chip { std::shared_ptr<const std::vector<uint32_t>> program_fri16_layers(uint32_t n_public); }      // poseidon2_chip.cpp
namespace p24chip { std::shared_ptr<const std::vector<uint32_t>> program_fri16_rows(uint32_t n_public); }
namespace p2chip { std::vector<uint32_t> permutation_body(uint32_t col_offset, uint32_t* count); }                // poseidon2_chip.cpp: the permutation's constraints behind preprocessed columns
namespace frichip {                                                                                               // fri_chip.hip: the SAMPLES chip
std::shared_ptr<const std::vector<uint32_t>> samples_chip_program(int index_bits, int pow_bits, uint32_t n_public);
const std::vector<uint32_t>& samples_chip_interactions();
size_t samples_chip_rows(size_t nq);
void samples_chip_pre(size_t nq, int log_rows, int first_row, std::vector<uint32_t>& t);
}
namespace fri16 {
namespace {
using namespace airb;

constexpr uint32_t BUS_L16 = 70, BUS_Q16 = 71, BUS_FIN16 = 72, BUS_COEF = 73;
constexpr uint32_t FJ = 0, FFIRST = 1, FLAST = 2, FACT = 3, FNL = 4;                                  // FINAL's schedule; its main columns in the combined row:
constexpr uint32_t CFC = FIN_PRE + FC, CFACC = FIN_PRE + FACC, CFAX = FIN_PRE + FAX, CFX = FIN_PRE + FX;
constexpr uint32_t LAY_PRE = 84, LAY_LN = 0, LAY_KEY = 1, LAY_M = 17, LAY_E = 20, Q_PRE = 8, C_PRE = 8, TAB_MAIN = 4;
// ONE numbering of the tables for all kinds: a later kind appends tables (5; 6, 7; 8, 9; 10; 11, 12) or puts a chip where a key table stood (2, 3, 9)
enum : int { T_FOLD16 = 0, T_FINAL = 1, T_LAYERS = 2, T_P24L = 2, T_QUERIES = 3, T_QUERY16 = 3, T_COEFFS = 4, T_ROOTS = 5, T_P2T = 6, T_SAMPLES = 7, T_ROWSUM16 = 8, T_ROWS = 9,
              T_P24R = 9, T_OPENED16 = 10, T_AIR16 = 11, T_SCALARS16 = 12, MAX_TABLES = 13 };
inline uint32_t canon_nibble_factor(uint32_t first_bit, uint32_t nbits, uint32_t j) { return from_monty(nibble_factor(first_bit, nbits, j)); }

// The machines are ONE description read at eight kinds, each kind the one before it with a step more of the inner verifier inside.  What a kind adds to the shape
// (pow_bits, C S NT from INDICES on; W from OPENINGS on) stays zero below it.  shape_of, program_of, interactions_of and machine_of are further down, behind the chips.
enum Kind : int { LAYERS = 0, PATHS, INDICES, OPENINGS, ROWPATHS, HEAD, IDENTITY, LIFT };
struct Shape {
    Kind kind = LAYERS;
    int R = 0, F = 0, b = 0, lf = 0, H = 0, pow_bits = 0, n_tables = 0;
    size_t Q = 0, C = 0, S = 0, NT = 0;      // C, S, NT: coefficient rows, rows that hand words out, rows of the transcript's chain
    uint32_t W = 0;                          // the inner proof's trace width
    uint32_t NP = 0;                         // HEAD: the inner proof's public values; A sponge rows up to alpha, HD rows in front of the commit phase's
    size_t A = 0, HD = 0;
    int log_rows[MAX_TABLES];                // by table number
    uint32_t main_w[MAX_TABLES], pre_w[MAX_TABLES];
};
// what an entry is given of a shape: the kind and the words its signature has (the rest zero); shape_of reads what the kind takes
struct ShapeArgs {
    Kind kind = LAYERS;
    int R = 0, F = 0, b = 0;
    size_t Q = 0;
    int pow_bits = 0;
    uint32_t W = 0, NP = 0;
};
// every array and word a prover or key entry takes (host, canonical; not owned), null or zero where the kind has none, in the order the prove entries take them: a
// prove entry fills its view by position.  Fri16FullView (context.h) owns one.
struct View {
    int hash_width = 0;
    const uint32_t *betas = nullptr, *final_poly = nullptr, *indices = nullptr, *values = nullptr, *siblings = nullptr, *roots = nullptr, *paths = nullptr, *capacity = nullptr;
    uint32_t witness = 0;
    const uint32_t *trace_rows = nullptr, *quotient_rows = nullptr, *constants = nullptr, *trace_paths = nullptr, *quotient_paths = nullptr;
    const uint32_t *trace_root = nullptr, *quotient_root = nullptr, *inner_public = nullptr, *opened = nullptr;
};
inline int lg(size_t n) { int l = 5; while (((size_t)1 << l) < n) l++; return l; }

std::vector<uint32_t> build_fold16_program(int R, int lf, bool beta_bus = false, uint32_t n_public = 0) {      // beta_bus: FOLD16B, BETA is received, not public
    Builder b;
    const uint32_t END = L + (uint32_t)R - 1u, W = fold16_width((uint32_t)lf), inv2 = (P + 1) / 2;
    const W16Inv w16 = w16_inverse_powers();
    auto ext_product = [&](uint32_t out, uint32_t x, uint32_t y) {      // out = x y in F_p[t] / (t^4 - 11)
        for (uint32_t c = 0; c < 4; c++) {
            Terms t{{1u, {var(out + c)}}};
            for (uint32_t i = 0; i < 4; i++)
                for (uint32_t j = 0; j < 4; j++)
                    if ((i + j) % 4 == c) t.push_back(Term{neg(i + j >= 4 ? EXT_W : 1u), {var(x + i), var(y + j)}});
            b.add(ALL, t);
        }
    };
    {
        Terms t{{1u, {var(ACTIVE)}}}, n{{1u, {var(LN)}}};
        for (int l = 0; l < R; l++) { t.push_back(Term{P - 1, {var(L + l)}}); n.push_back(Term{neg((uint64_t)l), {var(L + l)}}); }
        b.add(ALL, t);
        b.add(ALL, n);
    }
    b.add(ALL, Terms{{1u, {var(ACTIVE), var(ACTIVE)}}, {P - 1, {var(ACTIVE)}}});
    for (int l = 0; l < 8; l++) {
        if (l < R) b.add(ALL, Terms{{1u, {var(L + l), var(L + l)}}, {P - 1, {var(L + l)}}});
        else b.add(ALL, Terms{{1u, {var(L + l)}}});
    }
    for (uint32_t j = 0; j < 16; j++) b.add(ALL, Terms{{1u, {var(OF + j), var(OF + j)}}, {P - 1, {var(OF + j)}}});
    {
        Terms t{{1u, {var(ACTIVE)}}};
        for (uint32_t j = 0; j < 16; j++) t.push_back(Term{P - 1, {var(OF + j)}});
        b.add(ALL, t);
    }
    for (uint32_t c = 0; c < 4 && !beta_bus; c++) {      // BETA = the layer's public challenge
        Terms t{{1u, {var(BETA + c)}}};
        for (int l = 0; l < R; l++) t.push_back(Term{P - 1, {var(L + l), pub(4u * (uint32_t)l + c)}});
        b.add(ALL, t);
    }
    ext_product(B2, BETA, BETA);
    ext_product(B4, B2, B2);
    ext_product(B8, B4, B4);
    b.add(ALL, Terms{{1u, {var(G)}}, {P - 1, {var(ACTIVE)}}, {1u, {var(END)}}});
    const uint32_t squares[7][2] = {{X2, X}, {X4, X2}, {X8, X4}, {X16, X8}, {XI2, XI}, {XI4, XI2}, {XI8, XI4}};
    for (const auto& sq : squares) b.add(ALL, Terms{{1u, {var(sq[0])}}, {P - 1, {var(sq[1]), var(sq[1])}}});
    b.add(ALL, Terms{{1u, {var(ACTIVE), var(X), var(XI)}}, {P - 1, {var(ACTIVE)}}});
    b.add(ALL, Terms{{1u, {var(GX16)}}, {P - 1, {var(G), var(X16)}}});
    b.add(ALL, Terms{{1u, {var(GT)}}, {P - 1, {var(G), var(T)}}});
    {
        Terms t{{1u, {var(IDX)}}, {P - 16, {var(ROW)}}};
        for (uint32_t j = 0; j < 16; j++) t.push_back(Term{neg(j), {var(OF + j)}});
        b.add(ALL, t);
    }
    for (uint32_t j = 0; j < 16; j++) b.add(ALL, Terms{{1u, {var(KJ + j)}}, {P - 16, {var(ROW)}}, {neg(j), {var(ACTIVE)}}});
    for (uint32_t c = 0; c < 4; c++) {      // OWN = sum_j O_j E_j
        Terms t{{1u, {var(OWN + c)}}};
        for (uint32_t j = 0; j < 16; j++) t.push_back(Term{P - 1, {var(OF + j), var(E + 4 * j + c)}});
        b.add(ALL, t);
    }
    const uint32_t step_in[4] = {E, F1, F2, F3}, step_out[4] = {F1, F2, F3, FOLD}, step_beta[4] = {BETA, B2, B4, B8}, step_xi[4] = {XI, XI2, XI4, XI8};
    for (uint32_t s = 0; s < 4; s++)        // out = (e0 + e1)/2 + beta_s (e0 - e1) xi_s c / 2, c = 1 / w_{2^(4-s)}^bitrev(t, 3-s)
        for (uint32_t t = 0; t < (8u >> s); t++) {
            const uint32_t e0 = step_in[s] + 8 * t, e1 = e0 + 4, ci = from_monty(w16.v[step_exponent(s, t)]);
            for (uint32_t c = 0; c < 4; c++) {
                Terms ts{{1u, {var(step_out[s] + 4 * t + c)}}, {neg(inv2), {var(e0 + c)}}, {neg(inv2), {var(e1 + c)}}};
                for (uint32_t a = 0; a < 4; a++)
                    for (uint32_t d = 0; d < 4; d++) {
                        if ((a + d) % 4 != c) continue;
                        const uint32_t w = mulm(mulm(inv2, ci), a + d >= 4 ? EXT_W : 1u);
                        ts.push_back(Term{neg(w), {var(step_beta[s] + a), var(e0 + d), var(step_xi[s])}});
                        ts.push_back(Term{w, {var(step_beta[s] + a), var(e1 + d), var(step_xi[s])}});
                    }
                b.add(ALL, ts);
            }
        }
    {   // T = L_0 + sum_{l >= 1} sum_j (factor of nibble l - 1 holding j) L_l O_j
        Terms t{{1u, {var(T)}}, {P - 1, {var(L)}}};
        for (int l = 1; l < R; l++)
            for (uint32_t j = 0; j < 16; j++) t.push_back(Term{neg(canon_nibble_factor(4u * (uint32_t)(l - 1), 4u, j)), {var(L + l), var(OF + j)}});
        b.add(ALL, t);
    }
    // the last row's nibbles: one-hot on a last row, zero elsewhere; their linear forms
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> forms;
    uint32_t col = N;
    for (uint32_t k = 0; k < 3 && nibble_bits((uint32_t)lf, k); k++) {
        const uint32_t nb = nibble_bits((uint32_t)lf, k);
        Terms sum{{1u, {var(END)}}};
        std::vector<std::pair<uint32_t, uint32_t>> form;
        for (uint32_t j = 0; j < (1u << nb); j++) b.add(ALL, Terms{{1u, {var(col + j), var(col + j)}}, {P - 1, {var(col + j)}}});
        for (uint32_t j = 0; j < (1u << nb); j++) {
            sum.push_back(Term{P - 1, {var(col + j)}});
            form.push_back({canon_nibble_factor(4u * (uint32_t)(R - 1) + 4u * k, nb, j), col + j});
        }
        b.add(ALL, sum);
        forms.push_back(form);
        col += 1u << nb;
    }
    for (uint32_t c = col; c < W; c++) b.add(ALL, Terms{{1u, {var(c)}}});
    {
        Terms t{{1u, {var(END), var(ROW)}}};
        uint32_t c0 = N;
        for (uint32_t k = 0; k < forms.size(); k++) {
            const uint32_t nb = nibble_bits((uint32_t)lf, k);
            for (uint32_t j = 0; j < (1u << nb); j++) t.push_back(Term{neg((uint64_t)j << (4 * k)), {var(c0 + j)}});
            c0 += 1u << nb;
        }
        b.add(ALL, t);
    }
    {
        Terms u{{1u, {var(U)}}};
        if (forms.size() == 1) for (const auto& f : forms[0]) u.push_back(Term{neg(f.first), {var(f.second)}});
        else for (const auto& f0 : forms[0]) for (const auto& f1 : forms[1]) u.push_back(Term{neg(mulm(f0.first, f1.first)), {var(f0.second), var(f1.second)}});
        b.add(ALL, u);
        Terms tl{{1u, {var(TL)}}};
        if (forms.size() == 3) for (const auto& f : forms[2]) tl.push_back(Term{neg(f.first), {var(U), var(f.second)}});
        else tl.push_back(Term{P - 1, {var(U)}});
        b.add(ALL, tl);
    }
    b.add(ALL, Terms{{1u, {var(END), var(B)}}, {P - 1, {var(END), var(T), var(TL)}}});
    b.add(ALL, Terms{{1u, {var(L), var(X)}}, {P - 1, {var(L), var(B)}}});
    // the chain
    for (int l = 0; l + 1 < R; l++) b.add(TRANSITION, Terms{{1u, {var(L + l + 1, true)}}, {P - 1, {var(L + l)}}});
    b.add(TRANSITION, Terms{{1u, {var(G), var(ROW)}}, {P - 1, {var(G), var(IDX, true)}}});
    {
        Terms t{{1u, {var(G), var(X, true)}}};
        for (uint32_t j = 0; j < 16; j++) t.push_back(Term{neg(from_monty(w16.v[reverse_bits(j, 4)])), {var(GX16), var(OF + j, true)}});
        b.add(TRANSITION, t);
    }
    b.add(TRANSITION, Terms{{1u, {var(G), var(B)}}, {P - 1, {var(GT), var(B, true)}}});
    for (uint32_t c = 0; c < 4; c++) b.add(TRANSITION, Terms{{1u, {var(G), var(FOLD + c)}}, {P - 1, {var(G), var(OWN + c, true)}}});
    b.add(FIRST, Terms{{1u, {var(ACTIVE)}}, {P - 1, {var(L)}}});
    b.add(LAST, Terms{{1u, {var(G)}}});
    return b.finish(W, beta_bus ? n_public : 4u * (uint32_t)R);
}
std::vector<uint32_t> build_final_program(uint32_t n_public) {
    Builder b;
    for (uint32_t c = 0; c < 4; c++) b.add(ALL, Terms{{1u, {var(CFAX + c)}}, {P - 1, {var(CFACC + c), var(CFX)}}});
    for (uint32_t c = 0; c < 4; c++) b.add(ALL, Terms{{1u, {var(FFIRST), var(CFACC + c)}}, {P - 1, {var(FFIRST), var(CFC + c)}}});
    b.add(TRANSITION, Terms{{1u, {var(FNL), var(CFX, true)}}, {P - 1, {var(FNL), var(CFX)}}});
    for (uint32_t c = 0; c < 4; c++)
        b.add(TRANSITION, Terms{{1u, {var(FNL), var(CFACC + c, true)}}, {P - 1, {var(FNL), var(CFAX + c)}}, {P - 1, {var(FNL), var(CFC + c, true)}}});
    return b.finish(FIN_PRE + FIN_MAIN, n_public);
}
// (pinned: the main column the identity names, by default the last; the lift machine's COEFFS holds c_j in its last four and names the last UNUSED one)
std::vector<uint32_t> build_table_program(uint32_t n_public, uint32_t pre_width, uint32_t main_width = TAB_MAIN, uint32_t pinned = ~0u) {          // the contents are fixed by the KEY: one harmless identity
    return std::vector<uint32_t>{AIR_MAGIC, 1u, pre_width + main_width, 1u, n_public, 6u + 5u, FIRST, 1u, 1u, 1u, var(pre_width + (pinned == ~0u ? main_width - 1u : pinned))};
}

inline Ext ext_from_canon(const uint32_t* p) { return Ext{{to_monty(p[0]), to_monty(p[1]), to_monty(p[2]), to_monty(p[3])}}; }
bool canonical(const uint32_t* v, size_t n) { for (size_t i = 0; i < n; i++) if (v[i] >= P) return false; return true; }
int check_view(const Shape& s, const View& v, const char* who) {
    if (!v.betas || !v.final_poly || !v.indices || !v.values || !v.siblings) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!canonical(v.betas, 4 * (size_t)s.R) || !canonical(v.final_poly, (size_t)4 << s.F) || !canonical(v.values, 4 * s.Q) || !canonical(v.siblings, 60 * s.Q * (size_t)s.R))
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    for (size_t q = 0; q < s.Q; q++) if (v.indices[q] >> s.H) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": a query index has more bits than the proof's domain");
    return ZKHIP_OK;
}
// the fold of one row on the host (the kernels' arithmetic, portable forms)
Ext fold_row_host(uint32_t row, int lh, const Ext& beta, const Ext* entries) {
    const W16Inv w16 = w16_inverse_powers();
    const uint32_t w = two_adic_generator(lh + 4), br = reverse_bits(row, lh), mask = (1u << (lh + 4)) - 1u;
    uint32_t xi = fpow(w, (mask + 1u - br) & mask);
    Ext cur[16], bs = beta;
    for (int j = 0; j < 16; j++) cur[j] = entries[j];
    for (uint32_t s = 0; s < 4; s++) {
        for (uint32_t t = 0; t < (8u >> s); t++) {
            const Ext even = ext_mul_base(ext_add(cur[2 * t], cur[2 * t + 1]), MONTY_INV2);
            const Ext odd = ext_mul_base(ext_sub(cur[2 * t], cur[2 * t + 1]), fmul(fmul(xi, MONTY_INV2), w16.v[step_exponent(s, t)]));
            cur[t] = ext_add(even, ext_mul(bs, odd));
        }
        bs = ext_mul(bs, bs);
        xi = fmul(xi, xi);
    }
    return cur[0];
}
// FINAL's schedule, QUERIES and COEFFS (zeroed, at their heights): what both machines' keys share
void fill_schedule_queries_coeffs(const Shape& s, const uint32_t* final_poly, const std::map<std::array<uint32_t, 5>, uint32_t>& queries, std::vector<uint32_t>& fin,
                                  std::vector<uint32_t>& qs, std::vector<uint32_t>& cs) {
    const size_t n = (size_t)1 << s.F;
    for (size_t r = 0; r < s.Q * n; r++) {
        uint32_t* w = fin.data() + FIN_PRE * r;
        const size_t i = r & (n - 1);
        w[FJ] = to_monty((uint32_t)(n - 1 - i)); w[FFIRST] = i == 0 ? MONTY_R1 : 0u; w[FLAST] = i == n - 1 ? MONTY_R1 : 0u; w[FACT] = MONTY_R1; w[FNL] = i == n - 1 ? 0u : MONTY_R1;
    }
    size_t r = 0;
    for (const auto& e : queries) {
        uint32_t* w = qs.data() + Q_PRE * r++;
        for (int i = 0; i < 5; i++) w[i] = to_monty(e.first[i]);
        w[5] = to_monty(e.second);
    }
    for (size_t j = 0; j < n; j++) {
        uint32_t* w = cs.data() + C_PRE * j;
        w[0] = to_monty((uint32_t)j);
        for (int i = 0; i < 4; i++) w[1 + i] = to_monty(final_poly[4 * j + i]);
        w[5] = to_monty((uint32_t)s.Q);
    }
}
// The three key tables and FINAL's schedule from a view (host, canonical -> Montgomery), by table number.  Walks every chain: queries that meet must
// agree about the row, and every chain must end in the final polynomial at its last point -- a view taken from an accepted proof always does.
int build_tables(const Shape& s, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values, const uint32_t* siblings,
                 std::vector<uint32_t> pre[]) {
    const size_t R = (size_t)s.R, n = (size_t)1 << s.F;
    std::map<std::pair<uint32_t, uint32_t>, std::pair<std::array<uint32_t, 64>, uint32_t>> layers;      // (layer, row) -> entries (Montgomery), count
    std::map<std::array<uint32_t, 5>, uint32_t> queries;                                                 // (index, value) canonical -> count
    for (size_t q = 0; q < s.Q; q++) {
        std::array<uint32_t, 5> qk{indices[q], values[4 * q], values[4 * q + 1], values[4 * q + 2], values[4 * q + 3]};
        queries[qk]++;
        uint32_t idx = indices[q];
        Ext val = ext_from_canon(values + 4 * q);
        for (size_t l = 0; l < R; l++) {
            const uint32_t row = idx >> 4, own = idx & 15u;
            const int lh = s.H - 4 * ((int)l + 1);
            Ext e[16];
            const uint32_t* sib = siblings + 60 * (q * R + l);
            for (uint32_t j = 0, k = 0; j < 16; j++) e[j] = j == own ? val : ext_from_canon(sib + 4 * k++);
            std::array<uint32_t, 64> flat;
            for (int j = 0; j < 16; j++) for (int c = 0; c < 4; c++) flat[4 * j + c] = e[j].c[c];
            auto it = layers.find({(uint32_t)l, row});
            if (it == layers.end()) layers.emplace(std::make_pair((uint32_t)l, row), std::make_pair(flat, 1u));
            else {
                if (it->second.first != flat) return fail(ZKHIP_ERR_INVALID, "fri16: two queries disagree about a layer row");
                it->second.second++;
            }
            val = fold_row_host(row, lh, ext_from_canon(betas + 4 * l), e);
            idx = row;
        }
        const uint32_t xf = fpow(two_adic_generator(s.lf), reverse_bits(idx, s.lf));
        Ext v = ext_zero();
        for (size_t i = n; i-- > 0;) v = ext_add(ext_mul_base(v, xf), ext_from_canon(final_poly + 4 * i));
        if (!ext_eq(v, val)) return fail(ZKHIP_ERR_INVALID, "fri16: the chain of query " + std::to_string(q) + " does not end in the final polynomial");
    }
    for (int t = 1; t < 5; t++) pre[t].assign((size_t)s.pre_w[t] << s.log_rows[t], 0u);
    pre[0].clear();
    size_t r = 0;
    for (const auto& e : layers) {
        uint32_t* w = pre[T_LAYERS].data() + LAY_PRE * r++;
        w[LAY_LN] = to_monty(e.first.first);
        for (uint32_t j = 0; j < 16; j++) w[LAY_KEY + j] = to_monty(16u * e.first.second + j);
        w[LAY_M] = to_monty(e.second.second);
        std::memcpy(w + LAY_E, e.second.first.data(), 256);
    }
    fill_schedule_queries_coeffs(s, final_poly, queries, pre[T_FINAL], pre[T_QUERIES], pre[T_COEFFS]);
    return ZKHIP_OK;
}

// ---------------------------------------------------------------- the PATHS machine: P24L where LAYERS stood, and the ROOTS table
// Table numbers 0 FOLD16, 1 FINAL, 2 P24L, 3 QUERIES, 4 COEFFS, 5 ROOTS.  FOLD16, FINAL, QUERIES and COEFFS are the machine's above, word for word; P24L is the
// width-24 chip's layer-paths variant (p24chip.h, poseidon2_chip.cpp): its sponge rows receive on BUS_L16 what FOLD16 sends, its END rows send
// (layer, depth, digest) in two halves to ROOTS (preprocessed layer, depth, root[8]; main: the number of path ends of the layer, the prover's).
constexpr uint32_t BUS_RT0 = 74, BUS_RT1 = 75, ROOTS_PRE16 = 12, RT_LN = 0, RT_DEP = 1, RT_ROOT = 2;
int check_hash_width(int inner_hash_width, const char* who) {
    if (inner_hash_width == 24) return ZKHIP_OK;
    return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the paths machine opens width-24 Poseidon2 commitments (inner hash_width 24); a fold-16 proof with the width-16 hash is taken by zkhip_prove_fri16 only");
}
// the key's tables by table number: FINAL's schedule, QUERIES, COEFFS, ROOTS -- from the shape, the final coefficients, the queries and the layer roots alone
int build_paths_key_tables(const Shape& s, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values, const uint32_t* roots, std::vector<uint32_t> pre[],
                           const char* who) {
    if (!final_poly || !indices || !values || !roots) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!canonical(final_poly, (size_t)4 << s.F) || !canonical(values, 4 * s.Q) || !canonical(roots, 8 * (size_t)s.R)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    std::map<std::array<uint32_t, 5>, uint32_t> queries;
    for (size_t q = 0; q < s.Q; q++) {
        if (indices[q] >> s.H) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": a query index has more bits than the proof's domain");
        queries[std::array<uint32_t, 5>{indices[q], values[4 * q], values[4 * q + 1], values[4 * q + 2], values[4 * q + 3]}]++;
    }
    for (int t = 0; t < s.n_tables; t++) pre[t].assign((size_t)s.pre_w[t] << s.log_rows[t], 0u);
    fill_schedule_queries_coeffs(s, final_poly, queries, pre[T_FINAL], pre[T_QUERIES], pre[T_COEFFS]);
    for (int l = 0; l < s.R; l++) {
        uint32_t* w = pre[T_ROOTS].data() + ROOTS_PRE16 * (size_t)l;
        w[RT_LN] = to_monty((uint32_t)l); w[RT_DEP] = to_monty((uint32_t)(s.H - 4 * (l + 1)));
        for (int j = 0; j < 8; j++) w[RT_ROOT + j] = to_monty(roots[8 * l + j]);
    }
    return ZKHIP_OK;
}
// One path per distinct (layer, row), ascending: the kernel's descriptors, every path's readers (rows of the FOLD16 trace, query order) and what the refusals name.
// Queries that share a row must bring the same authentication path.
struct PathPlan {
    std::vector<uint32_t> desc, readers, layer_of, first_query, counts;     // [n][8], [Q R], [n], [n], [R]
    size_t n = 0, used_rows = 0, path_words = 0;
};
int plan_paths(const Shape& s, const uint32_t* indices, const uint32_t* paths, PathPlan& pl) {
    const size_t R = (size_t)s.R;
    std::vector<size_t> off(R + 1, 0);
    for (size_t l = 0; l < R; l++) off[l + 1] = off[l] + 8 * (size_t)(s.H - 4 * ((int)l + 1));
    pl.path_words = off[R];
    if (!canonical(paths, s.Q * pl.path_words)) return fail(ZKHIP_ERR_INVALID, "fri16 paths: values must be canonical");
    std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> rows;
    for (size_t q = 0; q < s.Q; q++)
        for (size_t l = 0; l < R; l++) rows[{(uint32_t)l, indices[q] >> (4 * (l + 1))}].push_back((uint32_t)q);
    pl.n = rows.size();
    pl.counts.assign(R, 0u);
    for (const auto& e : rows) {
        const uint32_t l = e.first.first, depth = (uint32_t)(s.H - 4 * ((int)l + 1)), q0 = e.second[0];
        const uint32_t* mine = paths + q0 * pl.path_words + off[l];
        for (uint32_t q : e.second)
            if (std::memcmp(mine, paths + q * pl.path_words + off[l], 32 * (size_t)depth) != 0)
                return fail(ZKHIP_ERR_INVALID, "fri16 paths: query " + std::to_string(q) + " layer " + std::to_string(l) + " disagrees with query " + std::to_string(q0) +
                                                   " about the path of a shared row");
        const uint32_t d[8] = {l, e.first.second, depth, (uint32_t)e.second.size(), (uint32_t)pl.used_rows, (uint32_t)pl.readers.size(), (uint32_t)(q0 * pl.path_words + off[l]), 0u};
        pl.desc.insert(pl.desc.end(), d, d + 8);
        for (uint32_t q : e.second) pl.readers.push_back((uint32_t)(q * R + l));
        pl.layer_of.push_back(l); pl.first_query.push_back(q0);
        pl.counts[l]++;
        pl.used_rows += p24chip::LEAF_ROWS + depth;
    }
    return ZKHIP_OK;
}

// ---------------------------------------------------------------- the INDICES machine: the paths machine with the transcript inside
// Table numbers 0 FOLD16B, 1 FINAL, 2 P24L, 3 QUERIES, 4 COEFFS, 5 ROOTS, 6 P2T, 7 SAMPLES.  Public values: the 8 capacity words of the duplex challenger as the commit
// phase finds it (pending inputs zero: the step before is a sample).  The sponge chain (P2T, one width-16 permutation per row, rows 0 .. NT - 1):
//   R root rows        row l absorbs root_l as one full rate block; beta_l = (out[7], out[6], out[5], out[4])
//   C coefficient rows (F >= 1: C = 2^(F-1), row R + i absorbs c_2i, c_2i+1; F = 0: none)
//   the witness row    F >= 1: rate word 0 <- the witness, words 1..7 keep the previous output; F = 0: words 0..3 <- c_0, word 4 <- the witness, 5..7 kept
//   S - 1 permute rows (S = ceil((1 + Q) / 8)) the whole previous output
// The witness row and the permute rows hand their eight rate words out from out[7] down: the proof-of-work word, then one word per query.
// FOLD16B is FOLD16 without the constraints BETA = public and with a receive of (LN, BETA) on every active row; FINAL and P24L are the paths machine's word for word
// (but the public-value count in the header); QUERIES: preprocessed (q, value[4], 1), main the index, received from SAMPLES by query number and handed to the chain's
// first row; COEFFS: one more send (j, c_j), multiplicity 1 (column 6), to P2T; ROOTS: preprocessed (layer, depth, root[8], 1), main (path ends, beta[4], fold rows):
// root and beta received from the layer's root row, beta sent on to the fold rows -- by listed rows only (build_roots_program); SAMPLES: fri_chip.hip's chip with H index bits, first row number R + C.
constexpr uint32_t BUS_TR0 = 76, BUS_TR1 = 77, BUS_TB = 78, BUS_BF16 = 79, BUS_CT = 80, N_PUBLIC_I = 8, ROOTS_MAIN_I = 8;
constexpr uint32_t PT_PRE = 20, PT_SPG = 0, PT_K = 1, PT_ROOT = 9, PT_LN = 10, PT_C0 = 11, PT_KEY0 = 12, PT_C1 = 13, PT_KEY1 = 14, PT_SMP = 15, PT_ROW = 16;
// P2T's program: the permutation; D and BIT pinned (no path in this table); the chain behind the preprocessed schedule
std::vector<uint32_t> build_p2t_program(uint32_t n_public) {
    using namespace p2chip;
    const uint32_t M0 = PT_PRE, OUT = M0 + oute(7);
    Builder b;
    b.body = permutation_body(M0, &b.count);
    for (uint32_t j = 0; j < 8; j++) b.add(ALL, Terms{{1u, {var(M0 + D + j)}}, {P - 1, {var(M0 + IN + j)}}});
    b.add(ALL, Terms{{1u, {var(M0 + BIT)}}});
    for (uint32_t j = 0; j < 8; j++) b.add(FIRST, Terms{{1u, {var(M0 + IN + 8 + j)}}, {P - 1, {pub(j)}}});
    for (uint32_t j = 0; j < 8; j++) b.add(TRANSITION, Terms{{1u, {var(PT_SPG, true), var(M0 + IN + 8 + j, true)}}, {P - 1, {var(PT_SPG, true), var(OUT + 8 + j)}}});
    for (uint32_t j = 0; j < 8; j++) b.add(TRANSITION, Terms{{1u, {var(PT_K + j, true), var(M0 + IN + j, true)}}, {P - 1, {var(PT_K + j, true), var(OUT + j)}}});
    return b.finish(PT_PRE + T_WIDTH, n_public);
}
// ROOTS' program: the harmless identity of a key table, and FOLDROWS (1 - LISTED) = 0 -- the multiplicity of the send (layer, beta) to FOLD16B is a MAIN column, and a
// padding row's preprocessed cells are zero (layer 0, nothing received from the transcript): without this a padding row could hand layer 0 a challenge of the prover's choice
// (lift: the root words are eight more MAIN columns behind these, so the first-row identity keeps naming the spare column 7, not the last one; and the receive
// multiplicity ENDS is gated by the preprocessed ACT as FOLDROWS is by LISTED -- a padding row's digest is free there, so it must receive nothing)
std::vector<uint32_t> build_roots_program(uint32_t n_public, uint32_t pre_w = ROOTS_PRE16, bool lift = false) {      // (the head machine's ROOTS has eight more preprocessed columns)
    Builder b;
    b.add(FIRST, Terms{{1u, {var(pre_w + ROOTS_MAIN_I - 1u)}}});
    b.add(ALL, Terms{{1u, {var(pre_w + 5u)}}, {P - 1, {var(pre_w + 5u), var(10u)}}});
    if (lift) b.add(ALL, Terms{{1u, {var(pre_w)}}, {P - 1, {var(pre_w), var(RT_ROOT)}}});                              // ENDS (1 - ACT) = 0; ACT sits where root word 0 stood
    return b.finish(pre_w + (lift ? ROOTS_MAIN_L : ROOTS_MAIN_I), n_public);
}
// the key's tables by table number: FINAL's schedule, QUERIES by query number, COEFFS, ROOTS, and the schedules of P2T and SAMPLES -- no index and no challenge
int build_indices_key_tables(const Shape& s, const uint32_t* final_poly, const uint32_t* values, const uint32_t* roots, std::vector<uint32_t> pre[], const char* who) {
    if (!final_poly || !values || !roots) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!canonical(final_poly, (size_t)4 << s.F) || !canonical(values, 4 * s.Q) || !canonical(roots, 8 * (size_t)s.R)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    for (int t = 0; t < s.n_tables; t++) pre[t].assign((size_t)s.pre_w[t] << s.log_rows[t], 0u);
    fill_schedule_queries_coeffs(s, final_poly, std::map<std::array<uint32_t, 5>, uint32_t>(), pre[T_FINAL], pre[T_QUERIES], pre[T_COEFFS]);
    for (size_t q = 0; q < s.Q; q++) {
        uint32_t* w = pre[T_QUERIES].data() + Q_PRE * q;
        w[0] = to_monty((uint32_t)q);
        for (int i = 0; i < 4; i++) w[1 + i] = to_monty(values[4 * q + i]);
        w[5] = MONTY_R1;
    }
    for (size_t j = 0; j < ((size_t)1 << s.F); j++) pre[T_COEFFS][C_PRE * j + 6] = MONTY_R1;
    for (int l = 0; l < s.R; l++) {
        uint32_t* w = pre[T_ROOTS].data() + ROOTS_PRE16 * (size_t)l;
        w[RT_LN] = to_monty((uint32_t)l); w[RT_DEP] = to_monty((uint32_t)(s.H - 4 * (l + 1)));
        for (int j = 0; j < 8; j++) w[RT_ROOT + j] = to_monty(roots[8 * l + j]);
        w[10] = MONTY_R1;
    }
    const size_t R = (size_t)s.R;
    for (size_t r = 0; r < s.NT; r++) {
        uint32_t* w = pre[T_P2T].data() + PT_PRE * r;
        if (r) w[PT_SPG] = MONTY_R1;
        uint32_t kept_from = 8;                                  // rate words kept_from .. 7 keep the previous output
        if (r < R) { w[PT_ROOT] = MONTY_R1; w[PT_LN] = to_monty((uint32_t)r); }
        else if (r < R + s.C) {
            const uint32_t i = (uint32_t)(r - R);
            w[PT_C0] = w[PT_C1] = MONTY_R1; w[PT_KEY0] = to_monty(2u * i); w[PT_KEY1] = to_monty(2u * i + 1u);
        } else if (r == R + s.C) {
            if (s.F == 0) { w[PT_C0] = MONTY_R1; kept_from = 5; } else kept_from = 1;
        } else kept_from = 0;
        for (uint32_t j = kept_from; j < 8; j++) w[PT_K + j] = MONTY_R1;
        if (r >= R + s.C) { w[PT_SMP] = MONTY_R1; w[PT_ROW] = to_monty((uint32_t)r); }
    }
    frichip::samples_chip_pre(s.Q, s.log_rows[T_SAMPLES], (int)(R + s.C), pre[T_SAMPLES]);
    return ZKHIP_OK;
}
// the chain walked on the host (NT permutations): every row's input state, the challenges and the words it hands out -- canonical
struct Chain { std::vector<uint32_t> inputs, words, betas, drawn; };
void walk_chain(const Shape& s, const uint32_t* capacity, const uint32_t* roots, const uint32_t* final_poly, uint32_t witness, Chain& c) {
    const size_t R = (size_t)s.R;
    c.inputs.assign(16 * s.NT, 0u); c.words.assign(8 * s.S, 0u); c.betas.assign(4 * R, 0u); c.drawn.assign(s.Q, 0u);
    uint32_t st[16];
    size_t r = 0;
    auto step = [&]() { for (int j = 0; j < 16; j++) c.inputs[16 * r + j] = from_monty(st[j]); r++; p2_permute(st); };
    for (int j = 0; j < 8; j++) st[8 + j] = to_monty(capacity[j]);
    for (size_t l = 0; l < R; l++) {
        for (int j = 0; j < 8; j++) st[j] = to_monty(roots[8 * l + j]);
        step();
        for (int j = 0; j < 4; j++) c.betas[4 * l + j] = from_monty(st[7 - j]);
    }
    for (size_t i = 0; i < s.C; i++) {
        for (int j = 0; j < 8; j++) st[j] = to_monty(final_poly[8 * i + j]);
        step();
    }
    if (s.F == 0) { for (int j = 0; j < 4; j++) st[j] = to_monty(final_poly[j]); st[4] = to_monty(witness); }
    else st[0] = to_monty(witness);
    for (size_t i = 0; i < s.S; i++) {
        step();
        for (int j = 0; j < 8; j++) c.words[8 * i + j] = from_monty(st[7 - j]);
    }
    const uint32_t mask = (1u << s.H) - 1u;
    for (size_t q = 0; q < s.Q; q++) c.drawn[q] = c.words[q + 1] & mask;
}

// ---------------------------------------------------------------- the OPENINGS machine: the indices machine with the reduced openings computed in-circuit
// Table numbers 0 FOLD16C, 1 FINAL, 2 P24L, 3 QUERY16, 4 COEFFS, 5 ROOTS, 6 P2T, 7 SAMPLES, 8 ROWSUM16, 9 ROWS.  40 public values: the capacity, then fa, zeta, zeta g_N,
// YL, YN, YQ, OFFN = fa^W, OFFQ = fa^(2W) -- PUBLIC in this step, as beta was public in the first machine before the transcript came in; the step that brings them in
// over buses is a later one.  The key commits the layer roots, the final coefficients and by query number the opened trace row and quotient row: no reduced opening.
//   FOLD16C  FOLD16B plus the column XQ = X sum_j O_j w_16^bitrev(j, 4) (the query's point without the coset shift; degree 2, zero on a padding row) behind the last
//            column, three unused cells beside it; the send on a chain's first row is (IDX, XQ, OWN[4]) on the same bus
//   QUERY16  where QUERIES stood, one row per query number.  Preprocessed (q, ACT); main the columns of the shard verifier's QUERY chip (IDX XQ RO AT AQ I1 I2 P1 P2 P2O
//            P3 P3O and the seven constants), every constant tied to its public value on every row, the eight product constraints with x = g XQ.  Receives (q, IDX)
//            from SAMPLES, (IDX, XQ, RO) from FOLD16C's first rows, (q, AT) and (q, AQ) from ROWSUM16
//   ROWSUM16 one row per 8 words of an opened row, per query the trace blocks from the last to the first, then the quotient block: V[8] ACCIN[4] T[8][4] FA[4], FA tied
//            to the public values; preprocessed TAG = 2 q + tree, ACT, NOTFIRST, LAST0, LAST1, QN, K0 = 2 block, K1 = K0 + 1.  Sends (TAG, K0, V0..V3) and
//            (TAG, K1, V4..V7) to ROWS, (QN, T_0) to QUERY16 on a trace's block 0 (LAST0) and on the quotient block (LAST1)
//   ROWS     preprocessed (TAG, K, w0..w3, 1): one row per 4-word group of every opened row, the tuple form in which P24L's sponge rows receive theirs.  In THIS
//            machine the Merkle paths of the trace and quotient rows are NOT proven: the ROW-PATHS machine below is this one with the width-24 chip variant P24R
//            on the same bus where ROWS stands here
// STILL OUTSIDE: those paths (proven by the row-paths machine), the transcript before the commit phase (so the eight constants), lookups, the AIR identity.
// tests/fri16_openings_air.py writes it again.
constexpr uint32_t BUS_ROW16 = 81, BUS_AT16 = 82, BUS_AQ16 = 83, N_PUBLIC_O = 40, Q16_PRE = 8, QP_QN = 0, QP_ACT = 1, RS16_PRE = 8, ROWS_PRE16 = 8, QROW16 = 8;
constexpr uint32_t RP_TAG = 0, RP_ACT = 1, RP_NOTFIRST = 2, RP_LAST0 = 3, RP_LAST1 = 4, RP_QN = 5, RP_K0 = 6, RP_K1 = 7;
constexpr uint32_t PUB_FA = 8, PUB_ZETA = 12;       // public values: FA, then ZETA ZNX YL YN YQ OFFN OFFQ in QUERY16's column order

std::vector<uint32_t> build_fold16c_program(int R, int lf, uint32_t n_public = N_PUBLIC_O) {
    const std::vector<uint32_t> p = build_fold16_program(R, lf, true, n_public);
    const uint32_t XQ = fold16_width((uint32_t)lf);
    Builder b;
    b.body.assign(p.begin() + 6, p.end());
    b.count = p[3];
    Terms t{{1u, {var(XQ)}}};
    for (uint32_t j = 0; j < 16; j++) t.push_back(Term{neg(from_monty(fpow(two_adic_generator(4), reverse_bits(j, 4)))), {var(X), var(OF + j)}});
    b.add(ALL, t);
    return b.finish(XQ + 4u, n_public);
}
// QUERY16's columns in the combined row: the shard verifier's QUERY chip's
constexpr uint32_t QC_IDX = Q16_PRE + QM_IDX, QC_XQ = Q16_PRE + QM_XQ, QC_RO = Q16_PRE + QM_RO, QC_AT = QC_RO + 4, QC_AQ = QC_RO + 8, QC_I1 = QC_RO + 12, QC_I2 = QC_RO + 16,
                   QC_P1 = QC_RO + 20, QC_P2 = QC_RO + 24, QC_P2O = QC_RO + 28, QC_P3 = QC_RO + 32, QC_P3O = QC_RO + 36, QC_ZETA = Q16_PRE + QM_ZETA, QC_ZNX = QC_ZETA + 4,
                   QC_YL = QC_ZETA + 8, QC_YN = QC_ZETA + 12, QC_YQ = QC_ZETA + 16, QC_OFFN = QC_ZETA + 20, QC_OFFQ = QC_ZETA + 24;
void query16_products(Builder& b) {      // the eight product constraints with x = g XQ: what QUERY16 and QUERY16H share
    const EE x = eb(pscale(pv(QC_XQ), GEN));
    const Terms act = pv(QP_ACT);
    add_ext(b, ALL, egate(act, esub(emul(esub(x, ev(QC_ZETA)), ev(QC_I1)), eone())));
    add_ext(b, ALL, egate(act, esub(emul(esub(x, ev(QC_ZNX)), ev(QC_I2)), eone())));
    add_ext(b, ALL, esub(ev(QC_P1), emul(esub(ev(QC_AT), ev(QC_YL)), ev(QC_I1))));
    add_ext(b, ALL, esub(ev(QC_P2), emul(esub(ev(QC_AT), ev(QC_YN)), ev(QC_I2))));
    add_ext(b, ALL, esub(ev(QC_P2O), emul(ev(QC_OFFN), ev(QC_P2))));
    add_ext(b, ALL, esub(ev(QC_P3), emul(esub(ev(QC_AQ), ev(QC_YQ)), ev(QC_I1))));
    add_ext(b, ALL, esub(ev(QC_P3O), emul(ev(QC_OFFQ), ev(QC_P3))));
    add_ext(b, ALL, esub(ev(QC_RO), eadd(eadd(ev(QC_P1), ev(QC_P2O)), ev(QC_P3O))));
}
std::vector<uint32_t> build_query16_program() {
    Builder b;
    for (uint32_t i = 0; i < 7; i++) add_ext(b, ALL, esub(ev(QC_ZETA + 4 * i), epub(PUB_ZETA + 4 * i)));
    query16_products(b);
    return b.finish(Q16_PRE + Q16_MAIN, N_PUBLIC_O);
}
// (head: ROWSUM16H -- twelve preprocessed columns, FA one constant down the table, received on the first row, in place of FA = its public value)
std::vector<uint32_t> build_rowsum16_program(uint32_t M0 = RS16_PRE, bool head = false, uint32_t n_public = N_PUBLIC_O) {
    Builder b;
    const EE fa = ev(M0 + RS_FA);
    if (head) add_ext(b, TRANSITION, esub(ev(M0 + RS_FA, true), fa));
    else add_ext(b, ALL, esub(fa, epub(PUB_FA)));
    EE prev = ev(M0 + RS_ACCIN);
    for (int s = 7; s >= 0; s--) {
        const EE cur = ev(M0 + RS_T + 4u * (uint32_t)s);
        add_ext(b, ALL, esub(cur, eadd(emul(prev, fa), eb(pv(M0 + RS_V + (uint32_t)s)))));
        prev = cur;
    }
    add_ext(b, TRANSITION, egate(pv(RP_NOTFIRST, true), esub(ev(M0 + RS_ACCIN, true), ev(M0 + RS_T))));
    add_ext(b, ALL, egate(padd(pv(RP_ACT), pneg(pv(RP_NOTFIRST))), ev(M0 + RS_ACCIN)));
    return b.finish(M0 + RS_MAIN16, n_public);
}
// ROWSUM16's schedule: per query the trace blocks from the last to the first, then the quotient block
void rowsum16_schedule(size_t Q, size_t W, int log_rows, std::vector<uint32_t>& t) {
    const size_t WB = W / 8;
    t.assign((size_t)RS16_PRE << log_rows, 0u);
    size_t r = 0;
    for (size_t q = 0; q < Q; q++)
        for (size_t pos = 0; pos <= WB; pos++) {
            const bool quot = pos == WB;
            const size_t blk = quot ? 0 : WB - 1 - pos;
            uint32_t* w = t.data() + RS16_PRE * r++;
            w[RP_TAG] = to_monty((uint32_t)(2 * q + (quot ? 1 : 0))); w[RP_ACT] = MONTY_R1; w[RP_NOTFIRST] = pos == 0 || quot ? 0u : MONTY_R1;
            w[RP_LAST0] = !quot && blk == 0 ? MONTY_R1 : 0u; w[RP_LAST1] = quot ? MONTY_R1 : 0u; w[RP_QN] = to_monty((uint32_t)q);
            w[RP_K0] = to_monty((uint32_t)(2 * blk)); w[RP_K1] = to_monty((uint32_t)(2 * blk + 1));
        }
}
// the key's tables by table number: the indices machine's (QUERY16's schedule where its QUERIES stood), ROWSUM16's schedule and ROWS -- the rows go in, no reduced opening
int build_openings_key_tables(const Shape& s, const uint32_t* final_poly, const uint32_t* trows, const uint32_t* qrows, const uint32_t* roots, std::vector<uint32_t> pre[],
                              const char* who) {
    const size_t Q = s.Q, W = s.W;
    if (!trows || !qrows) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!canonical(trows, Q * W) || !canonical(qrows, Q * QROW16)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    const std::vector<uint32_t> no_values(4 * Q, 0u);
    ZK_TRY(build_indices_key_tables(s, final_poly, no_values.data(), roots, pre, who));
    pre[T_QUERY16].assign((size_t)Q16_PRE << s.log_rows[T_QUERY16], 0u);
    for (size_t q = 0; q < Q; q++) { pre[T_QUERY16][Q16_PRE * q + QP_QN] = to_monty((uint32_t)q); pre[T_QUERY16][Q16_PRE * q + QP_ACT] = MONTY_R1; }
    rowsum16_schedule(Q, W, s.log_rows[T_ROWSUM16], pre[T_ROWSUM16]);
    pre[T_ROWS].assign((size_t)ROWS_PRE16 << s.log_rows[T_ROWS], 0u);
    size_t g = 0;
    for (size_t q = 0; q < Q; q++) {
        for (int tree = 0; tree < 2; tree++) {
            const uint32_t* row = tree ? qrows + QROW16 * q : trows + W * q;
            for (size_t k = 0; k < (tree ? QROW16 : W) / 4; k++) {
                uint32_t* w = pre[T_ROWS].data() + ROWS_PRE16 * g++;
                w[0] = to_monty((uint32_t)(2 * q + tree)); w[1] = to_monty((uint32_t)k);
                for (int i = 0; i < 4; i++) w[2 + i] = to_monty(row[4 * k + i]);
                w[6] = MONTY_R1;
            }
        }
    }
    return ZKHIP_OK;
}
// the constants among themselves: zeta g_N, fa^W, fa^(2W)
int check_openings_constants(const Shape& s, const uint32_t* consts, const char* who) {
    if (!consts) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!canonical(consts, 32)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    const Ext fa = ext_from_canon(consts), zeta = ext_from_canon(consts + 4);
    if (!ext_eq(ext_from_canon(consts + 8), ext_mul_base(zeta, two_adic_generator(s.H - s.b))) || !ext_eq(ext_from_canon(consts + 24), ext_pow(fa, s.W)) ||
        !ext_eq(ext_from_canon(consts + 28), ext_pow(fa, 2 * (uint64_t)s.W)))
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the constants do not match each other (zeta g_N, OFFN = fa^W, OFFQ = fa^(2W))");
    return ZKHIP_OK;
}

// ---------------------------------------------------------------- the ROW-PATHS machine: the openings machine with the opened rows' Merkle paths proven
// Table numbers as in the openings machine with P24R at 9; the 40 public values stay.  FOLD16C, FINAL, P24L, COEFFS, ROOTS, P2T, SAMPLES and ROWSUM16: the openings
// machine's programs and interaction tables word for word (program_of and interactions_of have no case for this kind there).  The key commits the layer roots, the final coefficients, the trace root
// and the quotient root: NO opened word.
//   ROOTS    key table: two more rows, (LN = R, DEP = H, trace root, LISTED = 0) and (LN = R + 1, DEP = H, quotient root, LISTED = 0) -- not listed: nothing comes from
//            the transcript, and FOLDROWS (1 - LISTED) = 0 keeps them from handing FOLD16C a challenge; their path-end count is the prover's main column
//   QUERY16  program unchanged; preprocessed (q, ACT, TG0 = 2 q, TG1 = 2 q + 1, LN0 = R, LN1 = R + 1); two more sends on BUS_TAG16, (TG0, LN0, IDX) and (TG1, LN1, IDX),
//            multiplicity ACT: which tree a tag belongs to and at which index it is opened (the parity of a tag means nothing in the field)
//   P24R     p24chip.h's row-paths variant, main only: one path per (query, tree), 2 Q paths, none shared; a sponge row receives (TAG, K_i, IN[4 i .. 4 i + 4]) with the
//            multiplicities M0, G1, G2, G3 on ROWSUM16's bus, the SS row (TAG, LNR, IX) from QUERY16, the END row sends (LNR, DEP, digest) in two halves to ROOTS.
//            The leaf's length is pinned by the bus: ROWSUM16's sends are preprocessed, every group (TAG, k) is sent once, and with K_i = 4 BL + i and BL restarting at
//            0 on SS it can be received in block k / 4 of a chain that starts at SS only
// P24R has lg(Q (ceil(W / 16) + 1 + 2 H)) rows, at least 2^6 as ROWS had.  STILL OUTSIDE: the transcript before the commit phase (so the eight constants and where the
// two roots come from), lookups, the AIR identity at zeta.  tests/fri16_rowpaths_air.py writes it again.
constexpr uint32_t BUS_TAG16 = 84, QP_TG0 = 2, QP_TG1 = 3, QP_LN0 = 4, QP_LN1 = 5;
enum : int { MAX_SAME_HEIGHT = 8 };
// the key's tables by table number: the indices machine's, QUERY16's schedule with the tags and tree numbers, ROWSUM16's schedule, the two roots in ROOTS -- no row
int build_rowpaths_key_tables(const Shape& s, const uint32_t* final_poly, const uint32_t* roots, const uint32_t* trace_root, const uint32_t* quotient_root,
                              std::vector<uint32_t> pre[], const char* who) {
    const size_t Q = s.Q, R = (size_t)s.R;
    if (!trace_root || !quotient_root) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!canonical(trace_root, 8) || !canonical(quotient_root, 8)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    const std::vector<uint32_t> no_values(4 * Q, 0u);
    ZK_TRY(build_indices_key_tables(s, final_poly, no_values.data(), roots, pre, who));
    pre[T_QUERY16].assign((size_t)Q16_PRE << s.log_rows[T_QUERY16], 0u);
    for (size_t q = 0; q < Q; q++) {
        uint32_t* w = pre[T_QUERY16].data() + Q16_PRE * q;
        w[QP_QN] = to_monty((uint32_t)q); w[QP_ACT] = MONTY_R1; w[QP_TG0] = to_monty((uint32_t)(2 * q)); w[QP_TG1] = to_monty((uint32_t)(2 * q + 1));
        w[QP_LN0] = to_monty((uint32_t)R); w[QP_LN1] = to_monty((uint32_t)R + 1u);
    }
    for (size_t tree = 0; tree < 2; tree++) {                  // (R + 2 <= 7 rows of 2^5; column 10, LISTED, stays zero)
        uint32_t* w = pre[T_ROOTS].data() + ROOTS_PRE16 * (R + tree);
        w[RT_LN] = to_monty((uint32_t)(R + tree)); w[RT_DEP] = to_monty((uint32_t)s.H);
        for (int j = 0; j < 8; j++) w[RT_ROOT + j] = to_monty((tree ? quotient_root : trace_root)[j]);
    }
    rowsum16_schedule(Q, s.W, s.log_rows[T_ROWSUM16], pre[T_ROWSUM16]);
    pre[T_P24R].clear();
    return ZKHIP_OK;
}

// ---------------------------------------------------------------- the HEAD machine: the row-paths machine with the head of the transcript inside
// Eleven tables, numbered as in the row-paths machine with OPENED16 at 10.  The public values are the NP public values of the inner proof (1 .. 30) and nothing else: no
// capacity word, no constant.  FOLD16C, FINAL, P24L, COEFFS, SAMPLES and P24R: the row-paths machine's programs and interaction tables word for word but the public-value
// count in the header (and the first row number in SAMPLES' key table).  The sponge chain now starts from the ALL-ZERO state and walks, before the commit phase's rows:
//   A = ceil((18 + NP) / 8) rows   the stream (log_n, W, log_blowup, Q, inner_pow_bits, NP, 0, 4, F, 24 | trace root | public values), eight words a row; the last one is
//                                  partial unless 18 + NP is a multiple of 8: its remaining rate words keep the previous output (a sample with pending inputs permutes in
//                                  overwrite mode).  alpha = (out[7], out[6], out[5], out[4]) of row A - 1 -- drawn, and USED BY NOTHING in this machine: the AIR identity at
//                                  zeta is the step that consumes it
//   1 row                          the quotient root; zeta is its output (a sample right after a full block costs no permutation)
//   W + 4 rows                     the 2 W + 8 opened extension values (values at zeta, at zeta g, quotient values: the order the verifier observes them in), two a row;
//                                  fa is the last row's output, and the commit phase continues from that very state
// HD = A + 1 + W + 4 rows in front of the R + C + S rows P2T has in the kinds before.
//   P2TH     P2T's 352 permutation columns and chain constraints; row 0's capacity is ZERO where it was public; preprocessed (64 columns): P2T's twenty, then per rate word
//            a header flag and value (HF_j (IN_j - HV_j) = 0), six public-value indicators (PUBI_i (IN_j - public value 8 i + j - 18) = 0 where row i, word j holds one),
//            per rate word a key and a multiplicity for the receive of a root word from ROOTS (key 8 tree + word; the trace root sits at stream words 10 .. 17: 6 + 2 over
//            rows 1 and 2), a flag OPN for the receive of the row's eight rate words from OPENED16 keyed by the row number, and the multiplicities of the two sends of
//            (out[7], out[6], out[5], out[4]): zeta from the quotient root's row (1: to QUERY16H), fa from the last opened-value row (2: to ROWSUM16H and OPENED16)
//   ROOTS    rows R and R + 1 gain the sends (8 tree + j, root_j) under the preprocessed multiplicity HM, 1 on those two rows only; LISTED stays 0 there
//   OPENED16 one row per opened-value row: V[8] FA FA2 PW T PT Y PWN (fri16_rows.cuh); FA2 = FA FA, T = V0 + FA V1, PT = PW T, PWN = PW FA2 on every row; PW = 1 and Y = PT on
//            a segment's first row; PW' = PWN and Y' = Y + PT' inside a segment; FA' = FA on every transition.  Preprocessed ACT NOTFIRST ROW ENDL ENDN ENDQ FIRST.  Sends
//            the two halves of V to P2TH, Y at the three segment ends as YL YN YQ, PWN at the end of the first as OFFN = fa^W; receives fa on its first row
//   QUERY16H QUERY16 with every constant one value down the table (c' = c) and received on the first row (ZETA YL YN YQ OFFN), ZNX = g_N ZETA, OFFQ = OFFN OFFN
//   ROWSUM16H ROWSUM16 with FA' = FA and fa received on the first row (twelve preprocessed columns: the first-row multiplicity needs one)
// Every multiplicity of the head is preprocessed.  The key holds roots, final coefficients and header constants: no opened word, no constant, no challenge.  NP = 0 is
// refused (a keyed machine without public values is not something any test here has carried), NP > 30 too (six indicator columns).
// STILL OUTSIDE: the AIR identity at zeta (alpha unused), lookups, version-7 and version-8 inner proofs, roots leaving the key, the wiring into shard_verifier.inl.
// tests/fri16_head_air.py writes it again.
constexpr uint32_t BUS_HR = 85, BUS_OV0 = 86, BUS_OV1 = 87, BUS_ZETA = 88, BUS_FAH = 89, BUS_YL = 90, BUS_YN = 91, BUS_YQ = 92, BUS_OFFN = 93, MAX_NP = 30;
constexpr uint32_t PTH_PRE = 64, PH_HF = 20, PH_HV = 28, PH_PUBI = 36, PH_RK = 42, PH_RM = 50, PH_OPN = 58, PH_ZM = 59, PH_FM = 60, HEAD_STREAM = 18;
constexpr uint32_t ROOTS_PRE_H = 20, RT_HM = 11, RT_HK = 12, QP_FIRST = 6, RS16H_PRE = 12, RP_FIRST = 8;
constexpr uint32_t OPN_PRE = 8, OQ_ACT = 0, OQ_NOTFIRST = 1, OQ_ROW = 2, OQ_ENDL = 3, OQ_ENDN = 4, OQ_ENDQ = 5, OQ_FIRST = 6;
// the ten header words: transcript_init for a version-3 proof (sh.ext, no program, no code group, no lookup pairs)
void head_header(const Shape& s, uint32_t h[10]) {
    const uint32_t w[10] = {(uint32_t)(s.H - s.b), s.W, (uint32_t)s.b, (uint32_t)s.Q, (uint32_t)s.pow_bits, s.NP, 0u, 4u, (uint32_t)s.F, 24u};
    std::memcpy(h, w, sizeof w);
}
std::vector<uint32_t> build_p2th_program(const Shape& s) {
    using namespace p2chip;
    const uint32_t M0 = PTH_PRE, OUT = M0 + oute(7);
    Builder b;
    b.body = permutation_body(M0, &b.count);
    for (uint32_t j = 0; j < 8; j++) b.add(ALL, Terms{{1u, {var(M0 + D + j)}}, {P - 1, {var(M0 + IN + j)}}});
    b.add(ALL, Terms{{1u, {var(M0 + BIT)}}});
    for (uint32_t j = 0; j < 8; j++) b.add(FIRST, Terms{{1u, {var(M0 + IN + 8 + j)}}});
    for (uint32_t j = 0; j < 8; j++) b.add(TRANSITION, Terms{{1u, {var(PT_SPG, true), var(M0 + IN + 8 + j, true)}}, {P - 1, {var(PT_SPG, true), var(OUT + 8 + j)}}});
    for (uint32_t j = 0; j < 8; j++) b.add(TRANSITION, Terms{{1u, {var(PT_K + j, true), var(M0 + IN + j, true)}}, {P - 1, {var(PT_K + j, true), var(OUT + j)}}});
    for (uint32_t j = 0; j < 8; j++) b.add(ALL, Terms{{1u, {var(PH_HF + j), var(M0 + IN + j)}}, {P - 1, {var(PH_HF + j), var(PH_HV + j)}}});
    for (uint32_t i = 0; i < (uint32_t)s.A; i++)
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t pos = 8 * i + j;
            if (pos < HEAD_STREAM || pos >= HEAD_STREAM + s.NP) continue;
            b.add(ALL, Terms{{1u, {var(PH_PUBI + i), var(M0 + IN + j)}}, {P - 1, {var(PH_PUBI + i), pub(pos - HEAD_STREAM)}}});
        }
    return b.finish(PTH_PRE + T_WIDTH, s.NP);
}
std::vector<uint32_t> build_query16h_program(const Shape& s) {
    Builder b;
    for (uint32_t i = 0; i < 7; i++) add_ext(b, TRANSITION, esub(ev(QC_ZETA + 4 * i, true), ev(QC_ZETA + 4 * i)));
    add_ext(b, ALL, esub(ev(QC_ZNX), escale(ev(QC_ZETA), from_monty(two_adic_generator(s.H - s.b)))));
    add_ext(b, ALL, esub(ev(QC_OFFQ), emul(ev(QC_OFFN), ev(QC_OFFN))));
    query16_products(b);
    return b.finish(Q16_PRE + Q16_MAIN, s.NP);
}
std::vector<uint32_t> build_opened16_program(uint32_t n_public, uint32_t M0 = OPN_PRE) {      // (the identity machine's OPENED16 has four more preprocessed columns)
    Builder b;
    const EE fa = ev(M0 + OP_FA), fa2 = ev(M0 + OP_FA2), pw = ev(M0 + OP_PW), t = ev(M0 + OP_T), pt = ev(M0 + OP_PT), y = ev(M0 + OP_Y), pwn = ev(M0 + OP_PWN);
    add_ext(b, ALL, esub(fa2, emul(fa, fa)));
    add_ext(b, ALL, esub(t, eadd(ev(M0 + OP_V), emul(fa, ev(M0 + OP_V + 4)))));
    add_ext(b, ALL, esub(pt, emul(pw, t)));
    add_ext(b, ALL, esub(pwn, emul(pw, fa2)));
    const Terms seg_first = padd(pv(OQ_ACT), pneg(pv(OQ_NOTFIRST)));
    add_ext(b, ALL, egate(seg_first, esub(pw, eone())));
    add_ext(b, ALL, egate(seg_first, esub(y, pt)));
    add_ext(b, TRANSITION, egate(pv(OQ_NOTFIRST, true), esub(ev(M0 + OP_PW, true), pwn)));
    add_ext(b, TRANSITION, egate(pv(OQ_NOTFIRST, true), esub(ev(M0 + OP_Y, true), eadd(y, ev(M0 + OP_PT, true)))));
    add_ext(b, TRANSITION, esub(ev(M0 + OP_FA, true), fa));
    return b.finish(M0 + OP_MAIN16, n_public);
}
int shape_of(const ShapeArgs& a, Shape& s);
// the key's tables by table number: the row-paths machine's at the head machine's widths, the head's schedule in front of P2T's, OPENED16's schedule -- functions of the
// shape and NP alone but for the roots and the final coefficients
int build_head_key_tables(const Shape& s, const uint32_t* final_poly, const uint32_t* roots, const uint32_t* trace_root, const uint32_t* quotient_root, std::vector<uint32_t> pre[],
                          const char* who) {
    Shape so;                                                  // the kinds before, at their own widths (the openings shape: no shape of the head's is refused for its heights)
    ZK_TRY(shape_of({OPENINGS, s.R, s.F, s.b, s.Q, s.pow_bits, s.W}, so));
    std::vector<uint32_t> t[MAX_TABLES];
    ZK_TRY(build_rowpaths_key_tables(so, final_poly, roots, trace_root, quotient_root, t, who));
    const size_t R = (size_t)s.R, W = s.W;
    for (int i = 0; i < s.n_tables; i++) pre[i].assign((size_t)s.pre_w[i] << s.log_rows[i], 0u);
    pre[T_FINAL] = t[T_FINAL]; pre[T_COEFFS] = t[T_COEFFS]; pre[T_QUERY16] = t[T_QUERY16];
    pre[T_QUERY16][QP_FIRST] = MONTY_R1;
    for (size_t r = 0; r < ((size_t)1 << s.log_rows[T_ROOTS]); r++) std::memcpy(pre[T_ROOTS].data() + ROOTS_PRE_H * r, t[T_ROOTS].data() + ROOTS_PRE16 * r, 4 * ROOTS_PRE16);
    for (size_t tree = 0; tree < 2; tree++) {
        uint32_t* w = pre[T_ROOTS].data() + ROOTS_PRE_H * (R + tree);
        w[RT_HM] = MONTY_R1;
        for (uint32_t j = 0; j < 8; j++) w[RT_HK + j] = to_monty((uint32_t)(8 * tree + j));
    }
    for (size_t r = 0; r < ((size_t)1 << s.log_rows[T_ROWSUM16]); r++) std::memcpy(pre[T_ROWSUM16].data() + RS16H_PRE * r, t[T_ROWSUM16].data() + RS16_PRE * r, 4 * RS16_PRE);
    pre[T_ROWSUM16][RP_FIRST] = MONTY_R1;
    uint32_t hdr[10];
    head_header(s, hdr);
    for (size_t r = 0; r < s.HD; r++) {
        uint32_t* w = pre[T_P2T].data() + PTH_PRE * r;
        if (r) w[PT_SPG] = MONTY_R1;
        if (r < s.A) {
            for (uint32_t j = 0; j < 8; j++) {
                const size_t pos = 8 * r + j;
                if (pos >= HEAD_STREAM + s.NP) w[PT_K + j] = MONTY_R1;
                else if (pos < 10) { w[PH_HF + j] = MONTY_R1; w[PH_HV + j] = to_monty(hdr[pos]); }
                else if (pos < HEAD_STREAM) { w[PH_RK + j] = to_monty((uint32_t)(pos - 10)); w[PH_RM + j] = MONTY_R1; }
                else w[PH_PUBI + r] = MONTY_R1;
            }
        } else if (r == s.A) {
            for (uint32_t j = 0; j < 8; j++) { w[PH_RK + j] = to_monty(8u + j); w[PH_RM + j] = MONTY_R1; }
            w[PH_ZM] = MONTY_R1;
        } else {
            w[PH_OPN] = MONTY_R1; w[PT_ROW] = to_monty((uint32_t)r);
            if (r + 1 == s.HD) w[PH_FM] = to_monty(2u);
        }
    }
    for (size_t r = 0; r < s.NT; r++) {
        uint32_t* w = pre[T_P2T].data() + PTH_PRE * (s.HD + r);
        std::memcpy(w, t[T_P2T].data() + PT_PRE * r, 4 * PT_PRE);
        w[PT_SPG] = MONTY_R1;
        if (w[PT_SMP]) w[PT_ROW] = to_monty((uint32_t)(s.HD + r));
    }
    frichip::samples_chip_pre(s.Q, s.log_rows[T_SAMPLES], (int)(s.HD + R + s.C), pre[T_SAMPLES]);
    for (size_t i = 0; i < W + 4; i++) {
        uint32_t* w = pre[T_OPENED16].data() + (size_t)s.pre_w[T_OPENED16] * i;
        const size_t first = i < W / 2 ? 0 : (i < W ? W / 2 : W);
        w[OQ_ACT] = MONTY_R1; w[OQ_NOTFIRST] = i != first ? MONTY_R1 : 0u; w[OQ_ROW] = to_monty((uint32_t)(s.A + 1 + i));
        w[OQ_ENDL] = i + 1 == W / 2 ? MONTY_R1 : 0u; w[OQ_ENDN] = i + 1 == W ? MONTY_R1 : 0u; w[OQ_ENDQ] = i == W + 3 ? MONTY_R1 : 0u; w[OQ_FIRST] = i == 0 ? MONTY_R1 : 0u;
    }
    pre[T_P24R].clear();
    return ZKHIP_OK;
}
// the head of the chain walked on the host (HD permutations): every row's input state, the three challenges and the capacity the commit phase finds -- canonical
struct Head { std::vector<uint32_t> inputs; uint32_t alpha[4], zeta[4], fa[4], capacity[8]; };
void walk_head(const Shape& s, const uint32_t* inner_public, const uint32_t* trace_root, const uint32_t* quotient_root, const uint32_t* opened, Head& h) {
    std::vector<uint32_t> stream(HEAD_STREAM + s.NP);
    head_header(s, stream.data());
    std::memcpy(stream.data() + 10, trace_root, 32);
    std::memcpy(stream.data() + HEAD_STREAM, inner_public, 4 * (size_t)s.NP);
    h.inputs.assign(16 * s.HD, 0u);
    uint32_t st[16] = {0};
    size_t r = 0;
    auto step = [&]() { for (int j = 0; j < 16; j++) h.inputs[16 * r + j] = from_monty(st[j]); r++; p2_permute(st); };
    for (size_t i = 0; i < s.A; i++) {
        for (size_t j = 0; j < 8 && 8 * i + j < stream.size(); j++) st[j] = to_monty(stream[8 * i + j]);
        step();
    }
    for (int j = 0; j < 4; j++) h.alpha[j] = from_monty(st[7 - j]);
    for (int j = 0; j < 8; j++) st[j] = to_monty(quotient_root[j]);
    step();
    for (int j = 0; j < 4; j++) h.zeta[j] = from_monty(st[7 - j]);
    for (size_t i = 0; i < (size_t)s.W + 4; i++) {
        for (int j = 0; j < 8; j++) st[j] = to_monty(opened[8 * i + j]);
        step();
    }
    for (int j = 0; j < 4; j++) h.fa[j] = from_monty(st[7 - j]);
    for (int j = 0; j < 8; j++) h.capacity[j] = from_monty(st[8 + j]);
}
// the eight constants from the head's challenges and the four sums the OPENED16 launch leaves (YL YN YQ OFFN, canonical): zeta g_N and OFFQ = OFFN^2 on the host
void head_constants(const Shape& s, const Head& h, const uint32_t sums[16], uint32_t consts[32]) {
    std::memcpy(consts, h.fa, 16); std::memcpy(consts + 4, h.zeta, 16);
    const Ext znx = ext_mul_base(ext_from_canon(h.zeta), two_adic_generator(s.H - s.b)), offn = ext_from_canon(sums + 12), offq = ext_mul(offn, offn);
    for (int i = 0; i < 4; i++) { consts[8 + i] = from_monty(znx.c[i]); consts[28 + i] = from_monty(offq.c[i]); }
    std::memcpy(consts + 12, sums, 48); std::memcpy(consts + 24, sums + 12, 16);
}

// ---------------------------------------------------------------- the IDENTITY machine: the head machine with the AIR identity at zeta inside
// Thirteen tables: the head machine's eleven, AIR16 at 11, SCALARS16 at 12.  The public values stay the inner proof's.  What it states beside the head machine's
// statement is (a) of verify_shard_impl (verifier.cpp) for air == nullptr, LQ == 0, lqd = 1: with G = W / 4 groups a, b, c, d = loc[4 g .. 4 g + 3], dn = nxt[4 g + 3],
//     c1 = c - a^2 b - (g + 1),  c2 = sel_trans (dn - a b - c - (2 g + 3)),  c3 = sel_first (d - (5 g + 7)),  acc <- ((acc alpha + c1) alpha + c2) alpha + c3 from 0,
//     sel_trans = zeta - 1 / g_N,  sel_first = (zeta^N - 1) / (zeta - 1),  quot = sum_{k < 2} (a_k zeta^N + b_k) sum_e X^e opq[4 k + e]  (airb::zps_consts),
//     acc = quot (zeta^N - 1)
// with alpha, zeta and the opened values the ones the transcript chain itself draws and absorbs.
//   AIR16     one row per group, max(6, lg G) log-rows.  Preprocessed (12): ACT FIRST NOTFIRST LAST, K1 = g + 1, K2 = 2 g + 3, K3 = 5 g + 7, the three OPENED16 row keys
//             it reads (A + 1 + 2 g, A + 1 + 2 g + 1, A + 1 + W / 2 + 2 g + 1), two unused.  Main A B C D DN ALPHA SELT SELF A2 AB ACCIN U1 U2 ACCO (fri16_rows.cuh); the
//             constraints are the non-air tail of the shard verifier's OPENED chip (shard_verifier.inl: opened_program).  Receives A, C on the first-half bus and B, D, DN
//             on the second-half bus under their row keys, ALPHA SELT SELF on its first row; sends ACCO on its LAST row.  An all-zero row satisfies it and moves nothing
//   SCALARS16 2^7 rows, ONE row repeated (c' = c for every column: (zeta - 1) INVF = 1 has no all-zero row).  Preprocessed (8): FIRST, the four quotient rows' keys.
//             Main ALPHA ZETA ZP_1 .. ZP_n INVF SELF SELT QZ_0 .. QZ_7 QK0 QK1 QUO ACC; the matching lines of the shard verifier's SCALARS chip (scalars_program).
//             On its first row: receives alpha and zeta from P2TH, the eight quotient values from OPENED16, ACC from AIR16; sends ALPHA SELT SELF to AIR16.
//             The program depends on n = H - b
//   P2TH      one more send, alpha = (out[7 .. 4]) of row A - 1, multiplicity in preprocessed column 61; zeta's multiplicity is 2 in this key (QUERY16H and SCALARS16)
//   OPENED16  twelve preprocessed columns: H0 (column 8; 1 on loc and quotient rows) and H1 (column 9; those and the odd nxt rows) are the multiplicities of two more
//             sends, (ROW, V[0 .. 3]) and (ROW, V[4 .. 7])
// STILL OUTSIDE: lookups, version-7 and version-8 inner proofs, roots leaving the key, the wiring into shard_verifier.inl.  tests/fri16_identity_air.py writes it again.
constexpr uint32_t BUS_OH0 = 94, BUS_OH1 = 95, BUS_ALPHA = 96, BUS_KA16 = 97, BUS_KSELT = 98, BUS_KSELF = 99, BUS_ACC16 = 100;
constexpr uint32_t PH_AM = 61, OPN_PRE_I = 12, OQ_H0 = 8, OQ_H1 = 9;
constexpr uint32_t AIR16_PRE = 12, AP_ACT = 0, AP_FIRST = 1, AP_NOTFIRST = 2, AP_LAST = 3, AP_K1 = 4, AP_K2 = 5, AP_K3 = 6, AP_KL0 = 7, AP_KL1 = 8, AP_KN1 = 9;
constexpr uint32_t SC16_PRE = 8, SP_FIRST = 0, SP_KQ = 1;
std::vector<uint32_t> build_air16_program(uint32_t n_public) {
    const uint32_t M0 = AIR16_PRE;
    Builder b;
    auto e = [&](uint32_t col, bool nxt = false) { return ev(M0 + col, nxt); };
    const Terms first = pv(AP_FIRST), nf = pv(AP_NOTFIRST, true);
    for (uint32_t c : {AI_ALPHA, AI_SELT, AI_SELF}) add_ext(b, TRANSITION, egate(nf, esub(e(c, true), e(c))));
    add_ext(b, ALL, esub(e(AI_A2), emul(e(AI_A), e(AI_A))));
    add_ext(b, ALL, esub(e(AI_AB), emul(e(AI_A), e(AI_B))));
    const EE al = e(AI_ALPHA);
    add_ext(b, ALL, egate(first, e(AI_ACCIN)));
    add_ext(b, ALL, esub(e(AI_U1), eadd(emul(e(AI_ACCIN), al), esub(esub(e(AI_C), emul(e(AI_A2), e(AI_B))), eb(pv(AP_K1))))));
    add_ext(b, ALL, esub(e(AI_U2), eadd(emul(e(AI_U1), al), emul(e(AI_SELT), esub(esub(esub(e(AI_DN), e(AI_AB)), e(AI_C)), eb(pv(AP_K2)))))));
    add_ext(b, ALL, esub(e(AI_ACCO), eadd(emul(e(AI_U2), al), emul(e(AI_SELF), esub(e(AI_D), eb(pv(AP_K3)))))));
    add_ext(b, TRANSITION, egate(nf, esub(e(AI_ACCIN, true), e(AI_ACCO))));
    return b.finish(AIR16_PRE + AIR_MAIN16, n_public);
}
std::vector<uint32_t> build_scalars16_program(const Shape& s) {
    const uint32_t M0 = SC16_PRE, n = (uint32_t)(s.H - s.b), c = M0 + sc16_invf(n), INVF = c, SELF = c + 4, SELT = c + 8, QZ = c + 12, QK0 = c + 44, QK1 = c + 48, QUO = c + 52, ACC = c + 56;
    Builder b;
    const EE zeta = ev(M0 + SC_ZETA);
    EE prev = zeta;
    for (uint32_t i = 0; i < n; i++) { add_ext(b, ALL, esub(ev(M0 + SC_ZP + 4 * i), emul(prev, prev))); prev = ev(M0 + SC_ZP + 4 * i); }
    const EE znn = prev;
    add_ext(b, ALL, esub(emul(esub(zeta, ec(1)), ev(INVF)), ec(1)));
    add_ext(b, ALL, esub(ev(SELF), emul(esub(znn, ec(1)), ev(INVF))));
    add_ext(b, ALL, esub(ev(SELT), esub(zeta, ec(from_monty(finv(two_adic_generator((int)n)))))));
    for (int k = 0; k < 2; k++) {
        EE q = ec(0);
        for (int t = 0; t < 4; t++) {
            uint64_t basis[4] = {0, 0, 0, 0};
            basis[t] = 1;
            q = eadd(q, emul(ec(basis[0], basis[1], basis[2], basis[3]), ev(QZ + 4u * (uint32_t)(4 * k + t))));
        }
        add_ext(b, ALL, esub(ev(k ? QK1 : QK0), q));
    }
    uint32_t za[2], zb[2];
    zps_consts((int)n, za, zb);
    const EE z0 = eadd(escale(znn, za[0]), ec(zb[0])), z1 = eadd(escale(znn, za[1]), ec(zb[1]));
    add_ext(b, ALL, esub(ev(QUO), eadd(emul(z0, ev(QK0)), emul(z1, ev(QK1)))));
    add_ext(b, ALL, esub(ev(ACC), emul(ev(QUO), esub(znn, ec(1)))));
    for (uint32_t col = M0; col < M0 + sc16_width(n); col += 4) add_ext(b, TRANSITION, esub(ev(col, true), ev(col)));      // every row behind row 0 repeats row 0
    return b.finish(M0 + sc16_width(n), s.NP);
}
// the key's tables by table number: the head machine's (alpha's multiplicity, zeta's second receiver, OPENED16's two half-row multiplicities) and the schedules of AIR16
// and SCALARS16 -- functions of the shape and NP alone but for the roots and the final coefficients
int build_identity_key_tables(const Shape& s, const uint32_t* final_poly, const uint32_t* roots, const uint32_t* trace_root, const uint32_t* quotient_root, std::vector<uint32_t> pre[],
                              const char* who) {
    ZK_TRY(build_head_key_tables(s, final_poly, roots, trace_root, quotient_root, pre, who));
    const size_t W = s.W, G = W / 4, row0 = s.A + 1;
    pre[T_P2T][PTH_PRE * (s.A - 1) + PH_AM] = MONTY_R1;
    pre[T_P2T][PTH_PRE * s.A + PH_ZM] = to_monty(2u);
    for (size_t i = 0; i < W + 4; i++) {
        uint32_t* w = pre[T_OPENED16].data() + OPN_PRE_I * i;
        const bool whole = i < W / 2 || i >= W;                                    // loc and quotient rows
        w[OQ_H0] = whole ? MONTY_R1 : 0u; w[OQ_H1] = whole || ((i - W / 2) & 1) ? MONTY_R1 : 0u;
    }
    for (size_t g = 0; g < G; g++) {
        uint32_t* w = pre[T_AIR16].data() + AIR16_PRE * g;
        w[AP_ACT] = MONTY_R1; w[AP_FIRST] = g == 0 ? MONTY_R1 : 0u; w[AP_NOTFIRST] = g ? MONTY_R1 : 0u; w[AP_LAST] = g + 1 == G ? MONTY_R1 : 0u;
        w[AP_K1] = to_monty((uint32_t)g + 1u); w[AP_K2] = to_monty(2u * (uint32_t)g + 3u); w[AP_K3] = to_monty(5u * (uint32_t)g + 7u);
        w[AP_KL0] = to_monty((uint32_t)(row0 + 2 * g)); w[AP_KL1] = to_monty((uint32_t)(row0 + 2 * g + 1)); w[AP_KN1] = to_monty((uint32_t)(row0 + W / 2 + 2 * g + 1));
    }
    pre[T_SCALARS16][SP_FIRST] = MONTY_R1;
    for (uint32_t i = 0; i < 4; i++) pre[T_SCALARS16][SP_KQ + i] = to_monty((uint32_t)(row0 + W) + i);
    return ZKHIP_OK;
}

// ---------------------------------------------------------------- the LIFT machine: the identity machine with the roots and the final coefficients OUT of the key
// The identity machine's thirteen tables, heights, inner proofs and public values.  What changes: ROOTS' eight root words are MAIN columns 8 .. 15 (ENDS BETA[4] FOLDROWS
// and the two spare columns stay in front of them), on the R layer rows and on the two tree rows; the tuples of BUS_RT0 / RT1, BUS_TR0 / TR1 and BUS_HR read them there.
// LN, DEP, LISTED, HM and the HK keys stay preprocessed; preprocessed column 2, where root word 0 stood, is ACT (1 on rows 0 .. R + 1) and columns 3 .. 9 are zero;
// ENDS (1 - ACT) = 0 keeps a padding row, whose digest is now free, from receiving a path end.  COEFFS' c_j are MAIN columns 4 .. 7 behind its four unused ones; j, the
// multiplicity Q of the send to FINAL and the multiplicity 1 of the send to P2T stay preprocessed, columns 1 .. 4 are zero.  Both first-row identities name a spare
// column, not a moved word.  Every multiplicity that gates a tuple with a moved word is preprocessed or constrained (DESIGN.md 3c has the table), and Fiat-Shamir pins
// the values: the chain starts from zero and absorbs every root and coefficient over a bus.  So the key is a function of the SHAPE and NP alone: it states "some valid
// segment proof of this shape with THESE public values exists".
// (The JOIN of several lift proofs and the lift BATCH over the lock-step lanes are at the end of this file.)  STILL OUTSIDE: lookups, version-7 and version-8 inner proofs, the
// wiring into shard_verifier.inl.  tests/fri16_lift_air.py writes it again.
int build_lift_key_tables(const Shape& s, std::vector<uint32_t> pre[], const char* who) {
    const std::vector<uint32_t> no_coeffs((size_t)4 << s.F, 0u), no_roots(8 * (size_t)s.R, 0u);
    const uint32_t no_root[8] = {0};
    ZK_TRY(build_identity_key_tables(s, no_coeffs.data(), no_roots.data(), no_root, no_root, pre, who));
    for (size_t r = 0; r < (size_t)s.R + 2; r++) pre[T_ROOTS][ROOTS_PRE_H * r + RT_ROOT] = MONTY_R1;      // ACT
    return ZKHIP_OK;
}

// ---------------------------------------------------------------- the one description: shape, programs, interaction tables, machine, and what every entry does with them
constexpr int N_TABLES[8] = {5, 6, 8, 10, 10, 11, 13, 13};
inline uint32_t n_public_of(const Shape& s) { return s.kind <= PATHS ? 4u * (uint32_t)s.R : s.kind == INDICES ? N_PUBLIC_I : s.kind >= HEAD ? s.NP : N_PUBLIC_O; }

// pow_bits is read from INDICES on, W from OPENINGS on.  ROWSUM16, ROWS and P24R have at least 2^6 rows: a keyed machine takes at most 8 tables of one height, and the
// other eight can all have 2^5 rows; from 2^6 rows on ROOTS (2^5 always) and SAMPLES (fewer rows than QUERY16 / 4) keep nine tables from meeting where ROWS stands --
// P24R can still meet eight others, and that shape is refused
int shape_of(const ShapeArgs& a, Shape& s) {
    const auto [kind, R, F, b, Q, pow_bits, W, NP] = a;
    if (R < 1 || R > MAX_R || F < 0 || F > MAX_F || b < 1 || b > 3 || F + b > MAX_LF || Q < 1 || Q > MAX_Q || 4 * R + F + b > TWO_ADICITY)
        return fail(ZKHIP_ERR_INVALID, "fri16: 1..5 layers, log_final 0..8, log_blowup 1..3 (log_final + log_blowup <= 11), 1..1024 queries, and a domain of at most 2^27 points");
    if (kind >= INDICES && (pow_bits < 0 || pow_bits > 30)) return fail(ZKHIP_ERR_INVALID, "fri16 indices: inner_pow_bits in [0, 30]");
    if (kind >= OPENINGS && (W < 8 || W > MAX_OPEN_W || W % 8))
        return fail(ZKHIP_ERR_INVALID, "fri16 openings: a trace width of 8 .. 1024 in multiples of 8 (inner proofs without lookup pairs and with a quotient row of 8 words)");
    if (kind >= HEAD && (NP < 1 || NP > MAX_NP))
        return fail(ZKHIP_ERR_INVALID, "fri16 head: 1 .. 30 inner public values (the machine's public values are the inner proof's: none cannot be carried, and P2TH has six indicator columns)");
    s = Shape{};
    s.kind = kind; s.R = R; s.F = F; s.b = b; s.lf = F + b; s.H = 4 * R + s.lf; s.Q = Q; s.n_tables = N_TABLES[kind];
    if (kind >= INDICES) { s.pow_bits = pow_bits; s.C = F >= 1 ? (size_t)1 << (F - 1) : 0; s.S = frichip::samples_chip_rows(Q); s.NT = (size_t)R + s.C + s.S; }
    if (kind >= OPENINGS) s.W = W;
    if (kind >= HEAD) { s.NP = NP; s.A = (HEAD_STREAM + NP + 7) / 8; s.HD = s.A + 1 + (size_t)W + 4; }
    size_t layer_paths = 0;                                      // rows of P24L per query: every layer's leaf and path
    for (int l = 0; l < R; l++) layer_paths += (size_t)p24chip::LEAF_ROWS + (size_t)(s.H - 4 * (l + 1));
    const size_t row_paths = (size_t)(W + 15) / 16 + 1 + 2 * (size_t)s.H;      // rows of P24R per query: the two leaves and the two paths
    auto table = [&](int t, int log_rows, uint32_t main_w, uint32_t pre_w) { s.log_rows[t] = log_rows; s.main_w[t] = main_w; s.pre_w[t] = pre_w; };
    table(T_FOLD16, lg(Q * (size_t)R), fold16_width((uint32_t)s.lf) + (kind >= OPENINGS ? 4u : 0u), 0u);
    table(T_FINAL, lg(Q << F), FIN_MAIN, FIN_PRE);
    if (kind == LAYERS) table(T_LAYERS, lg(Q * (size_t)R), TAB_MAIN, LAY_PRE);
    else table(T_P24L, lg(Q * layer_paths), p24chip::WIDTH_L, 0u);
    if (kind < OPENINGS) table(T_QUERIES, lg(Q), TAB_MAIN, Q_PRE);
    else table(T_QUERY16, lg(Q), Q16_MAIN, Q16_PRE);
    table(T_COEFFS, lg((size_t)1 << F), kind == LIFT ? COEFFS_MAIN_L : TAB_MAIN, C_PRE);
    table(T_ROOTS, lg((size_t)R), kind == LIFT ? ROOTS_MAIN_L : kind >= INDICES ? ROOTS_MAIN_I : TAB_MAIN, kind >= HEAD ? ROOTS_PRE_H : ROOTS_PRE16);
    table(T_P2T, lg(s.HD + s.NT), p2chip::T_WIDTH, kind >= HEAD ? PTH_PRE : PT_PRE);
    table(T_SAMPLES, lg(s.S), frichip::S_MAIN, frichip::S_PRE);
    table(T_ROWSUM16, std::max(6, lg(Q * (size_t)(W / 8 + 1))), RS_MAIN16, kind >= HEAD ? RS16H_PRE : RS16_PRE);
    if (kind == OPENINGS) table(T_ROWS, std::max(6, lg(Q * (size_t)(W + QROW16) / 4)), TAB_MAIN, ROWS_PRE16);
    else table(T_P24R, std::max(6, lg(Q * row_paths)), p24chip::WIDTH_R, 0u);
    table(T_OPENED16, std::max(6, lg((size_t)W + 4)), OP_MAIN16, kind >= IDENTITY ? OPN_PRE_I : OPN_PRE);
    // (IDENTITY: the floors 2^6 and 2^7 keep AIR16 and SCALARS16 from making nine tables of one height where the head machine has eight of 2^5)
    table(T_AIR16, std::max(6, lg((size_t)W / 4)), AIR_MAIN16, AIR16_PRE);
    table(T_SCALARS16, (int)SC16_LOG_ROWS, sc16_width((uint32_t)(s.H - s.b)), SC16_PRE);
    for (int t = 0; kind >= ROWPATHS && t < s.n_tables; t++)          // (below ROWPATHS the floors above keep nine tables from meeting)
        if (std::count(s.log_rows, s.log_rows + s.n_tables, s.log_rows[t]) > MAX_SAME_HEIGHT)
            return fail(ZKHIP_ERR_INVALID, std::string(kind == LIFT ? "fri16 lift" : kind == IDENTITY ? "fri16 identity" : kind == HEAD ? "fri16 head" : "fri16 rowpaths") + ": nine tables of this shape have 2^" + std::to_string(s.log_rows[t]) + " rows; a keyed machine takes at most 8 tables of one height");
    return ZKHIP_OK;
}

// the program of table t: per table, from which kind on it is which chip
std::vector<uint32_t> program_of(const Shape& s, int t) {
    const Kind k = s.kind;
    const uint32_t np = n_public_of(s);
    switch (t) {
    case T_FOLD16: return k >= OPENINGS ? build_fold16c_program(s.R, s.lf, np) : build_fold16_program(s.R, s.lf, k >= INDICES, np);
    case T_FINAL: return build_final_program(np);
    case T_P24L: if (k >= PATHS) return *p24chip::program_fri16_layers(np); break;                                 // (LAYERS: a key table)
    case T_QUERY16: if (k >= OPENINGS) return k >= HEAD ? build_query16h_program(s) : build_query16_program(); break;                                     // (below: QUERIES, a key table)
    case T_ROOTS: if (k >= INDICES) return build_roots_program(np, s.pre_w[T_ROOTS], k == LIFT); break;                                        // (PATHS: a key table)
    case T_P2T: return k >= HEAD ? build_p2th_program(s) : build_p2t_program(np);
    case T_SAMPLES: return *frichip::samples_chip_program(s.H, s.pow_bits, np);
    case T_ROWSUM16: return k >= HEAD ? build_rowsum16_program(RS16H_PRE, true, np) : build_rowsum16_program();
    case T_P24R: if (k >= ROWPATHS) return *p24chip::program_fri16_rows(np); break;                               // (OPENINGS: ROWS, a key table)
    case T_OPENED16: return build_opened16_program(np, s.pre_w[T_OPENED16]);
    case T_AIR16: return build_air16_program(np);
    case T_SCALARS16: return build_scalars16_program(s);
    case T_COEFFS: if (k == LIFT) return build_table_program(np, C_PRE, COEFFS_MAIN_L, CL_C - 1u); break;          // (below: the last of four unused columns is the last column)
    default: break;
    }
    return build_table_program(np, s.pre_w[t], s.main_w[t]);
}

// the interaction table of table t: per table, what each kind adds to or changes in the kind before it -- the ORDER of the entries is part of the words
std::vector<uint32_t> interactions_of(const Shape& s, int t) {
    if (t == T_SAMPLES) return frichip::samples_chip_interactions();
    const Kind k = s.kind;
    const uint32_t R = (uint32_t)s.R, XQ = fold16_width((uint32_t)s.lf), RM = s.pre_w[T_ROOTS], in = s.pre_w[T_P2T] + p2chip::IN, o = s.pre_w[T_P2T] + p2chip::oute(7),
                   rv = s.pre_w[T_ROWSUM16] + RS_V, rt = s.pre_w[T_ROWSUM16] + RS_T, rfa = s.pre_w[T_ROWSUM16] + RS_FA;
    Interactions v;
    switch (t) {
    case T_FOLD16:
        for (uint32_t j = 0; j < 16; j++) v.add(0u, ACTIVE, BUS_L16, {LN, KJ + j, E + 4 * j, E + 4 * j + 1, E + 4 * j + 2, E + 4 * j + 3});
        if (k < OPENINGS) v.add(0u, L, BUS_Q16, {IDX, OWN, OWN + 1, OWN + 2, OWN + 3});
        else v.add(0u, L, BUS_Q16, {IDX, XQ, OWN, OWN + 1, OWN + 2, OWN + 3});                                     // FOLD16C: the query's point goes with it
        v.add(0u, L + R - 1u, BUS_FIN16, {X16, FOLD, FOLD + 1, FOLD + 2, FOLD + 3});
        if (k >= INDICES) v.add(1u, ACTIVE, BUS_BF16, {LN, BETA, BETA + 1, BETA + 2, BETA + 3});                   // FOLD16B: the challenge is received
        break;
    case T_FINAL:
        v.add(1u, FACT, BUS_COEF, {FJ, CFC, CFC + 1, CFC + 2, CFC + 3});
        v.add(1u, FLAST, BUS_FIN16, {CFX, CFACC, CFACC + 1, CFACC + 2, CFACC + 3});
        break;
    case T_LAYERS:
        if (k == LAYERS) {
            for (uint32_t j = 0; j < 16; j++) v.add(1u, LAY_M, BUS_L16, {LAY_LN, LAY_KEY + j, LAY_E + 4 * j, LAY_E + 4 * j + 1, LAY_E + 4 * j + 2, LAY_E + 4 * j + 3});
        } else {                                                                                                   // P24L
            using namespace p24chip;
            const uint32_t o7 = oute(7);
            for (uint32_t i = 0; i < 4; i++) v.add(1u, L_M, BUS_L16, {L_LN, L_K + i, IN + 4 * i, IN + 4 * i + 1, IN + 4 * i + 2, IN + 4 * i + 3});
            v.add(0u, END, BUS_RT0, {L_LN, L_DEP, o7, o7 + 1, o7 + 2, o7 + 3});
            v.add(0u, END, BUS_RT1, {L_LN, L_DEP, o7 + 4, o7 + 5, o7 + 6, o7 + 7});
        }
        break;
    case T_QUERIES:
        if (k < INDICES) v.add(1u, 5u, BUS_Q16, {0u, 1u, 2u, 3u, 4u});
        else if (k == INDICES) {                                                                                   // by query number; the index is a main column, from SAMPLES
            v.add(1u, 5u, BUS_Q16, {Q_PRE, 1u, 2u, 3u, 4u});
            v.add(1u, 5u, frichip::BUS_I, {0u, Q_PRE});
        } else {                                                                                                   // QUERY16
            v.add(1u, QP_ACT, frichip::BUS_I, {QP_QN, QC_IDX});
            v.add(1u, QP_ACT, BUS_Q16, {QC_IDX, QC_XQ, QC_RO, QC_RO + 1, QC_RO + 2, QC_RO + 3});
            v.add(1u, QP_ACT, BUS_AT16, {QP_QN, QC_AT, QC_AT + 1, QC_AT + 2, QC_AT + 3});
            v.add(1u, QP_ACT, BUS_AQ16, {QP_QN, QC_AQ, QC_AQ + 1, QC_AQ + 2, QC_AQ + 3});
            if (k >= ROWPATHS) {                                                                                   // which tree a tag belongs to and at which index it is opened
                v.add(0u, QP_ACT, BUS_TAG16, {QP_TG0, QP_LN0, QC_IDX});
                v.add(0u, QP_ACT, BUS_TAG16, {QP_TG1, QP_LN1, QC_IDX});
            }
            if (k >= HEAD) {                                                                                       // QUERY16H: the constants arrive on the first row
                const uint32_t bus[5] = {BUS_ZETA, BUS_YL, BUS_YN, BUS_YQ, BUS_OFFN}, col[5] = {QC_ZETA, QC_YL, QC_YN, QC_YQ, QC_OFFN};
                for (int i = 0; i < 5; i++) v.add(1u, QP_FIRST, bus[i], {col[i], col[i] + 1, col[i] + 2, col[i] + 3});
            }
        }
        break;
    case T_COEFFS: {
        const uint32_t c = k == LIFT ? C_PRE + CL_C : 1u;                                                          // (lift: c_j is a main column)
        v.add(0u, 5u, BUS_COEF, {0u, c, c + 1, c + 2, c + 3});
        if (k >= INDICES) v.add(0u, 6u, BUS_CT, {0u, c, c + 1, c + 2, c + 3});                                     // one more send, to P2T
        break;
    }
    case T_ROOTS: {
        const uint32_t rt = k == LIFT ? RM + RL_ROOT : RT_ROOT;                                                    // (lift: the root words are main columns)
        v.add(1u, RM, BUS_RT0, {RT_LN, RT_DEP, rt, rt + 1, rt + 2, rt + 3});
        v.add(1u, RM, BUS_RT1, {RT_LN, RT_DEP, rt + 4, rt + 5, rt + 6, rt + 7});
        if (k >= INDICES) {                                                                                        // root and beta from the layer's root row, beta on to the fold rows
            v.add(1u, 10u, BUS_TR0, {RT_LN, rt, rt + 1, rt + 2, rt + 3});
            v.add(1u, 10u, BUS_TR1, {RT_LN, rt + 4, rt + 5, rt + 6, rt + 7});
            v.add(1u, 10u, BUS_TB, {RT_LN, RM + 1, RM + 2, RM + 3, RM + 4});
            v.add(0u, RM + 5, BUS_BF16, {RT_LN, RM + 1, RM + 2, RM + 3, RM + 4});
        }
        if (k >= HEAD) for (uint32_t j = 0; j < 8; j++) v.add(0u, RT_HM, BUS_HR, {RT_HK + j, rt + j});                 // the trace root and the quotient root, word by word, to P2TH
        break;
    }
    case T_P2T:
        v.add(1u, PT_C0, BUS_CT, {PT_KEY0, in, in + 1, in + 2, in + 3});
        v.add(1u, PT_C1, BUS_CT, {PT_KEY1, in + 4, in + 5, in + 6, in + 7});
        v.add(0u, PT_ROOT, BUS_TR0, {PT_LN, in, in + 1, in + 2, in + 3});
        v.add(0u, PT_ROOT, BUS_TR1, {PT_LN, in + 4, in + 5, in + 6, in + 7});
        v.add(0u, PT_ROOT, BUS_TB, {PT_LN, o + 7, o + 6, o + 5, o + 4});
        v.add(0u, PT_SMP, frichip::BUS_S0, {PT_ROW, o + 7, o + 6, o + 5, o + 4});
        v.add(0u, PT_SMP, frichip::BUS_S1, {PT_ROW, o + 3, o + 2, o + 1, o});
        if (k >= HEAD) {                                                                                           // P2TH: roots in, opened values in, zeta and fa out
            for (uint32_t j = 0; j < 8; j++) v.add(1u, PH_RM + j, BUS_HR, {PH_RK + j, in + j});
            v.add(1u, PH_OPN, BUS_OV0, {PT_ROW, in, in + 1, in + 2, in + 3});
            v.add(1u, PH_OPN, BUS_OV1, {PT_ROW, in + 4, in + 5, in + 6, in + 7});
            v.add(0u, PH_ZM, BUS_ZETA, {o + 7, o + 6, o + 5, o + 4});
            v.add(0u, PH_FM, BUS_FAH, {o + 7, o + 6, o + 5, o + 4});
        }
        if (k >= IDENTITY) v.add(0u, PH_AM, BUS_ALPHA, {o + 7, o + 6, o + 5, o + 4});                                   // alpha, from row A - 1, to SCALARS16
        break;
    case T_ROWSUM16:
        v.add(0u, RP_ACT, BUS_ROW16, {RP_TAG, RP_K0, rv, rv + 1, rv + 2, rv + 3});
        v.add(0u, RP_ACT, BUS_ROW16, {RP_TAG, RP_K1, rv + 4, rv + 5, rv + 6, rv + 7});
        v.add(0u, RP_LAST0, BUS_AT16, {RP_QN, rt, rt + 1, rt + 2, rt + 3});
        v.add(0u, RP_LAST1, BUS_AQ16, {RP_QN, rt, rt + 1, rt + 2, rt + 3});
        if (k >= HEAD) v.add(1u, RP_FIRST, BUS_FAH, {rfa, rfa + 1, rfa + 2, rfa + 3});                                 // ROWSUM16H: fa arrives on the first row
        break;
    case T_OPENED16: {
        const uint32_t m = s.pre_w[T_OPENED16], y = m + OP_Y, pwn = m + OP_PWN, fa = m + OP_FA;
        v.add(0u, OQ_ACT, BUS_OV0, {OQ_ROW, m + OP_V, m + OP_V + 1, m + OP_V + 2, m + OP_V + 3});
        v.add(0u, OQ_ACT, BUS_OV1, {OQ_ROW, m + OP_V + 4, m + OP_V + 5, m + OP_V + 6, m + OP_V + 7});
        v.add(0u, OQ_ENDL, BUS_YL, {y, y + 1, y + 2, y + 3});
        v.add(0u, OQ_ENDN, BUS_YN, {y, y + 1, y + 2, y + 3});
        v.add(0u, OQ_ENDQ, BUS_YQ, {y, y + 1, y + 2, y + 3});
        v.add(0u, OQ_ENDL, BUS_OFFN, {pwn, pwn + 1, pwn + 2, pwn + 3});
        v.add(1u, OQ_FIRST, BUS_FAH, {fa, fa + 1, fa + 2, fa + 3});
        if (k >= IDENTITY) {                                                                                       // the row's two halves under its row number, to AIR16 and SCALARS16
            v.add(0u, OQ_H0, BUS_OH0, {OQ_ROW, m + OP_V, m + OP_V + 1, m + OP_V + 2, m + OP_V + 3});
            v.add(0u, OQ_H1, BUS_OH1, {OQ_ROW, m + OP_V + 4, m + OP_V + 5, m + OP_V + 6, m + OP_V + 7});
        }
        break;
    }
    case T_AIR16: {
        const uint32_t m = AIR16_PRE, half[5] = {BUS_OH0, BUS_OH1, BUS_OH0, BUS_OH1, BUS_OH1}, key[5] = {AP_KL0, AP_KL0, AP_KL1, AP_KL1, AP_KN1}, col[5] = {AI_A, AI_B, AI_C, AI_D, AI_DN};
        for (int i = 0; i < 5; i++) v.add(1u, AP_ACT, half[i], {key[i], m + col[i], m + col[i] + 1, m + col[i] + 2, m + col[i] + 3});
        const uint32_t bus[3] = {BUS_KA16, BUS_KSELT, BUS_KSELF}, cst[3] = {AI_ALPHA, AI_SELT, AI_SELF};
        for (int i = 0; i < 3; i++) v.add(1u, AP_FIRST, bus[i], {m + cst[i], m + cst[i] + 1, m + cst[i] + 2, m + cst[i] + 3});
        v.add(0u, AP_LAST, BUS_ACC16, {m + AI_ACCO, m + AI_ACCO + 1, m + AI_ACCO + 2, m + AI_ACCO + 3});
        break;
    }
    case T_SCALARS16: {
        const uint32_t m = SC16_PRE, c = m + sc16_invf((uint32_t)(s.H - s.b)), qz = c + 12u, acc = c + 56u;
        v.add(1u, SP_FIRST, BUS_ALPHA, {m + SC_ALPHA, m + SC_ALPHA + 1, m + SC_ALPHA + 2, m + SC_ALPHA + 3});
        v.add(1u, SP_FIRST, BUS_ZETA, {m + SC_ZETA, m + SC_ZETA + 1, m + SC_ZETA + 2, m + SC_ZETA + 3});
        for (uint32_t i = 0; i < 4; i++) {
            v.add(1u, SP_FIRST, BUS_OH0, {SP_KQ + i, qz + 8 * i, qz + 8 * i + 1, qz + 8 * i + 2, qz + 8 * i + 3});
            v.add(1u, SP_FIRST, BUS_OH1, {SP_KQ + i, qz + 8 * i + 4, qz + 8 * i + 5, qz + 8 * i + 6, qz + 8 * i + 7});
        }
        v.add(1u, SP_FIRST, BUS_ACC16, {acc, acc + 1, acc + 2, acc + 3});
        const uint32_t bus[3] = {BUS_KA16, BUS_KSELT, BUS_KSELF}, cst[3] = {m + SC_ALPHA, c + 8u, c + 4u};
        for (int i = 0; i < 3; i++) v.add(0u, SP_FIRST, bus[i], {cst[i], cst[i] + 1, cst[i] + 2, cst[i] + 3});
        break;
    }
    default:
        if (k == OPENINGS) v.add(1u, 6u, BUS_ROW16, {0u, 1u, 2u, 3u, 4u, 5u});                                     // ROWS
        else {                                                                                                     // P24R
            using namespace p24chip;
            const uint32_t o7 = oute(7), mult[4] = {R_M0, p24chip::G(1), p24chip::G(2), p24chip::G(3)};
            for (uint32_t i = 0; i < 4; i++) v.add(1u, mult[i], BUS_ROW16, {R_TAG, R_K + i, IN + 4 * i, IN + 4 * i + 1, IN + 4 * i + 2, IN + 4 * i + 3});
            v.add(1u, SS, BUS_TAG16, {R_TAG, R_LNR, R_IX});
            v.add(0u, END, BUS_RT0, {R_LNR, R_DEP, o7, o7 + 1, o7 + 2, o7 + 3});
            v.add(0u, END, BUS_RT1, {R_LNR, R_DEP, o7 + 4, o7 + 5, o7 + 6, o7 + 7});
        }
        break;
    }
    return v.finish();
}

// a shape and its keyed machine (keyed_machine.h: programs and interaction tables in MACHINE order, tallest table first)
struct Machine { Shape s; keyed::KeyedMachine km; };
// (P24L's, P24R's and P2T's programs follow the Poseidon2 tables in effect: the cache is dropped when they change)
std::shared_ptr<const Machine> machine_of(const Shape& s) {
    static std::mutex mu;
    static std::map<std::array<uint64_t, 8>, std::shared_ptr<const Machine>> cache;
    static uint64_t cached_gen = ~0ull;
    std::lock_guard<std::mutex> lk(mu);
    const uint64_t gen = g_p2_generation.load();
    if (cached_gen != gen || cache.size() > 64) { cache.clear(); cached_gen = gen; }
    const std::array<uint64_t, 8> key{(uint64_t)s.kind, (uint64_t)s.R, (uint64_t)s.F, (uint64_t)s.b, (uint64_t)s.Q, (uint64_t)s.pow_bits, (uint64_t)s.W, (uint64_t)s.NP};
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    auto m = std::make_shared<Machine>();
    m->s = s;
    keyed::build(m->km, s.n_tables, s.log_rows, s.main_w, s.pre_w, [&](int t, std::vector<uint32_t>& prog, std::vector<uint32_t>& tab) { prog = program_of(s, t); tab = interactions_of(s, t); });
    cache.emplace(key, m);
    return m;
}

// what the entries of every kind do with a shape
size_t describe(const ShapeArgs& a, int which, int what, uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table) {
    Shape s;
    if (which < 0 || which >= N_TABLES[a.kind] || what < 0 || what > 1 || shape_of(a, s) != ZKHIP_OK) return 0;
    const auto m = machine_of(s);
    if (table) *table = m->km.order[which];
    return keyed::describe(m->km, which, what, [](int, int, std::vector<uint32_t>&) {}, out, cap_words, log_rows, main_width, pre_width);
}
// pre: the key's tables by table number (host, Montgomery), uploaded each with preprocessed columns into its scratch slot (slots: by table number)
int key_upload(zkhip_ctx* ctx, const Shape& s, const std::vector<uint32_t>* pre, const int* slots, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    const auto m = machine_of(s);
    const uint32_t* d_pre[MAX_TABLES] = {};
    for (int i = 0; i < s.n_tables; i++) {
        const int t = m->km.order[i];
        if (!s.pre_w[t]) continue;
        void* dp;
        ZK_TRY(ctx_reserve(ctx, slots[t], pre[t].size() * 4, &dp));
        ZK_TRY(dev_h2d(ctx, dp, pre[t].data(), pre[t].size() * 4));
        d_pre[t] = (const uint32_t*)dp;
    }
    return keyed::key_setup(ctx, m->km, d_pre, prm, key, vk);
}
size_t proof_size(const ShapeArgs& a, const zkhip_params* prm) {
    Shape s;
    if (!prm || shape_of(a, s) != ZKHIP_OK) return 0;
    return keyed::proof_size(machine_of(s)->km, prm, n_public_of(s));
}
int verify(const ShapeArgs& a, const uint8_t* proof, size_t len, const uint32_t* public_values, const uint32_t vk[8], const zkhip_params* prm, int* reason, const char* who) {
    Shape s;
    if (!proof || !public_values || !vk || !prm || shape_of(a, s) != ZKHIP_OK) {
        if (reason) *reason = 1;
        return fail(ZKHIP_ERR_VERIFY, std::string(who) + ": bad arguments");
    }
    return keyed::verify(machine_of(s)->km, proof, len, vk, public_values, n_public_of(s), prm, reason);
}

struct fold_rows_bargs { FoldRowsArgs a; static fold_rows_bargs make(FoldRowsArgs a) { return fold_rows_bargs{a}; } };
__global__ void __launch_bounds__(64) fri16_fold_rows_kernel_batch(const fold_rows_bargs* __restrict__ zk_arr) { fri16_fold_rows_body(zk_arr[blockIdx.z].a); }
struct final_rows_bargs { FinalRowsArgs a; static final_rows_bargs make(FinalRowsArgs a) { return final_rows_bargs{a}; } };
__global__ void __launch_bounds__(64) fri16_final_rows_kernel_batch(const final_rows_bargs* __restrict__ zk_arr) { fri16_final_rows_body(zk_arr[blockIdx.z].a); }
struct openings_rows_bargs { OpeningsRowsArgs a; static openings_rows_bargs make(OpeningsRowsArgs a) { return openings_rows_bargs{a}; } };
__global__ void __launch_bounds__(64) fri16_openings_rows_kernel_batch(const openings_rows_bargs* __restrict__ zk_arr) { fri16_openings_rows_body<false>(zk_arr[blockIdx.z].a); }
__global__ void __launch_bounds__(64) fri16_openings_rows_tall_kernel_batch(const openings_rows_bargs* __restrict__ zk_arr) { fri16_openings_rows_body<true>(zk_arr[blockIdx.z].a); }
struct xq_cols_bargs { XqColsArgs a; static xq_cols_bargs make(XqColsArgs a) { return xq_cols_bargs{a}; } };
__global__ void __launch_bounds__(64) fri16_xq_cols_kernel_batch(const xq_cols_bargs* __restrict__ zk_arr) { fri16_xq_cols_body(zk_arr[blockIdx.z].a); }
struct opened_rows_bargs { OpenedRowsArgs a; static opened_rows_bargs make(OpenedRowsArgs a) { return opened_rows_bargs{a}; } };
__global__ void __launch_bounds__(OPENED_LANES) fri16_opened_rows_kernel_batch(const opened_rows_bargs* __restrict__ zk_arr) { fri16_opened_rows_body(zk_arr[blockIdx.z].a); }
struct identity_rows_bargs { IdentityRowsArgs a; static identity_rows_bargs make(IdentityRowsArgs a) { return identity_rows_bargs{a}; } };
__global__ void __launch_bounds__(IDENTITY_LANES) fri16_identity_rows_kernel_batch(const identity_rows_bargs* __restrict__ zk_arr) { fri16_identity_rows_body(zk_arr[blockIdx.z].a); }
struct lift_tables_bargs { LiftTablesArgs a; static lift_tables_bargs make(LiftTablesArgs a) { return lift_tables_bargs{a}; } };
__global__ void __launch_bounds__(64) fri16_lift_tables_kernel_batch(const lift_tables_bargs* __restrict__ zk_arr) { fri16_lift_tables_body(zk_arr[blockIdx.z].a); }

}  // namespace
}  // namespace fri16
}  // namespace zk

using namespace zk;

#define CHECK_CTX(ctx)                                                  \
    do {                                                                \
        if (!(ctx)) return fail(ZKHIP_ERR_INVALID, "null context");     \
        ZK_HIP(hipSetDevice((ctx)->device));                            \
    } while (0)

// both main traces from the view's arrays, uploaded once; every chain's end (FOLD16's last row) against its block's end (FINAL's last row)
static int fri16_gen_traces_impl(zkhip_ctx* ctx, const fri16::Shape& s, const fri16::View& view, uint32_t* d_fold, size_t ld_fold, uint32_t* d_final, size_t ld_final,
                                 const uint32_t* d_values = nullptr) {
    const size_t R = (size_t)s.R, Q = s.Q, nb = 4 * R, nf = (size_t)4 << s.F, ni = (Q + 3) & ~(size_t)3, nv = 4 * Q, ns = 60 * Q * R, up_words = nb + nf + ni + nv + ns;
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_STAGE, (up_words + 16 * Q) * 4, &stage));
    uint32_t* d = (uint32_t*)stage;
    {
        std::vector<uint32_t> up(up_words, 0u);
        std::memcpy(up.data(), view.betas, nb * 4);
        std::memcpy(up.data() + nb, view.final_poly, nf * 4);
        std::memcpy(up.data() + nb + nf, view.indices, Q * 4);
        std::memcpy(up.data() + nb + nf + ni, view.values, nv * 4);
        std::memcpy(up.data() + nb + nf + ni + nv, view.siblings, ns * 4);
        ZK_TRY(dev_h2d(ctx, d, up.data(), up_words * 4));
    }
    // (d_values: the chains start from values already on the device -- the openings machine's, computed there from the opened rows)
    fri16::ViewArgs v{d, d + nb, d + nb + nf, d_values ? d_values : d + nb + nf + ni, d + nb + nf + ni + nv, (uint32_t)Q, (uint32_t)s.R, (uint32_t)s.F, (uint32_t)s.lf, (uint32_t)s.H};
    uint32_t* d_ends = d + up_words;
    fri16::FoldRowsArgs fa{v, fri16::fold16_width((uint32_t)s.lf), (uint64_t)1 << s.log_rows[0], d_fold, ld_fold, d_ends};
    const size_t pad = (size_t)fa.rows - Q * R, fold_lanes = Q * R + (pad < 4096 ? pad : 4096);        // the padding rows are shared among up to 4096 extra lanes
    ZK_LAUNCH(fri16::fri16_fold_rows_kernel, fri16::fri16_fold_rows_kernel_batch, fri16::fold_rows_bargs, dim3((unsigned)((fold_lanes + 63) / 64)), dim3(64), 0, ctx->stream, fa);
    ZK_HIP(hipGetLastError());
    fri16::FinalRowsArgs na{v, (uint64_t)1 << s.log_rows[1], d_final, ld_final, d_ends + 8 * Q};
    const size_t per = s.F > 6 ? (size_t)1 << (s.F - 6) : 1, final_lanes = (size_t)na.rows / per;
    ZK_LAUNCH(fri16::fri16_final_rows_kernel, fri16::fri16_final_rows_kernel_batch, fri16::final_rows_bargs, dim3((unsigned)((final_lanes + 63) / 64)), dim3(64), 0, ctx->stream, na);
    ZK_HIP(hipGetLastError());
    std::vector<uint32_t> ends(16 * Q);
    ZK_TRY(dev_d2h(ctx, ends.data(), d_ends, ends.size() * 4));
    for (size_t q = 0; q < Q; q++)
        if (std::memcmp(ends.data() + 8 * q, ends.data() + 8 * (Q + q), 20) != 0)
            return fail(ZKHIP_ERR_INVALID, "fri16: the chain of query " + std::to_string(q) + " does not end in the final polynomial");
    return ZKHIP_OK;
}

// P24L from the caller's plan of the view's paths (fri16::plan_paths, which refuses queries that disagree about the path of a shared row) and the FOLD16 trace already on
// the device (its E columns are the leaves); ends [n][8]: where every path ends.  Refused here: two queries that disagree about a shared row.
static int fri16_paths_gen_p24l_impl(zkhip_ctx* ctx, const fri16::Shape& s, const uint32_t* paths, const uint32_t* d_fold, size_t ld_fold, uint32_t* d_trace, size_t ld,
                                     const fri16::PathPlan& pl, std::vector<uint32_t>& ends) {
    const size_t rows = (size_t)1 << s.log_rows[fri16::T_P24L];
    if (pl.used_rows > rows) return fail(ZKHIP_ERR_INVALID, "fri16 paths: the paths do not fit the table");
    const size_t nd = 8 * pl.n, nr = (pl.readers.size() + 3) & ~(size_t)3, ns = s.Q * pl.path_words, up_words = nd + nr + ns;
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_REC_I, (up_words + 9 * pl.n) * 4, &stage));
    uint32_t* d = (uint32_t*)stage;
    {
        std::vector<uint32_t> up(up_words, 0u);
        std::memcpy(up.data(), pl.desc.data(), nd * 4);
        std::memcpy(up.data() + nd, pl.readers.data(), pl.readers.size() * 4);
        std::memcpy(up.data() + nd + nr, paths, ns * 4);
        ZK_TRY(dev_h2d(ctx, d, up.data(), up_words * 4));
    }
    p24chip::LayerPathsArgs a{};
    a.desc = d; a.readers = d + nd; a.fold = d_fold; a.fold_ld = ld_fold; a.siblings = d + nd + nr; a.n_paths = pl.n; a.rows = rows; a.used_rows = pl.used_rows;
    a.trace = d_trace; a.ld = ld; a.ends = d + up_words; a.differs = d + up_words + 8 * pl.n;
    ZK_HIP(launch_p24chip_layer_paths(a, ctx->stream));
    ends.resize(9 * pl.n);
    ZK_TRY(dev_d2h(ctx, ends.data(), a.ends, ends.size() * 4));
    for (size_t p = 0; p < pl.n; p++)
        if (const uint32_t k = ends[8 * pl.n + p])
            return fail(ZKHIP_ERR_INVALID, "fri16 paths: query " + std::to_string(pl.readers[pl.desc[8 * p + 5] + k - 1] / (uint32_t)s.R) + " layer " + std::to_string(pl.layer_of[p]) +
                                               " disagrees with query " + std::to_string(pl.first_query[p]) + " about a shared row");
    ends.resize(8 * pl.n);
    return ZKHIP_OK;
}
static int fri16_paths_check_view(const fri16::Shape& s, const fri16::View& v, const char* who) {
    ZK_TRY(fri16::check_hash_width(v.hash_width, who));
    if (!v.paths) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    return fri16::check_view(s, v, who);
}

// P2T, SAMPLES and (non-null) the main columns of QUERIES and ROOTS in one launch from one staging block; status: what the kernel found different from the view
static int fri16_transcript_impl(zkhip_ctx* ctx, const fri16::Shape& s, const fri16::Chain& c, const uint32_t* view_betas, const uint32_t* view_indices, const uint32_t* counts,
                                 uint32_t* d_p2t, uint32_t* d_samples, uint32_t* d_qmain, uint32_t* d_rmain, uint32_t* status, const uint32_t** d_chain = nullptr) {
    const size_t R = (size_t)s.R, Q = s.Q, ni = (Q + 3) & ~(size_t)3, nr = (R + 3) & ~(size_t)3;
    const size_t o_words = c.inputs.size(), o_betas = o_words + 8 * s.S, o_vbetas = o_betas + 4 * R, o_vidx = o_vbetas + 4 * R, o_counts = o_vidx + ni, o_status = o_counts + nr, up_words = o_status + 4;
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_REC_E, up_words * 4, &stage));
    uint32_t* d = (uint32_t*)stage;
    {
        std::vector<uint32_t> up(up_words, 0u);
        std::memcpy(up.data(), c.inputs.data(), c.inputs.size() * 4);
        std::memcpy(up.data() + o_words, c.words.data(), c.words.size() * 4);
        std::memcpy(up.data() + o_betas, c.betas.data(), 16 * R);
        if (view_betas) std::memcpy(up.data() + o_vbetas, view_betas, 16 * R);
        if (view_indices) std::memcpy(up.data() + o_vidx, view_indices, 4 * Q);
        if (counts) std::memcpy(up.data() + o_counts, counts, 4 * R);
        ZK_TRY(dev_h2d(ctx, d, up.data(), up_words * 4));
    }
    p2chip::Fri16TranscriptArgs a{};
    a.chain_inputs = d; a.words = d + o_words; a.drawn_betas = d + o_betas; a.view_betas = view_betas ? d + o_vbetas : nullptr; a.view_indices = view_indices ? d + o_vidx : nullptr;
    a.counts = counts ? d + o_counts : nullptr;
    a.n_chain = (uint32_t)(c.inputs.size() / 16); a.n_sample_rows = (uint32_t)s.S; a.R = (uint32_t)R; a.Q = (uint32_t)Q; a.index_bits = (uint32_t)s.H;
    a.p2t_rows = d_p2t ? (uint64_t)1 << s.log_rows[fri16::T_P2T] : 0; a.samples_rows = (uint64_t)1 << s.log_rows[fri16::T_SAMPLES];
    a.queries_rows = (uint64_t)1 << s.log_rows[fri16::T_QUERIES]; a.roots_rows = (uint64_t)1 << s.log_rows[fri16::T_ROOTS];
    a.p2t = d_p2t; a.samples = d_samples; a.queries_main = d_qmain; a.roots_main = d_rmain; a.status = d + o_status;
    ZK_HIP(launch_fri16_transcript(a, ctx->stream));
    if (d_chain) *d_chain = d;                                   // (the chain's input states stay where they were uploaded: the lift machine's tables are read off them)
    return dev_d2h(ctx, status, a.status, 4);
}
static int fri16_indices_check_inputs(const fri16::Shape& s, const fri16::View& v, const char* who) {
    if (!v.capacity || !v.roots || !v.final_poly) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!fri16::canonical(v.capacity, 8) || !fri16::canonical(v.roots, 8 * (size_t)s.R) || !fri16::canonical(v.final_poly, (size_t)4 << s.F) || v.witness >= P)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    return ZKHIP_OK;
}

// ROWSUM16 and QUERY16 in one launch from one staging block (rows, constants, indices, the view's values); the reduced openings stay on the device (*d_openings,
// canonical, where the fold kernel reads its chains' first values); status[0] / status[1]: the least query whose opening differs from view_values / whose point has no
// inverse (0xFFFFFFFF: none)
static int fri16_openings_rows_impl(zkhip_ctx* ctx, const fri16::Shape& s, const uint32_t* trows, const uint32_t* qrows, const uint32_t* consts, const uint32_t* indices,
                                    const uint32_t* view_values, uint32_t* d_rowsum, uint32_t* d_query, uint32_t** d_openings, uint32_t status[2], const uint32_t** d_indices = nullptr,
                                    const uint32_t** d_rows = nullptr) {      // d_rows: where the raw rows lie on the device, [Q][W] then [Q][8]
    const size_t Q = s.Q, W = s.W, nt = Q * W, nq = Q * fri16::QROW16, ni = (Q + 3) & ~(size_t)3, nv = 4 * Q;
    const size_t o_q = nt, o_c = o_q + nq, o_i = o_c + 32, o_v = o_i + ni, o_open = o_v + nv, o_status = o_open + nv, words = o_status + 4;
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_REC_J, words * 4, &stage));
    uint32_t* d = (uint32_t*)stage;
    {
        std::vector<uint32_t> up(words, 0u);
        std::memcpy(up.data(), trows, nt * 4);
        std::memcpy(up.data() + o_q, qrows, nq * 4);
        std::memcpy(up.data() + o_c, consts, 32 * 4);
        std::memcpy(up.data() + o_i, indices, Q * 4);
        if (view_values) std::memcpy(up.data() + o_v, view_values, nv * 4);
        for (int i = 0; i < 4; i++) up[o_status + i] = 0xFFFFFFFFu;
        ZK_TRY(dev_h2d(ctx, d, up.data(), words * 4));
    }
    fri16::OpeningsRowsArgs a{};
    a.trows = d; a.qrows = d + o_q; a.consts = d + o_c; a.indices = d + o_i; a.view_values = view_values ? d + o_v : nullptr;
    a.Q = (uint32_t)Q; a.W = (uint32_t)W; a.H = (uint32_t)s.H;
    a.rowsum_rows = (uint64_t)1 << s.log_rows[fri16::T_ROWSUM16]; a.query_rows = (uint64_t)1 << s.log_rows[fri16::T_QUERY16];
    a.rowsum = d_rowsum; a.query = d_query; a.openings = d + o_open; a.status = d + o_status;
    const size_t per = W / 8 + 1;
    if (per <= 64) {
        const size_t qpw = 64 / per;
        ZK_LAUNCH(fri16::fri16_openings_rows_kernel, fri16::fri16_openings_rows_kernel_batch, fri16::openings_rows_bargs, dim3((unsigned)((Q + qpw - 1) / qpw)), dim3(64), 0, ctx->stream, a);
    } else
        ZK_LAUNCH(fri16::fri16_openings_rows_tall_kernel, fri16::fri16_openings_rows_tall_kernel_batch, fri16::openings_rows_bargs, dim3((unsigned)Q), dim3(64), 0, ctx->stream, a);
    ZK_HIP(hipGetLastError());
    uint32_t st[4];
    ZK_TRY(dev_d2h(ctx, st, a.status, 16));
    status[0] = st[0]; status[1] = st[1];
    *d_openings = a.openings;
    if (d_indices) *d_indices = a.indices;
    if (d_rows) *d_rows = d;
    return ZKHIP_OK;
}
static int fri16_openings_check_rows(const fri16::Shape& s, const fri16::View& v, const char* who) {
    if (!v.trace_rows || !v.quotient_rows || !v.constants || !v.indices) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!fri16::canonical(v.trace_rows, s.Q * (size_t)s.W) || !fri16::canonical(v.quotient_rows, s.Q * fri16::QROW16) || !fri16::canonical(v.constants, 32))
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    for (size_t q = 0; q < s.Q; q++) if (v.indices[q] >> s.H) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": a query index has more bits than the proof's domain");
    return ZKHIP_OK;
}
static int fri16_openings_no_inverse(const char* who, uint32_t q) {
    return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the point of query " + std::to_string(q) + " is zeta or zeta g: its reduced opening has no inverse");
}

// P24R in one launch: a path per (query, tree), tag order.  d_rows: the raw rows where fri16_openings_rows_impl left them on the device ([Q][W], then [Q][8]), or null:
// they are uploaded here.  ends [2 Q][8]: where every path ends (canonical).
static int fri16_rowpaths_gen_p24r_impl(zkhip_ctx* ctx, const fri16::Shape& s, const uint32_t* d_rows, const fri16::View& v, uint32_t* d_trace, size_t ld,
                                        std::vector<uint32_t>& ends) {
    const uint32_t *trows = v.trace_rows, *qrows = v.quotient_rows, *indices = v.indices, *tpaths = v.trace_paths, *qpaths = v.quotient_paths;
    const size_t Q = s.Q, W = s.W, H = (size_t)s.H, n = 2 * Q, blocks = (W + 15) / 16, rows = (size_t)1 << s.log_rows[fri16::T_P24R];
    const size_t nd = 8 * n, ns = 8 * H * n, nr = d_rows ? 0 : Q * (W + fri16::QROW16), up_words = nd + ns + nr;
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_STAGE, (up_words + 8 * n) * 4, &stage));
    uint32_t* d = (uint32_t*)stage;
    size_t used = 0;
    {
        std::vector<uint32_t> up(up_words, 0u);
        for (size_t q = 0; q < Q; q++)
            for (size_t tree = 0; tree < 2; tree++) {
                const size_t p = 2 * q + tree;
                const uint32_t desc[8] = {(uint32_t)p, (uint32_t)((size_t)s.R + tree), indices[q], (uint32_t)(tree ? fri16::QROW16 : W), (uint32_t)used,
                                          (uint32_t)(tree ? Q * W + fri16::QROW16 * q : W * q), (uint32_t)(8 * H * p), 0u};
                std::memcpy(up.data() + 8 * p, desc, 32);
                std::memcpy(up.data() + nd + 8 * H * p, (tree ? qpaths : tpaths) + 8 * H * q, 32 * H);
                used += (tree ? 1 : blocks) + H;
            }
        if (!d_rows) {
            std::memcpy(up.data() + nd + ns, trows, Q * W * 4);
            std::memcpy(up.data() + nd + ns + Q * W, qrows, Q * fri16::QROW16 * 4);
        }
        ZK_TRY(dev_h2d(ctx, d, up.data(), up_words * 4));
    }
    if (used > rows) return fail(ZKHIP_ERR_INVALID, "fri16 rowpaths: the paths do not fit the table");
    p24chip::RowPathsArgs a{};
    a.desc = d; a.siblings = d + nd; a.rows = d_rows ? d_rows : d + nd + ns; a.n_paths = n; a.trace_rows = rows; a.used_rows = used; a.depth = (uint32_t)H;
    a.trace = d_trace; a.ld = ld; a.ends = d + up_words;
    ZK_HIP(launch_p24chip_row_paths(a, ctx->stream));
    ends.resize(8 * n);
    return dev_d2h(ctx, ends.data(), a.ends, ends.size() * 4);
}
// refused before anything is hashed: null or non-canonical path words, by query and tree
static int fri16_rowpaths_check_paths(const fri16::Shape& s, const fri16::View& v, const char* who) {      // (the roots: checked where the view has them)
    const uint32_t *tpaths = v.trace_paths, *qpaths = v.quotient_paths, *troot = v.trace_root, *qroot = v.quotient_root;
    if (!tpaths || !qpaths) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (troot && (!qroot || !fri16::canonical(troot, 8) || !fri16::canonical(qroot, 8))) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the roots must be canonical");
    const size_t per = 8 * (size_t)s.H;
    for (size_t q = 0; q < s.Q; q++)
        for (int tree = 0; tree < 2; tree++)
            if (!fri16::canonical((tree ? qpaths : tpaths) + per * q, per))
                return fail(ZKHIP_ERR_INVALID, std::string(who) + ": query " + std::to_string(q) + ", " + (tree ? "quotient" : "trace") + " tree: path words must be canonical");
    return ZKHIP_OK;
}

// OPENED16 in one launch from one staging block (the opened values, fa); sums: YL YN YQ OFFN (canonical), where the lanes at the segment ends leave them -- one copy back
static int fri16_head_opened_impl(zkhip_ctx* ctx, const fri16::Shape& s, const uint32_t* opened, const uint32_t fa[4], uint32_t* d_opened, uint32_t sums[16]) {
    const size_t nv = 8 * ((size_t)s.W + 4), words = nv + 4 + 16;
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_STAGE, words * 4, &stage));
    uint32_t* d = (uint32_t*)stage;
    {
        std::vector<uint32_t> up(words, 0u);
        std::memcpy(up.data(), opened, nv * 4);
        std::memcpy(up.data() + nv, fa, 16);
        ZK_TRY(dev_h2d(ctx, d, up.data(), words * 4));
    }
    fri16::OpenedRowsArgs a{};
    a.opened = d; a.fa = d + nv; a.W = s.W; a.rows = (uint64_t)1 << s.log_rows[fri16::T_OPENED16]; a.trace = d_opened; a.sums = d + nv + 4;
    ZK_LAUNCH(fri16::fri16_opened_rows_kernel, fri16::fri16_opened_rows_kernel_batch, fri16::opened_rows_bargs, dim3(1), dim3(fri16::OPENED_LANES), 0, ctx->stream, a);
    ZK_HIP(hipGetLastError());
    return dev_d2h(ctx, sums, a.sums, 64);
}
static int fri16_head_check_inputs(const fri16::Shape& s, const fri16::View& v, const char* who) {
    if (!v.inner_public || !v.trace_root || !v.quotient_root || !v.opened) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (!fri16::canonical(v.inner_public, s.NP)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the inner public values must be canonical");
    if (!fri16::canonical(v.opened, 8 * ((size_t)s.W + 4))) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the opened values must be canonical");
    if (!fri16::canonical(v.trace_root, 8) || !fri16::canonical(v.quotient_root, 8)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the roots must be canonical");
    return ZKHIP_OK;
}

// AIR16 and SCALARS16 in one launch from one staging block (the opened values, alpha, zeta); accs: ACCO of the last group, then QUO (zeta^N - 1), canonical -- one copy back
static int fri16_identity_rows_impl(zkhip_ctx* ctx, const fri16::Shape& s, const uint32_t* opened, const uint32_t alpha[4], const uint32_t zeta[4], uint32_t* d_air,
                                    uint32_t* d_scalars, uint32_t accs[8]) {
    const size_t nv = 8 * ((size_t)s.W + 4), words = nv + 8 + 8;
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_STAGE, words * 4, &stage));
    uint32_t* d = (uint32_t*)stage;
    {
        std::vector<uint32_t> up(words, 0u);
        std::memcpy(up.data(), opened, nv * 4);
        std::memcpy(up.data() + nv, alpha, 16);
        std::memcpy(up.data() + nv + 4, zeta, 16);
        ZK_TRY(dev_h2d(ctx, d, up.data(), words * 4));
    }
    const int n = s.H - s.b;
    uint32_t za[2], zb[2];
    airb::zps_consts(n, za, zb);
    fri16::IdentityRowsArgs a{};
    a.opened = d; a.alpha = d + nv; a.zeta = d + nv + 4; a.W = s.W; a.n = (uint32_t)n; a.gn_inv = finv(two_adic_generator(n));
    for (int k = 0; k < 2; k++) { a.za[k] = to_monty(za[k]); a.zb[k] = to_monty(zb[k]); }
    a.air_rows = (uint64_t)1 << s.log_rows[fri16::T_AIR16]; a.air = d_air; a.scalars = d_scalars; a.accs = d + nv + 8;
    ZK_LAUNCH(fri16::fri16_identity_rows_kernel, fri16::fri16_identity_rows_kernel_batch, fri16::identity_rows_bargs, dim3(1), dim3(fri16::IDENTITY_LANES), 0, ctx->stream, a);
    ZK_HIP(hipGetLastError());
    return dev_d2h(ctx, accs, a.accs, 32);
}
static int fri16_identity_check_zeta(const uint32_t zeta[4], const char* who) {
    if (zeta[0] == 1u && !(zeta[1] | zeta[2] | zeta[3])) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": zeta is 1: the first-row selector has no value there");
    return ZKHIP_OK;
}

// ROOTS' and COEFFS' main columns of the lift machine in one launch, from the chain's input states where the transcript stage uploaded them (d_chain; row_quotient and
// row_layers: the rows of the quotient root and of layer root 0) and ROOTS' first eight columns as the transcript launch wrote them (d_base, or null: zero)
static int fri16_lift_tables_impl(zkhip_ctx* ctx, const fri16::Shape& s, const uint32_t* d_chain, uint32_t row_quotient, uint32_t row_layers, const uint32_t* d_base,
                                  uint32_t* d_roots_main, uint32_t* d_coeffs_main) {
    fri16::LiftTablesArgs a{};
    a.chain = d_chain; a.roots_base = d_base; a.R = (uint32_t)s.R; a.F = (uint32_t)s.F; a.row_quotient = row_quotient; a.row_layers = row_layers;
    a.roots_rows = (uint64_t)1 << s.log_rows[fri16::T_ROOTS]; a.coeffs_rows = (uint64_t)1 << s.log_rows[fri16::T_COEFFS];
    a.roots_main = d_roots_main; a.coeffs_main = d_coeffs_main;
    const uint64_t lanes = 4 * a.roots_rows + 2 * a.coeffs_rows;
    ZK_LAUNCH(fri16::fri16_lift_tables_kernel, fri16::fri16_lift_tables_kernel_batch, fri16::lift_tables_bargs, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, ctx->stream, a);
    ZK_HIP(hipGetLastError());
    return ZKHIP_OK;
}

// ---------------------------------------------------------------- the provers' stages.  Each reserves what it makes, launches, and refuses in the caller's name (who).
// FOLD16's and FINAL's traces (S_REC_A, S_REC_B): what every prover starts with
static int fri16_reserve_fold_final(zkhip_ctx* ctx, const fri16::Shape& s, uint32_t** d_fold, uint32_t** d_final) {
    void *t_fold, *t_final;
    ZK_TRY(ctx_reserve(ctx, S_REC_A, ((size_t)s.main_w[fri16::T_FOLD16] << s.log_rows[fri16::T_FOLD16]) * 4, &t_fold));
    ZK_TRY(ctx_reserve(ctx, S_REC_B, ((size_t)s.main_w[fri16::T_FINAL] << s.log_rows[fri16::T_FINAL]) * 4, &t_final));
    *d_fold = (uint32_t*)t_fold; *d_final = (uint32_t*)t_final;
    return ZKHIP_OK;
}
// the small tables' main columns, one region each of one block (S_CHIP).  QUERIES from OPENINGS on is no table of the machine (QUERY16 holds the index in its own row):
// a scratch block of the plain table's width, which the transcript kernel fills with the indices
struct Fri16SmallTables {
    uint32_t* d = nullptr;
    size_t off[fri16::MAX_TABLES] = {0}, words[fri16::MAX_TABLES] = {0}, total = 0, off_scratch = 0;
    uint32_t* at(int t) const { return d + off[t]; }
    uint32_t* scratch() const { return d + off_scratch; }        // (the lift machine: ROOTS' first eight main columns as the transcript launch writes them, dense)
};
static int fri16_reserve_small_tables(zkhip_ctx* ctx, const fri16::Shape& s, const std::vector<int>& tables, Fri16SmallTables& z, size_t scratch_words = 0) {
    for (int t : tables) {
        z.off[t] = z.total;
        z.words[t] = (size_t)(t == fri16::T_QUERIES && s.kind >= fri16::OPENINGS ? fri16::TAB_MAIN : s.main_w[t]) << s.log_rows[t];
        z.total += z.words[t];
    }
    z.off_scratch = z.total;
    z.total += scratch_words;
    void* p;
    ZK_TRY(ctx_reserve(ctx, S_CHIP, z.total * 4, &p));
    z.d = (uint32_t*)p;
    return ZKHIP_OK;
}
// P2T and SAMPLES (S_REC_C, S_REC_D) and the main columns of QUERIES and ROOTS from the chain walked on the host.  Refused: challenges and indices the chain does not
// draw, a witness that fails the proof of work
static int fri16_transcript_stage(zkhip_ctx* ctx, const fri16::Shape& s, const fri16::View& v, const fri16::PathPlan& pl, uint32_t* d_qmain, uint32_t* d_rmain,
                                  const uint32_t** d_p2t, const uint32_t** d_samples, const char* who, const std::vector<uint32_t>* head_inputs,      // head_inputs: the HD rows in front (HEAD on), or null
                                  const uint32_t** d_chain) {                                                                                         // d_chain: where the chain's input states lie on the device
    void *t_p2t, *t_smp;
    ZK_TRY(ctx_reserve(ctx, S_REC_C, ((size_t)p2chip::T_WIDTH << s.log_rows[fri16::T_P2T]) * 4, &t_p2t));
    ZK_TRY(ctx_reserve(ctx, S_REC_D, ((size_t)frichip::S_MAIN << s.log_rows[fri16::T_SAMPLES]) * 4, &t_smp));
    fri16::Chain c;
    fri16::walk_chain(s, v.capacity, v.roots, v.final_poly, v.witness, c);
    if (head_inputs) c.inputs.insert(c.inputs.begin(), head_inputs->begin(), head_inputs->end());
    uint32_t status = 0;
    ZK_TRY(fri16_transcript_impl(ctx, s, c, v.betas, v.indices, pl.counts.data(), (uint32_t*)t_p2t, (uint32_t*)t_smp, d_qmain, d_rmain, &status, d_chain));
    if (status & 1u) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the challenges are not the ones the transcript draws from these roots and this capacity");
    if (s.pow_bits && (c.words[0] & ((1u << s.pow_bits) - 1u))) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the witness does not satisfy the proof of work");
    if (status & 2u) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the query indices are not the ones the transcript draws");
    *d_p2t = (const uint32_t*)t_p2t; *d_samples = (const uint32_t*)t_smp;
    return ZKHIP_OK;
}
// P24L (S_REC_H) from the plan of the view's paths and the FOLD16 trace.  Refused: queries that disagree about a shared row, paths that do not end in their layer's root.
// (The plan is the caller's: from INDICES on the transcript stage, which comes first, takes the path counts from it.)
static int fri16_layer_paths_stage(zkhip_ctx* ctx, const fri16::Shape& s, const fri16::View& v, const uint32_t* d_fold, size_t ld_fold, const fri16::PathPlan& pl,
                                   const uint32_t** d_p24) {
    void* t_p24;
    ZK_TRY(ctx_reserve(ctx, S_REC_H, ((size_t)p24chip::WIDTH_L << s.log_rows[fri16::T_P24L]) * 4, &t_p24));
    std::vector<uint32_t> ends;
    ZK_TRY(fri16_paths_gen_p24l_impl(ctx, s, v.paths, d_fold, ld_fold, (uint32_t*)t_p24, p24chip::WIDTH_L, pl, ends));
    for (size_t p = 0; p < pl.n; p++)
        if (std::memcmp(ends.data() + 8 * p, v.roots + 8 * pl.layer_of[p], 32) != 0)
            return fail(ZKHIP_ERR_INVALID, "fri16 paths: query " + std::to_string(pl.first_query[p]) + " layer " + std::to_string(pl.layer_of[p]) +
                                               " does not open: its path does not end in the layer's root");
    *d_p24 = (const uint32_t*)t_p24;
    return ZKHIP_OK;
}
// ROWSUM16 and QUERY16 (S_REC_F, S_REC_G), then FOLD16C and FINAL with the chains starting from the openings the device computed, XQ beside the fold kernel's columns.
// Refused: points without an inverse, openings the rows do not give, chains that do not end in the final polynomial.  d_rows: where the raw rows stay on the device
static int fri16_openings_stage(zkhip_ctx* ctx, const fri16::Shape& s, const fri16::View& v, uint32_t* d_fold, uint32_t* d_final, const uint32_t** d_rowsum,
                                const uint32_t** d_query, const uint32_t** d_rows, const char* who) {
    using namespace fri16;
    const size_t ld_fold = s.main_w[T_FOLD16];
    void *t_rs, *t_q;
    ZK_TRY(ctx_reserve(ctx, S_REC_F, ((size_t)RS_MAIN16 << s.log_rows[T_ROWSUM16]) * 4, &t_rs));
    ZK_TRY(ctx_reserve(ctx, S_REC_G, ((size_t)Q16_MAIN << s.log_rows[T_QUERY16]) * 4, &t_q));
    uint32_t ost[2], *d_open = nullptr;
    const uint32_t* d_idx = nullptr;
    ZK_TRY(fri16_openings_rows_impl(ctx, s, v.trace_rows, v.quotient_rows, v.constants, v.indices, v.values, (uint32_t*)t_rs, (uint32_t*)t_q, &d_open, ost, &d_idx, d_rows));
    if (ost[1] != 0xFFFFFFFFu) return fri16_openings_no_inverse(who, ost[1]);
    if (ost[0] != 0xFFFFFFFFu)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the reduced opening of query " + std::to_string(ost[0]) + " computed from its rows and the constants is not the view's");
    ZK_TRY(fri16_gen_traces_impl(ctx, s, v, d_fold, ld_fold, d_final, s.main_w[T_FINAL], d_open));
    XqColsArgs xa{};
    xa.indices = d_idx; xa.Q = (uint32_t)s.Q; xa.R = (uint32_t)s.R; xa.H = (uint32_t)s.H;
    xa.rows = (uint64_t)1 << s.log_rows[T_FOLD16]; xa.trace = d_fold; xa.ld = ld_fold; xa.col = (uint32_t)ld_fold - 4u;
    ZK_LAUNCH(fri16_xq_cols_kernel, fri16_xq_cols_kernel_batch, xq_cols_bargs, dim3((unsigned)((xa.rows + 63) / 64)), dim3(64), 0, ctx->stream, xa);
    ZK_HIP(hipGetLastError());
    *d_rowsum = (const uint32_t*)t_rs; *d_query = (const uint32_t*)t_q;
    return ZKHIP_OK;
}

// ---------------------------------------------------------------- the one key path and the one prover: a kind's key and prove entries below are wrappers around them
// the key's tables by table number from what the kind's key takes of the view (the builders chain: each kind's calls the one before it)
static int fri16_build_key_tables(const fri16::Shape& s, const fri16::View& v, std::vector<uint32_t> pre[], const char* who) {
    using namespace fri16;
    switch (s.kind) {
    case LAYERS: ZK_TRY(check_view(s, v, who)); return build_tables(s, v.betas, v.final_poly, v.indices, v.values, v.siblings, pre);
    case PATHS: return build_paths_key_tables(s, v.final_poly, v.indices, v.values, v.roots, pre, who);
    case INDICES: return build_indices_key_tables(s, v.final_poly, v.values, v.roots, pre, who);
    case OPENINGS: return build_openings_key_tables(s, v.final_poly, v.trace_rows, v.quotient_rows, v.roots, pre, who);
    case ROWPATHS: return build_rowpaths_key_tables(s, v.final_poly, v.roots, v.trace_root, v.quotient_root, pre, who);
    case HEAD: return build_head_key_tables(s, v.final_poly, v.roots, v.trace_root, v.quotient_root, pre, who);
    case IDENTITY: return build_identity_key_tables(s, v.final_poly, v.roots, v.trace_root, v.quotient_root, pre, who);
    case LIFT: return build_lift_key_tables(s, pre, who);
    }
    return fail(ZKHIP_ERR_INVALID, std::string(who) + ": no such machine");
}
// the key's scratch slots by table number.  LAYERS and PATHS give them out by machine position; from INDICES on one table serves every kind: those with preprocessed
// columns, a later kind's (OPENED16's schedule; AIR16's and SCALARS16's) behind an earlier one's (P24R has no preprocessed columns: its slot is not read)
static void fri16_key_slots(const fri16::Shape& s, int slots[fri16::MAX_TABLES]) {
    static const int by_position[6] = {S_REC_C, S_REC_D, S_REC_E, S_REC_F, S_REC_G, S_REC_J};
    static const int by_table[fri16::MAX_TABLES] = {-1, S_REC_C, -1, S_REC_D, S_REC_E, S_REC_F, S_REC_G, S_REC_J, S_REC_A, S_REC_B, S_REC_H, S_REC_I, S_STAGE};
    const auto m = fri16::machine_of(s);
    for (int i = 0; i < s.n_tables; i++) {
        const int t = m->km.order[i];
        slots[t] = s.kind <= fri16::PATHS ? by_position[i] : by_table[t];
    }
}
// the key of every kind (who: the entry's name in the refusals).  ctx null: the host key, vk alone
static int fri16_key(const fri16::ShapeArgs& a, const char* who, zkhip_ctx* ctx, const fri16::View& v, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    fri16::Shape s;
    ZK_TRY(fri16::shape_of(a, s));
    if (a.kind >= fri16::PATHS) ZK_TRY(fri16::check_hash_width(v.hash_width, who));
    if (!prm || !vk || (ctx && !key)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    std::vector<uint32_t> pre[fri16::MAX_TABLES];
    ZK_TRY(fri16_build_key_tables(s, v, pre, who));
    if (!ctx) return keyed::key_host(fri16::machine_of(s)->km, pre, prm, vk);
    int slots[fri16::MAX_TABLES];
    fri16_key_slots(s, slots);
    return fri16::key_upload(ctx, s, pre, slots, prm, key, vk);
}

// the prover of every kind (who: the entry's name in the refusals): a kind is the kind before it plus one stage, and every stage is gated on the kind.  Where two kinds
// differ in the ORDER of their stages the gate keeps the difference: the context's slots are reused, and the first refusal of a bad view is part of the entry
static int fri16_prove(const fri16::ShapeArgs& a, const char* who, zkhip_ctx* ctx, const zkhip_machine_key* key, const fri16::View& view, const zkhip_params* prm,
                       uint8_t* proof, size_t cap, size_t* len) {
    CHECK_CTX(ctx);
    using namespace fri16;
    const Kind kind = a.kind;
    const bool lift = kind == LIFT;
    Shape s;
    if (kind >= HEAD && a.NP > MAX_NP) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": more than 30 inner public values");
    ZK_TRY(shape_of(a, s));
    if (!key || !prm || !proof || !len || (kind == PATHS && !view.roots) || (kind >= ROWPATHS && (!view.trace_root || !view.quotient_root)))
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (kind == LAYERS) ZK_TRY(check_view(s, view, who));
    else ZK_TRY(fri16_paths_check_view(s, view, who));
    if (kind == PATHS && !canonical(view.roots, 8 * (size_t)s.R)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    if (kind >= INDICES) ZK_TRY(fri16_indices_check_inputs(s, view, who));
    if (kind >= OPENINGS) {
        ZK_TRY(fri16_openings_check_rows(s, view, who));
        ZK_TRY(check_openings_constants(s, view.constants, who));
    }
    if (kind >= ROWPATHS) ZK_TRY(fri16_rowpaths_check_paths(s, view, who));
    if (kind >= HEAD) ZK_TRY(fri16_head_check_inputs(s, view, who));
    const size_t Q = s.Q, R = (size_t)s.R, ld_fold = s.main_w[T_FOLD16];
    uint32_t *t_fold, *t_final;
    void* t_p24r = nullptr;
    ZK_TRY(fri16_reserve_fold_final(ctx, s, &t_fold, &t_final));
    if (kind >= ROWPATHS) ZK_TRY(ctx_reserve(ctx, S_CHIP_B, ((size_t)p24chip::WIDTH_R << s.log_rows[T_P24R]) * 4, &t_p24r));
    // the small tables' main columns.  The key's tables (LAYERS; QUERIES below OPENINGS; COEFFS below LIFT; ROWS) are unused, zero; QUERIES from INDICES on holds the
    // indices (from OPENINGS on as a scratch block); ROOTS path ends, challenge and fold rows per layer; OPENED16, AIR16 and SCALARS16 their chips
    // (LIFT: the transcript launch writes ROOTS' first eight columns into a dense scratch block; the lift launch makes both tables whole from it and the chain's inputs)
    std::vector<int> small{T_QUERIES, T_COEFFS};
    if (kind == LAYERS) small.insert(small.begin(), T_LAYERS);
    if (kind >= PATHS) small.push_back(T_ROOTS);
    if (kind == OPENINGS) small.push_back(T_ROWS);
    if (kind >= HEAD) small.push_back(T_OPENED16);
    if (kind >= IDENTITY) small.insert(small.end(), {T_AIR16, T_SCALARS16});
    Fri16SmallTables z;
    ZK_TRY(fri16_reserve_small_tables(ctx, s, small, z, lift ? (size_t)ROOTS_MAIN_I << s.log_rows[T_ROOTS] : 0));
    uint32_t* const d_rmain = lift ? z.scratch() : z.at(T_ROOTS);
    const size_t roots_ld = lift ? ROOTS_MAIN_I : s.main_w[T_ROOTS];
    if (kind == LAYERS) ZK_TRY(dev_memset(ctx, z.d, 0, z.total * 4));      // (PATHS uploads the whole block below)
    if (kind >= INDICES && !lift) ZK_TRY(dev_memset(ctx, z.at(T_COEFFS), 0, z.words[T_COEFFS] * 4));
    if (kind == OPENINGS) ZK_TRY(dev_memset(ctx, z.at(T_ROWS), 0, z.words[T_ROWS] * 4));
    const uint32_t* traces[MAX_TABLES] = {t_fold, t_final};
    traces[T_COEFFS] = z.at(T_COEFFS);
    if (kind == LAYERS) traces[T_LAYERS] = z.at(T_LAYERS);
    if (kind < OPENINGS) traces[T_QUERIES] = z.at(T_QUERIES);
    if (kind >= PATHS) traces[T_ROOTS] = z.at(T_ROOTS);
    if (kind == OPENINGS) traces[T_ROWS] = z.at(T_ROWS);
    // everything below is refused before anything is proven.  HEAD on, the head first: the chain from the all-zero state, OPENED16, the eight constants and the capacity
    // DERIVED -- refused here: a derived constant or capacity that is not the view's; the later stages then read the derived values (v)
    View v = view;
    Head h;
    uint32_t derived[32];
    if (kind >= HEAD) {
        walk_head(s, v.inner_public, v.trace_root, v.quotient_root, v.opened, h);
        uint32_t sums[16];
        ZK_TRY(fri16_head_opened_impl(ctx, s, v.opened, h.fa, z.at(T_OPENED16), sums));
        head_constants(s, h, sums, derived);
        static const char* const names[8] = {"fa", "zeta", "zeta g_N", "YL", "YN", "YQ", "OFFN", "OFFQ"};
        for (int k = 0; k < 8; k++)
            if (std::memcmp(derived + 4 * k, v.constants + 4 * k, 16) != 0)
                return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the constant " + names[k] + " derived from the head of the transcript is not the view's");
        if (std::memcmp(h.capacity, v.capacity, 32) != 0) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the capacity the head of the transcript leaves is not the view's");
        v.constants = derived; v.capacity = h.capacity;
        traces[T_OPENED16] = z.at(T_OPENED16);
    }
    // INDICES on, the transcript before the chains (the plan first: the stage takes the path counts from it).  Refused: challenges and indices the chain does not draw,
    // a witness that fails the proof of work
    PathPlan pl;
    const uint32_t *d_rows = nullptr, *d_chain = nullptr;
    if (kind >= INDICES) {
        ZK_TRY(plan_paths(s, v.indices, v.paths, pl));
        ZK_TRY(fri16_transcript_stage(ctx, s, v, pl, z.at(T_QUERIES), d_rmain, &traces[T_P2T], &traces[T_SAMPLES], who, kind >= HEAD ? &h.inputs : nullptr, &d_chain));
    }
    if (kind >= ROWPATHS) {
        const uint32_t ends_of_tree = to_monty((uint32_t)Q);      // ROOTS' main column 0 on the two trees' rows: Q paths end in each
        for (size_t tree = 0; tree < 2; tree++) ZK_TRY(dev_h2d(ctx, d_rmain + roots_ld * (R + tree), &ends_of_tree, 4));
    }
    // (the staging block the chain's inputs lie in is not reserved again before this launch has read them: the next stage's d2h waits for the stream)
    if (lift) ZK_TRY(fri16_lift_tables_impl(ctx, s, d_chain, (uint32_t)s.A, (uint32_t)s.HD, d_rmain, z.at(T_ROOTS), z.at(T_COEFFS)));
    // FOLD16 and FINAL; from OPENINGS on behind ROWSUM16 and QUERY16, the chains starting from the openings the device computed.  Refused: chains that do not end in the
    // final polynomial; openings the rows do not give, points without an inverse
    if (kind >= OPENINGS) ZK_TRY(fri16_openings_stage(ctx, s, v, t_fold, t_final, &traces[T_ROWSUM16], &traces[T_QUERY16], &d_rows, who));
    else ZK_TRY(fri16_gen_traces_impl(ctx, s, v, t_fold, ld_fold, t_final, s.main_w[T_FINAL]));
    // P24L.  Refused: queries that disagree, paths that do not end in their layer's root.  (PATHS plans here, and builds ROOTS' counts on the host.)
    if (kind == PATHS) ZK_TRY(plan_paths(s, v.indices, v.paths, pl));
    if (kind >= PATHS) ZK_TRY(fri16_layer_paths_stage(ctx, s, v, t_fold, ld_fold, pl, &traces[T_P24L]));
    if (kind == PATHS) {
        std::vector<uint32_t> tabs(z.total, 0u);
        for (size_t l = 0; l < R; l++) tabs[z.off[T_ROOTS] + (size_t)TAB_MAIN * l] = to_monty(pl.counts[l]);
        ZK_TRY(dev_h2d(ctx, z.d, tabs.data(), z.total * 4));
    }
    if (kind >= ROWPATHS) {
        // P24R from the raw rows the openings launch left on the device (the staging block of S_REC_J is not reserved again before this)
        std::vector<uint32_t> ends;
        ZK_TRY(fri16_rowpaths_gen_p24r_impl(ctx, s, d_rows, v, (uint32_t*)t_p24r, p24chip::WIDTH_R, ends));
        for (size_t p = 0; p < 2 * Q; p++)
            if (std::memcmp(ends.data() + 8 * p, p & 1 ? v.quotient_root : v.trace_root, 32) != 0)
                return fail(ZKHIP_ERR_INVALID, std::string(who) + ": query " + std::to_string(p / 2) + ", " + (p & 1 ? "quotient" : "trace") + " tree: the opened row's path does not end in the root");
        traces[T_P24R] = (const uint32_t*)t_p24r;
    }
    if (kind >= IDENTITY) {      // AIR16 and SCALARS16 from alpha, zeta and the opened values; refused here, still before anything is proven: zeta = 1, an identity that does not hold
        uint32_t accs[8];
        ZK_TRY(fri16_identity_check_zeta(h.zeta, who));
        ZK_TRY(fri16_identity_rows_impl(ctx, s, v.opened, h.alpha, h.zeta, z.at(T_AIR16), z.at(T_SCALARS16), accs));
        if (std::memcmp(accs, accs + 4, 16) != 0) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the inner proof's AIR identity at zeta does not hold");
        traces[T_AIR16] = z.at(T_AIR16); traces[T_SCALARS16] = z.at(T_SCALARS16);
    }
    // the public values: the challenges; the capacity; the capacity, then the eight constants; the inner proof's
    uint32_t pub[N_PUBLIC_O];
    if (kind == OPENINGS || kind == ROWPATHS) {
        std::memcpy(pub, view.capacity, 32);
        std::memcpy(pub + 8, view.constants, 128);
    }
    const uint32_t* public_values = kind <= PATHS ? view.betas : kind == INDICES ? view.capacity : kind >= HEAD ? view.inner_public : pub;
    return keyed::prove(ctx, key, machine_of(s)->km, traces, public_values, n_public_of(s), prm, proof, cap, len);
}

extern "C" {

// ---------------------------------------------------------------- LAYERS: the first machine's entries
size_t zkhip_fri16_describe(int R, int F, int log_blowup, size_t n_queries, int which, int kind, uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width,
                            uint32_t* pre_width, int* table) {
    return fri16::describe({fri16::LAYERS, R, F, log_blowup, n_queries}, which, kind, out, cap_words, log_rows, main_width, pre_width, table);
}

int zkhip_fri16_key_host(int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                         const uint32_t* siblings, const zkhip_params* prm, uint32_t vk[8]) {
    fri16::View v;
    v.betas = betas; v.final_poly = final_poly; v.indices = indices; v.values = values; v.siblings = siblings;
    return fri16_key({fri16::LAYERS, R, F, log_blowup, n_queries}, "fri16_key_host", nullptr, v, prm, nullptr, vk);
}

int zkhip_fri16_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices,
                    const uint32_t* values, const uint32_t* siblings, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    fri16::View v;
    v.betas = betas; v.final_poly = final_poly; v.indices = indices; v.values = values; v.siblings = siblings;
    return fri16_key({fri16::LAYERS, R, F, log_blowup, n_queries}, "fri16_key", ctx, v, prm, key, vk);
}

int zkhip_fri16_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices,
                           const uint32_t* values, const uint32_t* siblings, uint32_t* d_fold, size_t ld_fold, uint32_t* d_final, size_t ld_final) {
    CHECK_CTX(ctx);
    fri16::Shape s;
    ZK_TRY(fri16::shape_of({fri16::LAYERS, R, F, log_blowup, n_queries}, s));
    fri16::View v;
    v.betas = betas; v.final_poly = final_poly; v.indices = indices; v.values = values; v.siblings = siblings;
    ZK_TRY(fri16::check_view(s, v, "fri16_gen_traces"));
    if (!d_fold || !d_final || ld_fold < s.main_w[0] || ld_final < fri16::FIN_MAIN || ld_fold % 4 || ld_final % 4 || ((uintptr_t)d_fold | (uintptr_t)d_final) % 16)
        return fail(ZKHIP_ERR_INVALID, "fri16_gen_traces: 16-byte aligned traces, leading dimensions multiples of 4 that hold the tables' widths");
    return fri16_gen_traces_impl(ctx, s, v, d_fold, ld_fold, d_final, ld_final);
}

size_t zkhip_fri16_proof_size(int R, int F, int log_blowup, size_t n_queries, const zkhip_params* prm) {
    return fri16::proof_size({fri16::LAYERS, R, F, log_blowup, n_queries}, prm);
}

int zkhip_prove_fri16(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t* final_poly,
                      const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len) {
    const fri16::View v{0, betas, final_poly, indices, values, siblings};
    return fri16_prove({fri16::LAYERS, R, F, log_blowup, n_queries}, "prove_fri16", ctx, key, v, prm, proof, cap, len);
}

int zkhip_verify_fri16(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t vk[8], const zkhip_params* prm,
                       int* reason) {
    return fri16::verify({fri16::LAYERS, R, F, log_blowup, n_queries}, proof, len, betas, vk, prm, reason, "verify_fri16");
}

// ---------------------------------------------------------------- PATHS
size_t zkhip_fri16_paths_describe(int R, int F, int log_blowup, size_t n_queries, int which, int kind, uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width,
                                  uint32_t* pre_width, int* table) {
    return fri16::describe({fri16::PATHS, R, F, log_blowup, n_queries}, which, kind, out, cap_words, log_rows, main_width, pre_width, table);
}

int zkhip_fri16_paths_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                               const uint32_t* roots, const zkhip_params* prm, uint32_t vk[8]) {
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.indices = indices; v.values = values; v.roots = roots;
    return fri16_key({fri16::PATHS, R, F, log_blowup, n_queries}, "fri16_paths_key_host", nullptr, v, prm, nullptr, vk);
}

int zkhip_fri16_paths_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, const uint32_t* final_poly, const uint32_t* indices,
                          const uint32_t* values, const uint32_t* roots, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.indices = indices; v.values = values; v.roots = roots;
    return fri16_key({fri16::PATHS, R, F, log_blowup, n_queries}, "fri16_paths_key", ctx, v, prm, key, vk);
}

int zkhip_fri16_paths_gen_trace(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, const uint32_t* betas, const uint32_t* final_poly,
                                const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const uint32_t* paths, uint32_t* d_trace, size_t ld,
                                uint32_t* ends, size_t cap_paths, size_t* n_paths) {
    CHECK_CTX(ctx);
    fri16::Shape s;
    ZK_TRY(fri16::shape_of({fri16::PATHS, R, F, log_blowup, n_queries}, s));
    fri16::View v;
    v.hash_width = inner_hash_width; v.betas = betas; v.final_poly = final_poly; v.indices = indices; v.values = values; v.siblings = siblings; v.paths = paths;
    ZK_TRY(fri16_paths_check_view(s, v, "fri16_paths_gen_trace"));
    if (!d_trace || !ends || !n_paths || ld < p24chip::WIDTH_L || ld % 4 || (uintptr_t)d_trace % 16)
        return fail(ZKHIP_ERR_INVALID, "fri16_paths_gen_trace: a 16-byte aligned trace, a leading dimension that is a multiple of 4 and holds 552 columns, ends and n_paths");
    uint32_t *t_fold, *t_final;
    ZK_TRY(fri16_reserve_fold_final(ctx, s, &t_fold, &t_final));
    ZK_TRY(fri16_gen_traces_impl(ctx, s, v, t_fold, s.main_w[0], t_final, s.main_w[1]));
    fri16::PathPlan pl;
    std::vector<uint32_t> e;
    ZK_TRY(fri16::plan_paths(s, indices, paths, pl));
    ZK_TRY(fri16_paths_gen_p24l_impl(ctx, s, paths, t_fold, s.main_w[0], d_trace, ld, pl, e));
    *n_paths = pl.n;
    if (cap_paths < pl.n) return fail(ZKHIP_ERR_INVALID, "fri16_paths_gen_trace: more paths than `ends` holds");
    std::memcpy(ends, e.data(), e.size() * 4);
    return ZKHIP_OK;
}

size_t zkhip_fri16_paths_proof_size(int R, int F, int log_blowup, size_t n_queries, const zkhip_params* prm) {
    return fri16::proof_size({fri16::PATHS, R, F, log_blowup, n_queries}, prm);
}

int zkhip_prove_fri16_paths(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, const uint32_t* betas,
                            const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const uint32_t* roots,
                            const uint32_t* paths, const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len) {
    const fri16::View v{inner_hash_width, betas, final_poly, indices, values, siblings, roots, paths};
    return fri16_prove({fri16::PATHS, R, F, log_blowup, n_queries}, "prove_fri16_paths", ctx, key, v, prm, proof, cap, len);
}

int zkhip_verify_fri16_paths(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t vk[8],
                             const zkhip_params* prm, int* reason) {
    return fri16::verify({fri16::PATHS, R, F, log_blowup, n_queries}, proof, len, betas, vk, prm, reason, "verify_fri16_paths");
}

// ---------------------------------------------------------------- INDICES
size_t zkhip_fri16_indices_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, int which, int kind, uint32_t* out, size_t cap_words, int* log_rows,
                                    uint32_t* main_width, uint32_t* pre_width, int* table) {
    return fri16::describe({fri16::INDICES, R, F, log_blowup, n_queries, inner_pow_bits}, which, kind, out, cap_words, log_rows, main_width, pre_width, table);
}

int zkhip_fri16_indices_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, const uint32_t* final_poly, const uint32_t* values,
                                 const uint32_t* roots, const zkhip_params* prm, uint32_t vk[8]) {
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.values = values; v.roots = roots;
    return fri16_key({fri16::INDICES, R, F, log_blowup, n_queries, inner_pow_bits}, "fri16_indices_key_host", nullptr, v, prm, nullptr, vk);
}

int zkhip_fri16_indices_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, const uint32_t* final_poly,
                            const uint32_t* values, const uint32_t* roots, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.values = values; v.roots = roots;
    return fri16_key({fri16::INDICES, R, F, log_blowup, n_queries, inner_pow_bits}, "fri16_indices_key", ctx, v, prm, key, vk);
}

size_t zkhip_fri16_indices_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, const zkhip_params* prm) {
    return fri16::proof_size({fri16::INDICES, R, F, log_blowup, n_queries, inner_pow_bits}, prm);
}

int zkhip_fri16_indices_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, const uint32_t capacity[8], const uint32_t* roots,
                                   const uint32_t* final_poly, uint32_t witness, uint32_t* d_p2t, uint32_t* d_samples, uint32_t* betas, uint32_t* indices) {
    CHECK_CTX(ctx);
    fri16::Shape s;
    ZK_TRY(fri16::shape_of({fri16::INDICES, R, F, log_blowup, n_queries, inner_pow_bits}, s));
    fri16::View v;
    v.capacity = capacity; v.roots = roots; v.final_poly = final_poly; v.witness = witness;
    ZK_TRY(fri16_indices_check_inputs(s, v, "fri16_indices_gen_traces"));
    if (!d_p2t || !d_samples || !betas || !indices || ((uintptr_t)d_p2t | (uintptr_t)d_samples) % 16)
        return fail(ZKHIP_ERR_INVALID, "fri16_indices_gen_traces: 16-byte aligned dense traces (352 and 288 columns), betas and indices");
    fri16::Chain c;
    fri16::walk_chain(s, capacity, roots, final_poly, witness, c);
    uint32_t status = 0;
    ZK_TRY(fri16_transcript_impl(ctx, s, c, nullptr, nullptr, nullptr, d_p2t, d_samples, nullptr, nullptr, &status));
    std::memcpy(betas, c.betas.data(), c.betas.size() * 4);
    std::memcpy(indices, c.drawn.data(), c.drawn.size() * 4);
    return ZKHIP_OK;
}

int zkhip_fri16_samples_gen_trace(zkhip_ctx* ctx, int index_bits, size_t n_queries, const uint32_t* words, uint32_t* d_samples) {
    CHECK_CTX(ctx);
    if (index_bits < 1 || index_bits > TWO_ADICITY || n_queries < 1 || n_queries > fri16::MAX_Q || !words || !d_samples || (uintptr_t)d_samples % 16)
        return fail(ZKHIP_ERR_INVALID, "fri16_samples_gen_trace: 1..27 index bits, 1..1024 queries, the words and a 16-byte aligned dense trace of 288 columns");
    const size_t S = frichip::samples_chip_rows(n_queries);
    if (!fri16::canonical(words, 8 * S)) return fail(ZKHIP_ERR_INVALID, "fri16_samples_gen_trace: values must be canonical");
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_REC_E, (8 * S + 4) * 4, &stage));
    uint32_t* d = (uint32_t*)stage;
    {
        std::vector<uint32_t> up(8 * S + 4, 0u);
        std::memcpy(up.data(), words, 32 * S);
        ZK_TRY(dev_h2d(ctx, d, up.data(), up.size() * 4));
    }
    p2chip::Fri16TranscriptArgs a{};
    a.words = d; a.n_sample_rows = (uint32_t)S; a.Q = (uint32_t)n_queries; a.index_bits = (uint32_t)index_bits; a.samples_rows = (uint64_t)1 << fri16::lg(S);
    a.samples = d_samples; a.status = d + 8 * S;
    ZK_HIP(launch_fri16_transcript(a, ctx->stream));
    return dev_sync(ctx);
}

int zkhip_prove_fri16_indices(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                              const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const uint32_t* roots,
                              const uint32_t* paths, const uint32_t capacity[8], uint32_t witness, const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len) {
    const fri16::View v{inner_hash_width, betas, final_poly, indices, values, siblings, roots, paths, capacity, witness};
    return fri16_prove({fri16::INDICES, R, F, log_blowup, n_queries, inner_pow_bits}, "prove_fri16_indices", ctx, key, v, prm, proof, cap, len);
}

int zkhip_verify_fri16_indices(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, const uint32_t capacity[8],
                               const uint32_t vk[8], const zkhip_params* prm, int* reason) {
    return fri16::verify({fri16::INDICES, R, F, log_blowup, n_queries, inner_pow_bits}, proof, len, capacity, vk, prm, reason, "verify_fri16_indices");
}

// ---------------------------------------------------------------- OPENINGS
size_t zkhip_fri16_openings_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, int which, int kind, uint32_t* out,
                                     size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table) {
    return fri16::describe({fri16::OPENINGS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, which, kind, out, cap_words, log_rows, main_width, pre_width, table);
}

int zkhip_fri16_openings_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, const uint32_t* final_poly,
                                  const uint32_t* trace_rows, const uint32_t* quotient_rows, const uint32_t* roots, const zkhip_params* prm, uint32_t vk[8]) {
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.trace_rows = trace_rows; v.quotient_rows = quotient_rows; v.roots = roots;
    return fri16_key({fri16::OPENINGS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, "fri16_openings_key_host", nullptr, v, prm, nullptr, vk);
}

int zkhip_fri16_openings_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                             const uint32_t* final_poly, const uint32_t* trace_rows, const uint32_t* quotient_rows, const uint32_t* roots, const zkhip_params* prm,
                             zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.trace_rows = trace_rows; v.quotient_rows = quotient_rows; v.roots = roots;
    return fri16_key({fri16::OPENINGS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, "fri16_openings_key", ctx, v, prm, key, vk);
}

size_t zkhip_fri16_openings_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, const zkhip_params* prm) {
    return fri16::proof_size({fri16::OPENINGS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, prm);
}

int zkhip_fri16_openings_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, const uint32_t* trace_rows,
                                    const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* indices, uint32_t* d_rowsum, uint32_t* d_query,
                                    uint32_t* openings) {
    CHECK_CTX(ctx);
    fri16::Shape s;
    ZK_TRY(fri16::shape_of({fri16::OPENINGS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, s));
    fri16::View v;
    v.trace_rows = trace_rows; v.quotient_rows = quotient_rows; v.constants = constants; v.indices = indices;
    ZK_TRY(fri16_openings_check_rows(s, v, "fri16_openings_gen_traces"));
    if (!d_rowsum || !d_query || !openings || ((uintptr_t)d_rowsum | (uintptr_t)d_query) % 16)
        return fail(ZKHIP_ERR_INVALID, "fri16_openings_gen_traces: 16-byte aligned dense traces (48 and 72 columns) and the openings");
    uint32_t status[2], *d_open = nullptr;
    ZK_TRY(fri16_openings_rows_impl(ctx, s, trace_rows, quotient_rows, constants, indices, nullptr, d_rowsum, d_query, &d_open, status));
    if (status[1] != 0xFFFFFFFFu) return fri16_openings_no_inverse("fri16_openings_gen_traces", status[1]);
    return dev_d2h(ctx, openings, d_open, 16 * n_queries);
}

int zkhip_prove_fri16_openings(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                               uint32_t trace_width, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                               const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness,
                               const uint32_t* trace_rows, const uint32_t* quotient_rows, const uint32_t constants[32], const zkhip_params* prm, uint8_t* proof, size_t cap,
                               size_t* len) {
    const fri16::View v{inner_hash_width, betas, final_poly, indices, values, siblings, roots, paths, capacity, witness, trace_rows, quotient_rows, constants};
    return fri16_prove({fri16::OPENINGS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, "prove_fri16_openings", ctx, key, v, prm, proof, cap, len);
}

int zkhip_verify_fri16_openings(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                                const uint32_t public_values[40], const uint32_t vk[8], const zkhip_params* prm, int* reason) {
    return fri16::verify({fri16::OPENINGS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, proof, len, public_values, vk, prm, reason, "verify_fri16_openings");
}

// ---------------------------------------------------------------- ROWPATHS
size_t zkhip_fri16_rowpaths_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, int which, int kind, uint32_t* out,
                                     size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table) {
    return fri16::describe({fri16::ROWPATHS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, which, kind, out, cap_words, log_rows, main_width, pre_width, table);
}

int zkhip_fri16_rowpaths_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, const uint32_t* final_poly,
                                  const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm, uint32_t vk[8]) {
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.roots = roots; v.trace_root = trace_root; v.quotient_root = quotient_root;
    return fri16_key({fri16::ROWPATHS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, "fri16_rowpaths_key_host", nullptr, v, prm, nullptr, vk);
}

int zkhip_fri16_rowpaths_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                             const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm,
                             zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.roots = roots; v.trace_root = trace_root; v.quotient_root = quotient_root;
    return fri16_key({fri16::ROWPATHS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, "fri16_rowpaths_key", ctx, v, prm, key, vk);
}

size_t zkhip_fri16_rowpaths_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, const zkhip_params* prm) {
    return fri16::proof_size({fri16::ROWPATHS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, prm);
}

int zkhip_fri16_rowpaths_gen_trace(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, const uint32_t* trace_rows,
                                   const uint32_t* quotient_rows, const uint32_t* indices, const uint32_t* trace_paths, const uint32_t* quotient_paths, uint32_t* d_trace,
                                   uint32_t* ends) {
    CHECK_CTX(ctx);
    fri16::Shape s;
    ZK_TRY(fri16::shape_of({fri16::ROWPATHS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, s));
    if (!trace_rows || !quotient_rows || !indices || !d_trace || !ends || (uintptr_t)d_trace % 16)
        return fail(ZKHIP_ERR_INVALID, "fri16_rowpaths_gen_trace: null argument, or a trace that is not 16-byte aligned (dense, 552 columns)");
    if (!fri16::canonical(trace_rows, s.Q * (size_t)s.W) || !fri16::canonical(quotient_rows, s.Q * fri16::QROW16))
        return fail(ZKHIP_ERR_INVALID, "fri16_rowpaths_gen_trace: values must be canonical");
    for (size_t q = 0; q < s.Q; q++) if (indices[q] >> s.H) return fail(ZKHIP_ERR_INVALID, "fri16_rowpaths_gen_trace: a query index has more bits than the proof's domain");
    fri16::View v;
    v.trace_rows = trace_rows; v.quotient_rows = quotient_rows; v.indices = indices; v.trace_paths = trace_paths; v.quotient_paths = quotient_paths;
    ZK_TRY(fri16_rowpaths_check_paths(s, v, "fri16_rowpaths_gen_trace"));
    std::vector<uint32_t> e;
    ZK_TRY(fri16_rowpaths_gen_p24r_impl(ctx, s, nullptr, v, d_trace, p24chip::WIDTH_R, e));
    std::memcpy(ends, e.data(), e.size() * 4);
    return ZKHIP_OK;
}

int zkhip_prove_fri16_rowpaths(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                               uint32_t trace_width, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                               const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness,
                               const uint32_t* trace_rows, const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* trace_paths,
                               const uint32_t* quotient_paths, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm, uint8_t* proof,
                               size_t cap, size_t* len) {
    const fri16::View v{inner_hash_width, betas, final_poly, indices, values, siblings, roots, paths, capacity, witness, trace_rows, quotient_rows, constants,
                        trace_paths, quotient_paths, trace_root, quotient_root};
    return fri16_prove({fri16::ROWPATHS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, "prove_fri16_rowpaths", ctx, key, v, prm, proof, cap, len);
}

int zkhip_verify_fri16_rowpaths(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                                const uint32_t public_values[40], const uint32_t vk[8], const zkhip_params* prm, int* reason) {
    return fri16::verify({fri16::ROWPATHS, R, F, log_blowup, n_queries, inner_pow_bits, trace_width}, proof, len, public_values, vk, prm, reason, "verify_fri16_rowpaths");
}

// ---------------------------------------------------------------- HEAD
size_t zkhip_fri16_head_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, int which, int kind,
                                 uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table) {
    return fri16::describe({fri16::HEAD, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, which, kind, out, cap_words, log_rows, main_width, pre_width, table);
}

int zkhip_fri16_head_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                              const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm,
                              uint32_t vk[8]) {
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.roots = roots; v.trace_root = trace_root; v.quotient_root = quotient_root;
    return fri16_key({fri16::HEAD, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "fri16_head_key_host", nullptr, v, prm, nullptr, vk);
}

int zkhip_fri16_head_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                         uint32_t n_inner_public, const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8],
                         const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.roots = roots; v.trace_root = trace_root; v.quotient_root = quotient_root;
    return fri16_key({fri16::HEAD, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "fri16_head_key", ctx, v, prm, key, vk);
}

size_t zkhip_fri16_head_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* prm) {
    return fri16::proof_size({fri16::HEAD, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, prm);
}

int zkhip_fri16_head_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                const uint32_t* inner_public, const uint32_t trace_root[8], const uint32_t quotient_root[8], const uint32_t* opened, const uint32_t* roots,
                                const uint32_t* final_poly, uint32_t witness, uint32_t* d_p2th, uint32_t* d_samples, uint32_t* d_opened, uint32_t constants[32],
                                uint32_t capacity[8]) {
    CHECK_CTX(ctx);
    const char* who = "fri16_head_gen_traces";
    fri16::Shape s;
    ZK_TRY(fri16::shape_of({fri16::HEAD, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, s));
    fri16::View v;
    v.inner_public = inner_public; v.trace_root = trace_root; v.quotient_root = quotient_root; v.opened = opened; v.roots = roots; v.final_poly = final_poly; v.witness = witness;
    ZK_TRY(fri16_head_check_inputs(s, v, who));
    if (!d_p2th || !d_samples || !d_opened || !constants || !capacity || ((uintptr_t)d_p2th | (uintptr_t)d_samples | (uintptr_t)d_opened) % 16)
        return fail(ZKHIP_ERR_INVALID, "fri16_head_gen_traces: 16-byte aligned dense traces (352, 288 and 36 columns), constants and capacity");
    fri16::Head h;
    fri16::walk_head(s, inner_public, trace_root, quotient_root, opened, h);
    v.capacity = h.capacity;
    ZK_TRY(fri16_indices_check_inputs(s, v, who));
    uint32_t sums[16];
    ZK_TRY(fri16_head_opened_impl(ctx, s, opened, h.fa, d_opened, sums));
    fri16::head_constants(s, h, sums, constants);
    std::memcpy(capacity, h.capacity, 32);
    fri16::Chain c;
    fri16::walk_chain(s, h.capacity, roots, final_poly, witness, c);
    c.inputs.insert(c.inputs.begin(), h.inputs.begin(), h.inputs.end());
    uint32_t status = 0;
    return fri16_transcript_impl(ctx, s, c, nullptr, nullptr, nullptr, d_p2th, d_samples, nullptr, nullptr, &status);
}

int zkhip_prove_fri16_head(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                           uint32_t trace_width, uint32_t n_inner_public, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                           const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness, const uint32_t* trace_rows,
                           const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* trace_paths, const uint32_t* quotient_paths,
                           const uint32_t trace_root[8], const uint32_t quotient_root[8], const uint32_t* inner_public, const uint32_t* opened, const zkhip_params* prm,
                           uint8_t* proof, size_t cap, size_t* len) {
    const fri16::View v{inner_hash_width, betas, final_poly, indices, values, siblings, roots, paths, capacity, witness, trace_rows, quotient_rows, constants,
                        trace_paths, quotient_paths, trace_root, quotient_root, inner_public, opened};
    return fri16_prove({fri16::HEAD, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "prove_fri16_head", ctx, key, v, prm, proof, cap, len);
}

int zkhip_verify_fri16_head(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                            uint32_t n_inner_public, const uint32_t* inner_public, const uint32_t vk[8], const zkhip_params* prm, int* reason) {
    return fri16::verify({fri16::HEAD, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, proof, len, inner_public, vk, prm, reason, "verify_fri16_head");
}

// ---------------------------------------------------------------- IDENTITY
size_t zkhip_fri16_identity_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, int which, int kind,
                                     uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table) {
    return fri16::describe({fri16::IDENTITY, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, which, kind, out, cap_words, log_rows, main_width, pre_width, table);
}

int zkhip_fri16_identity_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                  const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm,
                                  uint32_t vk[8]) {
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.roots = roots; v.trace_root = trace_root; v.quotient_root = quotient_root;
    return fri16_key({fri16::IDENTITY, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "fri16_identity_key_host", nullptr, v, prm, nullptr, vk);
}

int zkhip_fri16_identity_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                             uint32_t n_inner_public, const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8],
                             const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    fri16::View v;
    v.hash_width = inner_hash_width; v.final_poly = final_poly; v.roots = roots; v.trace_root = trace_root; v.quotient_root = quotient_root;
    return fri16_key({fri16::IDENTITY, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "fri16_identity_key", ctx, v, prm, key, vk);
}

size_t zkhip_fri16_identity_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* prm) {
    return fri16::proof_size({fri16::IDENTITY, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, prm);
}

int zkhip_fri16_identity_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                    const uint32_t alpha[4], const uint32_t zeta[4], const uint32_t* opened, uint32_t* d_air, uint32_t* d_scalars, uint32_t accumulators[8]) {
    CHECK_CTX(ctx);
    const char* who = "fri16_identity_gen_traces";
    fri16::Shape s;
    ZK_TRY(fri16::shape_of({fri16::IDENTITY, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, s));
    if (!alpha || !zeta || !opened || !d_air || !d_scalars || !accumulators || ((uintptr_t)d_air | (uintptr_t)d_scalars) % 16)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": alpha, zeta, the opened values, 16-byte aligned dense traces (56 and 4 (17 + log_n) columns) and the accumulators");
    if (!fri16::canonical(alpha, 4) || !fri16::canonical(zeta, 4)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the challenges must be canonical");
    if (!fri16::canonical(opened, 8 * ((size_t)s.W + 4))) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the opened values must be canonical");
    ZK_TRY(fri16_identity_check_zeta(zeta, who));
    return fri16_identity_rows_impl(ctx, s, opened, alpha, zeta, d_air, d_scalars, accumulators);
}

int zkhip_prove_fri16_identity(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                               uint32_t trace_width, uint32_t n_inner_public, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                               const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness, const uint32_t* trace_rows,
                               const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* trace_paths, const uint32_t* quotient_paths,
                               const uint32_t trace_root[8], const uint32_t quotient_root[8], const uint32_t* inner_public, const uint32_t* opened, const zkhip_params* prm,
                               uint8_t* proof, size_t cap, size_t* len) {
    const fri16::View v{inner_hash_width, betas, final_poly, indices, values, siblings, roots, paths, capacity, witness, trace_rows, quotient_rows, constants,
                        trace_paths, quotient_paths, trace_root, quotient_root, inner_public, opened};
    return fri16_prove({fri16::IDENTITY, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "prove_fri16_identity", ctx, key, v, prm, proof, cap, len);
}

int zkhip_verify_fri16_identity(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                                uint32_t n_inner_public, const uint32_t* inner_public, const uint32_t vk[8], const zkhip_params* prm, int* reason) {
    return fri16::verify({fri16::IDENTITY, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, proof, len, inner_public, vk, prm, reason, "verify_fri16_identity");
}

// ---------------------------------------------------------------- LIFT
size_t zkhip_fri16_lift_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, int which, int kind,
                                 uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table) {
    return fri16::describe({fri16::LIFT, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, which, kind, out, cap_words, log_rows, main_width, pre_width, table);
}

int zkhip_fri16_lift_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                              const zkhip_params* prm, uint32_t vk[8]) {
    fri16::View v;
    v.hash_width = inner_hash_width;
    return fri16_key({fri16::LIFT, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "fri16_lift_key_host", nullptr, v, prm, nullptr, vk);
}

int zkhip_fri16_lift_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                         uint32_t n_inner_public, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    fri16::View v;
    v.hash_width = inner_hash_width;
    return fri16_key({fri16::LIFT, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "fri16_lift_key", ctx, v, prm, key, vk);
}

size_t zkhip_fri16_lift_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* prm) {
    return fri16::proof_size({fri16::LIFT, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, prm);
}

// the lift launch alone, for the table tests: the words are staged as the transcript stage leaves them (a chain of input states: three stream rows with the trace root
// at stream words 10 .. 17, the quotient root's row, the R root rows, the coefficient rows) and ROOTS' first eight columns come out zero
int zkhip_fri16_lift_gen_tables(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, const uint32_t* roots, const uint32_t trace_root[8],
                                const uint32_t quotient_root[8], const uint32_t* final_poly, uint32_t* d_roots_main, uint32_t* d_coeffs_main) {
    CHECK_CTX(ctx);
    const char* who = "fri16_lift_gen_tables";
    // ROOTS and COEFFS depend on R and F alone, so every pair of 1..5 layers and log_final 0..8 is taken here, also those whose domain no whole machine has
    if (R < 1 || R > fri16::MAX_R || F < 0 || F > fri16::MAX_F || log_blowup < 1 || log_blowup > 3 || n_queries < 1 || n_queries > fri16::MAX_Q)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": 1..5 layers, log_final 0..8, log_blowup 1..3, 1..1024 queries");
    fri16::Shape s{};
    s.kind = fri16::LIFT; s.R = R; s.F = F; s.C = F >= 1 ? (size_t)1 << (F - 1) : 0;
    s.log_rows[fri16::T_ROOTS] = fri16::lg((size_t)R); s.log_rows[fri16::T_COEFFS] = fri16::lg((size_t)1 << F);
    if (!roots || !trace_root || !quotient_root || !final_poly || !d_roots_main || !d_coeffs_main || ((uintptr_t)d_roots_main | (uintptr_t)d_coeffs_main) % 16)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the roots, the final coefficients and 16-byte aligned dense traces (16 and 8 columns)");
    if (!fri16::canonical(roots, 8 * (size_t)s.R) || !fri16::canonical(final_poly, (size_t)4 << s.F)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": values must be canonical");
    if (!fri16::canonical(trace_root, 8) || !fri16::canonical(quotient_root, 8)) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the roots must be canonical");
    const size_t row_quotient = 3, row_layers = 4, rows = row_layers + (size_t)s.R + std::max<size_t>(s.C, 1);
    std::vector<uint32_t> up(16 * rows, 0u);
    for (size_t j = 0; j < 8; j++) { const size_t pos = fri16::LIFT_STREAM_ROOT + j; up[16 * (pos >> 3) + (pos & 7)] = trace_root[j]; }
    std::memcpy(up.data() + 16 * row_quotient, quotient_root, 32);
    for (size_t l = 0; l < (size_t)s.R; l++) std::memcpy(up.data() + 16 * (row_layers + l), roots + 8 * l, 32);
    for (size_t j = 0; j < ((size_t)1 << s.F); j++) std::memcpy(up.data() + 16 * (row_layers + (size_t)s.R + (j >> 1)) + 4 * (j & 1), final_poly + 4 * j, 16);
    void* stage;
    ZK_TRY(ctx_reserve(ctx, S_STAGE, up.size() * 4, &stage));
    ZK_TRY(dev_h2d(ctx, stage, up.data(), up.size() * 4));
    ZK_TRY(fri16_lift_tables_impl(ctx, s, (const uint32_t*)stage, (uint32_t)row_quotient, (uint32_t)row_layers, nullptr, d_roots_main, d_coeffs_main));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    return ZKHIP_OK;
}

int zkhip_prove_fri16_lift(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                           uint32_t trace_width, uint32_t n_inner_public, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                           const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness, const uint32_t* trace_rows,
                           const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* trace_paths, const uint32_t* quotient_paths,
                           const uint32_t trace_root[8], const uint32_t quotient_root[8], const uint32_t* inner_public, const uint32_t* opened, const zkhip_params* prm,
                           uint8_t* proof, size_t cap, size_t* len) {
    const fri16::View v{inner_hash_width, betas, final_poly, indices, values, siblings, roots, paths, capacity, witness, trace_rows, quotient_rows, constants,
                        trace_paths, quotient_paths, trace_root, quotient_root, inner_public, opened};
    return fri16_prove({fri16::LIFT, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, "prove_fri16_lift", ctx, key, v, prm, proof, cap, len);
}

int zkhip_verify_fri16_lift(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                            uint32_t n_inner_public, const uint32_t* inner_public, const uint32_t vk[8], const zkhip_params* prm, int* reason) {
    return fri16::verify({fri16::LIFT, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, proof, len, inner_public, vk, prm, reason, "verify_fri16_lift");
}

// segment proof in, lift proof out: ONE pass of the host verifier with every fold-16 view sink attached (verifier.cpp: fri16_view_all -- it fails with the verifier's
// code and message when the inner proof does not verify, and with the views' messages on a form they do not take), then the lift prover on what it left
}  // extern "C"

// (the body of zkhip_prove_fri16_lift_segment: the join's one-call entry makes its lift proofs with it)
static int fri16_lift_segment(zkhip_ctx* ctx, const zkhip_machine_key* key, const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values,
                              size_t n_public, const zkhip_params* inner_prm, const zkhip_params* outer_prm, uint8_t* out, size_t cap, size_t* out_len) {
    CHECK_CTX(ctx);
    if (!key || !proof || !public_values || !inner_prm || !outer_prm || !out || !out_len) return fail(ZKHIP_ERR_INVALID, "prove_fri16_lift_segment: null argument");
    if (n_public > fri16::MAX_NP) return fail(ZKHIP_ERR_INVALID, "prove_fri16_lift_segment: more than 30 inner public values");
    Fri16FullView f;
    ZK_TRY(fri16_view_all(proof, len, log_n, width, public_values, n_public, inner_prm, f));
    const fri16::View v{f.hash_width, f.betas.data(), f.final_poly.data(), f.indices.data(), f.values.data(), f.siblings.data(), f.roots.data(), f.paths.data(), f.transcript,
                        f.transcript[9], f.trace_rows.data(), f.quotient_rows.data(), f.constants, f.trace_paths.data(), f.quotient_paths.data(), f.trace_root, f.quotient_root,
                        public_values, f.opened.data()};
    return fri16_prove({fri16::LIFT, f.R, f.F, inner_prm->log_blowup, (size_t)inner_prm->num_queries, inner_prm->pow_bits, width, (uint32_t)n_public}, "prove_fri16_lift", ctx, key,
                       v, outer_prm, out, cap, out_len);
}

// ---------------------------------------------------------------- JOIN: N lift proofs of one shape -> one proof
// A lift proof is a version-11 proof of the thirteen-table lift machine, and the lift key depends on the shape alone: N lift proofs of one shape are N proofs of ONE keyed
// machine, which machine mode (machine_verifier.inl) verifies in-circuit.  The entries below are a SHAPE CALL: they put the zkhip_machine_desc together from what
// zkhip_fri16_lift_describe reads (the machine's programs and tables in machine order, the shape's key as key_root, the lift's queries and proof-of-work bits) and hand it
// to the function behind the generic entry of the same name -- no second prover, the same bytes.
namespace zk {
namespace mrec {      // (machine_verifier.inl: the bodies of the zkhip_*machine_verifier* entries)
int m_machine_verifier_setup(zkhip_ctx* ctx, const zkhip_machine_desc* inner, size_t n_proofs, const zkhip_params* outer, zkhip_machine_key** key, uint32_t vk[8]);
int m_machine_verifier_key_host(const zkhip_machine_desc* inner, size_t n_proofs, const zkhip_params* outer, uint32_t vk[8]);
size_t m_machine_verifier_proof_size(const zkhip_machine_desc* inner, size_t n_proofs, const zkhip_params* outer);
size_t m_machine_verifier_max_proofs(const zkhip_machine_desc* inner);
int m_prove_machine_verifier(zkhip_ctx* ctx, const zkhip_machine_key* key, const zkhip_machine_desc* inner, const uint8_t* const* proofs, const size_t* proof_lens, size_t n_proofs,
                             const uint32_t* public_values, size_t n_public, const zkhip_params* outer, uint8_t* proof, size_t cap, size_t* len);
int m_verify_machine_recursive(const zkhip_machine_desc* inner, const uint8_t* proof, size_t len, const uint32_t* public_values, size_t n_public, size_t n_proofs, const uint32_t vk[8],
                               const zkhip_params* outer, int* reason);
// (the tree above the join: a machine-mode machine as the description of the level above it, and the top over joins that the caller makes)
using JoinSink = std::function<int(size_t, const uint8_t*, size_t)>;
int m_machine_verifier_self_desc(const zkhip_machine_desc* inner, size_t n_proofs, const zkhip_params* outer, const uint32_t key_root[8], std::shared_ptr<const void>& keep,
                                 zkhip_machine_desc& d);
int m_prove_tree_top(zkhip_ctx* ctx, const zkhip_machine_key* top_key, const zkhip_machine_desc* join_machine, size_t n_joins, const uint32_t* public_values,
                     const zkhip_params* top_outer, const std::function<int(const JoinSink&)>& run_joins, uint8_t* proof, size_t cap, size_t* len);
}  // namespace mrec
}  // namespace zk

namespace {
struct JoinDesc { std::shared_ptr<const fri16::Machine> m; zkhip_machine_desc d; };      // (d points into m)
// the shape's key is a host commitment of the thirteen tables' preprocessed columns, and every entry of a prove / verify pair asks for it again: kept per (shape, lift
// parameters, Poseidon2 table set)
std::mutex g_join_mu;
std::map<std::array<uint64_t, 16>, std::array<uint32_t, 8>> g_join_roots;
// the lift machine of a shape as machine mode takes it
int fri16_join_desc(const fri16::ShapeArgs& a, int inner_hash_width, const zkhip_params* lift_prm, const char* who, JoinDesc& j) {
    if (!lift_prm) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    fri16::Shape s;
    ZK_TRY(fri16::shape_of(a, s));
    ZK_TRY(fri16::check_hash_width(inner_hash_width, who));
    j.m = fri16::machine_of(s);
    const keyed::KeyedMachine& km = j.m->km;
    j.d = zkhip_machine_desc{};
    j.d.n_chips = km.n; j.d.log_ns = km.log_ns; j.d.widths = km.widths; j.d.pre_widths = km.pre_widths;
    j.d.programs = km.progs; j.d.program_words = km.prog_words; j.d.tables = km.tabs; j.d.table_words = km.tab_words;
    j.d.num_queries = lift_prm->num_queries; j.d.pow_bits = lift_prm->pow_bits; j.d.n_public = a.NP;
    const std::array<uint64_t, 16> id{(uint64_t)a.R, (uint64_t)a.F, (uint64_t)a.b, (uint64_t)a.Q, (uint64_t)a.pow_bits, (uint64_t)a.W, (uint64_t)a.NP,
                                      (uint64_t)lift_prm->log_blowup, (uint64_t)lift_prm->num_queries, (uint64_t)lift_prm->pow_bits, (uint64_t)lift_prm->logup_pairs,
                                      (uint64_t)lift_prm->log_fold, (uint64_t)lift_prm->log_final, (uint64_t)lift_prm->hash_width, (uint64_t)lift_prm->code_width,
                                      zk::g_p2_generation.load()};
    {
        std::lock_guard<std::mutex> lk(g_join_mu);
        const auto it = g_join_roots.find(id);
        if (it != g_join_roots.end()) { std::memcpy(j.d.key_root, it->second.data(), 32); return ZKHIP_OK; }
    }
    fri16::View v;
    v.hash_width = inner_hash_width;
    ZK_TRY(fri16_key(a, who, nullptr, v, lift_prm, nullptr, j.d.key_root));
    std::array<uint32_t, 8> root;
    std::memcpy(root.data(), j.d.key_root, 32);
    std::lock_guard<std::mutex> lk(g_join_mu);
    if (g_join_roots.size() > 16) g_join_roots.clear();
    g_join_roots.emplace(id, root);
    return ZKHIP_OK;
}
// machine mode refused (rc, its message in zkhip_last_error): where n_proofs is what it did not take, the message names the bound -- found only now, on the way out, so
// that a call that goes through builds the machine's shape once
int fri16_join_refused(const JoinDesc& j, size_t n_proofs, const char* who, int rc) {
    const std::string why = zkhip_last_error();
    const size_t most = zk::mrec::m_machine_verifier_max_proofs(&j.d);
    if (most && (n_proofs < 1 || n_proofs > most))
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": 1 .. " + std::to_string(most) + " lift proofs of this shape go into one join, not " + std::to_string(n_proofs));
    return fail(rc, why);
}
int fri16_join_check_public(const JoinDesc& j, size_t n_proofs, const uint32_t* public_values, size_t n_public_total, const char* who) {
    if (!public_values || n_public_total != n_proofs * (size_t)j.d.n_public)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": public_values holds n_proofs x n_inner_public words in proof order (" + std::to_string(n_proofs * (size_t)j.d.n_public) +
                                       " here), not " + std::to_string(n_public_total));
    return ZKHIP_OK;
}
}  // namespace

#define FRI16_JOIN_GUARD(expr, on_error)                                                                                     \
    try { return expr; }                                                                                                     \
    catch (const std::bad_alloc&) { (void)fail(ZKHIP_ERR_NOMEM, "fri16 join: out of host memory"); return on_error; }        \
    catch (const std::exception& e) { (void)fail(ZKHIP_ERR_INTERNAL, std::string("fri16 join: ") + e.what()); return on_error; }

static int fri16_join_key_host(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm, uint32_t vk[8]) {
    JoinDesc j;
    ZK_TRY(fri16_join_desc(a, hw, lift_prm, "fri16_join_key_host", j));
    const int rc = zk::mrec::m_machine_verifier_key_host(&j.d, n_proofs, join_prm, vk);
    return rc == ZKHIP_ERR_INVALID ? fri16_join_refused(j, n_proofs, "fri16_join_key_host", rc) : rc;
}
static int fri16_join_setup(zkhip_ctx* ctx, const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm, zkhip_machine_key** key,
                            uint32_t vk[8]) {
    CHECK_CTX(ctx);
    JoinDesc j;
    ZK_TRY(fri16_join_desc(a, hw, lift_prm, "fri16_join_setup", j));
    const int rc = zk::mrec::m_machine_verifier_setup(ctx, &j.d, n_proofs, join_prm, key, vk);
    return rc == ZKHIP_ERR_INVALID ? fri16_join_refused(j, n_proofs, "fri16_join_setup", rc) : rc;
}
static size_t fri16_join_proof_size(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm) {
    JoinDesc j;
    if (fri16_join_desc(a, hw, lift_prm, "fri16_join_proof_size", j) != ZKHIP_OK) return 0;
    const size_t size = zk::mrec::m_machine_verifier_proof_size(&j.d, n_proofs, join_prm);
    if (!size) (void)fri16_join_refused(j, n_proofs, "fri16_join_proof_size", ZKHIP_ERR_INVALID);
    return size;
}
static size_t fri16_join_max_proofs(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm) {
    JoinDesc j;
    if (fri16_join_desc(a, hw, lift_prm, "fri16_join_max_proofs", j) != ZKHIP_OK) return 0;
    return zk::mrec::m_machine_verifier_max_proofs(&j.d);
}
static int fri16_join_prove_desc(zkhip_ctx* ctx, const zkhip_machine_key* key, const JoinDesc& j, const uint8_t* const* lift_proofs, const size_t* lens, size_t n_proofs,
                                 const uint32_t* public_values, size_t n_public_total, const zkhip_params* join_prm, uint8_t* out, size_t cap, size_t* len) {
    ZK_TRY(fri16_join_check_public(j, n_proofs, public_values, n_public_total, "prove_fri16_join"));
    const int rc = zk::mrec::m_prove_machine_verifier(ctx, key, &j.d, lift_proofs, lens, n_proofs, public_values, j.d.n_public, join_prm, out, cap, len);
    return rc == ZKHIP_ERR_INVALID ? fri16_join_refused(j, n_proofs, "prove_fri16_join", rc) : rc;
}
static int fri16_join_prove(zkhip_ctx* ctx, const zkhip_machine_key* key, const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, const uint8_t* const* lift_proofs,
                            const size_t* lens, size_t n_proofs, const uint32_t* public_values, size_t n_public_total, const zkhip_params* join_prm, uint8_t* out, size_t cap,
                            size_t* len) {
    CHECK_CTX(ctx);
    JoinDesc j;
    ZK_TRY(fri16_join_desc(a, hw, lift_prm, "prove_fri16_join", j));
    return fri16_join_prove_desc(ctx, key, j, lift_proofs, lens, n_proofs, public_values, n_public_total, join_prm, out, cap, len);
}
static int fri16_join_verify(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, const uint8_t* proof, size_t len, const uint32_t* public_values, size_t n_public_total,
                             size_t n_proofs, const uint32_t vk[8], const zkhip_params* join_prm, int* reason) {
    JoinDesc j;
    int rc = fri16_join_desc(a, hw, lift_prm, "verify_fri16_join", j);
    if (rc == ZKHIP_OK) rc = fri16_join_check_public(j, n_proofs, public_values, n_public_total, "verify_fri16_join");
    if (rc != ZKHIP_OK) { if (reason) *reason = 1; return rc; }
    int why = 0;
    rc = zk::mrec::m_verify_machine_recursive(&j.d, proof, len, public_values, j.d.n_public, n_proofs, vk, join_prm, &why);
    if (reason) *reason = why;
    return rc != ZKHIP_OK && why == 1 ? fri16_join_refused(j, n_proofs, "verify_fri16_join", rc) : rc;      // (reason 1: the arguments, the number of proofs among them)
}
// segment proofs in, one proof out, on ONE context: the lift proofs one after the other, then the join.  (The faster route to the same bytes is
// zkhip_prove_fri16_lift_batch -- the lifts side by side on the lock-step lanes, the key with the pooled contexts -- followed by zkhip_prove_fri16_join.)
static int fri16_join_segments(zkhip_ctx* ctx, const zkhip_machine_key* lift_key, const zkhip_machine_key* join_key, const uint8_t* const* segment_proofs, const size_t* lens,
                               size_t n_proofs, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public_total, const zkhip_params* inner_prm,
                               const zkhip_params* lift_prm, const zkhip_params* join_prm, uint8_t* out, size_t cap, size_t* len) {
    const char* who = "prove_fri16_join_segments";
    CHECK_CTX(ctx);
    if (!lift_key || !join_key || !segment_proofs || !lens || !public_values || !inner_prm || !lift_prm || !join_prm || !out || !len) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (n_proofs < 1 || n_public_total % n_proofs)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": at least one segment proof, and public_values with the same number of words for every segment, in segment order");
    if (inner_prm->log_fold != 4 || log_n <= inner_prm->log_final || (log_n - inner_prm->log_final) % 4)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": inner_prm is not a fold-by-16 shape with a committed layer at this height");
    const size_t n_public = n_public_total / n_proofs;
    // every segment has one shape -- the layers inner_prm gives at this height --, so the join's description, the number of proofs it takes and a lift proof's size are
    // known before the first segment is lifted
    const fri16::ShapeArgs a{fri16::LIFT, (log_n - inner_prm->log_final) / 4, inner_prm->log_final, inner_prm->log_blowup, (size_t)inner_prm->num_queries, inner_prm->pow_bits, width,
                             (uint32_t)n_public};
    JoinDesc j;
    ZK_TRY(fri16_join_desc(a, inner_prm->hash_width, lift_prm, who, j));
    if (!zk::mrec::m_machine_verifier_proof_size(&j.d, n_proofs, join_prm)) return fri16_join_refused(j, n_proofs, who, ZKHIP_ERR_INVALID);
    const size_t room = fri16::proof_size(a, lift_prm);
    // the lift proofs, one after the other on ctx
    std::vector<std::vector<uint8_t>> lifted(n_proofs);
    std::vector<const uint8_t*> ptrs(n_proofs);
    std::vector<size_t> lift_lens(n_proofs);
    for (size_t i = 0; i < n_proofs; i++) {
        if (!segment_proofs[i]) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
        lifted[i].resize(room);
        const int rc = fri16_lift_segment(ctx, lift_key, segment_proofs[i], lens[i], log_n, width, public_values + i * n_public, n_public, inner_prm, lift_prm, lifted[i].data(),
                                          room, &lift_lens[i]);
        if (rc != ZKHIP_OK) return fail(rc, std::string(who) + ": segment " + std::to_string(i) + ": " + zkhip_last_error());
        ptrs[i] = lifted[i].data();
    }
    return fri16_join_prove_desc(ctx, join_key, j, ptrs.data(), lift_lens.data(), n_proofs, public_values, n_public_total, join_prm, out, cap, len);
}

// ---------------------------------------------------------------- SEVERAL JOINS, and the TREE above them: more than one join's worth of segments -> one proof
// n_proofs / J joins of ONE shape (hence one key), zkhip_prove_shard_verifier_batch's way: join j takes the lift proofs [j J, (j + 1) J), goes to devices[j mod n_devices]
// and is proven on a pooled context that keeps the join's key (the rec_key slot: the signature below starts with a tag no shard-verifier signature starts with and has
// another length).  Every join is m_prove_machine_verifier on the lift machine's description: the bytes of zkhip_prove_fri16_join.  The joins in flight share the sixteen
// CPUs a caller may count on: each is told its share (t_query_threads_cap), which bounds the pool that fills its lift proofs' tables and what every fill starts.
// want_vk (the tree): the key every context must arrive at, checked before its first join is proven.  on_join: zk::mrec::JoinSink, run on the worker's thread right
// after join j exists; its failure is the join's.
static int fri16_join_batch(const char* who, const int* devices, int n_devices, const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, const uint8_t* const* lift_proofs,
                            const size_t* lens, size_t n_proofs, size_t J, const uint32_t* public_values, size_t n_public_total, const zkhip_params* join_prm,
                            int in_flight_per_device, int verify, uint8_t* joined, size_t joined_stride, size_t* joined_lens, uint32_t vk[8], const uint32_t* want_vk,
                            const zk::mrec::JoinSink* on_join) {
    const std::string me = who;
    if (!lift_proofs || !lens || !public_values || !lift_prm || !join_prm || !joined || !joined_lens || !vk) return fail(ZKHIP_ERR_INVALID, me + ": null argument");
    if (J == 0 || n_proofs == 0 || n_proofs % J != 0)
        return fail(ZKHIP_ERR_INVALID, me + ": the number of lift proofs must be a positive multiple of proofs_per_join, not " + std::to_string(n_proofs) + " for joins of " +
                                       std::to_string(J));
    const size_t n_joins = n_proofs / J;
    if (n_joins > (size_t)1 << 20) return fail(ZKHIP_ERR_INVALID, me + ": more than 2^20 joins");
    JoinDesc j;
    ZK_TRY(fri16_join_desc(a, hw, lift_prm, who, j));
    ZK_TRY(fri16_join_check_public(j, n_proofs, public_values, n_public_total, who));
    const size_t need = zk::mrec::m_machine_verifier_proof_size(&j.d, J, join_prm);
    if (!need) return fri16_join_refused(j, J, who, ZKHIP_ERR_INVALID);
    if (joined_stride < need) return fail(ZKHIP_ERR_INVALID, me + ": joined_stride is below zkhip_fri16_join_proof_size (" + std::to_string(need) + ")");
    for (size_t k = 0; k < n_proofs; k++) if (!lift_proofs[k]) return fail(ZKHIP_ERR_INVALID, me + ": null argument");
    for (size_t k = 0; k < n_joins; k++) joined_lens[k] = 0;
    std::memset(vk, 0, 32);
    std::vector<int> devs;
    ZK_TRY(resolve_devices(devices, n_devices, who, devs));
    std::vector<uint64_t> sig = {0x4A4F494E46523136ull /* "JOINFR16" */, (uint64_t)a.R, (uint64_t)a.F, (uint64_t)a.b, (uint64_t)a.Q, (uint64_t)(uint32_t)a.pow_bits, a.W, a.NP, (uint64_t)(uint32_t)hw, J};
    for (const zkhip_params* p : {lift_prm, join_prm})
        for (int v : {p->log_blowup, p->num_queries, p->pow_bits, p->logup_pairs, p->log_fold, p->log_final, p->hash_width, p->code_width}) sig.push_back((uint64_t)(uint32_t)v);
    sig.push_back(zk::g_p2_generation.load());
    const int nd = (int)devs.size();
    const size_t workers = std::min<size_t>(n_joins, (size_t)(in_flight_per_device > 0 ? in_flight_per_device : 4) * (size_t)nd);
    const int host_threads = workers >= 16 ? 1 : (int)(16 / workers);      // (a join's share of the sixteen CPUs, whatever the machine shows)
    const size_t NP = j.d.n_public;
    std::mutex mu;
    bool have_vk = false;
    std::vector<char> ran;
    auto run = [&](zkhip_ctx* ctx, int k) {
        int r = ZKHIP_OK;
        const int cap_before = t_query_threads_cap;
        t_query_threads_cap = host_threads;
        if (ctx->rec_key && ctx->rec_key_sig != sig) { (void)dev_sync(ctx); zkhip_machine_key_destroy(ctx->rec_key); ctx->rec_key = nullptr; }
        if (!ctx->rec_key) {
            r = zk::mrec::m_machine_verifier_setup(ctx, &j.d, J, join_prm, &ctx->rec_key, ctx->rec_vk);
            if (r == ZKHIP_OK) ctx->rec_key_sig = sig;
            else ctx->rec_key = nullptr;
        }
        if (r == ZKHIP_OK && want_vk && std::memcmp(want_vk, ctx->rec_vk, 32) != 0)
            r = fail(ZKHIP_ERR_INVALID, me + ": join_vk is not the key of joins of " + std::to_string(J) + " lift proofs of this shape (zkhip_fri16_join_key_host)");
        if (r == ZKHIP_OK) {
            std::lock_guard<std::mutex> lk(mu);
            if (!have_vk) { std::memcpy(vk, ctx->rec_vk, 32); have_vk = true; }
            else if (std::memcmp(vk, ctx->rec_vk, 32) != 0) r = fail(ZKHIP_ERR_INTERNAL, me + ": two contexts disagree about the key of the shape");
        }
        size_t len = 0;
        uint8_t* const out = joined + (size_t)k * joined_stride;
        const uint32_t* const pv = public_values + (size_t)k * J * NP;
        if (r == ZKHIP_OK) {
            r = zk::mrec::m_prove_machine_verifier(ctx, ctx->rec_key, &j.d, lift_proofs + (size_t)k * J, lens + (size_t)k * J, J, pv, NP, join_prm, out, joined_stride, &len);
            if (r == ZKHIP_OK && verify) r = zk::mrec::m_verify_machine_recursive(&j.d, out, len, pv, NP, J, ctx->rec_vk, join_prm, nullptr);
            if (r == ZKHIP_OK && on_join) r = (*on_join)((size_t)k, out, len);
            if (r != ZKHIP_OK) r = fail(r, me + ": join " + std::to_string(k) + ": " + zkhip_last_error());      // (machine mode's code, the join's name)
        }
        joined_lens[(size_t)k] = r == ZKHIP_OK ? len : 0;
        t_query_threads_cap = cap_before;
        return r;
    };
    return deal_jobs(devs.data(), nd, (int)n_joins, in_flight_per_device, run, ran);          // (0: four)
}

// the join machine of (shape, join size) as machine mode takes it one level up: the ten chips of the machine-mode machine over the lift machine, join_vk as key_root,
// join_prm's queries and proof-of-work bits, J x n_inner_public public values.  The lift's key is kept by fri16_join_desc and the machine by machine mode's own cache, per
// (description, join size): a call that comes again builds neither
namespace {
struct TreeDesc { JoinDesc lift; std::shared_ptr<const void> m; zkhip_machine_desc d; size_t J = 0; };      // (d points into m)
const uint32_t NO_KEY[8] = {0};                              // (the bounds do not depend on the key)
int fri16_tree_desc(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t J, const zkhip_params* join_prm, const uint32_t* join_vk, const char* who, TreeDesc& t) {
    if (!join_prm || !join_vk) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    ZK_TRY(fri16_join_desc(a, hw, lift_prm, who, t.lift));
    t.J = J;
    const int rc = zk::mrec::m_machine_verifier_self_desc(&t.lift.d, J, join_prm, join_vk, t.m, t.d);
    return rc == ZKHIP_ERR_INVALID ? fri16_join_refused(t.lift, J, who, rc) : rc;
}
// the top refused (its message in zkhip_last_error): where the number of joins, or the join size, is what it did not take, the message names the bound
int fri16_tree_refused(const TreeDesc& t, size_t n_joins, const char* who, int rc) {
    const std::string why = zkhip_last_error();
    const size_t most = zk::mrec::m_machine_verifier_max_proofs(&t.d);
    if (!most)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": no top takes a join of " + std::to_string(t.J) + " lift proofs of this shape (zkhip_fri16_tree_max_join gives the largest): " +
                                       zkhip_last_error());
    if (n_joins < 1 || n_joins > most)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": 1 .. " + std::to_string(most) + " joins of " + std::to_string(t.J) + " lift proofs of this shape go under one top, not " +
                                       std::to_string(n_joins));
    return fail(rc, why);
}
int fri16_tree_check_public(const TreeDesc& t, size_t n_joins, const uint32_t* public_values, size_t n_public_total, const char* who) {
    if (!public_values || n_public_total != n_joins * (size_t)t.d.n_public)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": public_values holds n_joins x proofs_per_join x n_inner_public words in segment order (" +
                                       std::to_string(n_joins * (size_t)t.d.n_public) + " here), not " + std::to_string(n_public_total));
    return ZKHIP_OK;
}
}  // namespace

static size_t fri16_tree_max_joins(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t J, const zkhip_params* join_prm) {
    TreeDesc t;
    if (fri16_tree_desc(a, hw, lift_prm, J, join_prm, NO_KEY, "fri16_tree_max_joins", t) != ZKHIP_OK) return 0;
    const size_t most = zk::mrec::m_machine_verifier_max_proofs(&t.d);
    if (!most) (void)fri16_tree_refused(t, 1, "fri16_tree_max_joins", ZKHIP_ERR_INVALID);
    return most;
}
// the largest join size whose join machine a top takes.  What machine mode bounds (the chips' heights, the public values per proof, the terms) grows with the join
// size, so the sizes a top takes are 1 .. the answer: found by bisection below what one join takes
static size_t fri16_tree_max_join(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, const zkhip_params* join_prm) {
    const char* who = "fri16_tree_max_join";
    if (!join_prm) { (void)fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument"); return 0; }
    JoinDesc j;
    if (fri16_join_desc(a, hw, lift_prm, who, j) != ZKHIP_OK) return 0;
    const size_t most = zk::mrec::m_machine_verifier_max_proofs(&j.d);
    if (!most) return 0;
    auto takes = [&](size_t J) {
        TreeDesc t;
        return fri16_tree_desc(a, hw, lift_prm, J, join_prm, NO_KEY, who, t) == ZKHIP_OK && zk::mrec::m_machine_verifier_max_proofs(&t.d) >= 1;
    };
    if (!takes(1)) { (void)fail(ZKHIP_ERR_INVALID, std::string(who) + ": no top takes a join of this shape, not even a join of one: " + zkhip_last_error()); return 0; }
    size_t lo = 1, hi = most;
    while (lo < hi) { const size_t mid = (lo + hi + 1) / 2; if (takes(mid)) lo = mid; else hi = mid - 1; }
    return lo;
}
static int fri16_tree_key_host(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t J, const zkhip_params* join_prm, const uint32_t* join_vk, size_t n_joins,
                               const zkhip_params* top_prm, uint32_t vk[8]) {
    TreeDesc t;
    ZK_TRY(fri16_tree_desc(a, hw, lift_prm, J, join_prm, join_vk, "fri16_tree_key_host", t));
    const int rc = zk::mrec::m_machine_verifier_key_host(&t.d, n_joins, top_prm, vk);
    return rc == ZKHIP_ERR_INVALID ? fri16_tree_refused(t, n_joins, "fri16_tree_key_host", rc) : rc;
}
static int fri16_tree_setup(zkhip_ctx* ctx, const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t J, const zkhip_params* join_prm, const uint32_t* join_vk,
                            size_t n_joins, const zkhip_params* top_prm, zkhip_machine_key** key, uint32_t vk[8]) {
    CHECK_CTX(ctx);
    TreeDesc t;
    ZK_TRY(fri16_tree_desc(a, hw, lift_prm, J, join_prm, join_vk, "fri16_tree_setup", t));
    const int rc = zk::mrec::m_machine_verifier_setup(ctx, &t.d, n_joins, top_prm, key, vk);
    return rc == ZKHIP_ERR_INVALID ? fri16_tree_refused(t, n_joins, "fri16_tree_setup", rc) : rc;
}
static size_t fri16_tree_proof_size(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t J, const zkhip_params* join_prm, const uint32_t* join_vk, size_t n_joins,
                                    const zkhip_params* top_prm) {
    TreeDesc t;
    if (fri16_tree_desc(a, hw, lift_prm, J, join_prm, join_vk, "fri16_tree_proof_size", t) != ZKHIP_OK) return 0;
    const size_t size = zk::mrec::m_machine_verifier_proof_size(&t.d, n_joins, top_prm);
    if (!size) (void)fri16_tree_refused(t, n_joins, "fri16_tree_proof_size", ZKHIP_ERR_INVALID);
    return size;
}
// m_prove_shard_tree for this side: the top's session begun, the join batch whose sink fills a join's tables for the top on the worker's thread the moment the join
// exists, the top finished on ctx -- the bytes of zkhip_prove_machine_verifier over the same joins
static int fri16_tree_prove(zkhip_ctx* ctx, const zkhip_machine_key* top_key, const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, const int* devices, int n_devices,
                            const uint8_t* const* lift_proofs, const size_t* lens, size_t n_proofs, size_t J, const uint32_t* public_values, size_t n_public_total,
                            const zkhip_params* join_prm, const uint32_t* join_vk, const zkhip_params* top_prm, int in_flight_per_device, uint8_t* joined, size_t joined_stride,
                            size_t* joined_lens, uint8_t* out, size_t cap, size_t* len) {
    const char* who = "prove_fri16_tree";
    CHECK_CTX(ctx);
    if (!top_key || !top_prm || !out || !len || !join_vk) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
    if (J == 0 || n_proofs == 0 || n_proofs % J != 0)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": the number of lift proofs must be a positive multiple of proofs_per_join, not " + std::to_string(n_proofs) +
                                       " for joins of " + std::to_string(J) + " (the caller pads by repeating the last)");
    if (joined_stride % 4 != 0) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": joined_stride must be a multiple of 4");
    const size_t n_joins = n_proofs / J;
    TreeDesc t;
    ZK_TRY(fri16_tree_desc(a, hw, lift_prm, J, join_prm, join_vk, who, t));
    ZK_TRY(fri16_tree_check_public(t, n_joins, public_values, n_public_total, who));
    if (!zk::mrec::m_machine_verifier_proof_size(&t.d, n_joins, top_prm)) return fri16_tree_refused(t, n_joins, who, ZKHIP_ERR_INVALID);
    uint32_t made_vk[8];
    return zk::mrec::m_prove_tree_top(ctx, top_key, &t.d, n_joins, public_values, top_prm, [&](const zk::mrec::JoinSink& on_join) -> int {
        return fri16_join_batch(who, devices, n_devices, a, hw, lift_prm, lift_proofs, lens, n_proofs, J, public_values, n_public_total, join_prm, in_flight_per_device, 0, joined,
                                joined_stride, joined_lens, made_vk, join_vk, &on_join);
    }, out, cap, len);
}
static int fri16_tree_verify(const fri16::ShapeArgs& a, int hw, const zkhip_params* lift_prm, size_t J, const zkhip_params* join_prm, const uint32_t* join_vk, size_t n_joins,
                             const uint8_t* proof, size_t len, const uint32_t* public_values, size_t n_public_total, const uint32_t* top_vk, const zkhip_params* top_prm, int* reason) {
    const char* who = "verify_fri16_tree";
    TreeDesc t;
    int rc = fri16_tree_desc(a, hw, lift_prm, J, join_prm, join_vk, who, t);
    if (rc == ZKHIP_OK) rc = fri16_tree_check_public(t, n_joins, public_values, n_public_total, who);
    if (rc != ZKHIP_OK) { if (reason) *reason = 1; return rc; }
    int why = 0;
    rc = zk::mrec::m_verify_machine_recursive(&t.d, proof, len, public_values, t.d.n_public, n_joins, top_vk, top_prm, &why);
    if (reason) *reason = why;
    return rc != ZKHIP_OK && why == 1 ? fri16_tree_refused(t, n_joins, who, rc) : rc;      // (reason 1: the arguments, the number of joins among them)
}

extern "C" {
int zkhip_prove_fri16_lift_segment(zkhip_ctx* ctx, const zkhip_machine_key* key, const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values,
                                   size_t n_public, const zkhip_params* inner_prm, const zkhip_params* outer_prm, uint8_t* out, size_t cap, size_t* out_len) {
    return fri16_lift_segment(ctx, key, proof, len, log_n, width, public_values, n_public, inner_prm, outer_prm, out, cap, out_len);
}

// ---- many segment proofs lifted in one call: what stands between the segments and the join (RISC Zero: segments -> lift -> join).  Per job: every fold-16 view of
// the segment proof from ONE pass of the host verifier (on a small pool that runs ahead of the device work), then the lift prover -- fri16_prove at kind LIFT, the body
// of zkhip_prove_fri16_lift_segment -- under the shape's key, which stays with the pooled context.  A lift proof is a few hundred launches over thirteen small
// tables: the jobs are dealt over the lock-step lanes (batch.h) like every launch-bound batch of this library, one context per worker otherwise.  All jobs share
// (log_n, width, n_public, inner_prm): one machine shape, one key.
int zkhip_prove_fri16_lift_batch(const int* devices, int n_devices, zkhip_fri16_lift_job* jobs, int n_jobs, int log_n, uint32_t width, size_t n_public,
                                 const zkhip_params* inner_prm, const zkhip_params* outer_prm, int in_flight_per_device, int verify, uint32_t vk[8]) {
    const char* who = "prove_fri16_lift_batch";
    if (!jobs || n_jobs < 0 || !inner_prm || !outer_prm || !vk) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": bad arguments");
    for (int i = 0; i < n_jobs; i++) { jobs[i].status = ZKHIP_ERR_INVALID; jobs[i].proof_len = 0; }
    std::memset(vk, 0, 32);
    if (inner_prm->log_fold != 4 || log_n <= inner_prm->log_final || (log_n - inner_prm->log_final) % 4)
        return fail(ZKHIP_ERR_INVALID, std::string(who) + ": inner_prm is not a fold-by-16 shape with a committed layer at this height");
    if (n_public > fri16::MAX_NP) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": more than 30 inner public values");
    const fri16::ShapeArgs a{fri16::LIFT, (log_n - inner_prm->log_final) / 4, inner_prm->log_final, inner_prm->log_blowup, (size_t)inner_prm->num_queries, inner_prm->pow_bits,
                             width, (uint32_t)n_public};
    fri16::Shape s;
    ZK_TRY(fri16::shape_of(a, s));
    const size_t need = fri16::proof_size(a, outer_prm);
    if (!need) return fail(ZKHIP_ERR_INVALID, std::string(who) + ": outer_prm gives the lift machine of this shape no proof");
    std::vector<int> devs;
    const int rc = resolve_devices(devices, n_devices, who, devs);
    if (rc == ZKHIP_ERR_NO_DEVICE) {
        for (int i = 0; i < n_jobs; i++) jobs[i].status = ZKHIP_ERR_NO_DEVICE;
        return n_jobs == 0 ? ZKHIP_OK : rc;
    }
    if (rc != ZKHIP_OK) return rc;
    if (n_jobs == 0) return ZKHIP_OK;
    // which way the jobs are dealt, known first: the host threads of the views are what the lanes (or workers) leave of the sixteen CPUs a caller may count on
    const auto m = fri16::machine_of(s);
    uint64_t cells = 0;
    for (int c = 0; c < m->km.n; c++) cells += ((uint64_t)(m->km.widths[c] + m->km.pre_widths[c])) << m->km.log_ns[c];
    const int nd = (int)devs.size(), max_batch = lockstep_batch();
    const bool lanes = max_batch > 1 && cells <= LOCKSTEP_MAX_CELLS && n_jobs >= 2 * nd;
    const int busy = lanes ? lockstep_lanes() * nd : (in_flight_per_device > 0 ? in_flight_per_device : 4) * nd;
    const int host_cpus = 16 - busy < 2 ? 2 : 16 - busy;
    const int n_viewers = n_jobs < host_cpus ? n_jobs : (host_cpus > 8 ? 8 : host_cpus);
    const int view_threads = host_cpus / n_viewers;              // (few jobs: each view's query checks spread over what is left)
    const int check_threads = lanes ? 1 : (16 / busy < 1 ? 1 : 16 / busy);      // verify: one thread per check on the pool beside the lanes, a worker's share on its own thread
    // (a) the views: one host pass over every segment proof, ahead of the device work (job i waits for view i only)
    struct View { Fri16FullView f; int rc = ZKHIP_OK; std::string msg; std::mutex mu; std::condition_variable cv; bool done = false; };
    std::vector<View> views((size_t)n_jobs);
    HostPool viewers(n_viewers);
    for (int i = 0; i < n_jobs; i++)
        viewers.submit([&, i] {
            View& v = views[(size_t)i];
            const zkhip_fri16_lift_job& j = jobs[i];
            t_query_threads_cap = view_threads;
            try {
                if (!j.segment_proof || !j.public_values) v.rc = fail(ZKHIP_ERR_INVALID, std::string(who) + ": null argument");
                else v.rc = fri16_view_all(j.segment_proof, j.segment_proof_len, log_n, width, j.public_values, n_public, inner_prm, v.f);
                if (v.rc != ZKHIP_OK) v.msg = zkhip_last_error();
            } catch (const std::bad_alloc&) { v.rc = ZKHIP_ERR_NOMEM; v.msg = std::string(who) + ": out of host memory"; }
            catch (const std::exception& e) { v.rc = ZKHIP_ERR_INTERNAL; v.msg = std::string(who) + ": " + e.what(); }
            t_query_threads_cap = 0;
            { std::lock_guard<std::mutex> lk(v.mu); v.done = true; }
            v.cv.notify_all();
        });
    // (b) the shape's key (once per context) and the proof per job on the devices
    const std::vector<uint64_t> sig = {(uint64_t)a.R, (uint64_t)a.F, (uint64_t)a.b, (uint64_t)a.Q, (uint64_t)(uint32_t)a.pow_bits, a.W, a.NP, (uint64_t)(uint32_t)inner_prm->hash_width,
                                       (uint64_t)(uint32_t)outer_prm->log_blowup, (uint64_t)(uint32_t)outer_prm->num_queries, (uint64_t)(uint32_t)outer_prm->pow_bits,
                                       (uint64_t)(uint32_t)outer_prm->logup_pairs, (uint64_t)(uint32_t)outer_prm->log_fold, (uint64_t)(uint32_t)outer_prm->log_final,
                                       (uint64_t)(uint32_t)outer_prm->hash_width, (uint64_t)(uint32_t)outer_prm->code_width, zk::g_p2_generation.load()};
    std::mutex mu;
    bool have_vk = false;
    std::unique_ptr<HostPool> checkers;
    std::vector<std::string> check_msg((size_t)n_jobs);
    std::vector<char> ran;
    auto run = [&](zkhip_ctx* ctx, int i) {
        zkhip_fri16_lift_job& j = jobs[i];
        View& v = views[(size_t)i];
        { std::unique_lock<std::mutex> lk(v.mu); v.cv.wait(lk, [&] { return v.done; }); }
        if (v.rc != ZKHIP_OK) { batch_leave(); j.status = v.rc; set_error(v.msg); return v.rc; }      // (nothing of this job reaches the device; the other members do not wait for it)
        int r = j.proof && j.proof_cap >= need ? ZKHIP_OK : fail(ZKHIP_ERR_INVALID, std::string(who) + ": proof buffer too small (zkhip_fri16_lift_proof_size)");
        if (r == ZKHIP_OK && ctx->lift_key && ctx->lift_key_sig != sig) { (void)dev_sync(ctx); zkhip_machine_key_destroy(ctx->lift_key); ctx->lift_key = nullptr; }
        if (r == ZKHIP_OK && !ctx->lift_key) {
            fri16::View kv;
            kv.hash_width = inner_prm->hash_width;
            r = fri16_key(a, who, ctx, kv, outer_prm, &ctx->lift_key, ctx->lift_vk);
            if (r == ZKHIP_OK) ctx->lift_key_sig = sig;
            else ctx->lift_key = nullptr;
        }
        if (r == ZKHIP_OK) {
            std::lock_guard<std::mutex> lk(mu);
            if (!have_vk) { std::memcpy(vk, ctx->lift_vk, 32); have_vk = true; }
            else if (std::memcmp(vk, ctx->lift_vk, 32) != 0) r = fail(ZKHIP_ERR_INTERNAL, std::string(who) + ": two contexts disagree about the key of the shape");
        }
        size_t len = 0;
        if (r == ZKHIP_OK) {
            const Fri16FullView& f = v.f;
            const fri16::View fv{f.hash_width, f.betas.data(), f.final_poly.data(), f.indices.data(), f.values.data(), f.siblings.data(), f.roots.data(), f.paths.data(),
                                 f.transcript, f.transcript[9], f.trace_rows.data(), f.quotient_rows.data(), f.constants, f.trace_paths.data(), f.quotient_paths.data(),
                                 f.trace_root, f.quotient_root, j.public_values, f.opened.data()};
            r = fri16_prove(a, "prove_fri16_lift", ctx, ctx->lift_key, fv, outer_prm, j.proof, j.proof_cap, &len);
        }
        batch_leave();                                           // (lock-step batch: the rest is host work)
        j.status = r;
        j.proof_len = r == ZKHIP_OK ? len : 0;
        if (r == ZKHIP_OK && verify) {
            uint32_t key[8];
            std::memcpy(key, ctx->lift_vk, 32);
            auto check = [&jobs, &check_msg, i, len, a, n_public, p = *outer_prm, key, check_threads] {
                zkhip_fri16_lift_job& jj = jobs[i];
                const int cap_before = t_query_threads_cap;      // (the checks run beside the lanes or workers: the same budget as the views)
                t_query_threads_cap = check_threads;
                const int c = zkhip_verify_fri16_lift(jj.proof, len, a.R, a.F, a.b, a.Q, a.pow_bits, a.W, (uint32_t)n_public, jj.public_values, key, &p, nullptr);
                t_query_threads_cap = cap_before;
                if (c != ZKHIP_OK) { jj.status = c; jj.proof_len = 0; check_msg[(size_t)i] = zkhip_last_error(); }
            };
            if (checkers && t_batcher) checkers->submit(check);
            else { check(); r = j.status; if (r != ZKHIP_OK) set_error(check_msg[(size_t)i]); }
        }
        return r;
    };
    int rcj;
    if (lanes) {
        if (verify) checkers.reset(new HostPool(host_cpus > 8 ? 8 : host_cpus));
        std::vector<int> shape((size_t)n_jobs, 0);
        rcj = deal_jobs_lockstep(devs.data(), nd, n_jobs, shape.data(), max_batch, lockstep_lanes(), run, ran,
                                 cells << (outer_prm->log_blowup > 1 ? outer_prm->log_blowup - 1 : 0));
    } else
        rcj = deal_jobs(devs.data(), nd, n_jobs, in_flight_per_device, run, ran);
    std::string msg = rcj != ZKHIP_OK ? zkhip_last_error() : "";
    viewers.wait();                                              // (a failing call may return before every view was looked at)
    if (checkers) {
        checkers->wait();
        for (int i = 0; i < n_jobs && rcj == ZKHIP_OK; i++)
            if (!check_msg[(size_t)i].empty()) { rcj = jobs[i].status; msg = check_msg[(size_t)i]; }
    }
    if (rcj != ZKHIP_OK) set_error(msg);
    return rcj;
}

#define FRI16_JOIN_SHAPE int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public
#define FRI16_JOIN_ARGS fri16::ShapeArgs{fri16::LIFT, R, F, log_blowup, n_queries, inner_pow_bits, trace_width, n_inner_public}, inner_hash_width
int zkhip_fri16_join_key_host(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm, uint32_t vk[8]) {
    FRI16_JOIN_GUARD(fri16_join_key_host(FRI16_JOIN_ARGS, lift_prm, n_proofs, join_prm, vk), ZKHIP_ERR_NOMEM)
}
int zkhip_fri16_join_setup(zkhip_ctx* ctx, FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm, zkhip_machine_key** key, uint32_t vk[8]) {
    FRI16_JOIN_GUARD(fri16_join_setup(ctx, FRI16_JOIN_ARGS, lift_prm, n_proofs, join_prm, key, vk), ZKHIP_ERR_NOMEM)
}
size_t zkhip_fri16_join_proof_size(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm) {
    FRI16_JOIN_GUARD(fri16_join_proof_size(FRI16_JOIN_ARGS, lift_prm, n_proofs, join_prm), 0)
}
size_t zkhip_fri16_join_max_proofs(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm) { FRI16_JOIN_GUARD(fri16_join_max_proofs(FRI16_JOIN_ARGS, lift_prm), 0) }
int zkhip_prove_fri16_join(zkhip_ctx* ctx, const zkhip_machine_key* key, FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, const uint8_t* const* lift_proofs, const size_t* lens,
                           size_t n_proofs, const uint32_t* public_values, size_t n_public_total, const zkhip_params* join_prm, uint8_t* out, size_t cap, size_t* len) {
    FRI16_JOIN_GUARD(fri16_join_prove(ctx, key, FRI16_JOIN_ARGS, lift_prm, lift_proofs, lens, n_proofs, public_values, n_public_total, join_prm, out, cap, len), ZKHIP_ERR_NOMEM)
}
int zkhip_verify_fri16_join(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, const uint8_t* proof, size_t len, const uint32_t* public_values, size_t n_public_total, size_t n_proofs,
                            const uint32_t vk[8], const zkhip_params* join_prm, int* reason) {
    FRI16_JOIN_GUARD(fri16_join_verify(FRI16_JOIN_ARGS, lift_prm, proof, len, public_values, n_public_total, n_proofs, vk, join_prm, reason), ZKHIP_ERR_NOMEM)
}
int zkhip_prove_fri16_join_segments(zkhip_ctx* ctx, const zkhip_machine_key* lift_key, const zkhip_machine_key* join_key, const uint8_t* const* segment_proofs, const size_t* lens,
                                    size_t n_proofs, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public_total, const zkhip_params* inner_prm,
                                    const zkhip_params* lift_prm, const zkhip_params* join_prm, uint8_t* out, size_t cap, size_t* len) {
    FRI16_JOIN_GUARD(fri16_join_segments(ctx, lift_key, join_key, segment_proofs, lens, n_proofs, log_n, width, public_values, n_public_total, inner_prm, lift_prm, join_prm, out, cap,
                                         len), ZKHIP_ERR_NOMEM)
}
// ---- several joins of one shape in one call, and the tree above them (the shape calls' bodies: fri16_join_batch, fri16_tree_* above)
int zkhip_prove_fri16_join_batch(const int* devices, int n_devices, FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, const uint8_t* const* lift_proofs, const size_t* lens,
                                 size_t n_proofs, size_t proofs_per_join, const uint32_t* public_values, size_t n_public_total, const zkhip_params* join_prm,
                                 int in_flight_per_device, int verify, uint8_t* joined, size_t joined_stride, size_t* joined_lens, uint32_t vk[8]) {
    FRI16_JOIN_GUARD(fri16_join_batch("prove_fri16_join_batch", devices, n_devices, FRI16_JOIN_ARGS, lift_prm, lift_proofs, lens, n_proofs, proofs_per_join, public_values,
                                      n_public_total, join_prm, in_flight_per_device, verify, joined, joined_stride, joined_lens, vk, nullptr, nullptr), ZKHIP_ERR_NOMEM)
}
size_t zkhip_fri16_tree_max_join(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, const zkhip_params* join_prm) {
    FRI16_JOIN_GUARD(fri16_tree_max_join(FRI16_JOIN_ARGS, lift_prm, join_prm), 0)
}
size_t zkhip_fri16_tree_max_joins(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm) {
    FRI16_JOIN_GUARD(fri16_tree_max_joins(FRI16_JOIN_ARGS, lift_prm, proofs_per_join, join_prm), 0)
}
int zkhip_fri16_tree_key_host(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm, const uint32_t join_vk[8], size_t n_joins,
                              const zkhip_params* top_prm, uint32_t vk[8]) {
    FRI16_JOIN_GUARD(fri16_tree_key_host(FRI16_JOIN_ARGS, lift_prm, proofs_per_join, join_prm, join_vk, n_joins, top_prm, vk), ZKHIP_ERR_NOMEM)
}
int zkhip_fri16_tree_setup(zkhip_ctx* ctx, FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm, const uint32_t join_vk[8],
                           size_t n_joins, const zkhip_params* top_prm, zkhip_machine_key** key, uint32_t vk[8]) {
    FRI16_JOIN_GUARD(fri16_tree_setup(ctx, FRI16_JOIN_ARGS, lift_prm, proofs_per_join, join_prm, join_vk, n_joins, top_prm, key, vk), ZKHIP_ERR_NOMEM)
}
size_t zkhip_fri16_tree_proof_size(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm, const uint32_t join_vk[8], size_t n_joins,
                                   const zkhip_params* top_prm) {
    FRI16_JOIN_GUARD(fri16_tree_proof_size(FRI16_JOIN_ARGS, lift_prm, proofs_per_join, join_prm, join_vk, n_joins, top_prm), 0)
}
int zkhip_prove_fri16_tree(zkhip_ctx* ctx, const zkhip_machine_key* top_key, FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, const int* devices, int n_devices,
                           const uint8_t* const* lift_proofs, const size_t* lens, size_t n_proofs, size_t proofs_per_join, const uint32_t* public_values, size_t n_public_total,
                           const zkhip_params* join_prm, const uint32_t join_vk[8], const zkhip_params* top_prm, int in_flight_per_device, uint8_t* joined, size_t joined_stride,
                           size_t* joined_lens, uint8_t* out, size_t cap, size_t* len) {
    FRI16_JOIN_GUARD(fri16_tree_prove(ctx, top_key, FRI16_JOIN_ARGS, lift_prm, devices, n_devices, lift_proofs, lens, n_proofs, proofs_per_join, public_values, n_public_total,
                                      join_prm, join_vk, top_prm, in_flight_per_device, joined, joined_stride, joined_lens, out, cap, len), ZKHIP_ERR_NOMEM)
}
int zkhip_verify_fri16_tree(FRI16_JOIN_SHAPE, const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm, const uint32_t join_vk[8], size_t n_joins,
                            const uint8_t* proof, size_t len, const uint32_t* public_values, size_t n_public_total, const uint32_t top_vk[8], const zkhip_params* top_prm,
                            int* reason) {
    FRI16_JOIN_GUARD(fri16_tree_verify(FRI16_JOIN_ARGS, lift_prm, proofs_per_join, join_prm, join_vk, n_joins, proof, len, public_values, n_public_total, top_vk, top_prm, reason),
                     ZKHIP_ERR_NOMEM)
}
#undef FRI16_JOIN_SHAPE
#undef FRI16_JOIN_ARGS
#undef FRI16_JOIN_GUARD

}  // extern "C"
