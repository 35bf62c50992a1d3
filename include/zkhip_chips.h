/*
 * zkhip_chips.h -- the CHIP LEVEL of libzkhip.so: what include/zkhip.h's provers are made of, for callers that build machines of their own or look inside.
 *   - chip programs (constraint programs as data: the synthetic AIR, the SHA-256 compression chip, the Poseidon2 permutation chip, the FRI-fold chip
 *     and its variants) and their trace generators on the device;
 *   - the descriptions of the recursion machines (programs, interaction tables, preprocessed traces per chip) that a verifier derives keys from, and
 *     the host-side table hook the tests compare the device's witness kernels with;
 *   - the Poseidon2 chip's Merkle-path prover and the FRI-only recursion mode (zkhip_prove_fri_indices[_batch]: the cheap mode whose verifier reads
 *     the inner proof; the whole-verifier machines are zkhip.h's zkhip_prove_shard_verifier / zkhip_prove_machine_verifier).  Round 6 removed the
 *     three earlier FRI-only generations (zkhip_prove_fri_queries / _layers / _transcript with their keys, sizes, trace generators and verifiers):
 *     their chips live on as the FOLD, SAMPLES and Poseidon2 chips of the shard verifier machines, their programs and views below;
 *   - the fold-by-16 line (RISC Zero-shape inner proofs), one machine per verifier step: zkhip_prove_fri16, _paths, _indices, _openings, _rowpaths and _head
 *     (the head of the transcript: the machine whose public values are the inner proof's own);
 *   - diagnostics and self-tests.
 * Each entry names the upstream structure it stands in for (sp1-core-machine / sp1-recursion chips, reference Cargo.lock:5822, 6047, 6172).
 */
#ifndef ZKHIP_CHIPS_H
#define ZKHIP_CHIPS_H
#include "zkhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A second real chip: the width-16 Poseidon2 permutation with Merkle-path chaining -- what a recursion machine (a STARK verifier proven
 * inside a STARK: the compress / shrink / wrap stages behind SP1ProofMode::Groth16, crates/guest-prover-sp1/src/sp1.rs:116; sp1-recursion's
 * Poseidon2 chips, reference Cargo.lock:6172 ff.) spends its rows on.  One row = one permutation of the parameter set in effect, every
 * intermediate in a column (ZKHIP_P2CHIP_WIDTH = 360 columns, degree <= 3); flag columns chain rows into Merkle paths (a row's
 * digest-carrying input half = the previous row's digest), into LEAF HASHES (the overwrite-mode sponge over an opened row: a row's capacity
 * half = the previous row's) and count the paths that end in the public root.  Public values: root[8], count.  zkhip_p2chip_air writes the constraint program (returns its size in words; the program follows the Poseidon2 tables, so reload
 * it after zkhip_load_poseidon2_params).  zkhip_p2chip_gen_merkle_trace fills a device trace of 2^log_n rows from host arrays: with
 * row_width = 0 path p = `depth` rows and leaves[p][8] is its leaf digest; with row_width = 8 k, leaves[p][row_width] is the OPENED ROW and the
 * path starts with k sponge rows that hash it (a whole opening of a commitment: what a verifier checks per query and matrix);
 * siblings[p][l][8] the sibling at level l, bit l of indices[p] = "the node is a
 * right child at level l" (canonical words); roots[p][8] receives where each path ends.  zkhip_prove_merkle_paths = trace + proof of
 * "I know n_paths Merkle paths that end in root" (refuses paths that do not); zkhip_verify_merkle_paths checks one (the trace height is
 * read from the proof).  The proofs are zkhip_prove_shard_air proofs (version 7). */
#define ZKHIP_P2CHIP_WIDTH 360
size_t zkhip_p2chip_air(uint32_t* program, size_t cap_words);
int zkhip_p2chip_gen_merkle_trace(zkhip_ctx* ctx, const uint32_t* leaves, uint32_t row_width, const uint32_t* siblings, const uint32_t* indices, size_t n_paths,
                                  int depth, int log_n, uint32_t* d_trace, size_t ld, uint32_t* roots);
size_t zkhip_merkle_paths_proof_size(size_t n_paths, int depth, uint32_t row_width, const zkhip_params* prm);
int zkhip_prove_merkle_paths(zkhip_ctx* ctx, const uint32_t* leaves, uint32_t row_width, const uint32_t* siblings, const uint32_t* indices, size_t n_paths, int depth,
                             const uint32_t root[8], const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_merkle_paths(const uint8_t* proof, size_t len, const uint32_t root[8], size_t n_paths, const zkhip_params* prm, int* reason);

/* The same chip for RISC Zero-shape commitments: the width-24 Poseidon2 permutation (rate 16, overwrite-mode sponge from the zero state,
 * digest = state[0..8]; parent = permute(l || r || 0^8)[0..8]) -- the hash of zkhip_prove_segment, of every prover given hash_width = 24 and
 * of zkhip_merkle_commit_p24_colmajor.  One row = one width-24 permutation of the tables in effect (ZKHIP_P24CHIP_WIDTH = 540 columns,
 * degree <= 3); the flag columns are the width-16 chip's, plus three group flags for a partial last sponge block: opened rows are a multiple
 * of 4 wide, so a leaf's last block absorbs 4, 8, 12 or 16 values and the rate words it does not absorb carry over (zero on a leaf's first
 * row, the previous output on a later one).  Public values: root[8], count.  zkhip_p24chip_air writes the constraint program (it follows
 * the width-24 tables: reload it after zkhip_load_poseidon2_params with a width-24 file).  zkhip_p24chip_gen_merkle_trace fills a device
 * trace of 2^log_n rows (ld >= 540 and a multiple of 4, 16-byte aligned): with row_width = 0 leaves[p][8] is a leaf digest; with row_width
 * a positive multiple of 4 (up to 1024) leaves[p][row_width] is the OPENED ROW and the path starts with ceil(row_width / 16) sponge rows;
 * siblings, indices and roots as above.  zkhip_prove_merkle_paths_p24 / zkhip_verify_merkle_paths_p24: as the width-16 entries (paths that
 * do not end in root are refused before anything is proven; the verifier needs no GPU and reads the trace height from the proof).  Any
 * proof shape is accepted, the SP1 default and the RISC Zero shape (log_blowup 2, log_fold 4, hash_width 24) among them.  One bus variant
 * exists: the layer-paths table P24L of the fold-16 paths machine (zkhip_prove_fri16_paths below).  Not yet: its use inside the recursion
 * machines. */
#define ZKHIP_P24CHIP_WIDTH 540
size_t zkhip_p24chip_air(uint32_t* program, size_t cap_words);
int zkhip_p24chip_gen_merkle_trace(zkhip_ctx* ctx, const uint32_t* leaves, uint32_t row_width, const uint32_t* siblings, const uint32_t* indices, size_t n_paths,
                                   int depth, int log_n, uint32_t* d_trace, size_t ld, uint32_t* roots);
size_t zkhip_merkle_paths_p24_proof_size(size_t n_paths, int depth, uint32_t row_width, const zkhip_params* prm);
int zkhip_prove_merkle_paths_p24(zkhip_ctx* ctx, const uint32_t* leaves, uint32_t row_width, const uint32_t* siblings, const uint32_t* indices, size_t n_paths,
                                 int depth, const uint32_t root[8], const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_merkle_paths_p24(const uint8_t* proof, size_t len, const uint32_t root[8], size_t n_paths, const zkhip_params* prm, int* reason);

/* ---- a first step of recursion: the FRI part of a shard proof checked INSIDE a proof (second half).  The reference's
 * hot call is client.prove(.., SP1ProofMode::Groth16) (crates/guest-prover-sp1/src/sp1.rs:116): core -> compress -> shrink -> wrap, and
 * compress verifies shard proofs in-circuit (sp1-recursion, reference Cargo.lock:6172 ff.; RISC Zero lift -> join, prover.rs:90).
 * zkhip_fri_view_shard runs the verifier of a zkhip_prove_shard proof (fold by 2, constant final value: the SP1 shape) and hands out what
 * its FRI check reads: layers = log_n folding challenges (4 words each), the final value, and per query the index (layers + 1 bits), the
 * reduced opening it starts from and one sibling per layer -- canonical words; fails like zkhip_verify_shard if the proof is rejected.
 * The FRI-fold chip (fri_chip.hip; 32 + layers columns rounded up to a multiple of 4, one row per (query, layer), degree 3) folds these
 * chains; its rows send the layer pairs on two lookup buses to a PREPROCESSED table that lists every distinct pair of the view with the
 * number of queries reading it -- fixed multiplicities, so every listed pair is folded exactly as often as the inner proof reads it.
 * That two-chip machine was the first generation (zkhip_prove_fri_queries; removed in round 6 with its key, size, trace generator and
 * verifier): the chip lives on as the fold chip of the machines below and of the shard verifier.  zkhip_fri_chip_air writes its
 * constraint program (its size in words), zkhip_fri_chip_width its width. */
int zkhip_fri_view_shard(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public,
                         const zkhip_params* prm, uint32_t* betas, uint32_t final_value[4], uint32_t* indices, uint32_t* values, uint32_t* siblings);
uint32_t zkhip_fri_chip_width(int layers);
size_t zkhip_fri_chip_air(int layers, uint32_t* program, size_t cap_words);
/* The same with the Merkle paths of the pairs IN-CIRCUIT (blowup-2 proofs): the FRI-fold chip wired by lookups to the Poseidon2 chip.
 * zkhip_fri_view_shard_paths also hands out the layer roots ([layers][8]) and, per query, the layers' authentication paths one after the
 * other (8 (layers - l) words for layer l; zkhip_fri_view_path_words(layers) words per query).  The machine has four chips: the Poseidon2
 * chip's FRI-layers variant (zkhip_p2chip_air_fri_layers: one path per (query, layer) -- a leaf row hashing the pair, then the compression
 * rows up to the layer's root; leaf rows receive the pairs from the bus, END rows send (layer, root) to the ROOTS table), the fold chip
 * in its wired form (zkhip_fri_layers_chip_air: sends the pairs, and (index, reduced opening) on a query's first row), and two
 * PREPROCESSED tables: QUERIES (index, reduced opening) and ROOTS (layer, root).  The key of that machine (the second generation, removed in round 6 with its entries) therefore held no FRI
 * layer value any more: a verifier needs the layer roots of the inner proof and the reduced openings it computes itself.  Statement: "for
 * the layer commitments and the (index, reduced opening) pairs in the key, every query's chain opens the commitments layer by layer and
 * folds, under the public challenges, to the public final value."  Still outside: the trace / quotient openings, the reduced openings,
 * the transcript. */
size_t zkhip_fri_view_path_words(int layers);
int zkhip_fri_view_shard_paths(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public,
                               const zkhip_params* prm, uint32_t* betas, uint32_t final_value[4], uint32_t* indices, uint32_t* values, uint32_t* siblings,
                               uint32_t* roots, uint32_t* paths);
/* the Fiat-Shamir side of the view: the layer roots (8 words each), the challenges they lead to (4 words each), and the duplex
 * challenger as the commit phase finds it -- transcript[0..8) = the capacity half of its state, transcript[8] = pending inputs (0);
 * transcript[9] = the proof-of-work witness the query phase absorbs behind the final value.
 * With these every challenge is one step of a sponge chain over the roots: state <- (root_l | capacity), permute,
 * beta_l = (state[7], state[6], state[5], state[4]), capacity <- state[8..16) -- what a transcript chip has to prove next
 * (docs/RECURSION_NEXT.md; p3-challenger DuplexChallenger, reference Cargo.lock:3875).  Canonical words; host only. */
int zkhip_fri_view_transcript(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public,
                              const zkhip_params* prm, uint32_t* roots, uint32_t* betas, uint32_t transcript[10]);
/* ... and both in ONE pass over the proof (what zkhip_prove_fri_indices_batch runs per shard proof) */
int zkhip_fri_view_all(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public,
                       const zkhip_params* prm, uint32_t* betas, uint32_t final_value[4], uint32_t* indices, uint32_t* values, uint32_t* siblings,
                       uint32_t* roots, uint32_t* paths, uint32_t transcript[10]);
size_t zkhip_fri_layers_chip_air(int layers, uint32_t* program, size_t cap_words);
size_t zkhip_p2chip_air_fri_layers(int layers, uint32_t* program, size_t cap_words);
/* The same machine with the FRI TRANSCRIPT in-circuit: the Poseidon2 chip's trace starts with transcript rows (zkhip_p2chip_air_fri_transcript,
 * 364 columns) -- a sponge chain over the layer roots from the duplex challenger's capacity (zkhip_fri_view_transcript): row l absorbs
 * root_l (sent to the ROOTS table like a path's end), keeps the capacity of row l - 1 (row 0: public) and sends
 * (l, out[7], out[6], out[5], out[4]) on a bus of its own.  The ROOTS table holds the challenges in its MAIN columns (the prover's),
 * receives each once from its transcript row and hands it to the layer's fold rows (zkhip_fri_transcript_chip_air: the fold chip without
 * public challenges).  Public values: the final value and the capacity.  NEITHER THE KEY NOR THE VERIFIER HOLDS A CHALLENGE -- statement:
 * "for the layer commitments and the (index, reduced opening) pairs in the key, every query's chain opens the commitments and folds to the
 * public final value under the challenges the transcript derives from these commitments, starting from this challenger state."  The
 * prover is still handed the view's challenges and refuses when its chain disagrees.  Still outside: how the challenger state came about
 * (the transcript before the commit phase), the query indices, the trace / quotient openings and the reduced openings.  Ref: p3-challenger
 * DuplexChallenger (reference Cargo.lock:3875) behind sp1.rs:116. */
size_t zkhip_fri_transcript_chip_air(int layers, uint32_t* program, size_t cap_words);
size_t zkhip_p2chip_air_fri_transcript(int layers, uint32_t* program, size_t cap_words);
/* The QUERY PHASE of the transcript in-circuit (zkhip_prove_fri_indices): the sponge chain of the transcript machine goes on as the inner
 * proof's verifier does (p3-fri verifier: observe the final polynomial, check the proof-of-work witness, sample the query indices;
 * reference Cargo.lock:3930, 3875) -- one row absorbs the final value and the witness over the front of the rate, further rows only
 * permute; a fifth chip, SAMPLES, takes the 31 bits of every word these rows hand out (canonical decomposition): the first word's low
 * inner_pow_bits bits must be zero, the low layers + 1 bits of the others are the query indices, which reach the QUERIES table's MAIN
 * column by query number and from there the first fold row of the query.  The key holds (query number, reduced opening) and the layer
 * roots -- no index; the verifier is handed the final value and the challenger's capacity: "every query, AT THE INDEX THE TRANSCRIPT
 * DRAWS FOR IT, opens these commitments and folds to this final value, and the transcript's proof of work holds."  inner_pow_bits = the
 * grinding bits of the INNER proof (zkhip_params.pow_bits of the proof the view was taken from); witness = its proof-of-work witness
 * (zkhip_fri_view_transcript: transcript[9]).  zkhip_fri_indices_program: the two programs that differ from the transcript machine's
 * (which = 0: the Poseidon2 chip with query-phase rows, 1: the SAMPLES chip).  Still outside: the transcript before the commit phase,
 * the trace / quotient openings and the reduced openings. */
size_t zkhip_fri_indices_program(int which, int layers, int inner_pow_bits, uint32_t* program, size_t cap_words);
int zkhip_fri_indices_key(zkhip_ctx* ctx, int layers, size_t n_queries, int inner_pow_bits, const uint32_t* values, const uint32_t* roots,
                          const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri_indices_proof_size(int layers, size_t n_queries, int inner_pow_bits, const zkhip_params* prm);
int zkhip_prove_fri_indices(zkhip_ctx* ctx, const zkhip_machine_key* key, int layers, size_t n_queries, int inner_pow_bits, const uint32_t* betas,
                            const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths,
                            const uint32_t capacity[8], uint32_t witness, const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_fri_indices(const uint8_t* proof, size_t len, int layers, size_t n_queries, int inner_pow_bits, const uint32_t final_value[4],
                             const uint32_t capacity[8], const uint32_t vk[8], const zkhip_params* prm, int* reason);
/* Many shard proofs in one call -- the compress-like step of the path (sp1.rs:116: core -> COMPRESS verifies the shard proofs; prover.rs:90:
 * lift): per job the FRI view of the shard proof (host), the key of its query-phase machine and the machine's proof; jobs are dealt over
 * `devices` (NULL / 0: every visible device) like every batch of this library -- lock-step lanes for the launch-bound sizes
 * (zkhip_set_lockstep), otherwise `in_flight_per_device` contexts per device.  All jobs share (log_n, width, inner).  Out per job: the
 * proof, and what zkhip_verify_fri_indices takes beside it (vk, final value, capacity).  verify != 0: every proof is checked on the host
 * right after it was made (sp1.rs:120).  Returns the status of the lowest failing job (every job still gets its own). */
typedef struct zkhip_fri_job {
    const uint8_t* shard_proof; size_t shard_proof_len;     /* in: a shard proof of this library (fold by 2, blowup 2, constant final value) */
    const uint32_t* public_values; size_t n_public;
    uint8_t* proof; size_t proof_cap;                       /* in: >= zkhip_fri_indices_proof_size(log_n, inner->num_queries, inner->pow_bits, outer) */
    size_t proof_len;                                       /* out */
    uint32_t vk[8], final_value[4], capacity[8];            /* out */
    int status;                                             /* out */
} zkhip_fri_job;
int zkhip_prove_fri_indices_batch(const int* devices, int n_devices, zkhip_fri_job* jobs, int n_jobs, int log_n, uint32_t width,
                                  const zkhip_params* inner, const zkhip_params* outer, int in_flight_per_device, int verify);

/* ---- the FRI check of a FOLD-BY-16 proof in-circuit (the RISC Zero shape, log_fold = 4: zkhip_prove_segment and every prover given that shape): the FOLD16
 * and FINAL chips (fri16_chip.hip), two of the pieces a lift -> join needs (prover.rs:90) beside the width-24 Poseidon2 chip above.  With
 * R = (log_n - log_final) / 4 committed layers a query reads, per layer, a row of 16 adjacent extension entries, folds it four times by 2 with beta, beta^2,
 * beta^4, beta^8, and after R layers compares with the final polynomial (2^log_final coefficients) at its last point.
 * zkhip_fri16_view_shard runs the host verifier on a proof zkhip_verify_shard accepts with log_fold = 4 (versions 3 and 8, either hash width, with or without
 * lookups and code groups) and hands out, in canonical words: betas [R][4], final_poly [2^F][4], per query the index, the reduced opening values [Q][4], the 15
 * other entries of every layer row in proof order siblings [Q][R][15][4], and -- roots / paths may be NULL -- the layer roots [R][8] and per query the layers'
 * authentication paths one after the other (8 (log_n + log_blowup - 4 (l + 1)) words for layer l; zkhip_fri16_view_path_words per query).  It fails like
 * zkhip_verify_shard when the proof is rejected; zkhip_fri_view_shard keeps refusing these proofs.
 * The machine (proof version 11, zkhip_prove_machine_keyed; any outer shape machines take) proves, for the public challenges beta_0 .. beta_{R-1} and the key:
 * "every query listed in QUERIES, taken as entry index & 15 of row index >> 4 of layer 0, folds through rows listed in LAYERS -- each listed row read exactly
 * as often as listed -- at the points its index fixes, to the value at its last point of the polynomial whose coefficients are listed in COEFFS."  Five tables,
 * tallest first (equal heights by table number): 0 FOLD16 (main, one row per (query, layer)), 1 FINAL (Horner, one block of 2^F rows per query; its schedule is
 * preprocessed), and the preprocessed 2 LAYERS (distinct (layer, row) with the 16 entries and the number of readers), 3 QUERIES ((index, reduced opening) with
 * multiplicity), 4 COEFFS.  zkhip_fri16_describe: program (kind 0) or interaction table (kind 1) of the chip at machine position `which` (0..4), its height and
 * widths, and which table it is.  zkhip_fri16_key_host (no GPU) / zkhip_fri16_key: the preprocessed tables of a view and their commitment vk -- what a verifier
 * recomputes from the inner proof.  zkhip_fri16_gen_traces: the two main traces alone on the device (d_fold [2^lr][ld_fold], d_final [2^lr][ld_final], 16-byte
 * aligned, ld a multiple of 4).  zkhip_prove_fri16 is handed the view and refuses, before proving, one whose chains do not end in the final polynomial;
 * zkhip_verify_fri16 is host only.  Shapes: 1 <= R <= 5, 0 <= log_final <= 8, log_final + log_blowup <= 11, 4 R + log_final + log_blowup <= 27, up to 1024
 * queries; anything else is refused with a message.
 * NOT in-circuit in THIS machine: the Merkle paths of the layer rows (its verifier must be handed the LAYERS rows and trust them; the paths machine below,
 * zkhip_prove_fri16_paths, puts a width-24 chip where LAYERS stands and proves them), the transcript (challenges, query indices), the reduced openings; the shard
 * verifier machines do not use these chips. */
size_t zkhip_fri16_view_path_words(int log_n, const zkhip_params* prm);
int zkhip_fri16_view_shard(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public, const zkhip_params* prm,
                           uint32_t* betas, uint32_t* final_poly, uint32_t* indices, uint32_t* values, uint32_t* siblings, uint32_t* roots, uint32_t* paths);
size_t zkhip_fri16_describe(int R, int F, int log_blowup, size_t n_queries, int which, int kind, uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width,
                            uint32_t* pre_width, int* table);
int zkhip_fri16_key_host(int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                         const uint32_t* siblings, const zkhip_params* prm, uint32_t vk[8]);
int zkhip_fri16_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices,
                    const uint32_t* values, const uint32_t* siblings, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]);
int zkhip_fri16_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices,
                           const uint32_t* values, const uint32_t* siblings, uint32_t* d_fold, size_t ld_fold, uint32_t* d_final, size_t ld_final);
size_t zkhip_fri16_proof_size(int R, int F, int log_blowup, size_t n_queries, const zkhip_params* prm);
int zkhip_prove_fri16(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t* final_poly,
                      const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_fri16(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t vk[8], const zkhip_params* prm,
                       int* reason);

/* ---- the same check with the layer rows' MERKLE PATHS in-circuit: the fold-16 PATHS machine.  A layer-paths variant of the width-24 chip, P24L, stands where
 * LAYERS stood and a preprocessed ROOTS table lists the layer commitments, so THE KEY HOLDS THE LAYER ROOTS AND NO LAYER VALUE.  Statement, for the public
 * challenges beta_0 .. beta_{R-1} and the key (QUERIES, COEFFS, ROOTS, FINAL's schedule): "every query listed in QUERIES, taken as entry index & 15 of row
 * index >> 4 of layer 0, opens the layer commitments listed in ROOTS row by row -- each of its R rows is the 64-word leaf at its row index of the width-24
 * Merkle tree whose root ROOTS lists for that layer -- and folds through these rows, at the points its index fixes, to the value at its last point of the
 * polynomial whose coefficients are listed in COEFFS."  Six tables, tallest first (equal heights by table number): 0 FOLD16 and 1 FINAL, 3 QUERIES and 4 COEFFS
 * exactly as above (FOLD16 keeps sending (layer, 16 row + j, entry_j) on its bus); 2 P24L, main only, 552 columns: the width-24 chip's 540 and a tail LN KP M DEP |
 * Z0..Z3 | K0..K3 -- one path per DISTINCT (layer, row), ascending: four sponge rows over the row's 64 words, each receiving four of FOLD16's tuples with
 * multiplicity M = the queries reading the row, then lh_l = log_n + log_blowup - 4 (l + 1) compression rows, the last of which sends (layer, lh_l, digest) to
 * ROOTS in two halves; its height, 2^ceil(lg(Q sum_l (4 + lh_l))), is a function of the shape alone; 5 ROOTS, preprocessed (layer, depth, root[8]), 2^5 rows,
 * with the number of path ends per layer in a main column.  The leaf is EXACTLY four full sponge rows followed by a compression row: a sponge over one 16-word
 * block equals the compression of its halves, so a leaf of floating length would let an inner node pass for a leaf.
 * Inner proofs: fold-16 proofs whose commitments are width-24 trees (hash_width 24: zkhip_prove_segment, versions 3 and 8).  Entries that take a view also take
 * inner_hash_width and refuse anything but 24 with a message (zkhip_prove_fri16 keeps taking width-16-hash proofs).  zkhip_fri16_paths_describe: as
 * zkhip_fri16_describe, six positions.  zkhip_fri16_paths_key_host (no GPU) / zkhip_fri16_paths_key: the key from the shape, the final coefficients, the
 * indices, the reduced openings and the layer roots [R][8] -- no sibling, no layer entry, no challenge.  zkhip_fri16_paths_gen_trace: P24L alone on the device
 * (d_trace [2^log_rows][ld], ld >= 552 and a multiple of 4, 16-byte aligned) from the whole view (paths as zkhip_fri16_view_shard hands them out); ends
 * [n_paths][8] receives where each path ends and *n_paths their number (cap_paths >= Q R always suffices).  zkhip_prove_fri16_paths refuses, before anything is
 * proven and with a message that names query and layer: a path that does not end in its layer's root ("query q layer l does not open"), two queries that
 * disagree about a shared row or its path, a chain that does not end in the final polynomial.  zkhip_verify_fri16_paths is host only: challenges, key, shape.
 * STILL OUTSIDE after this machine: the transcript (challenges, query indices: the indices machine below takes them in), the reduced openings, the trace /
 * quotient openings; the shard verifier machines (shard_verifier.inl) do not use these chips. */
#define ZKHIP_P24CHIP_LAYERS_WIDTH 552
size_t zkhip_fri16_paths_describe(int R, int F, int log_blowup, size_t n_queries, int which, int kind, uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width,
                                  uint32_t* pre_width, int* table);
int zkhip_fri16_paths_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                               const uint32_t* roots, const zkhip_params* prm, uint32_t vk[8]);
int zkhip_fri16_paths_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, const uint32_t* final_poly, const uint32_t* indices,
                          const uint32_t* values, const uint32_t* roots, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]);
int zkhip_fri16_paths_gen_trace(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, const uint32_t* betas, const uint32_t* final_poly,
                                const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const uint32_t* paths, uint32_t* d_trace, size_t ld,
                                uint32_t* ends, size_t cap_paths, size_t* n_paths);
size_t zkhip_fri16_paths_proof_size(int R, int F, int log_blowup, size_t n_queries, const zkhip_params* prm);
int zkhip_prove_fri16_paths(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, const uint32_t* betas,
                            const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const uint32_t* roots,
                            const uint32_t* paths, const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_fri16_paths(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, const uint32_t* betas, const uint32_t vk[8],
                             const zkhip_params* prm, int* reason);

/* ---- the same check with the FIAT-SHAMIR TRANSCRIPT in-circuit from the commit phase on: the fold-16 INDICES machine.  Public values: the 8 capacity words of
 * the duplex challenger as the commit phase finds it.  The key commits the layer roots, the final coefficients and (query number, reduced opening): IT HOLDS NO
 * INDEX AND NO CHALLENGE.  Statement: "a sponge chain starts from this capacity; it absorbs root_0 .. root_{R-1} and draws beta_l after each; it then absorbs the
 * listed final coefficients and a proof-of-work witness; the first word it hands out has its low inner_pow_bits bits zero; the low H = 4 R + F + log_blowup bits of
 * the following words are the indices of queries 0 .. Q - 1; every query, at the index drawn for it, opens the listed layer commitments row by row and folds under
 * the drawn challenges to the value of the listed polynomial at its last point."  The duplex rules (proof_common.h Challenger): pending inputs are zero when the
 * commit phase starts; a root is one full rate block and beta_l = (out[7], out[6], out[5], out[4]); for F >= 1 the 4 2^F coefficient words are 2^(F-1) full blocks
 * and the witness then overwrites rate word 0 only (words 1..7 keep the previous output); for F = 0 one block takes the coefficient in words 0..3 and the witness
 * in word 4; words are handed out from out[7] down, a permutation with no input follows whenever the eight are used up, and the proof-of-work word is always drawn.
 * Eight tables, tallest first (equal heights by table number): 0 FOLD16B = FOLD16 without the constraints that tie BETA to public values and with one receive of
 * (LN, BETA[4]) on every active row; 1 FINAL and 2 P24L as in the paths machine; 3 QUERIES, one row per query number: preprocessed (q, value[4], 1), main the index,
 * received as (q, index) from SAMPLES and handed as (index, value) to the chain's first row; 4 COEFFS with one more send (j, c_j), multiplicity 1, to the transcript
 * table; 5 ROOTS: preprocessed (layer, depth, root[8], 1), main (path ends, beta[4], fold rows of the layer) -- root and beta received from the layer's transcript
 * row, beta sent on to FOLD16B, and fold rows (1 - listed) = 0 so that a padding row (layer number 0, nothing received) sends no challenge; 6 P2T, the width-16 Poseidon2 chip as a transcript-only table: main the 352 permutation columns, preprocessed the chain's schedule
 * (chained, kept rate words [8], root row and its layer, the two coefficient receives and their keys, hands-out flag and the sponge row's number); 7 SAMPLES, the
 * chip of zkhip_prove_fri_indices with H index bits.  Shapes: the paths machine's, and inner_pow_bits <= 30.
 * zkhip_fri16_view_transcript (host only; fails like zkhip_fri16_view_shard): the layer roots [R][8], the challenges [R][4], and transcript[0..8) = the capacity,
 * transcript[8] = pending inputs (0), transcript[9] = the witness.  zkhip_fri16_indices_describe: as zkhip_fri16_paths_describe, eight positions.
 * zkhip_fri16_indices_key_host (no GPU) / _key: the key from the shape, inner_pow_bits, the final coefficients, the reduced openings BY QUERY NUMBER and the layer
 * roots.  zkhip_fri16_indices_gen_traces: the P2T and SAMPLES main traces on the device (dense: [2^lr][352] and [2^lr][288], 16-byte aligned) from the capacity,
 * the roots, the final coefficients and the witness alone; betas [R][4] and indices [Q] receive what the chain draws.  zkhip_fri16_samples_gen_trace: the SAMPLES
 * main trace (2^max(5, ceil lg ceil((1 + Q) / 8)) rows) from given canonical words [ceil((1 + Q) / 8)][8].  zkhip_prove_fri16_indices takes the paths machine's
 * view, the capacity and the witness, and refuses before anything is proven, each with a message: challenges the chain does not draw from these roots and this
 * capacity, a witness that fails the proof of work, indices that are not the drawn ones, everything zkhip_prove_fri16_paths refuses, width-16-hash inner proofs.
 * zkhip_verify_fri16_indices is host only: shape, inner_pow_bits, capacity, key.
 * STILL OUTSIDE after this machine: the reduced openings, the trace / quotient openings, the transcript before the commit phase; the shard verifier machines
 * (shard_verifier.inl) do not use these chips. */
int zkhip_fri16_view_transcript(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public, const zkhip_params* prm,
                                uint32_t* roots, uint32_t* betas, uint32_t transcript[10]);
size_t zkhip_fri16_indices_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, int which, int kind, uint32_t* out, size_t cap_words, int* log_rows,
                                    uint32_t* main_width, uint32_t* pre_width, int* table);
int zkhip_fri16_indices_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, const uint32_t* final_poly, const uint32_t* values,
                                 const uint32_t* roots, const zkhip_params* prm, uint32_t vk[8]);
int zkhip_fri16_indices_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, const uint32_t* final_poly,
                            const uint32_t* values, const uint32_t* roots, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri16_indices_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, const zkhip_params* prm);
int zkhip_fri16_indices_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, const uint32_t capacity[8], const uint32_t* roots,
                                   const uint32_t* final_poly, uint32_t witness, uint32_t* d_p2t, uint32_t* d_samples, uint32_t* betas, uint32_t* indices);
int zkhip_fri16_samples_gen_trace(zkhip_ctx* ctx, int index_bits, size_t n_queries, const uint32_t* words, uint32_t* d_samples);
int zkhip_prove_fri16_indices(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                              const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values, const uint32_t* siblings, const uint32_t* roots,
                              const uint32_t* paths, const uint32_t capacity[8], uint32_t witness, const zkhip_params* prm, uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_fri16_indices(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, const uint32_t capacity[8],
                               const uint32_t vk[8], const zkhip_params* prm, int* reason);

/* ---- the same check with the REDUCED OPENINGS computed in-circuit: the fold-16 OPENINGS machine (ROWSUM16 and QUERY16 chips).  40 public values: the 8 capacity
 * words of the indices machine, then fa, zeta, zeta g_N, YL, YN, YQ, OFFN = fa^W, OFFQ = fa^(2W), four words each (W = the inner proof's trace width; YL / YN / YQ =
 * the fa-weighted sums of the values opened at zeta, at zeta g_N, and of the quotient chunks).  The key commits the layer roots, the final coefficients and, by
 * query number, the opened trace row (W words) and quotient row (8 words): IT HOLDS NO REDUCED OPENING, no index and no challenge.  Statement: everything the
 * indices machine states, and "the value at which query q enters layer 0 is (AT_q - YL) / (x - zeta) + OFFN (AT_q - YN) / (x - zeta g) + OFFQ (AQ_q - YQ) / (x - zeta),
 * AT_q = sum_j fa^j t_{q,j} and AQ_q = sum_j fa^j u_{q,j} over the rows listed for query number q, x = g w_{2^H}^bitrev_H(index_q) at the index DRAWN for q".
 * THE EIGHT CONSTANTS ARE PUBLIC IN THIS STEP (as beta was public in zkhip_prove_fri16 before the transcript came in): nothing in this machine ties them to the
 * inner proof's transcript or opened values; bringing them in over buses is a later step.
 * Ten tables, tallest first (equal heights by table number): 0 FOLD16C = FOLD16B plus the column XQ = X sum_j O_j w_16^bitrev(j, 4) (one constraint on every row; three
 * unused cells keep the width a multiple of four), whose send on a chain's first row is (IDX, XQ, OWN[4]); 1 FINAL, 2 P24L, 4 COEFFS, 5 ROOTS, 6 P2T, 7 SAMPLES: the
 * indices machine's word for word but the public-value count in the header; 3 QUERY16 where QUERIES stood, one row per query number: preprocessed (q, active), main
 * IDX XQ RO AT AQ I1 I2 P1 P2 P2O P3 P3O and the seven constants, each tied to its public value on every row; receives (q, IDX) from SAMPLES, (IDX, XQ, RO) from
 * FOLD16C's first rows, (q, AT) and (q, AQ) from ROWSUM16; 8 ROWSUM16, one row per 8 words of an opened row (per query the trace blocks from the last to the first,
 * then the quotient block): main V[8] ACCIN[4] T[8][4] FA[4], preprocessed (tag = 2 q + tree, active, not-first, last-of-trace, last-of-quotient, q, K0 = 2 block,
 * K1 = K0 + 1); sends (tag, K0, V0..V3) and (tag, K1, V4..V7) to ROWS, (q, T_0) to QUERY16 on a trace's block 0 and on the quotient block; 9 ROWS, preprocessed
 * (tag, K, w0..w3, 1): one row per 4-word group of every opened row, in the tuple form in which P24L's sponge rows receive theirs -- the table the width-24 chip
 * variant P24R on the same bus replaces in the row-paths machine below.  Heights: ROWSUM16 lg(Q (W / 8 + 1)), ROWS lg(Q (W + 8) / 4), QUERY16 lg(Q), at least 2^5.  Shapes: the indices machine's, W a
 * multiple of 8 in 8 .. 1024, inner proofs without lookup pairs and with a quotient row of 8 words.
 * zkhip_fri16_view_openings (host only; fails like zkhip_fri16_view_shard; refuses proofs with lookup pairs; takes version-8 group-order proofs): per query the
 * trace row [Q][W] and the quotient row [Q][8] as the proof holds them, and the 32 constant words.  zkhip_fri16_openings_describe / _key_host (no GPU) / _key /
 * _proof_size: as the _indices_ entries, with the trace width behind inner_pow_bits; the key takes the rows where the indices machine's took the reduced openings.
 * zkhip_fri16_openings_gen_traces: the ROWSUM16 and QUERY16 main traces on the device (dense: [2^lr][48] and [2^lr][72], 16-byte aligned) from raw rows, constants
 * and indices alone, one launch; openings [Q][4] receives the reduced openings (canonical).  zkhip_prove_fri16_openings takes the indices machine's view, the rows
 * and the constants, and refuses before anything is proven, each with a message that names the query: everything zkhip_prove_fri16_indices refuses, a reduced
 * opening computed from the rows (on the device) that differs from the view's `values`, a query point with x = zeta or x = zeta g, and constants that do not
 * match each other (zeta g_N, fa^W, fa^(2W)).  zkhip_verify_fri16_openings is host only: shape, W, inner_pow_bits, the 40 public values, the key.
 * STILL OUTSIDE after this machine: the Merkle paths of the trace and quotient rows, the transcript before the commit phase (so the eight constants), lookups, the
 * AIR identity at zeta; the shard verifier machines (shard_verifier.inl) do not use these chips. */
int zkhip_fri16_view_openings(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public, const zkhip_params* prm,
                              uint32_t* trace_rows, uint32_t* quotient_rows, uint32_t constants[32]);
size_t zkhip_fri16_openings_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, int which, int kind, uint32_t* out,
                                     size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table);
int zkhip_fri16_openings_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, const uint32_t* final_poly,
                                  const uint32_t* trace_rows, const uint32_t* quotient_rows, const uint32_t* roots, const zkhip_params* prm, uint32_t vk[8]);
int zkhip_fri16_openings_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                             const uint32_t* final_poly, const uint32_t* trace_rows, const uint32_t* quotient_rows, const uint32_t* roots, const zkhip_params* prm,
                             zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri16_openings_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, const zkhip_params* prm);
int zkhip_fri16_openings_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, const uint32_t* trace_rows,
                                    const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* indices, uint32_t* d_rowsum, uint32_t* d_query,
                                    uint32_t* openings);
int zkhip_prove_fri16_openings(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                               uint32_t trace_width, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                               const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness,
                               const uint32_t* trace_rows, const uint32_t* quotient_rows, const uint32_t constants[32], const zkhip_params* prm, uint8_t* proof, size_t cap,
                               size_t* len);
int zkhip_verify_fri16_openings(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                                const uint32_t public_values[40], const uint32_t vk[8], const zkhip_params* prm, int* reason);

/* ---- The fold-by-16 ROW-PATHS machine (fri16_chip.hip): the openings machine with the Merkle paths of the opened rows proven.  Everything the openings machine
 * states, and: "the W words from which AT_q is summed are the leaf at the index drawn for query q of the width-24 Merkle tree of depth H = 4 R + F + log_blowup
 * whose root the key lists as the trace root; the 8 words from which AQ_q is summed are the leaf at that index of the tree whose root it lists as the quotient
 * root".  The 40 public values stay (the eight constants remain public in this step).  The key commits the layer roots, the final coefficients, the trace root
 * and the quotient root: NO opened word, no index, no value.  Ten tables, the openings machine's numbering with P24R at 9 (tests/fri16_rowpaths_air.py writes all
 * of it again): 0 FOLD16C, 1 FINAL, 2 P24L, 4 COEFFS, 5 ROOTS, 6 P2T, 7 SAMPLES, 8 ROWSUM16: the openings machine's programs and interaction tables word for word;
 * ROOTS' key table gains the rows (R, H, trace root, not listed) and (R + 1, H, quotient root, not listed): nothing reaches them from the transcript, the existing
 * constraint FOLDROWS (1 - LISTED) = 0 keeps them from handing FOLD16C a challenge, their path-end count is the prover's main column; 3 QUERY16: the program
 * unchanged, preprocessed (q, active, 2 q, 2 q + 1, R, R + 1), two more sends (2 q, R, IDX) and (2 q + 1, R + 1, IDX) on a bus of their own -- which tree a tag
 * belongs to and at which index it is opened; 9 P24R, a second layer-paths-style variant of the width-24 Poseidon2 chip, main only, 552 columns: the chip's 540
 * in place, then TAG LNR KP DEP | IX BL LSP M0 | K0..K3.  One path per (query, tree), 2 Q paths, none shared: ceil(W / 16) sponge rows (the last one partial when
 * W mod 16 = 8; one row of two groups for a quotient row), then H compression rows.  A sponge row receives (TAG, K_i = 4 BL + i, IN[4 i .. 4 i + 4]) with the
 * multiplicities M0 = SS + SPG, G1, G2, G3 on ROWSUM16's bus (an absorbed group is always received, one not absorbed never); the SS row receives (TAG, LNR, IX) from
 * QUERY16; the END row sends (LNR, DEP, digest) in two halves to ROOTS, whose tuple pins the depth to H.  The leaf's LENGTH is pinned by the bus, not by a one-hot
 * as in P24L: ROWSUM16's sends are preprocessed, every group (tag, k) is sent exactly once, and with BL = 0 on SS and BL' = BL + 1 it can be received in block k / 4
 * of a chain that starts at SS only (on the table's first row the chip's FIRST-row constraints CH = 0 and SPG = 0 stand in for the missing predecessor).  Heights: P24R lg(Q (ceil(W / 16) + 1 + 2 H)), at least 2^6 as ROWS had; a keyed machine takes at most 8 tables of one
 * height, and a shape at which nine would meet is refused with a message (none of the shapes the openings machine takes is).
 * zkhip_fri16_view_row_paths (host only; fails like zkhip_fri16_view_shard): per query the trace row's path and the quotient row's path, [Q][H][8] each, as the
 * proof holds them, and the two roots; refuses proofs with lookup pairs, with a preprocessed commitment of their own (the trace leaf is then not the whole row)
 * and with the width-16 hash.  zkhip_fri16_rowpaths_describe / _key_host (no GPU) / _key / _proof_size: as the _openings_ entries; the key takes the final
 * coefficients, the layer roots, the trace root and the quotient root.  zkhip_fri16_rowpaths_gen_trace: P24R's main trace on the device (dense [2^lr][552],
 * 16-byte aligned) from raw rows, indices and siblings alone, one launch (a wave per path); ends [2 Q][8] receives where every path ends, in tag order (query q's
 * trace path, then its quotient path; canonical).  zkhip_prove_fri16_rowpaths takes the openings machine's arguments, the two trees' paths and the two roots, and
 * refuses before anything is proven, each with a message that names query and tree: everything zkhip_prove_fri16_openings refuses, a path that does not end in its
 * root, path words that are not canonical.  zkhip_verify_fri16_rowpaths is host only: shape, W, inner_pow_bits, the 40 public values, the key.
 * STILL OUTSIDE after this machine: the transcript before the commit phase (so the eight constants and where the two roots come from), lookups, the AIR identity
 * at zeta, the wiring into the shard verifier machines (shard_verifier.inl). */
int zkhip_fri16_view_row_paths(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public, const zkhip_params* prm,
                               uint32_t* trace_paths, uint32_t* quotient_paths, uint32_t trace_root[8], uint32_t quotient_root[8]);
size_t zkhip_fri16_rowpaths_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, int which, int kind, uint32_t* out,
                                     size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table);
int zkhip_fri16_rowpaths_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, const uint32_t* final_poly,
                                  const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm, uint32_t vk[8]);
int zkhip_fri16_rowpaths_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                             const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm,
                             zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri16_rowpaths_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, const zkhip_params* prm);
int zkhip_fri16_rowpaths_gen_trace(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, const uint32_t* trace_rows,
                                   const uint32_t* quotient_rows, const uint32_t* indices, const uint32_t* trace_paths, const uint32_t* quotient_paths, uint32_t* d_trace,
                                   uint32_t* ends);
int zkhip_prove_fri16_rowpaths(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                               uint32_t trace_width, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                               const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness,
                               const uint32_t* trace_rows, const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* trace_paths,
                               const uint32_t* quotient_paths, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm, uint8_t* proof,
                               size_t cap, size_t* len);
int zkhip_verify_fri16_rowpaths(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                                const uint32_t public_values[40], const uint32_t vk[8], const zkhip_params* prm, int* reason);

/* ---- the fold-16 HEAD machine: the row-paths machine with the head of the transcript inside ----
 * Statement: everything the row-paths machine states, and: the sponge chain starts from the all-zero state, absorbs the ten header words of a version-3 proof
 * (log_n, W, log_blowup, Q, inner_pow_bits, NP, 0, 4, F, 24), the trace root listed in ROOTS and the NP public values of THIS proof, draws alpha, absorbs the
 * quotient root listed in ROOTS, draws zeta, absorbs the 2 W + 8 opened extension values, draws fa, and the commit phase continues from that very state; the
 * eight constants of the reduced opening are fa, zeta, zeta g_N and the sums and powers of fa over those opened values.  The machine's public values are the
 * inner proof's own public values (n_inner_public of them, 1 .. 30) and nothing else.  alpha is drawn and used by nothing in this step: the AIR identity at zeta
 * is the step that consumes it.  Eleven tables, the row-paths machine's numbering with OPENED16 at 10 (tests/fri16_head_air.py writes all of it again).
 * zkhip_fri16_view_head hands out what the prover needs beside the row-paths view: the opened values [2 W + 8][4] in the order they are observed (values at
 * zeta, at zeta g, quotient values; canonical) and alpha; it fails like zkhip_fri16_view_shard and refuses, each with its message, proofs with lookup pairs, with
 * a program (version 7), with a code group and with the width-16 hash.  zkhip_fri16_head_describe / _key_host (no GPU) / _key / _proof_size: as the _rowpaths_
 * entries with n_inner_public behind trace_width.  zkhip_fri16_head_gen_traces: P2TH, SAMPLES and OPENED16 on the device (dense, [2^lr][352], [2^lr][288],
 * [2^lr][36]) from the inner public values, the two roots, the opened values, the layer roots, the final coefficients and the witness alone; it hands back the
 * eight derived constants [8][4] and the capacity the commit phase finds.  zkhip_prove_fri16_head takes the row-paths prover's arguments, the inner public
 * values and the opened values; constants and capacity are what the view says, compared with what the head derives.  Refused before anything is proven: all
 * zkhip_prove_fri16_rowpaths refuses, a derived constant that is not the view's (named: fa, zeta, zeta g_N, YL, YN, YQ, OFFN, OFFQ), a derived capacity that is
 * not the view's, opened or public values that are not canonical, n_inner_public = 0 or > 30.  zkhip_verify_fri16_head is host only.
 * STILL OUTSIDE: the AIR identity at zeta, lookups, version-7 and version-8 inner proofs, roots leaving the key, the wiring into shard_verifier.inl. */
int zkhip_fri16_view_head(const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public, const zkhip_params* prm,
                          uint32_t* opened, uint32_t alpha[4]);
size_t zkhip_fri16_head_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, int which, int kind,
                                 uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table);
int zkhip_fri16_head_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                              const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm,
                              uint32_t vk[8]);
int zkhip_fri16_head_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                         uint32_t n_inner_public, const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8],
                         const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri16_head_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* prm);
int zkhip_fri16_head_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                const uint32_t* inner_public, const uint32_t trace_root[8], const uint32_t quotient_root[8], const uint32_t* opened, const uint32_t* roots,
                                const uint32_t* final_poly, uint32_t witness, uint32_t* d_p2th, uint32_t* d_samples, uint32_t* d_opened, uint32_t constants[32],
                                uint32_t capacity[8]);
int zkhip_prove_fri16_head(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                           uint32_t trace_width, uint32_t n_inner_public, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                           const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness, const uint32_t* trace_rows,
                           const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* trace_paths, const uint32_t* quotient_paths,
                           const uint32_t trace_root[8], const uint32_t quotient_root[8], const uint32_t* inner_public, const uint32_t* opened, const zkhip_params* prm,
                           uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_fri16_head(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                            uint32_t n_inner_public, const uint32_t* inner_public, const uint32_t vk[8], const zkhip_params* prm, int* reason);

/* ---- the fold-16 IDENTITY machine: the head machine with the AIR identity at zeta inside ----
 * Statement: everything the head machine states, and the synthetic AIR's identity at zeta (verify_shard_impl's step (a) for a version-3 proof without lookup
 * pairs): the constraints of the W / 4 groups of four trace columns, folded with the alpha the transcript chain draws and the selectors zeta - 1 / g_N and
 * (zeta^N - 1) / (zeta - 1), equal the quotient put together from the eight opened quotient values times zeta^N - 1.  Thirteen tables: the head machine's eleven,
 * AIR16 at 11 (one row per group) and SCALARS16 at 12 (one row, repeated); tests/fri16_identity_air.py writes all of it again.  The inner proofs are the head
 * machine's (version 3, no lookup pairs, no program, no code group, width-24 hash, W a multiple of 8, 1 .. 30 public values) and the public values are the
 * inner proof's own.  zkhip_fri16_identity_describe / _key_host (no GPU) / _key / _proof_size: the _head_ entries' arguments.
 * zkhip_fri16_identity_gen_traces: AIR16 and SCALARS16 on the device (dense, [2^lr][56] and [2^7][4 (17 + log_n)]) from the shape, alpha, zeta and the opened
 * values [2 W + 8][4] alone; it hands back (canonical) ACCO of the last group and QUO (zeta^N - 1), which an inner proof that holds makes equal.
 * zkhip_prove_fri16_identity takes the head prover's arguments (zkhip_fri16_view_head hands all of them out).  Refused before anything is proven: all
 * zkhip_prove_fri16_head refuses, zeta = 1, and "the inner proof's AIR identity at zeta does not hold".  zkhip_verify_fri16_identity is host only.
 * STILL OUTSIDE: lookups, version-7 and version-8 inner proofs, roots leaving the key, the wiring into shard_verifier.inl. */
size_t zkhip_fri16_identity_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, int which, int kind,
                                     uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table);
int zkhip_fri16_identity_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                  const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8], const zkhip_params* prm,
                                  uint32_t vk[8]);
int zkhip_fri16_identity_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                             uint32_t n_inner_public, const uint32_t* final_poly, const uint32_t* roots, const uint32_t trace_root[8], const uint32_t quotient_root[8],
                             const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri16_identity_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* prm);
int zkhip_fri16_identity_gen_traces(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                    const uint32_t alpha[4], const uint32_t zeta[4], const uint32_t* opened, uint32_t* d_air, uint32_t* d_scalars, uint32_t accumulators[8]);
int zkhip_prove_fri16_identity(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                               uint32_t trace_width, uint32_t n_inner_public, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                               const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness, const uint32_t* trace_rows,
                               const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* trace_paths, const uint32_t* quotient_paths,
                               const uint32_t trace_root[8], const uint32_t quotient_root[8], const uint32_t* inner_public, const uint32_t* opened, const zkhip_params* prm,
                               uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_fri16_identity(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                                uint32_t n_inner_public, const uint32_t* inner_public, const uint32_t vk[8], const zkhip_params* prm, int* reason);

/* ---- the fold-16 LIFT machine: the identity machine whose key depends on the SHAPE alone ----
 * Statement: "some valid segment proof of this shape with THESE public values exists" -- everything the identity machine states, with the layer roots, the trace
 * root, the quotient root and the final coefficients no longer in the key: they are MAIN columns of ROOTS (8 .. 15) and COEFFS (4 .. 7), pinned by Fiat-Shamir alone
 * (the transcript chain starts from the all-zero state and absorbs every one of them over a bus).  ROOTS' preprocessed column 2 is ACT (1 on rows 0 .. R + 1) and
 * ENDS (1 - ACT) = 0 keeps a padding row from receiving a path end; every other multiplicity that gates a moved word is preprocessed.  The same thirteen tables,
 * heights, inner proofs and public values as the identity machine; tests/fri16_lift_air.py writes the changed parts again.  One key per shape: two segments of one
 * execution share it, and whoever verifies needs no one who saw the inner proof.
 * zkhip_fri16_lift_describe / _proof_size: the _identity_ entries' arguments.  zkhip_fri16_lift_key_host (no GPU) / _key: the _identity_ entries' WITHOUT final_poly,
 * roots, trace_root and quotient_root.  zkhip_fri16_lift_gen_tables: the main columns of ROOTS (dense [2^5][16]; its first eight columns, which the transcript
 * launch makes, come out zero) and COEFFS (dense [max(2^5, 2^F)][8]) on the device from the canonical roots and coefficients -- one launch, Montgomery form made in
 * the kernel, rows past the active ones zero.  zkhip_prove_fri16_lift takes the identity prover's arguments and refuses what it refuses, with the same messages
 * (root or coefficient words >= P among them).  zkhip_verify_fri16_lift is host only.
 * zkhip_prove_fri16_lift_segment: segment proof in, lift proof out -- ONE pass of the host verifier over `proof` (log_n, width, public_values, inner_prm) with every
 * fold-16 view attached, then the lift prover under outer_prm.  It fails with the host verifier's code and message when the inner proof does not verify, and with
 * zkhip_fri16_view_head's message on a form that view does not take.
 * zkhip_prove_fri16_lift_batch: many segment proofs of ONE shape (log_n, width, n_public, inner_prm) lifted in one call -- what stands between the segments and the
 * join.  Per job the views of its segment proof (host, on a small pool ahead of the device work) and the lift prover under the shape's key, which is made once per
 * pooled context and kept with it; jobs are dealt over `devices` (NULL / 0: every visible device) like every batch of this library -- lock-step lanes
 * (zkhip_set_lockstep) when there are at least two jobs per device, otherwise `in_flight_per_device` contexts per device.  Every proof is byte for byte
 * zkhip_prove_fri16_lift_segment's; vk receives the shape's key (zkhip_fri16_lift_key_host's words).  A segment that does not verify fails ITS job with the host
 * verifier's code and message and proof_len 0; the others are proven.  verify != 0: every proof is checked with zkhip_verify_fri16_lift right after it was made.
 * Returns the status of the lowest failing job (every job still gets its own).
 * STILL OUTSIDE: lookups, version-7 and version-8 inner proofs, the wiring into shard_verifier.inl. */
size_t zkhip_fri16_lift_describe(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, int which, int kind,
                                 uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width, int* table);
int zkhip_fri16_lift_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                              const zkhip_params* prm, uint32_t vk[8]);
int zkhip_fri16_lift_key(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                         uint32_t n_inner_public, const zkhip_params* prm, zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri16_lift_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* prm);
int zkhip_fri16_lift_gen_tables(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, const uint32_t* roots, const uint32_t trace_root[8],
                                const uint32_t quotient_root[8], const uint32_t* final_poly, uint32_t* d_roots_main, uint32_t* d_coeffs_main);
int zkhip_prove_fri16_lift(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                           uint32_t trace_width, uint32_t n_inner_public, const uint32_t* betas, const uint32_t* final_poly, const uint32_t* indices, const uint32_t* values,
                           const uint32_t* siblings, const uint32_t* roots, const uint32_t* paths, const uint32_t capacity[8], uint32_t witness, const uint32_t* trace_rows,
                           const uint32_t* quotient_rows, const uint32_t constants[32], const uint32_t* trace_paths, const uint32_t* quotient_paths,
                           const uint32_t trace_root[8], const uint32_t quotient_root[8], const uint32_t* inner_public, const uint32_t* opened, const zkhip_params* prm,
                           uint8_t* proof, size_t cap, size_t* len);
int zkhip_verify_fri16_lift(const uint8_t* proof, size_t len, int R, int F, int log_blowup, size_t n_queries, int inner_pow_bits, uint32_t trace_width,
                            uint32_t n_inner_public, const uint32_t* inner_public, const uint32_t vk[8], const zkhip_params* prm, int* reason);
int zkhip_prove_fri16_lift_segment(zkhip_ctx* ctx, const zkhip_machine_key* key, const uint8_t* proof, size_t len, int log_n, uint32_t width, const uint32_t* public_values,
                                   size_t n_public, const zkhip_params* inner_prm, const zkhip_params* outer_prm, uint8_t* out, size_t cap, size_t* out_len);
typedef struct {
    const uint8_t* segment_proof; size_t segment_proof_len; /* in: a segment proof of this library (fold by 16) */
    const uint32_t* public_values;                          /* in: n_public words */
    uint8_t* proof; size_t proof_cap;                       /* in: >= zkhip_fri16_lift_proof_size */
    size_t proof_len; int status;                           /* out */
} zkhip_fri16_lift_job;
int zkhip_prove_fri16_lift_batch(const int* devices, int n_devices, zkhip_fri16_lift_job* jobs, int n_jobs, int log_n, uint32_t width, size_t n_public,
                                 const zkhip_params* inner_prm, const zkhip_params* outer_prm, int in_flight_per_device, int verify, uint32_t vk[8]);

/* ---- the JOIN of fold-16 lift proofs: N lift proofs of one shape -> ONE proof (RISC Zero: segments -> lift -> join) ----
 * A lift proof is a version-11 proof of the thirteen-table lift machine and the lift key depends on the shape alone, so N lift proofs of one shape are N proofs of ONE
 * keyed machine: machine mode (zkhip.h: zkhip_prove_machine_verifier) verifies them in-circuit.  These entries are a SHAPE CALL over it: each puts the
 * zkhip_machine_desc together -- the lift machine's programs and tables as zkhip_fri16_lift_describe gives them (positions 0 .. 12), zkhip_fri16_lift_key_host's key
 * as key_root, lift_prm's queries and proof-of-work bits, n_inner_public public values -- and calls the function behind the generic entry: the key, the size and the
 * bytes are zkhip_machine_verifier_key_host's, _proof_size's and zkhip_prove_machine_verifier's on that description.  Shape arguments: zkhip_fri16_lift_key's
 * (R, F, log_blowup, n_queries, inner_hash_width, inner_pow_bits, trace_width, n_inner_public); lift_prm: the outer parameters the lift proofs were made under;
 * join_prm: the join's own.  public_values: n_proofs x n_inner_public words in proof order (n_public_total says how many; any other count is refused).
 * zkhip_fri16_join_max_proofs: the most lift proofs of this shape one join takes (machine mode's bounds: 64 proofs, n_proofs x terms <= 2^22, 2^22 Poseidon2 rows);
 * 0 (zkhip_last_error) for a shape the lift refuses.  n_proofs 0 or above it is refused by every entry with a message that names the bound; inner hash width 16
 * with the lift's own message.
 * zkhip_verify_fri16_join is host only and takes (shape, public values, key): no byte of a lift or segment proof.
 * zkhip_prove_fri16_join_segments: segment proofs in, ONE proof out -- the lift proofs are made one after the other on ctx (zkhip_prove_fri16_lift_segment under
 * lift_key), then joined under join_key.  A segment that does not verify fails with the host verifier's code and a message that names the segment.  The faster
 * route to the same bytes: zkhip_prove_fri16_lift_batch (the lifts side by side on the lock-step lanes), then zkhip_prove_fri16_join.
 * More segments than one join takes: the tree below. */
int zkhip_fri16_join_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                              const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm, uint32_t vk[8]);
int zkhip_fri16_join_setup(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                           uint32_t n_inner_public, const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm, zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri16_join_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                   const zkhip_params* lift_prm, size_t n_proofs, const zkhip_params* join_prm);
size_t zkhip_fri16_join_max_proofs(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                   const zkhip_params* lift_prm);
int zkhip_prove_fri16_join(zkhip_ctx* ctx, const zkhip_machine_key* key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                           uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* lift_prm, const uint8_t* const* lift_proofs, const size_t* lens, size_t n_proofs,
                           const uint32_t* public_values, size_t n_public_total, const zkhip_params* join_prm, uint8_t* out, size_t cap, size_t* len);
int zkhip_verify_fri16_join(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                            const zkhip_params* lift_prm, const uint8_t* proof, size_t len, const uint32_t* public_values, size_t n_public_total, size_t n_proofs,
                            const uint32_t vk[8], const zkhip_params* join_prm, int* reason);
int zkhip_prove_fri16_join_segments(zkhip_ctx* ctx, const zkhip_machine_key* lift_key, const zkhip_machine_key* join_key, const uint8_t* const* segment_proofs,
                                    const size_t* lens, size_t n_proofs, int log_n, uint32_t width, const uint32_t* public_values, size_t n_public_total,
                                    const zkhip_params* inner_prm, const zkhip_params* lift_prm, const zkhip_params* join_prm, uint8_t* out, size_t cap, size_t* len);

/* ---- SEVERAL JOINS in one call, and the TREE above the join: more lift proofs than one join takes -> ONE proof (segments -> lift -> joins -> top) ----
 * A join is a machine-mode proof, and machine mode verifies its own proofs: the top is machine mode over the JOIN machine of (shape, join size).  Again shape calls, no
 * second prover and no second verifier.
 * zkhip_prove_fri16_join_batch: n_proofs / proofs_per_join joins of ONE shape.  Join j takes the lift proofs [j J, (j + 1) J) and their public values, goes to
 * devices[j mod n_devices] (NULL, 0: every visible device) and is proven on a pooled context that keeps the join's key, in_flight_per_device at a time on each (0: four);
 * its proof goes to joined + j joined_stride (stride >= zkhip_fri16_join_proof_size), its length to joined_lens[j]; vk: the joins' key.  Every join is the bytes of
 * zkhip_prove_fri16_join on the same inputs.  verify != 0: every join is checked by the host verifier on its worker's thread.  n_proofs that is not a positive multiple
 * of proofs_per_join is refused by message; a failing join fails the call with machine mode's code and a message that names the join.  The joins in flight share the
 * sixteen CPUs a caller may count on, whatever the machine shows.
 * zkhip_fri16_tree_max_join: the largest join size whose join machine a top takes (machine mode's bounds on an INNER machine: chips of at most 2^21 rows, the public
 * values, the terms), 0 (zkhip_last_error) if none.  zkhip_fri16_tree_max_joins: the most joins of that size one top takes.  Both are host only and computed from the
 * machine's shape, never tabulated.
 * zkhip_fri16_tree_key_host / _setup / _proof_size: join_vk is an INPUT -- what zkhip_fri16_join_key_host / _setup return for proofs_per_join -- and becomes key_root of
 * the join machine's description (the ten chips zkhip_machine_verifier_describe gives over the lift machine at n_proofs = proofs_per_join, join_prm's queries and
 * proof-of-work bits, proofs_per_join x n_inner_public public values).  The key, the size and the bytes are zkhip_machine_verifier_key_host's, _proof_size's and
 * zkhip_prove_machine_verifier's on that description at n_proofs = n_joins.
 * zkhip_prove_fri16_tree: the lift proofs -> joins (zkhip_prove_fri16_join_batch's way: dealt over `devices`, several in flight) -> ONE proof over the joins on ctx.  A
 * join's tables for the top are filled on its worker's thread the moment the join exists.  n_proofs must be a positive multiple of proofs_per_join (the caller pads by
 * repeating the last lift proof and its public values); a context whose join key is not join_vk fails the call by message before it proves.  joined / joined_stride
 * (a multiple of 4) / joined_lens: the joins, as above.
 * zkhip_verify_fri16_tree is host only and takes (shape, join size, the joins' key, the number of joins, every segment's public values in order, the top's key): no byte
 * of a segment, lift or join proof.  n_public_total must be n_joins x proofs_per_join x n_inner_public.
 * Every refusal names its entry and the bound it met; shapes the lift refuses keep the lift's message. */
int zkhip_prove_fri16_join_batch(const int* devices, int n_devices, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                                 uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* lift_prm, const uint8_t* const* lift_proofs, const size_t* lens,
                                 size_t n_proofs, size_t proofs_per_join, const uint32_t* public_values, size_t n_public_total, const zkhip_params* join_prm,
                                 int in_flight_per_device, int verify, uint8_t* joined, size_t joined_stride, size_t* joined_lens, uint32_t vk[8]);
size_t zkhip_fri16_tree_max_join(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                 const zkhip_params* lift_prm, const zkhip_params* join_prm);
size_t zkhip_fri16_tree_max_joins(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                  const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm);
int zkhip_fri16_tree_key_host(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                              const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm, const uint32_t join_vk[8], size_t n_joins,
                              const zkhip_params* top_prm, uint32_t vk[8]);
int zkhip_fri16_tree_setup(zkhip_ctx* ctx, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width,
                           uint32_t n_inner_public, const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm, const uint32_t join_vk[8],
                           size_t n_joins, const zkhip_params* top_prm, zkhip_machine_key** key, uint32_t vk[8]);
size_t zkhip_fri16_tree_proof_size(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                                   const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm, const uint32_t join_vk[8], size_t n_joins,
                                   const zkhip_params* top_prm);
int zkhip_prove_fri16_tree(zkhip_ctx* ctx, const zkhip_machine_key* top_key, int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits,
                           uint32_t trace_width, uint32_t n_inner_public, const zkhip_params* lift_prm, const int* devices, int n_devices,
                           const uint8_t* const* lift_proofs, const size_t* lens, size_t n_proofs, size_t proofs_per_join, const uint32_t* public_values,
                           size_t n_public_total, const zkhip_params* join_prm, const uint32_t join_vk[8], const zkhip_params* top_prm, int in_flight_per_device,
                           uint8_t* joined, size_t joined_stride, size_t* joined_lens, uint8_t* out, size_t cap, size_t* len);
int zkhip_verify_fri16_tree(int R, int F, int log_blowup, size_t n_queries, int inner_hash_width, int inner_pow_bits, uint32_t trace_width, uint32_t n_inner_public,
                            const zkhip_params* lift_prm, size_t proofs_per_join, const zkhip_params* join_prm, const uint32_t join_vk[8], size_t n_joins,
                            const uint8_t* proof, size_t len, const uint32_t* public_values, size_t n_public_total, const uint32_t top_vk[8],
                            const zkhip_params* top_prm, int* reason);

/* ---- chip programs, trace generators and machine descriptions whose statement-level entries are in zkhip.h (documented there, beside the prover that
 * uses them: the AIR-as-data section, the SHA-256 chip, the keyed SHA-256 machine, the shard verifier machines) ---- */
int zkhip_air_synthetic(uint32_t width, size_t n_public, uint32_t* out, size_t cap, size_t* words);
void zkhip_sha256_padding_publics(uint64_t message_len, uint64_t first_block, uint64_t n_active, uint32_t out[75]);
size_t zkhip_sha256_air(uint32_t* program, size_t cap_words);
size_t zkhip_sha256_pad(const uint8_t* message, size_t len, uint8_t* blocks, size_t cap);
int zkhip_sha256_gen_trace(zkhip_ctx* ctx, const uint8_t* blocks, size_t n_active, size_t n_blocks, uint64_t message_len, uint32_t* d_trace, size_t ld,
                           uint32_t publics[91]);
int zkhip_range_table(zkhip_ctx* ctx, const uint32_t* d_trace, size_t ld, size_t rows, const uint32_t* columns, int n_columns, int log_table,
                      uint32_t* d_table, size_t table_ld, uint32_t value_col, uint32_t mult_col);
size_t zkhip_sha256_air_chained(uint32_t* program, size_t cap_words);
int zkhip_sha256_gen_trace_chained(zkhip_ctx* ctx, const uint32_t chain_in[8], const uint8_t* blocks, size_t n_active, size_t n_blocks, uint64_t message_len,
                                   uint64_t first_block, uint32_t* d_trace, size_t ld, uint32_t publics[91]);
size_t zkhip_sha256_machine_describe(size_t message_len, int which, int kind, uint32_t* out, size_t cap, int* log_n, uint32_t* width, uint32_t* pre_width);
size_t zkhip_shard_verifier_describe(int log_n, uint32_t width, size_t n_queries, int inner_pow_bits, size_t n_public, size_t n_proofs, int which, int kind, uint32_t* out,
                                     size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width);
size_t zkhip_shard_verifier_describe_air(const uint32_t* program, size_t program_words, int log_n, uint32_t width, size_t n_queries, int inner_pow_bits, size_t n_public,
                                         size_t n_proofs, int which, int kind, uint32_t* out, size_t cap_words, int* log_rows, uint32_t* main_width, uint32_t* pre_width);
size_t zkhip_machine_verifier_describe(const zkhip_machine_desc* inner, size_t n_proofs, int which, int kind, uint32_t* out, size_t cap, int* log_rows, uint32_t* main_width,
                                       uint32_t* pre_width);
size_t zkhip_machine_verifier_host_tables(const zkhip_machine_desc* inner, const uint8_t* const* proofs, const size_t* proof_lens, size_t n_proofs, const uint32_t* public_values,
                                          size_t n_public, int which, uint32_t* out, size_t cap);
/* machine mode's EVAL rows on the device (mrec_eval_rows_kernel) alone, one launch, for the row tests: n_terms raw terms chip by chip (chips[i] < n_chips
 * non-decreasing, canonical coeffs[i], keys[3 i .. 3 i + 2] < kspan, firsts[i] 0 / 1), per proof a value table values[p][kspan][4] and alpha alphas[p][4]
 * (canonical).  Key 0 is the extension one (the table's entry 0 is not read); keys 1 .. n_stream are read the way a proof's opened-value stream is (canonical words,
 * Montgomery form made in the kernel), the keys behind them the way the public values and selectors are (the call's small block).  Out, canonical: rows
 * [n_proofs n_terms][32] = F0 F1 F2 | M | TV | ACCIN | ACCO | ALPHA per term, accs [n_proofs n_chips][4] = ACCO of every (proof, chip)'s last term (zero: none).
 * A device word of P or more is ZKHIP_ERR_INTERNAL. */
int zkhip_machine_verifier_gen_eval_rows(zkhip_ctx* ctx, size_t n_terms, const uint32_t* chips, const uint32_t* coeffs, const uint32_t* keys, const uint32_t* firsts,
                                         size_t n_chips, size_t n_proofs, size_t kspan, size_t n_stream, const uint32_t* values, const uint32_t* alphas, uint32_t* rows,
                                         uint32_t* accs);
int zkhip_ntt_pass(zkhip_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, size_t ld, int log_n,
                   uint32_t width, int which);
int zkhip_last_prove_debug(zkhip_ctx* ctx, zkhip_prove_debug* out);
int zkhip_selftest_lockstep(int members, int rounds);
int zkhip_selftest_host_simd(double* ns_x16, double* ns_scalar);
double zkhip_host_permutation_ns(int form);
void zkhip_lockstep_stats(uint64_t out[6]);
uint64_t zkhip_lockstep_stack_high_water(void);
/* Where the recursion machines (zkhip_prove_shard_verifier[_air], zkhip_prove_machine_verifier, zkhip_prove_shard_tree) make their per-query witness tables -- ROWSUM,
 * QUERY, the fold rows, the queries' Poseidon2 rows -- and machine mode its EVAL rows where that table has 2^15 rows or more (below, the host fills them under either
 * setting: the kernel's fixed cost is then more than the upload it saves): 0 (default) = device kernels over the inner proofs' words (round 6), 1 = the host's walk of rounds 4 - 5 (the same tables
 * word for word: the fallback, and what tests/test_gpu_recursion_machine.py compares the kernels with).  Process-wide; returns the previous setting. */
int zkhip_recursion_witnesses_on_host(int enable);

#ifdef __cplusplus
}
#endif
#endif /* ZKHIP_CHIPS_H */
