// C ABI of the kernel launchers: defined in kernels.hip, consumed by
// hip_bindings.cpp. Both include this header, so a signature mismatch is a
// compile error. All launches go to the null stream.
//
// One launcher per operation, for u64 and wide (u128) orders alike. An order
// travels as (order_lo, order_hi) and is wide iff order_hi != 0 (order >=
// 2^64); canonical values travel as (lo, hi) pointers to split u64 planes, hi
// null for u64 orders. A launcher given the order picks its kernel by
// order_hi, one without (pack, unpack, add_to_planes, K1 scatter) by the hi
// pointer; the bindings reject calls in which the two disagree. A third width
// class, multi-limb orders in [2^128, 2^320), enters through the *_limbs
// launchers at the end, which the bindings call for every width. This is the
// only layer that chooses between the u64, the u128 and the multi-limb
// kernels.
//
// dtype arguments follow mask::DataType: 0=f32 1=f64 2=i32 3=i64 (integer
// outputs truncate toward zero); anything else is hipErrorInvalidValue.
// Digit planes are [n_planes][len]; u64 orders take 32-bit digits only, wide
// orders digit_bits in 1..63.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "limbs.h"

extern "C" {

// ---- K1: ChaCha20 mask expansion (candidates -> scan -> scatter) ----
// each thread owns attempts_per_thread = 16/words_per_draw attempts
hipError_t xhip_k1_candidates(const uint32_t* key8_dev, uint64_t start_word,
                              uint64_t first_attempt, uint64_t n_attempts, int words_per_draw,
                              int nbytes, uint64_t order_lo, uint64_t order_hi,
                              uint64_t* cand_lo, uint64_t* cand_hi, uint32_t* wg_counts,
                              int attempts_per_thread, uint32_t* n_wgs_out);
// Up to this many counts xhip_k1_scan_hier runs one workgroup. It is also the
// batch rule: seeds are expanded together (xhip_k1_expand_batch, one scan
// workgroup per seed) only while one seed's launch has at most this many
// candidate workgroups.
#define XHIP_K1_SCAN_ONE_WG 2048
// seeds per batched launch (the grid's second dimension), rows per row sum
#define XHIP_K1_MAX_BATCH 65535
// blk_tmp must hold ceil(n/1024) u32
hipError_t xhip_k1_scan_hier(uint32_t* wg_counts, uint32_t n, uint32_t* blk_tmp,
                             uint64_t* total_dev);
hipError_t xhip_k1_scatter_compact(const uint64_t* cand_lo, const uint64_t* cand_hi,
                                   const uint32_t* wg_offsets, const uint64_t* total_dev,
                                   uint32_t n_wgs, int apt, uint64_t out_base, uint64_t* out_lo,
                                   uint64_t* out_hi, uint64_t out_len);
// Batched expansion for u64 and u128 orders: seed s (key keys_dev + 8*s, unit
// draw of start_words_dev[s] keystream words) gets n_attempts attempts from
// attempt 0, candidate segments at cand + s*cand_stride (>= wgs*256*apt), row
// s of wg_counts (counts_stride >= wgs), its accepted count in totals_dev[s]
// and its values in out_lo/out_hi + s*out_stride, cut at out_len.
// wgs = ceil(n_attempts / (256*apt)) must not exceed XHIP_K1_SCAN_ONE_WG.
hipError_t xhip_k1_expand_batch(const uint32_t* keys_dev, const uint64_t* start_words_dev,
                                uint32_t n_seeds, uint64_t n_attempts, int words_per_draw,
                                int nbytes, uint64_t order_lo, uint64_t order_hi,
                                uint64_t* cand_lo, uint64_t* cand_hi, uint64_t cand_stride,
                                uint32_t* wg_counts, uint32_t counts_stride,
                                uint64_t* totals_dev, int apt, uint64_t* out_lo,
                                uint64_t* out_hi, uint64_t out_stride, uint64_t out_len);

// ---- K3: batched aggregation (ept <= 0 picks the per-bpn default) ----
hipError_t xhip_k3_aggregate(uint64_t* acc, const uint8_t* updates, uint64_t stride,
                             uint32_t n_updates, uint64_t len, int bpn, int ept);

// How the tile-streaming K3 kernel (ept 401 / 402) splits a row of `len`
// elements: n_tiles full tiles of tile_elems elements through a ring of
// `depth` LDS slots per wave (`waves` per workgroup), and the remainder
// [rem_start, len), less than one tile, through plain loads in one more block
// of the same launch. max_byte is the highest row byte offset the tile blocks
// read, -1 if there is no tile. With n_tiles == 0 the generic kernel runs
// alone. All zero (and -1) when bpn has no tile kernel, the stride is not a
// multiple of 16 bytes, or the row has less than 16 bytes past its last
// element (row_stride() pads 16 elements).
struct XhipK3TilePlan {
    uint32_t tile_elems, depth, waves;
    uint64_t n_tiles, rem_start;
    int64_t max_byte;
};
void xhip_k3_tile_plan(uint64_t len, int bpn, uint64_t stride, XhipK3TilePlan* plan);

// What the loader-wave K3 kernel (ept 411 / 412) launches for the same row:
// it takes n_tiles, rem_start and max_byte from the tile plan above and runs
// tile_blocks workgroups of one loader wave and `consumers` consumer waves
// over `consumers` adjacent tiles each, through a ring of `depth` LDS slots,
// plus one remainder block if has_remainder; n_tiles, rem_start and max_byte
// repeat the tile plan's. All zero (and -1) when the tile plan has no tile or
// bpn has no loader kernel: the generic kernel runs then.
struct XhipK3LoaderPlan {
    uint32_t consumers, depth, tile_blocks, has_remainder;
    uint64_t n_tiles, rem_start;
    int64_t max_byte;
};
void xhip_k3_loader_plan(uint64_t len, int bpn, uint64_t stride, XhipK3LoaderPlan* plan);

// Read-only bandwidth probe (scripts/k3_sweep.py --ceiling): reads `bytes`
// (a multiple of 16, 16B-aligned) with coalesced 16-byte loads, default or
// nontemporal; sink is one device word that is practically never written.
hipError_t xhip_read_ceiling(const uint8_t* src, uint64_t bytes, bool nontemporal,
                             uint32_t* sink);

// ---- K2/K4: digit planes <-> canonical values, unmask ----
hipError_t xhip_k4_unmask(const uint64_t* planes, const uint64_t* mask_lo,
                          const uint64_t* mask_hi, int dtype, void* out, uint64_t len,
                          int n_planes, int digit_bits, uint64_t order_lo, uint64_t order_hi,
                          uint64_t exp_lo, uint64_t exp_hi, double n_add_shift,
                          double scalar_sum);
// u64 orders only: unmask (cross-rank sums of) canonical values. offset == 0:
// the shift-in-doubles kernel. offset = nb * add_shift * exp_shift (integer
// dtypes only): the exact-offset kernel of xhip_k4_unmask_limbs on one plane
// of whole-word values, `divisor` as there. Float dtypes with an offset and a
// divisor: the exact kernel (k4_unmask_exact), as there.
hipError_t xhip_k4_unmask_values(const uint64_t* vals, const uint64_t* mask, int dtype,
                                 void* out, uint64_t len, uint64_t order, uint64_t exp_shift,
                                 double n_add_shift, double scalar_sum, uint64_t offset,
                                 uint64_t divisor);
hipError_t xhip_k2_canonicalize(const uint64_t* planes, uint64_t* out_lo, uint64_t* out_hi,
                                uint64_t len, int n_planes, int digit_bits, uint64_t order_lo,
                                uint64_t order_hi);
hipError_t xhip_add_to_planes(uint64_t* planes, const uint64_t* lo, const uint64_t* hi,
                              uint64_t len, int n_planes, int digit_bits);
// wide orders only: 32-bit accumulator planes -> k compact planes
hipError_t xhip_k2_recode_planes(const uint64_t* acc, uint64_t* out, uint64_t len, int n_digits,
                                 uint64_t order_lo, uint64_t order_hi, int k, int digit_bits);
hipError_t xhip_k2_mod_add(uint64_t* a_lo, uint64_t* a_hi, const uint64_t* b_lo,
                           const uint64_t* b_hi, uint64_t len, uint64_t order_lo,
                           uint64_t order_hi);

// ---- K5: synthetic update rows, and masking of real weights ----
hipError_t xhip_k5_mask_pack(const uint64_t* mask_lo, const uint64_t* mask_hi, uint8_t* out,
                             uint64_t len, int bpn, uint64_t order_lo, uint64_t order_hi,
                             uint64_t participant, double scalar, double add_shift,
                             uint64_t exp_lo, uint64_t exp_hi);
hipError_t xhip_k5_mask_weights(const void* w, int dtype, const uint64_t* mask_lo,
                                const uint64_t* mask_hi, uint8_t* out, uint64_t len, int bpn,
                                uint64_t order_lo, uint64_t order_hi, double scalar,
                                double add_shift, uint64_t exp_lo, uint64_t exp_hi);

// ---- K6: wire limbs <-> canonical values ----
hipError_t xhip_k6_unpack(const uint8_t* in, uint64_t* out_lo, uint64_t* out_hi, uint64_t len,
                          int bpn);
hipError_t xhip_k6_pack(const uint64_t* in_lo, const uint64_t* in_hi, uint8_t* out, uint64_t len,
                        int bpn);

// ---- K7: model weights -> Option<Model> bincode body ----
//
// How the encoder splits `len` weights: blocks of block_elems elements, whose
// word totals are scanned to 64-bit bases in scan_levels levels. Up to
// XHIP_K7_SCAN_ONE_WG blocks one workgroup scans the block totals themselves
// (1 level, tiles == 0); more are scanned inside `tiles` tiles of tile_blocks
// blocks first, and that workgroup scans the tile totals (2 levels).
// work_bytes is the workspace both launchers take; all zero for len == 0 or
// len > 2^32 (the model decoder's own limit).
#define XHIP_K7_SCAN_ONE_WG 4096
struct XhipK7Plan {
    uint32_t block_elems, scan_levels, tile_blocks;
    uint64_t blocks, tiles, work_bytes;
};
void xhip_k7_plan(uint64_t len, XhipK7Plan* plan);
// Counts and scans: afterwards the first u64 of `work` (16-byte aligned,
// work_bytes long) is the number of u32 words of all elements, and the body
// is 9 + 4 * that many bytes. len in 1..2^32.
hipError_t xhip_k7_model_count(const void* w, int dtype, uint64_t len, void* work);
// Writes the body at out + 3 (so that its words are aligned dwords; out
// 4-byte aligned) from the workspace xhip_k7_model_count left for the same
// w, dtype and len. Nothing is stored at or past out + out_bytes.
hipError_t xhip_k7_model_emit(const void* w, int dtype, uint64_t len, const void* work,
                              uint8_t* out, uint64_t out_bytes);

// ---- K7d: Option<Model> bincode body -> model weights ----
//
// How the decoder splits a body of `words` element words (the body's bytes
// minus its 9-byte head, over 4): blocks of block_words words, whose 42-entry
// boundary maps are composed inside `tiles` tiles of tile_blocks blocks and
// then across the tiles (levels 2), or in the one tile alone (levels 1).
// tile_blocks 0 asks for the default, XHIP_K7D_TILE_BLOCKS, which is also the
// most a tile takes; a smaller one makes small bodies run both levels. All
// zero for a tile_blocks above that or more words than 2^32 elements have.
#define XHIP_K7D_TILE_BLOCKS 256
struct XhipK7dPlan {
    uint32_t block_words, tile_blocks, levels;
    uint64_t blocks, tiles, work_bytes;
};
void xhip_k7d_plan(uint64_t words, uint32_t tile_blocks, XhipK7dPlan* plan);
// Decodes the nbytes-long body at `body` (device memory, 3 bytes past a
// 4-byte boundary inside its buffer, as K7 places it) into n weights of
// `dtype` at `out`. `work` is 16-byte aligned and work_bytes long. *rejected
// is 0 exactly when the body is head 01, u64 n, n canonical elements of the
// dtype and nothing after; otherwise non-zero, and `out` is unspecified.
// A length that is not 9 + 4 * words with 7n <= words <= 42n is refused before
// any launch; the rest, the head included, is one status word read back after
// the last kernel (the caller with the bytes on the host checks the head
// there too). No word at or
// past body + nbytes is read.
hipError_t xhip_k7d_decode(const void* body, uint64_t nbytes, int dtype, uint64_t n, void* work,
                           void* out, uint32_t tile_blocks, uint32_t* rejected);

// ---- every width: u64, u128 and multi-limb orders below 2^320 ----
//
// The launchers the bindings call. The order travels by value as five u64
// limbs (xhip_limbs, limbs.h) and its limb count L = ceil(bits/64) is the
// width: L <= 2 forwards to the launcher above, L = 3..5 runs the multi-limb
// kernels. Canonical values stay a (lo, hi) pointer pair: for L >= 2 lo is
// limb row 0, hi row 1, and row j lives at lo + j*(hi - lo), so a column
// slice of an [L, n] tensor works as it does for [2, n].
hipError_t xhip_k1_candidates_limbs(const uint32_t* key8_dev, uint64_t start_word,
                                    uint64_t first_attempt, uint64_t n_attempts,
                                    int words_per_draw, int nbytes, xhip_limbs order,
                                    uint64_t* cand_lo, uint64_t* cand_hi, uint32_t* wg_counts,
                                    int attempts_per_thread, uint32_t* n_wgs_out);
hipError_t xhip_k1_scatter_compact_limbs(const uint64_t* cand_lo, const uint64_t* cand_hi,
                                         const uint32_t* wg_offsets, const uint64_t* total_dev,
                                         uint32_t n_wgs, int apt, uint64_t out_base,
                                         uint64_t* out_lo, uint64_t* out_hi, uint64_t out_len,
                                         xhip_limbs order);
// offset == 0: the shift-in-doubles unmask of the B0..B6 bounds (L <= 2,
// exp_shift below 2^128): float outputs, and integer outputs without an exact
// divisor, which are then within 1 of the exact truncated quotient. offset =
// nb * add_shift * exp_shift != 0 (every Bmax config, L = 2..5; B0..B6
// integer outputs that have a divisor, L = 1..2): the exact-offset unmask,
// weight = (t - offset) / (exp_shift * scalar_sum); n_add_shift is unused,
// `divisor` is exp_shift * scalar_sum where that is an exact integer below
// 2^64 (else 0) - integer outputs are then exact - and `scale` the double
// nearest 1/(exp_shift * scalar_sum). Integer dtypes need a one-word
// exp_shift; u64 orders (L = 1) 32-bit digits.
// Float dtypes with an offset AND a `divisor` (below 2^(64L), any limb count):
// exact mode, L = 1..5 - the weight is the rational (t - offset) / divisor
// rounded once to the output type in integers (unmask_round.h); exp_shift,
// scalar_sum and scale are unused. Float outputs without a divisor keep the
// kernels above.
hipError_t xhip_k4_unmask_limbs(const uint64_t* planes, const uint64_t* mask_lo,
                                const uint64_t* mask_hi, int dtype, void* out, uint64_t len,
                                int n_planes, int digit_bits, xhip_limbs order,
                                xhip_limbs exp_shift, double n_add_shift, double scalar_sum,
                                xhip_limbs offset, xhip_limbs divisor, double scale);
hipError_t xhip_k2_canonicalize_limbs(const uint64_t* planes, uint64_t* out_lo,
                                      uint64_t* out_hi, uint64_t len, int n_planes,
                                      int digit_bits, xhip_limbs order);
hipError_t xhip_add_to_planes_limbs(uint64_t* planes, const uint64_t* lo, const uint64_t* hi,
                                    uint64_t len, int n_planes, int digit_bits,
                                    xhip_limbs order);
hipError_t xhip_add_rows_to_planes_limbs(uint64_t* planes, const uint64_t* lo,
                                         const uint64_t* hi, uint64_t len, int n_planes,
                                         int digit_bits, xhip_limbs order, uint32_t rows,
                                         uint64_t row_stride);
hipError_t xhip_k2_recode_planes_limbs(const uint64_t* acc, uint64_t* out, uint64_t len,
                                       int n_digits, xhip_limbs order, int k, int digit_bits);
hipError_t xhip_k2_mod_add_limbs(uint64_t* a_lo, uint64_t* a_hi, const uint64_t* b_lo,
                                 const uint64_t* b_hi, uint64_t len, xhip_limbs order);
// offset == 0: the B0..B6 kernel (L <= 2). offset = add_shift * exp_shift
// (Bmax, L = 2..5): quantise and add the shift in integers.
hipError_t xhip_k5_mask_weights_limbs(const void* w, int dtype, const uint64_t* mask_lo,
                                      const uint64_t* mask_hi, uint8_t* out, uint64_t len,
                                      int bpn, xhip_limbs order, double scalar, double add_shift,
                                      xhip_limbs exp_shift, xhip_limbs offset);
// Exact mode, L = 1..5: the scalar is the fraction p/q (both below 2^63,
// already clamped to the unit config's bound), add_shift an integer, and
// every element is quantised in integers (mask_quant.h): the output is the
// rational masker's, byte for byte. Needs 2 * add_shift * exp_shift < order.
hipError_t xhip_k5_mask_weights_exact_limbs(const void* w, int dtype, const uint64_t* mask_lo,
                                            const uint64_t* mask_hi, uint8_t* out, uint64_t len,
                                            int bpn, xhip_limbs order, xhip_limbs add_shift,
                                            xhip_limbs exp_shift, uint64_t p, uint64_t q);
hipError_t xhip_k6_unpack_limbs(const uint8_t* in, uint64_t* out_lo, uint64_t* out_hi,
                                uint64_t len, int bpn, xhip_limbs order);
hipError_t xhip_k6_pack_limbs(const uint64_t* in_lo, const uint64_t* in_hi, uint8_t* out,
                              uint64_t len, int bpn, xhip_limbs order);

}  // extern "C"
