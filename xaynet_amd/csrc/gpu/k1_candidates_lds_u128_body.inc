// Body of k1_candidates_lds_u128 and k1_candidates_lds_u128_batch
// (kernels.hip), which include this text between their braces. In scope:
// key8, start_word, first_attempt, n_attempts, words_per_draw, nbytes,
// order_lo, order_hi, cand_lo, cand_hi, wg_counts and attempts_per_thread, as
// k1_candidates_lds_u128 declares them. Shared as text so that the
// single-seed kernel keeps its code (see k1_candidates_lds_body.inc).
    __shared__ uint32_t lds_words[K1_LDS_THREADS * 16 + 16];

    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = key8[i];

    const int apt = attempts_per_thread;  // 5 (wpd=3) or 4 (wpd=4)
    // words covered by this workgroup's attempts
    uint64_t A0 = first_attempt + uint64_t(blockIdx.x) * K1_LDS_THREADS * apt;
    uint64_t W0 = start_word + A0 * uint64_t(words_per_draw);
    uint64_t first_blk = W0 >> 4;
    int off0 = int(W0 & 15);
    // blocks needed: ceil((off0 + 256*apt*wpd) / 16), <= 257
    int need_blocks = (off0 + K1_LDS_THREADS * apt * words_per_draw + 15) >> 4;

    uint32_t tmp[16];
    if (int(threadIdx.x) < need_blocks) {
        chacha20_block_dev(key, first_blk + threadIdx.x, tmp);
#pragma unroll
        for (int i = 0; i < 16; ++i) lds_words[(threadIdx.x << 4) + i] = tmp[i];
    }
    if (need_blocks > K1_LDS_THREADS && threadIdx.x == 0) {
        chacha20_block_dev(key, first_blk + K1_LDS_THREADS, tmp);
#pragma unroll
        for (int i = 0; i < 16; ++i) lds_words[(K1_LDS_THREADS << 4) + i] = tmp[i];
    }
    __syncthreads();

    __shared__ uint32_t wave_tot[4];
    uint64_t a_rel0 = (uint64_t(blockIdx.x) * K1_LDS_THREADS + threadIdx.x) * apt;
    // bitmask + re-extract (see k1_candidates_lds): avoids dynamic-indexed
    // register value arrays
    int widx = off0 + int(uint64_t(threadIdx.x) * apt) * words_per_draw;
    auto extract = [&](int d, uint64_t& lo, uint64_t& hi) {
        const uint32_t* w = &lds_words[widx + d * words_per_draw];
        lo = uint64_t(w[0]) | (uint64_t(w[1]) << 32);
        if (nbytes >= 13) {
            hi = uint64_t(w[2]) | (uint64_t(w[3]) << 32);
            if (nbytes < 16) hi &= (1ULL << (8 * (nbytes - 8))) - 1;
        } else {
            hi = uint64_t(w[2]);
            if (nbytes < 12) hi &= (1ULL << (8 * (nbytes - 8))) - 1;
        }
    };
    uint32_t accept_bits = 0;
    uint32_t mine = 0;
    if (a_rel0 < n_attempts) {
        for (int d = 0; d < apt; ++d) {
            if (a_rel0 + d >= n_attempts) break;
            uint64_t lo, hi;
            extract(d, lo, hi);
            if ((hi < order_hi) || (hi == order_hi && lo < order_lo)) {
                accept_bits |= 1u << d;
                ++mine;
            }
        }
    }
    uint64_t k =
        uint64_t(blockIdx.x) * K1_LDS_THREADS * apt + block_excl_scan<4>(mine, wave_tot);
    while (accept_bits) {
        int d = __builtin_ctz(accept_bits);
        accept_bits &= accept_bits - 1;
        uint64_t lo, hi;
        extract(d, lo, hi);
        cand_lo[k] = lo;
        cand_hi[k] = hi;
        ++k;
    }
    if (threadIdx.x == K1_LDS_THREADS - 1)
        wg_counts[blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
