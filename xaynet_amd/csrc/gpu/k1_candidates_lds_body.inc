// Body of k1_candidates_lds and k1_candidates_lds_batch (kernels.hip), which
// include this text between their braces. In scope: key8, start_word,
// first_attempt, n_attempts, words_per_draw, nbytes, order, cand, wg_counts
// and draws_per_thread, as k1_candidates_lds declares them.
//
// Shared as text and not as a __device__ function: inlined through a call the
// single-seed kernel comes out with another schedule (4 bytes longer, the
// tail of the scan reordered), and K1's hottest kernel keeps its measured
// code (see the note at the scan below).
    __shared__ uint32_t lds_words[16 * 257];
    __shared__ uint32_t wave_tot[4];

    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = key8[i];

    // keystream words covered by this workgroup: [W0, W0 + 256*16)
    // (each thread's draws_per_thread * words_per_draw == 16 words)
    uint64_t W0 = start_word + first_attempt * uint64_t(words_per_draw) +
                  uint64_t(blockIdx.x) * K1_LDS_THREADS * 16;
    uint64_t first_blk = W0 >> 4;
    int off0 = int(W0 & 15);

    uint32_t tmp[16];
    chacha20_block_dev(key, first_blk + threadIdx.x, tmp);
#pragma unroll
    for (int i = 0; i < 16; ++i) lds_words[i * 257 + threadIdx.x] = tmp[i];
    if (off0 && threadIdx.x == 0) {  // boundary straddle block
        chacha20_block_dev(key, first_blk + K1_LDS_THREADS, tmp);
#pragma unroll
        for (int i = 0; i < 16; ++i) lds_words[i * 257 + K1_LDS_THREADS] = tmp[i];
    }
    __syncthreads();

    // Accepted draws are compacted IN ORDER into this workgroup's segment of
    // `cand` (base = wg * 256 * dpt, its worst-case capacity), so the
    // scatter pass is a coalesced segment copy.
    uint64_t t = uint64_t(blockIdx.x) * K1_LDS_THREADS + threadIdx.x;
    uint64_t a0 = t * draws_per_thread;
    // Accepted draws are recorded as a BITMASK and re-extracted from LDS in
    // a second pass after the scan: value arrays indexed by a dynamic
    // count (`vals[mine++]`) compile to per-element select chains, which
    // cost more than re-reading the LDS window.
    int wbase = off0 + (int(threadIdx.x) << 4);  // this thread's first word
    auto ldw = [&](int w) { return lds_words[(w & 15) * 257 + (w >> 4)]; };
    auto extract = [&](int d) {
        int w = wbase + d * words_per_draw;
        uint64_t v = uint64_t(ldw(w));
        if (nbytes > 4) {
            uint64_t hi = uint64_t(ldw(w + 1));
            int hb = nbytes - 4;
            hi &= (hb >= 4) ? 0xffffffffULL : ((1ULL << (8 * hb)) - 1);
            v |= hi << 32;
        } else if (nbytes < 4) {
            v &= (1ULL << (8 * nbytes)) - 1;
        }
        return v;
    };
    uint32_t accept_bits = 0;
    uint32_t mine = 0;
    if (a0 < n_attempts) {
#pragma unroll 4
        for (int d = 0; d < draws_per_thread; ++d) {
            if (a0 + d >= n_attempts) break;
            if (extract(d) < order) {
                accept_bits |= 1u << d;
                ++mine;
            }
        }
    }
    // block_excl_scan<4>, written out: calling the helper here changes this
    // kernel's register allocation (41 -> 40 SGPRs, acceptance loop
    // rescheduled), and K1's hottest kernel keeps its measured code
    uint32_t lane = threadIdx.x & 63;
    uint32_t wave = threadIdx.x >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t v = __shfl_up(incl, off, 64);
        if (int(lane) >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        if (w < wave) wave_base += wave_tot[w];
    }
    uint32_t excl = wave_base + incl - mine;
    uint64_t k = uint64_t(blockIdx.x) * K1_LDS_THREADS * draws_per_thread + excl;
    while (accept_bits) {
        int d = __builtin_ctz(accept_bits);
        accept_bits &= accept_bits - 1;
        cand[k++] = extract(d);
    }
    if (threadIdx.x == K1_LDS_THREADS - 1)
        wg_counts[blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
