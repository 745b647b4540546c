// lds_sort.h — the stable "rank inside the wave" step of every on-chip counting sort, and the chunk sort built on it.
//
// A wave owns consecutive rows of 64 keys. Per row, eight ballots (match_digit8) give every lane the mask of its peers:
// the valid lanes whose 8-bit digit equals its own. The lowest peer — the leader — does ONE returning LDS add of the
// group's size to the wave's histogram; what it gets back is the rank of the group's first key among the equal digits of
// the rows this wave ranked before. The other peers fetch that base from the leader with a shuffle and add the number
// of peers below them: ranks follow memory order, so the sort is stable.
//
// The step is split in two so that a kernel can vote for all its rows (the LDS adds of a wave stay in row order) and
// resolve afterwards, keep its own loop, its own scheduling barriers and its own packing of the 16-bit word in between:
//   rank_vote     the word: the add's return in the leader, `below | leader_lane << 8` elsewhere (below <= 63), and
//                 whether this lane leads: bit r of the caller's mask `leads`, r the row;
//   rank_resolve  the rank from that word.
// Users: scatter_kernel (sort_engine_impl.h; it spells rank_resolve out, see there) and sort_chunk below (bucket.hip,
// scatter1d.hip). sort_rows_kernel (sort_rows.hip) keeps the same two steps spelled out: measured, see there.
#pragma once
#include "common.h"

namespace ldssort {

__device__ inline uint64_t lanes_below(int lane) { return (lane == 0) ? 0ull : (~0ull >> (64 - lane)); }

// whist: this wave's 256 counters. A lane that is not valid gets a word nobody uses.
__device__ inline uint32_t rank_vote(uint32_t d, bool valid, uint32_t* whist, uint64_t below_mask, uint32_t& leads, int r) {
    const uint64_t m = match_digit8(d, __ballot(valid));   // valid lanes with my digit
    const uint32_t below = __popcll(m & below_mask);
    if (valid && below == 0) {
        leads |= 1u << r;
        return atomicAdd(&whist[d], (uint32_t)__popcll(m));
    }
    return below | ((uint32_t)(__ffsll((unsigned long long)m) - 1) << 8);
}

// rank among the equal digits of this wave; `word` may have travelled through 16 bits
__device__ inline uint32_t rank_resolve(uint32_t word, bool lead, int lane) {
    const int from = lead ? lane : (int)((word >> 8) & 63u);
    const uint32_t p = __shfl(word, from);
    return lead ? p : p + (word & 255u);
}

struct Item { uint32_t digit, payload; };

// Stable counting sort, in LDS, of n <= THREADS * ROUNDS (digit, payload) pairs, load(i) giving pair i: s_out gets the
// payloads grouped by digit in their original order, s_rowptr[0..256] the group boundaries. Returns the size of group
// `threadIdx.x`. THREADS == 256: thread d owns digit d. s_whist: THREADS / 64 x 256 words, s_tmp: THREADS / 64 words.
// The caller must have passed a barrier since the last readers of the LDS arrays; s_out / s_rowptr are valid after the
// caller's next barrier.
// CALLER_ZEROES: s_whist comes zeroed behind that barrier (a kernel that re-zeroes it under work of its own saves a
// barrier per chunk), and the digit scan takes ONE barrier: s_tmp is then next written a chunk later, behind the
// caller's barriers. Otherwise the histograms are zeroed here and the scan is block_excl_scan_u32.
template <int THREADS, int ROUNDS, bool CALLER_ZEROES, typename Load>
__device__ inline uint32_t sort_chunk(int n, Load load, uint32_t* s_out, uint32_t* s_whist, int32_t* s_rowptr, uint32_t* s_tmp) {
    static_assert(THREADS == 256, "thread d owns digit d");
    constexpr int WAVES = THREADS / 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t below_mask = lanes_below(lane);
    uint32_t* whist = s_whist + wave * 256;
    if constexpr (!CALLER_ZEROES) {
        for (int i = tid; i < WAVES * 256; i += THREADS) s_whist[i] = 0;
        __syncthreads();
    }
    const int rounds_n = (n + THREADS - 1) / THREADS;   // rows of 64 per wave
    const int wave_base = wave * rounds_n * 64;
    uint32_t dg[ROUNDS], vv[ROUNDS], rk[ROUNDS];
    uint32_t is_leader = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        dg[r] = 0; vv[r] = 0; rk[r] = 0;
        if (r < rounds_n) {
            const int i = wave_base + r * 64 + lane;
            const bool valid = i < n;
            if (valid) {
                const Item it = load(i);
                dg[r] = it.digit;
                vv[r] = it.payload;
            }
            rk[r] = rank_vote(dg[r], valid, whist, below_mask, is_leader, r);
        }
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
        if (r < rounds_n) rk[r] = rank_resolve(rk[r], (is_leader >> r) & 1u, lane);
    __syncthreads();
    // digit offsets: exclusive over waves, then over digits
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t c = s_whist[w * 256 + tid];
        s_whist[w * 256 + tid] = tot;
        tot += c;
    }
    uint32_t start;
    if constexpr (CALLER_ZEROES) {   // wave scan, wave totals through s_tmp
        const uint32_t incl = wave_incl_scan_u32(tot);
        if (lane == 63) s_tmp[wave] = incl;
        __syncthreads();
        start = incl - tot;
#pragma unroll
        for (int w = 0; w < WAVES; ++w)
            if (w < wave) start += s_tmp[w];
    } else {
        start = block_excl_scan_u32<WAVES>(tot, s_tmp, nullptr);
    }
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s_whist[w * 256 + tid] += start;
    s_rowptr[tid] = (int32_t)start;
    if (tid == 255) s_rowptr[256] = (int32_t)(start + tot);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (r < rounds_n) {
            const int i = wave_base + r * 64 + lane;
            if (i < n) s_out[whist[dg[r]] + rk[r]] = vv[r];
        }
    }
    return tot;
}

}  // namespace ldssort
