// spgemm.hip — row-wise (Gustavson) sparse x sparse behind spspmm(..., method="rowwise" | "auto"): C = A(m x k) @ B(k x n), both COO
// with int64 indices, viewed as CSR through the stable plan (rowptr, perm). The partial products never leave the chip: one wave owns
// an output row i, keeps fp32 accumulators for the row's column WINDOW [lo_i, lo_i + span_i) in LDS, and writes the row once.
//
//   row stats  per row of B: smallest and largest column (empty row: INT64_MAX / -1); call-wide flag "a row of B repeats a column",
//              found by marking an LDS bitmap over the row's own span (rows wider than MAX_SPAN are not checked: a product that
//              references one is too wide anyway)
//   symbolic   window of row i = [min, max] of the stats over the rows of B that row i of A references. Wider than MAX_SPAN: call-wide
//              flag "too wide", row skipped. Else the products' columns are marked in an LDS bitmap, popcount = nnz of the row;
//              a one-workgroup exclusive scan gives the row pointer of C. info = {nnz(C), too wide, B repeats, largest span}
//   numeric    accumulators start at +0.0f; the nonzeros of A's row are taken ONE AT A TIME in stored order, the lanes spread over
//              B's row in stored order: acc[col - lo] = acc[col - lo] + widen(round_to_storage(a * b)), a plain LDS read-add-write
//              (no row of B repeats a column, so no two lanes of a step meet; a wave-scope fence separates the steps). The bitmap is
//              then walked in ascending column order, 64 columns per step (ballot + popcount rank): row-major, sorted columns.
//
// Sums therefore run in the order expand-sort-compress (spspmm.hip + gnnops_coalesce) runs them: same bits. Product and sum are two
// roundings by construction (__fmul_rn, __fadd_rn), whatever the contraction flag says.
//
// LDS: a wave's row costs 4 B per window column plus one bit. MAX_SPAN = 4096 (the on-chip graph length of pool.hip's top-k):
// 4 waves x (16 KiB + 512 B) = 66 KiB per workgroup, dynamic (over the 64 KiB static limit), two workgroups per CU of 160 KiB. Calls
// whose largest span is at most 1024 take the small class: 4 x (4 KiB + 128 B) = 16.5 KiB, eight workgroups (32 waves) per CU.
//
// method="rowhash": the same three phases and the same order of summation for rows whose columns are spread too far for a window.
// The accumulator of a row is an open-addressing table in LDS: key = column - lo as 32 bits (0xFFFFFFFF = empty, so a row may span
// at most 2^32 - 1 columns), multiplicative hash, linear probing, a slot found or claimed by an LDS atomicCAS on the key.
//   row stats  smallest and largest column as above; a row of B of 2 .. HASH_MAX_ROW entries is checked for repeats by inserting
//              its keys (a key found present repeats) and marked, the row, not the call. Longer rows are not checked: the
//              symbolic pass refuses every output row that references one
//   symbolic   a referenced row of B that repeats a column raises "B repeats". Keys only; the number of claimed slots is the row's nnz. More than HASH_MAX_ROW: flag "too many", row skipped.
//              info = {nnz(C), 1 * too many + 2 * span too wide for a key, B repeats, largest row count}
//   numeric    find or claim the slot, then the plain read-add-write of its fp32 value. The occupied slots are compacted in place to
//              the front of the table, sorted by key in the wave and written once: up to 64 entries by counting the smaller keys
//              with shuffles, more by a stable LSD counting sort (8-bit digits over the significant bits of the row's span,
//              lds_sort.h's rank_vote / rank_resolve against a 256-counter histogram that holds the digits' start offsets) that
//              ping-pongs between the two halves of the table; its last pass writes to global memory.
// A row's table is the smallest power of two >= twice its entries (at least 64 slots), so at most half of it is ever claimed, a free
// slot always exists and the clear costs what the row needs; every probe loop is bounded by the table size all the same. LDS per
// wave: 8 B per slot + 1 KiB of histogram. Three classes by the call's largest row count: up to 256 / 1024 / 2048 entries = 512 /
// 2048 / 4096 slots per wave = 20 / 68 / 132 KiB per workgroup of 4 waves = 8 / 2 / 1 workgroups = 32 / 8 / 4 waves per CU.
#include "common.h"
#include "dispatch.h"
#include "lds_sort.h"

namespace {

constexpr int T = 256, NW = T / 64;
constexpr int MAX_SPAN = 4096;     // widest window: columns per output row held on chip
constexpr int SMALL_SPAN = 1024;   // the small window class
constexpr int INFO_WORDS = 4;      // int64 {nnz(C), too wide, B repeats, largest span}
constexpr int SCAN_T = 1024, SCAN_ITEMS = 8;

__device__ inline int64_t wave_min_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    return v;
}
__device__ inline int64_t wave_max_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}
__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// LDS accesses of one wave complete in order; this keeps the compiler from moving them across the step boundary
__device__ inline void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ inline int32_t at(const int32_t* __restrict__ perm, int32_t e) { return perm ? perm[e] : e; }

struct Layout {   // workspace: every array 256-byte aligned
    size_t bmin, bmax, brep, rowlo, rowptr, rowcnt, rowspan, total;
};
__host__ inline Layout layout_of(int64_t m, int64_t k) {
    Layout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += gnnops_align_up(bytes ? bytes : 1, 256); return at; };
    L.bmin = take((size_t)k * 8);
    L.bmax = take((size_t)k * 8);
    L.brep = take((size_t)k * 4);   // the hashed route's "this row of B repeats a column"
    L.rowlo = take((size_t)m * 8);
    L.rowptr = take((size_t)(m + 1) * 8);
    L.rowcnt = take((size_t)m * 4);
    L.rowspan = take((size_t)m * 4);
    L.total = o;
    return L;
}

// ---- row statistics of B: one wave per row, grid-stride ----
__global__ __launch_bounds__(T) void row_stats_kernel(const int32_t* __restrict__ rowptrB, const int32_t* __restrict__ permB,
                                                      const int64_t* __restrict__ colB, int64_t k, int64_t* __restrict__ bmin,
                                                      int64_t* __restrict__ bmax, int64_t* __restrict__ info) {
    __shared__ uint32_t s_bits[NW][MAX_SPAN / 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* bits = s_bits[wave];
    bool repeats = false;
    for (int64_t r = (int64_t)blockIdx.x * NW + wave; r < k; r += (int64_t)gridDim.x * NW) {
        const int32_t beg = rowptrB[r], end = rowptrB[r + 1];
        int64_t lo = INT64_MAX, hi = -1;
        for (int32_t e = beg + lane; e < end; e += 64) {
            const int64_t c = colB[at(permB, e)];
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
        lo = wave_min_i64(lo);
        hi = wave_max_i64(hi);
        if (lane == 0) { bmin[r] = lo; bmax[r] = hi; }
        if (end - beg < 2 || hi - lo >= MAX_SPAN) continue;   // nothing to repeat / wide: not checked (uniform over the wave)
        const int words = (int)((hi - lo) >> 5) + 1;
        for (int w = lane; w < words; w += 64) bits[w] = 0u;
        wave_fence();
        for (int32_t e = beg + lane; e < end; e += 64) {
            const uint32_t c = (uint32_t)(colB[at(permB, e)] - lo);       // < MAX_SPAN
            const uint32_t bit = 1u << (c & 31);
            if (atomicOr(&bits[c >> 5], bit) & bit) repeats = true;     // the LDS atomic orders two lanes that meet
        }
        wave_fence();
    }
    if (__any(repeats) && lane == 0) info[2] = 1;
}

// ---- symbolic: one wave per output row, grid-stride ----
__global__ __launch_bounds__(T) void symbolic_kernel(const int32_t* __restrict__ rowptrA, const int32_t* __restrict__ permA,
                                                     const int64_t* __restrict__ colA, int64_t m,
                                                     const int32_t* __restrict__ rowptrB, const int32_t* __restrict__ permB,
                                                     const int64_t* __restrict__ colB, const int64_t* __restrict__ bmin,
                                                     const int64_t* __restrict__ bmax, int64_t* __restrict__ rowlo,
                                                     uint32_t* __restrict__ rowcnt, uint32_t* __restrict__ rowspan,
                                                     int64_t* __restrict__ info) {
    __shared__ uint32_t s_bits[NW][MAX_SPAN / 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* bits = s_bits[wave];
    bool wide = false;
    uint32_t widest = 0;
    for (int64_t i = (int64_t)blockIdx.x * NW + wave; i < m; i += (int64_t)gridDim.x * NW) {
        const int32_t abeg = rowptrA[i], aend = rowptrA[i + 1];
        int64_t lo = INT64_MAX, hi = -1;
        for (int32_t p = abeg + lane; p < aend; p += 64) {
            const int64_t kk = colA[at(permA, p)];
            const int64_t l = bmin[kk], h = bmax[kk];
            lo = l < lo ? l : lo;
            hi = h > hi ? h : hi;
        }
        lo = wave_min_i64(lo);
        hi = wave_max_i64(hi);
        uint32_t cnt = 0, span = 0;
        if (hi >= lo) {
            if (hi - lo >= MAX_SPAN) {
                wide = true;
            } else {
                span = (uint32_t)(hi - lo) + 1;
                const int words = (int)((span + 31) >> 5);
                for (int w = lane; w < words; w += 64) bits[w] = 0u;
                wave_fence();
                for (int32_t p0 = abeg; p0 < aend; p0 += 64) {
                    const int32_t p = p0 + lane;
                    int32_t my_beg = 0, my_end = 0;
                    if (p < aend) {
                        const int64_t kk = colA[at(permA, p)];
                        my_beg = rowptrB[kk];
                        my_end = rowptrB[kk + 1];
                    }
                    const int steps = aend - p0 < 64 ? aend - p0 : 64;
                    for (int t = 0; t < steps; ++t) {
                        const int32_t beg = __shfl(my_beg, t), end = __shfl(my_end, t);
                        for (int32_t e = beg + lane; e < end; e += 64) {
                            const uint32_t c = (uint32_t)(colB[at(permB, e)] - lo);   // < span: lo and hi bound every referenced row
                            atomicOr(&bits[c >> 5], 1u << (c & 31));
                        }
                    }
                }
                wave_fence();
                for (int w = lane; w < words; w += 64) cnt += __popc(bits[w]);
                cnt = wave_sum_u32(cnt);
                wave_fence();
                widest = span > widest ? span : widest;
            }
        }
        if (lane == 0) { rowlo[i] = lo; rowcnt[i] = cnt; rowspan[i] = cnt ? span : 0u; }
    }
    if (lane == 0) {
        if (wide) info[1] = 1;
        if (widest) atomicMax((unsigned long long*)&info[3], (unsigned long long)widest);
    }
}

// exclusive scan of the row counts by one workgroup: rowptr[0..m], info[0] = nnz(C)
__global__ __launch_bounds__(SCAN_T) void scan_rows_kernel(const uint32_t* __restrict__ rowcnt, int64_t m, int64_t* __restrict__ rowptr,
                                                           int64_t* __restrict__ info) {
    __shared__ uint32_t s_tmp[SCAN_T / 64];
    int64_t carry = 0;
    for (int64_t base = 0; base < m; base += (int64_t)SCAN_T * SCAN_ITEMS) {
        const int64_t first = base + (int64_t)threadIdx.x * SCAN_ITEMS;
        uint32_t v[SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            v[j] = first + j < m ? rowcnt[first + j] : 0u;
            sum += v[j];   // a tile holds at most 8192 rows of at most 4096 entries: < 2^32
        }
        uint32_t tot;
        int64_t off = carry + block_excl_scan_u32<SCAN_T / 64>(sum, s_tmp, &tot);
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            if (first + j < m) rowptr[first + j] = off;
            off += v[j];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) {
        rowptr[m] = carry;
        info[0] = carry;
    }
}

// ---- numeric: one wave per output row, grid-stride; WIN columns of accumulator per wave ----
template <typename V, int WIN>
__global__ __launch_bounds__(T) void numeric_kernel(const int32_t* __restrict__ rowptrA, const int32_t* __restrict__ permA,
                                                    const int64_t* __restrict__ colA, const V* __restrict__ valA, int64_t m,
                                                    const int32_t* __restrict__ rowptrB, const int32_t* __restrict__ permB,
                                                    const int64_t* __restrict__ colB, const V* __restrict__ valB,
                                                    const int64_t* __restrict__ rowlo, const uint32_t* __restrict__ rowspan,
                                                    const int64_t* __restrict__ rowptrC, int64_t* __restrict__ out_row,
                                                    int64_t* __restrict__ out_col, V* __restrict__ out_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spgemm_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* acc = reinterpret_cast<float*>(spgemm_raw) + (size_t)wave * WIN;
    uint32_t* bits = reinterpret_cast<uint32_t*>(spgemm_raw + (size_t)NW * WIN * 4) + (size_t)wave * (WIN / 32);
    for (int64_t i = (int64_t)blockIdx.x * NW + wave; i < m; i += (int64_t)gridDim.x * NW) {
        uint32_t span = rowspan[i];   // 0: no products (or skipped as too wide: the caller never launches this pass then)
        if (span == 0) continue;
        if (span > (uint32_t)WIN) span = WIN;   // never taken: the host picks WIN from the largest span. Keeps every LDS index in bounds.
        const int64_t lo = rowlo[i];
        const int words = (int)((span + 31) >> 5);
        for (int c = lane; c < words * 32; c += 64) acc[c] = 0.0f;
        for (int w = lane; w < words; w += 64) bits[w] = 0u;
        wave_fence();
        const int32_t abeg = rowptrA[i], aend = rowptrA[i + 1];
        for (int32_t p0 = abeg; p0 < aend; p0 += 64) {
            const int32_t p = p0 + lane;
            int32_t my_beg = 0, my_end = 0;
            float my_a = 0.0f;
            if (p < aend) {
                const int32_t ea = at(permA, p);
                const int64_t kk = colA[ea];
                my_beg = rowptrB[kk];
                my_end = rowptrB[kk + 1];
                my_a = Elem<V>::load(valA + ea);
            }
            const int steps = aend - p0 < 64 ? aend - p0 : 64;
            for (int t = 0; t < steps; ++t) {   // one nonzero of A at a time, in stored order
                const int32_t beg = __shfl(my_beg, t), end = __shfl(my_end, t);
                const float a = __shfl(my_a, t);
                for (int32_t e0 = beg; e0 < end; e0 += 64) {   // trip count uniform over the wave
                    const int32_t e = e0 + lane;
                    if (e < end) {
                        const int32_t eb = at(permB, e);
                        uint32_t c = (uint32_t)(colB[eb] - lo);
                        c = c < span ? c : span - 1;   // never taken for columns the statistics saw; keeps the index in bounds
                        V stored;
                        Elem<V>::store(&stored, __fmul_rn(a, Elem<V>::load(valB + eb)));   // the product, rounded to the storage type
                        acc[c] = __fadd_rn(acc[c], Elem<V>::load(&stored));
                        atomicOr(&bits[c >> 5], 1u << (c & 31));
                    }
                    wave_fence();   // step t + 1 reads what step t wrote
                }
            }
        }
        // ascending columns, 64 per step: rank among the set bits of the step by ballot
        int64_t pos = rowptrC[i];
        for (int c0 = 0; c0 < words * 32; c0 += 64) {
            const int c = c0 + lane;
            const bool set = c < words * 32 && ((bits[c >> 5] >> (c & 31)) & 1u);
            const uint64_t mask = __ballot(set);
            if (set) {
                const int64_t q = pos + __popcll(mask & ((1ull << lane) - 1ull));
                out_row[q] = i;
                out_col[q] = lo + c;
                Elem<V>::store(out_val + q, acc[c]);
            }
            pos += __popcll(mask);
        }
        wave_fence();   // the next row clears what this one read
    }
}

inline int grid_for_rows(int64_t rows) { return gnnops_grid_cap(gnnops_cdiv(rows, NW), 256 * 8); }

template <typename V, int WIN>
int launch_numeric(hipStream_t stream, const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, const void* valA, int64_t m,
                   const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, const void* valB, const int64_t* rowlo,
                   const uint32_t* rowspan, const int64_t* rowptrC, int64_t* out_row, int64_t* out_col, void* out_val) {
    constexpr size_t lds = (size_t)NW * (WIN * 4 + WIN / 8);
    if (lds > 64 * 1024) {
        static bool raised = false;   // per kernel instantiation
        if (!raised) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&numeric_kernel<V, WIN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds) != hipSuccess)
                return gnnops_check_launch("spgemm_numeric: LDS attribute");
            raised = true;
        }
    }
    hipLaunchKernelGGL((numeric_kernel<V, WIN>), dim3(grid_for_rows(m)), dim3(T), lds, stream, rowptrA, permA, colA, (const V*)valA, m,
                       rowptrB, permB, colB, (const V*)valB, rowlo, rowspan, rowptrC, out_row, out_col, (V*)out_val);
    return gnnops_check_launch("spgemm_numeric");
}

// ---- the hashed route: accumulators addressed by hash instead of by offset ----
constexpr int HASH_MAX_ROW = 2048;                                        // most distinct columns of an output row
constexpr int HASH_SLOTS_S = 512, HASH_SLOTS_M = 2048, HASH_SLOTS_L = 2 * HASH_MAX_ROW;   // slots per wave by class; row limit = half
constexpr uint32_t HASH_EMPTY = 0xFFFFFFFFu;                              // the key no column offset may take
constexpr unsigned long long HASH_MANY = 1, HASH_WIDE = 2;                // bits of info[1]

// log2 of a row's table: the smallest power of two >= 2 * entries, at least 64 slots; entries <= HASH_MAX_ROW
__device__ inline int hash_log2_slots(uint32_t entries) {
    const uint32_t want = entries > 32 ? entries * 2 : 64;
    return 32 - __clz((int)(want - 1));
}

// The slot that holds `key`, claimed if need be (`fresh`); -1 after one probe of every slot, which cannot happen while at most
// half the table is claimed. Two lanes may race for one empty slot: the atomic picks one, the other probes on.
__device__ inline int hash_slot(uint32_t* keys, uint32_t mask, int shift, uint32_t key, bool& fresh) {
    uint32_t s = (key * 2654435761u) >> shift;
    for (uint32_t t = 0; t <= mask; ++t, s = (s + 1) & mask) {
        const uint32_t old = atomicCAS(&keys[s], HASH_EMPTY, key);
        if (old == HASH_EMPTY || old == key) {
            fresh = old == HASH_EMPTY;
            return (int)s;
        }
    }
    return -1;
}

__global__ __launch_bounds__(T) void hash_row_stats_kernel(const int32_t* __restrict__ rowptrB, const int32_t* __restrict__ permB,
                                                           const int64_t* __restrict__ colB, int64_t k, int64_t* __restrict__ bmin,
                                                           int64_t* __restrict__ bmax, uint32_t* __restrict__ brep) {
    __shared__ uint32_t s_keys[NW][HASH_SLOTS_L];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* keys = s_keys[wave];
    for (int64_t r = (int64_t)blockIdx.x * NW + wave; r < k; r += (int64_t)gridDim.x * NW) {
        const int32_t beg = rowptrB[r], end = rowptrB[r + 1];
        int64_t lo = INT64_MAX, hi = -1;
        for (int32_t e = beg + lane; e < end; e += 64) {
            const int64_t c = colB[at(permB, e)];
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
        lo = wave_min_i64(lo);
        hi = wave_max_i64(hi);
        if (lane == 0) { bmin[r] = lo; bmax[r] = hi; brep[r] = 0u; }
        // nothing to repeat / longer than a table or wider than a key: not checked, no output row may reference it (uniform)
        if (end - beg < 2 || end - beg > HASH_MAX_ROW || (uint64_t)(hi - lo) >= HASH_EMPTY) continue;
        bool repeats = false;
        const int lg = hash_log2_slots((uint32_t)(end - beg));
        const uint32_t mask = (1u << lg) - 1;
        for (uint32_t c = lane; c <= mask; c += 64) keys[c] = HASH_EMPTY;
        wave_fence();
        for (int32_t e = beg + lane; e < end; e += 64) {
            bool fresh = false;
            const int s = hash_slot(keys, mask, 32 - lg, (uint32_t)(colB[at(permB, e)] - lo), fresh);
            if (s < 0 || !fresh) repeats = true;   // found present: stored twice (a full table, which cannot be, is refused too)
        }
        wave_fence();
        if (__any(repeats) && lane == 0) brep[r] = 1u;   // lane 0 again: after its 0 above
    }
}

__global__ __launch_bounds__(T) void hash_symbolic_kernel(const int32_t* __restrict__ rowptrA, const int32_t* __restrict__ permA,
                                                          const int64_t* __restrict__ colA, int64_t m,
                                                          const int32_t* __restrict__ rowptrB, const int32_t* __restrict__ permB,
                                                          const int64_t* __restrict__ colB, const int64_t* __restrict__ bmin,
                                                          const int64_t* __restrict__ bmax, const uint32_t* __restrict__ brep,
                                                          int64_t* __restrict__ rowlo, uint32_t* __restrict__ rowcnt,
                                                          uint32_t* __restrict__ rowspan, int64_t* __restrict__ info) {
    __shared__ uint32_t s_keys[NW][HASH_SLOTS_L];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* keys = s_keys[wave];
    unsigned long long flags = 0;
    bool repeats = false;
    uint32_t most = 0;
    for (int64_t i = (int64_t)blockIdx.x * NW + wave; i < m; i += (int64_t)gridDim.x * NW) {
        const int32_t abeg = rowptrA[i], aend = rowptrA[i + 1];
        int64_t lo = INT64_MAX, hi = -1, longest = 0, products = 0;
        for (int32_t p = abeg + lane; p < aend; p += 64) {
            const int64_t kk = colA[at(permA, p)];
            const int64_t l = bmin[kk], h = bmax[kk], len = rowptrB[kk + 1] - rowptrB[kk];
            lo = l < lo ? l : lo;
            hi = h > hi ? h : hi;
            longest = len > longest ? len : longest;
            products += len;
            repeats |= brep[kk] != 0u;
        }
        lo = wave_min_i64(lo);
        hi = wave_max_i64(hi);
        longest = wave_max_i64(longest);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) products += __shfl_xor(products, o);
        uint32_t cnt = 0, span = 0;
        if (hi >= lo) {
            if (__any(repeats)) {   // two lanes of a step would meet on one value: the call is refused, the row skipped
            } else if ((uint64_t)(hi - lo) >= HASH_EMPTY) {
                flags |= HASH_WIDE;
            } else if (longest > HASH_MAX_ROW) {   // a row of B that the statistics could not check
                flags |= HASH_MANY;
            } else {
                span = (uint32_t)(hi - lo);
                const int lg = hash_log2_slots(products < HASH_MAX_ROW ? (uint32_t)products : (uint32_t)HASH_MAX_ROW);
                const uint32_t mask = (1u << lg) - 1;
                for (uint32_t c = lane; c <= mask; c += 64) keys[c] = HASH_EMPTY;
                wave_fence();
                bool over = false;   // uniform over the wave
                for (int32_t p0 = abeg; p0 < aend && !over; p0 += 64) {
                    const int32_t p = p0 + lane;
                    int32_t my_beg = 0, my_end = 0;
                    if (p < aend) {
                        const int64_t kk = colA[at(permA, p)];
                        my_beg = rowptrB[kk];
                        my_end = rowptrB[kk + 1];
                    }
                    const int steps = aend - p0 < 64 ? aend - p0 : 64;
                    for (int t = 0; t < steps && !over; ++t) {
                        const int32_t beg = __shfl(my_beg, t), end = __shfl(my_end, t);
                        for (int32_t e0 = beg; e0 < end && !over; e0 += 64) {
                            const int32_t e = e0 + lane;
                            bool fresh = false, full = false;
                            if (e < end) full = hash_slot(keys, mask, 32 - lg, (uint32_t)(colB[at(permB, e)] - lo), fresh) < 0;
                            cnt += __popcll(__ballot(fresh));
                            // at most HASH_MAX_ROW + 64 of the 2 * HASH_MAX_ROW slots are ever claimed: `full` cannot be
                            over = cnt > (uint32_t)HASH_MAX_ROW || __any(full);
                        }
                    }
                }
                wave_fence();   // the next row clears what this one probed
                if (over) {
                    flags |= HASH_MANY;
                    cnt = 0;
                }
                most = cnt > most ? cnt : most;
            }
        }
        if (lane == 0) { rowlo[i] = lo; rowcnt[i] = cnt; rowspan[i] = cnt ? span : 0u; }
    }
    if (__any(repeats) && lane == 0) info[2] = 1;
    if (lane == 0) {
        if (flags) atomicOr((unsigned long long*)&info[1], flags);
        if (most) atomicMax((unsigned long long*)&info[3], (unsigned long long)most);
    }
}

// SLOTS per wave: keys, then values, then the waves' 256-counter histograms
template <typename V, int SLOTS>
__global__ __launch_bounds__(T) void hash_numeric_kernel(const int32_t* __restrict__ rowptrA, const int32_t* __restrict__ permA,
                                                         const int64_t* __restrict__ colA, const V* __restrict__ valA, int64_t m,
                                                         const int32_t* __restrict__ rowptrB, const int32_t* __restrict__ permB,
                                                         const int64_t* __restrict__ colB, const V* __restrict__ valB,
                                                         const int64_t* __restrict__ rowlo, const uint32_t* __restrict__ rowcnt,
                                                         const uint32_t* __restrict__ rowspan, const int64_t* __restrict__ rowptrC,
                                                         int64_t* __restrict__ out_row, int64_t* __restrict__ out_col,
                                                         V* __restrict__ out_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spgemm_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* keys = reinterpret_cast<uint32_t*>(spgemm_raw) + (size_t)wave * SLOTS;
    float* vals = reinterpret_cast<float*>(spgemm_raw + (size_t)NW * SLOTS * 4) + (size_t)wave * SLOTS;
    uint32_t* hist = reinterpret_cast<uint32_t*>(spgemm_raw + (size_t)NW * SLOTS * 8) + (size_t)wave * 256;
    const uint64_t below_mask = ldssort::lanes_below(lane);
    for (int64_t i = (int64_t)blockIdx.x * NW + wave; i < m; i += (int64_t)gridDim.x * NW) {
        uint32_t cnt = rowcnt[i];   // 0: no products (or skipped: the caller never launches this pass then)
        if (cnt == 0) continue;
        if (cnt > (uint32_t)SLOTS / 2) cnt = SLOTS / 2;   // never taken: the host picks SLOTS from the largest row. Keeps every LDS index in bounds.
        const int lg = hash_log2_slots(cnt);
        const uint32_t slots = 1u << lg, mask = slots - 1;
        const int64_t lo = rowlo[i];
        for (uint32_t c = lane; c < slots; c += 64) {
            keys[c] = HASH_EMPTY;
            vals[c] = 0.0f;
        }
        wave_fence();
        const int32_t abeg = rowptrA[i], aend = rowptrA[i + 1];
        for (int32_t p0 = abeg; p0 < aend; p0 += 64) {
            const int32_t p = p0 + lane;
            int32_t my_beg = 0, my_end = 0;
            float my_a = 0.0f;
            if (p < aend) {
                const int32_t ea = at(permA, p);
                const int64_t kk = colA[ea];
                my_beg = rowptrB[kk];
                my_end = rowptrB[kk + 1];
                my_a = Elem<V>::load(valA + ea);
            }
            const int steps = aend - p0 < 64 ? aend - p0 : 64;
            for (int t = 0; t < steps; ++t) {   // one nonzero of A at a time, in stored order
                const int32_t beg = __shfl(my_beg, t), end = __shfl(my_end, t);
                const float a = __shfl(my_a, t);
                for (int32_t e0 = beg; e0 < end; e0 += 64) {   // trip count uniform over the wave
                    const int32_t e = e0 + lane;
                    if (e < end) {
                        const int32_t eb = at(permB, e);
                        bool fresh;
                        const int s = hash_slot(keys, mask, 32 - lg, (uint32_t)(colB[eb] - lo), fresh);
                        if (s >= 0) {   // always: the symbolic pass counted this row's keys, the table holds twice as many
                            V stored;
                            Elem<V>::store(&stored, __fmul_rn(a, Elem<V>::load(valB + eb)));   // the product, rounded to the storage type
                            vals[s] = __fadd_rn(vals[s], Elem<V>::load(&stored));
                        }
                    }
                    wave_fence();   // step t + 1 reads what step t wrote
                }
            }
        }
        // compact the occupied slots to the front, in place: a step writes below what it and the steps before it have read
        uint32_t n = 0;
        for (uint32_t c0 = 0; c0 < slots; c0 += 64) {
            const uint32_t key = keys[c0 + lane];
            const float val = vals[c0 + lane];
            const uint64_t occ = __ballot(key != HASH_EMPTY);
            if (key != HASH_EMPTY) {
                const uint32_t q = n + __popcll(occ & below_mask);
                keys[q] = key;
                vals[q] = val;
            }
            n += __popcll(occ);
            wave_fence();
        }
        n = n < cnt ? n : cnt;   // n == cnt; keeps the writes inside the row of C and the sort inside half the table
        const int64_t pos = rowptrC[i];
        if (n <= 64) {   // one key per lane: its place is the number of smaller keys
            const bool valid = (uint32_t)lane < n;
            const uint32_t key = valid ? keys[lane] : HASH_EMPTY;
            uint32_t rank = 0;
            for (uint32_t j = 0; j < n; ++j) rank += (uint32_t)__shfl(key, (int)j) < key;
            if (valid) {
                out_row[pos + rank] = i;
                out_col[pos + rank] = lo + key;
                Elem<V>::store(out_val + pos + rank, vals[lane]);
            }
        } else {   // stable LSD counting sort, 8 bits per pass, front half <-> back half; the last pass writes the row of C
            const int passes = (32 - __clz((int)rowspan[i]) + 7) >> 3;   // >= 1: more than 64 distinct keys span more than 64 columns
            uint32_t src = 0, dst = slots >> 1;
            for (int pass = 0; pass < passes; ++pass) {
                const int shift = 8 * pass;
                for (int d = lane; d < 256; d += 64) hist[d] = 0u;
                wave_fence();
                for (uint32_t r0 = 0; r0 < n; r0 += 64) {   // digit counts: the group's first lane adds the group
                    const bool valid = r0 + lane < n;
                    const uint32_t d = valid ? (keys[src + r0 + lane] >> shift) & 255u : 0u;
                    uint32_t leads = 0;
                    ldssort::rank_vote(d, valid, hist, below_mask, leads, 0);
                }
                wave_fence();
                uint32_t c[4], sum = 0;   // counts -> start offsets: lane l owns digits 4l .. 4l + 3
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    c[j] = hist[4 * lane + j];
                    sum += c[j];
                }
                uint32_t start = wave_incl_scan_u32(sum) - sum;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    hist[4 * lane + j] = start;
                    start += c[j];
                }
                wave_fence();
                for (uint32_t r0 = 0; r0 < n; r0 += 64) {   // the same adds now return each group's place
                    const bool valid = r0 + lane < n;
                    const uint32_t key = valid ? keys[src + r0 + lane] : 0u;
                    const float val = valid ? vals[src + r0 + lane] : 0.0f;
                    uint32_t leads = 0;
                    const uint32_t word = ldssort::rank_vote((key >> shift) & 255u, valid, hist, below_mask, leads, 0);
                    const uint32_t to = ldssort::rank_resolve(word, leads & 1u, lane);
                    if (valid && to < n) {   // always below n
                        if (pass == passes - 1) {
                            out_row[pos + to] = i;
                            out_col[pos + to] = lo + key;
                            Elem<V>::store(out_val + pos + to, val);
                        } else {
                            keys[dst + to] = key;
                            vals[dst + to] = val;
                        }
                    }
                }
                wave_fence();
                const uint32_t t = src;
                src = dst;
                dst = t;
            }
        }
        wave_fence();   // the next row clears what this one read
    }
}

template <typename V, int SLOTS>
int launch_hash_numeric(hipStream_t stream, const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, const void* valA, int64_t m,
                        const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, const void* valB, const int64_t* rowlo,
                        const uint32_t* rowcnt, const uint32_t* rowspan, const int64_t* rowptrC, int64_t* out_row, int64_t* out_col,
                        void* out_val) {
    constexpr size_t lds = (size_t)NW * (SLOTS * 8 + 256 * 4);
    static_assert(lds <= 160 * 1024, "one workgroup's tables must fit a CU's LDS");
    if (lds > 64 * 1024) {
        static bool raised = false;   // per kernel instantiation
        if (!raised) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&hash_numeric_kernel<V, SLOTS>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return gnnops_check_launch("spgemm_hash_numeric: LDS attribute");
            raised = true;
        }
    }
    hipLaunchKernelGGL((hash_numeric_kernel<V, SLOTS>), dim3(grid_for_rows(m)), dim3(T), lds, stream, rowptrA, permA, colA,
                       (const V*)valA, m, rowptrB, permB, colB, (const V*)valB, rowlo, rowcnt, rowspan, rowptrC, out_row, out_col,
                       (V*)out_val);
    return gnnops_check_launch("spgemm_hash_numeric");
}

}  // namespace

extern "C" int64_t gnnops_spgemm_max_span(void) { return MAX_SPAN; }

extern "C" size_t gnnops_spgemm_workspace_bytes(int64_t m, int64_t k) {
    if (m < 0 || k < 0) return 0;
    return layout_of(m, k).total;
}

// Phase 1: statistics of B's rows into `workspace`; clears info (int64[4], device) and raises info[2] when a row of B repeats a column.
extern "C" int gnnops_spgemm_row_stats(const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, int64_t k, int64_t nnzB,
                                       int64_t* d_info, void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(k >= 0 && nnzB >= 0 && nnzB < ((int64_t)1 << 31) && d_info, GNNOPS_EINVAL, "spgemm_row_stats: bad arguments");
    if (gnnops_memset_async(d_info, 0, INFO_WORDS * sizeof(int64_t), stream) != hipSuccess) return gnnops_check_launch("spgemm memset");
    if (k == 0 || nnzB == 0) return GNNOPS_OK;   // the symbolic pass returns early on the same sizes: the statistics are never read
    GNNOPS_REQUIRE(rowptrB && colB, GNNOPS_EINVAL, "spgemm_row_stats: null pointer");
    GNNOPS_REQUIRE(workspace && workspace_bytes >= layout_of(0, k).total, GNNOPS_EWORKSPACE, "spgemm_row_stats: workspace too small");
    const Layout L = layout_of(0, k);   // the statistics come first: their place does not depend on m
    unsigned char* ws = (unsigned char*)workspace;
    hipLaunchKernelGGL(row_stats_kernel, dim3(grid_for_rows(k)), dim3(T), 0, stream, rowptrB, permB, colB, k, (int64_t*)(ws + L.bmin),
                       (int64_t*)(ws + L.bmax), d_info);
    return gnnops_check_launch("spgemm_row_stats");
}

// Phase 2: windows and sizes of C's rows, its row pointer, and info = {nnz(C), too wide, B repeats, largest span}: the one host read.
extern "C" int gnnops_spgemm_symbolic(const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, int64_t m, int64_t nnzA,
                                      const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, int64_t k, int64_t nnzB,
                                      int64_t* d_info, void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(m >= 0 && k >= 0 && nnzA >= 0 && nnzB >= 0 && nnzA < ((int64_t)1 << 31) && nnzB < ((int64_t)1 << 31) && d_info,
                   GNNOPS_EINVAL, "spgemm_symbolic: bad arguments");
    if (m == 0 || k == 0 || nnzA == 0 || nnzB == 0) return GNNOPS_OK;   // info stays as row_stats cleared it: nnz(C) = 0
    GNNOPS_REQUIRE(rowptrA && colA && rowptrB && colB, GNNOPS_EINVAL, "spgemm_symbolic: null pointer");
    GNNOPS_REQUIRE(workspace && workspace_bytes >= layout_of(m, k).total, GNNOPS_EWORKSPACE, "spgemm_symbolic: workspace too small");
    const Layout L = layout_of(m, k);
    unsigned char* ws = (unsigned char*)workspace;
    hipLaunchKernelGGL(symbolic_kernel, dim3(grid_for_rows(m)), dim3(T), 0, stream, rowptrA, permA, colA, m, rowptrB, permB, colB,
                       (const int64_t*)(ws + L.bmin), (const int64_t*)(ws + L.bmax), (int64_t*)(ws + L.rowlo), (uint32_t*)(ws + L.rowcnt),
                       (uint32_t*)(ws + L.rowspan), d_info);
    hipLaunchKernelGGL(scan_rows_kernel, dim3(1), dim3(SCAN_T), 0, stream, (const uint32_t*)(ws + L.rowcnt), m, (int64_t*)(ws + L.rowptr),
                       d_info);
    return gnnops_check_launch("spgemm_symbolic");
}

// Phase 3: the rows of C, row-major with ascending columns, into out_row / out_col / out_val [nnz(C)]. Only for a call whose info
// raised neither flag; max_span is info[3] as the host read it (it picks the window class).
extern "C" int gnnops_spgemm_numeric(const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, const void* valA, int64_t m,
                                     int64_t nnzA, const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, const void* valB,
                                     int64_t k, int64_t nnzC, int64_t max_span, int64_t* out_row, int64_t* out_col, void* out_val,
                                     int dtype, const void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(m >= 0 && k >= 0 && nnzA >= 0 && nnzC >= 0, GNNOPS_EINVAL, "spgemm_numeric: negative size");
    if (nnzC == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(max_span >= 1 && max_span <= MAX_SPAN, GNNOPS_EINVAL, "spgemm_numeric: max_span %lld outside [1, %d]",
                   (long long)max_span, MAX_SPAN);
    GNNOPS_REQUIRE(rowptrA && colA && valA && rowptrB && colB && valB && out_row && out_col && out_val, GNNOPS_EINVAL,
                   "spgemm_numeric: null pointer");
    GNNOPS_REQUIRE(workspace && workspace_bytes >= layout_of(m, k).total, GNNOPS_EWORKSPACE, "spgemm_numeric: workspace too small");
    const Layout L = layout_of(m, k);
    const unsigned char* ws = (const unsigned char*)workspace;
    const int64_t* rowlo = (const int64_t*)(ws + L.rowlo);
    const uint32_t* rowspan = (const uint32_t*)(ws + L.rowspan);
    const int64_t* rowptrC = (const int64_t*)(ws + L.rowptr);
    return gnnops_with_dtype(dtype, "spgemm_numeric", [&](auto t) {
        using V = typename decltype(t)::type;
        auto* numeric = max_span <= SMALL_SPAN ? launch_numeric<V, SMALL_SPAN> : launch_numeric<V, MAX_SPAN>;
        return numeric(stream, rowptrA, permA, colA, valA, m, rowptrB, permB, colB, valB, rowlo, rowspan, rowptrC, out_row, out_col, out_val);
    });
}

// ---- the hashed route: same phases, same workspace, same arguments ----
extern "C" int64_t gnnops_spgemm_hash_max_row(void) { return HASH_MAX_ROW; }

// Phase 1: as gnnops_spgemm_row_stats; rows of B of up to gnnops_spgemm_hash_max_row() entries are checked for repeats.
extern "C" int gnnops_spgemm_hash_row_stats(const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, int64_t k, int64_t nnzB,
                                            int64_t* d_info, void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(k >= 0 && nnzB >= 0 && nnzB < ((int64_t)1 << 31) && d_info, GNNOPS_EINVAL, "spgemm_hash_row_stats: bad arguments");
    if (gnnops_memset_async(d_info, 0, INFO_WORDS * sizeof(int64_t), stream) != hipSuccess) return gnnops_check_launch("spgemm memset");
    if (k == 0 || nnzB == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(rowptrB && colB, GNNOPS_EINVAL, "spgemm_hash_row_stats: null pointer");
    GNNOPS_REQUIRE(workspace && workspace_bytes >= layout_of(0, k).total, GNNOPS_EWORKSPACE, "spgemm_hash_row_stats: workspace too small");
    const Layout L = layout_of(0, k);
    unsigned char* ws = (unsigned char*)workspace;
    hipLaunchKernelGGL(hash_row_stats_kernel, dim3(grid_for_rows(k)), dim3(T), 0, stream, rowptrB, permB, colB, k,
                       (int64_t*)(ws + L.bmin), (int64_t*)(ws + L.bmax), (uint32_t*)(ws + L.brep));
    return gnnops_check_launch("spgemm_hash_row_stats");
}

// Phase 2: d_info = {nnz(C), 1 * some output row has too many distinct columns + 2 * some output row spans too many columns for a
// 32-bit key, some row of B repeats a column, largest row count}.
extern "C" int gnnops_spgemm_hash_symbolic(const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, int64_t m, int64_t nnzA,
                                           const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, int64_t k, int64_t nnzB,
                                           int64_t* d_info, void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(m >= 0 && k >= 0 && nnzA >= 0 && nnzB >= 0 && nnzA < ((int64_t)1 << 31) && nnzB < ((int64_t)1 << 31) && d_info,
                   GNNOPS_EINVAL, "spgemm_hash_symbolic: bad arguments");
    if (m == 0 || k == 0 || nnzA == 0 || nnzB == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(rowptrA && colA && rowptrB && colB, GNNOPS_EINVAL, "spgemm_hash_symbolic: null pointer");
    GNNOPS_REQUIRE(workspace && workspace_bytes >= layout_of(m, k).total, GNNOPS_EWORKSPACE, "spgemm_hash_symbolic: workspace too small");
    const Layout L = layout_of(m, k);
    unsigned char* ws = (unsigned char*)workspace;
    hipLaunchKernelGGL(hash_symbolic_kernel, dim3(grid_for_rows(m)), dim3(T), 0, stream, rowptrA, permA, colA, m, rowptrB, permB, colB,
                       (const int64_t*)(ws + L.bmin), (const int64_t*)(ws + L.bmax), (const uint32_t*)(ws + L.brep),
                       (int64_t*)(ws + L.rowlo), (uint32_t*)(ws + L.rowcnt), (uint32_t*)(ws + L.rowspan), d_info);
    hipLaunchKernelGGL(scan_rows_kernel, dim3(1), dim3(SCAN_T), 0, stream, (const uint32_t*)(ws + L.rowcnt), m, (int64_t*)(ws + L.rowptr),
                       d_info);
    return gnnops_check_launch("spgemm_hash_symbolic");
}

// Phase 3: only for a call whose info raised no flag; max_row is info[3] as the host read it (it picks the table class).
extern "C" int gnnops_spgemm_hash_numeric(const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, const void* valA, int64_t m,
                                          int64_t nnzA, const int32_t* rowptrB, const int32_t* permB, const int64_t* colB,
                                          const void* valB, int64_t k, int64_t nnzC, int64_t max_row, int64_t* out_row, int64_t* out_col,
                                          void* out_val, int dtype, const void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(m >= 0 && k >= 0 && nnzA >= 0 && nnzC >= 0, GNNOPS_EINVAL, "spgemm_hash_numeric: negative size");
    if (nnzC == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(max_row >= 1 && max_row <= HASH_MAX_ROW, GNNOPS_EINVAL, "spgemm_hash_numeric: max_row %lld outside [1, %d]",
                   (long long)max_row, HASH_MAX_ROW);
    GNNOPS_REQUIRE(rowptrA && colA && valA && rowptrB && colB && valB && out_row && out_col && out_val, GNNOPS_EINVAL,
                   "spgemm_hash_numeric: null pointer");
    GNNOPS_REQUIRE(workspace && workspace_bytes >= layout_of(m, k).total, GNNOPS_EWORKSPACE, "spgemm_hash_numeric: workspace too small");
    const Layout L = layout_of(m, k);
    const unsigned char* ws = (const unsigned char*)workspace;
    const int64_t* rowlo = (const int64_t*)(ws + L.rowlo);
    const uint32_t* rowcnt = (const uint32_t*)(ws + L.rowcnt);
    const uint32_t* rowspan = (const uint32_t*)(ws + L.rowspan);
    const int64_t* rowptrC = (const int64_t*)(ws + L.rowptr);
    return gnnops_with_dtype(dtype, "spgemm_hash_numeric", [&](auto t) {
        using V = typename decltype(t)::type;
        auto* numeric = 2 * max_row <= HASH_SLOTS_S   ? launch_hash_numeric<V, HASH_SLOTS_S>
                        : 2 * max_row <= HASH_SLOTS_M ? launch_hash_numeric<V, HASH_SLOTS_M>
                                                      : launch_hash_numeric<V, HASH_SLOTS_L>;
        return numeric(stream, rowptrA, permA, colA, valA, m, rowptrB, permB, colB, valB, rowlo, rowcnt, rowspan, rowptrC, out_row, out_col,
                       out_val);
    });
}
