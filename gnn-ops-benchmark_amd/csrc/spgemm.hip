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
#include "common.h"

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
    size_t bmin, bmax, rowlo, rowptr, rowcnt, rowspan, total;
};
__host__ inline Layout layout_of(int64_t m, int64_t k) {
    Layout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += gnnops_align_up(bytes ? bytes : 1, 256); return at; };
    L.bmin = take((size_t)k * 8);
    L.bmax = take((size_t)k * 8);
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
    const Layout L = layout_of(0, k);   // bmin and bmax come first: their place does not depend on m
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
#define NUMERIC(V)                                                                                                                   \
    (max_span <= SMALL_SPAN                                                                                                          \
         ? launch_numeric<V, SMALL_SPAN>(stream, rowptrA, permA, colA, valA, m, rowptrB, permB, colB, valB, rowlo, rowspan, rowptrC,  \
                                         out_row, out_col, out_val)                                                                  \
         : launch_numeric<V, MAX_SPAN>(stream, rowptrA, permA, colA, valA, m, rowptrB, permB, colB, valB, rowlo, rowspan, rowptrC,    \
                                       out_row, out_col, out_val))
    switch (dtype) {
        case GNNOPS_F32: return NUMERIC(float);
        case GNNOPS_F16: return NUMERIC(__half);
        case GNNOPS_BF16: return NUMERIC(__hip_bfloat16);
        default: gnnops_set_error("spgemm_numeric: unknown dtype %d", dtype); return GNNOPS_EINVAL;
    }
#undef NUMERIC
}
