// segment_matmul.hip — pyg_lib.ops.segment_matmul: out[ptr[t] : ptr[t+1]] = x[ptr[t] : ptr[t+1]] @ W[t] (+ bias[t]), the
// per-type weight of HeteroLinear / RGCNConv. x [M, K], W [T, K, N], ptr int64 [T + 1] on the device, bias [T, N], out [M, N].
//
// It is the register-staged 128 x 128 tile of the dense product (gemm_tile.h) with three changes: a workgroup finds its
// segment, the row bound is the END OF ITS SEGMENT instead of M, and B starts at W + t * K * N. A segment of len rows is
// ceil(len / 128) tiles that start at the segment's first row, so tiles never straddle two weights; the last tile of a
// segment is partly empty (rows past the bound read as 0 and are not stored). Two launches:
//   1. segment_tiles_kernel (one workgroup): tile_start[t + 1] = tile_start[t] + ceil(len_t / 128), int32, in the workspace.
//   2. the product on a grid of (ceil(M / 128) + T, ceil(N / 128)) workgroups — an upper bound on the tile count that
//      needs no read-back of ptr. A workgroup binary-searches tile_start for its row-tile id and returns at once when the
//      id is at or past tile_start[T].
// Both kernels take a segment's rows from seg_bounds(), which CLAMPS ptr into [0, M] and treats a decreasing pair as an
// empty segment: whatever ptr holds, no row outside [0, M) is read or written (overlapping segments of a malformed ptr
// write the same rows twice, in bounds). No host synchronisation, no allocation, no atomics, nothing to clear.
#include "common.h"
#include "gemm_tile.h"

namespace {

__device__ inline void seg_bounds(const int64_t* __restrict__ ptr, int t, int64_t M, int64_t& lo, int64_t& hi) {
    lo = ptr[t];
    hi = ptr[t + 1];
    lo = lo < 0 ? 0 : (lo > M ? M : lo);
    hi = hi < 0 ? 0 : (hi > M ? M : hi);
    if (hi < lo) hi = lo;
}

// tile_start[0 .. T]: running tile count, capped at the grid's row-tile count (only a malformed ptr with overlapping
// segments can reach the cap; its surplus tiles are simply not computed). One workgroup of 256, 256 segments per round.
__global__ __launch_bounds__(256) void segment_tiles_kernel(const int64_t* __restrict__ ptr, int32_t* __restrict__ tile_start,
                                                            int T, int64_t M, int64_t max_tiles) {
    __shared__ int64_t s[256];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int base = 0; base < T; base += 256) {
        const int t = base + tid;
        int64_t cnt = 0;
        if (t < T) {
            int64_t lo, hi;
            seg_bounds(ptr, t, M, lo, hi);
            cnt = (hi - lo + BM - 1) / BM;
        }
        s[tid] = cnt;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int64_t v = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += v;
            __syncthreads();
        }
        const int64_t incl = carry + s[tid];
        if (t < T) tile_start[t + 1] = (int32_t)(incl < max_tiles ? incl : max_tiles);
        carry += s[255];
        __syncthreads();
    }
    if (tid == 0) tile_start[0] = 0;
}

// row-tile id -> (segment, first row, row bound); false: the id is past the last tile. Uniform per workgroup.
__device__ inline bool find_tile(const int64_t* __restrict__ ptr, const int32_t* __restrict__ tile_start, int T, int64_t M,
                                 int& t, int64_t& m0, int64_t& m_end) {
    const int32_t id = (int32_t)blockIdx.x;
    if (id >= tile_start[T]) return false;
    int lo = 0, hi = T;  // tile_start[lo] <= id < tile_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_start[mid] <= id) lo = mid; else hi = mid;
    }
    t = lo;
    int64_t r0;
    seg_bounds(ptr, t, M, r0, m_end);
    m0 = r0 + (int64_t)(id - tile_start[t]) * BM;
    return m0 < m_end;  // always true for a tile tile_start counts; keeps the tile inside [0, M) whatever the map holds
}

template <typename T, bool IS_BF16, int ALIGN>
__global__ __launch_bounds__(256, 2) void segment_matmul16_kernel(const uint16_t* __restrict__ X, const int64_t* __restrict__ ptr,
                                                                   const uint16_t* __restrict__ W, const T* __restrict__ bias,
                                                                   T* __restrict__ out, const int32_t* __restrict__ tile_start,
                                                                   int nt, int64_t M, int64_t N, int64_t K) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[TILE16_SMEM_BYTES];
    int t;
    int64_t m0, m_end;
    if (!find_tile(ptr, tile_start, nt, M, t, m0, m_end)) return;
    gemm_tile16<T, IS_BF16, ALIGN>(smem, X, W + (int64_t)t * K * N, bias ? bias + (int64_t)t * N : nullptr, out, m0,
                                   (int64_t)blockIdx.y * BN, m_end, N, K, K, N, 0);
}

__global__ __launch_bounds__(256, 4) void segment_matmul_f32_kernel(const float* __restrict__ X, const int64_t* __restrict__ ptr,
                                                                    const float* __restrict__ W, const float* __restrict__ bias,
                                                                    float* __restrict__ out, const int32_t* __restrict__ tile_start,
                                                                    int nt, int64_t M, int64_t N, int64_t K, bool a_vec, bool b_vec) {
    __shared__ __attribute__((aligned(16))) float smem[TILE_F32_SMEM_F];
    int t;
    int64_t m0, m_end;
    if (!find_tile(ptr, tile_start, nt, M, t, m0, m_end)) return;
    gemm_tile_f32(smem, X, W + (int64_t)t * K * N, bias ? bias + (int64_t)t * N : nullptr, out, m0, (int64_t)blockIdx.y * BN,
                  m_end, N, K, a_vec, b_vec, 0);
}

}  // namespace

extern "C" size_t gnnops_segment_matmul_workspace_bytes(int64_t T) {
    if (T < 0) return 0;
    return gnnops_align_up((size_t)(T + 1) * sizeof(int32_t), 256);
}

extern "C" int gnnops_segment_matmul_geometry(int dtype, int64_t* tile_m, int64_t* tile_n, int64_t* k_step) {
    GNNOPS_REQUIRE(dtype == GNNOPS_F16 || dtype == GNNOPS_BF16 || dtype == GNNOPS_F32, GNNOPS_EUNSUPPORTED,
                   "segment_matmul: unknown dtype code %d", dtype);
    if (tile_m) *tile_m = BM;
    if (tile_n) *tile_n = BN;
    if (k_step) *k_step = dtype == GNNOPS_F32 ? FBK : BK;
    return GNNOPS_OK;
}

extern "C" int gnnops_segment_matmul(const void* x, const int64_t* ptr, const void* w, const void* bias, void* out, int64_t M,
                                     int64_t K, int64_t N, int64_t T, int dtype, void* workspace, size_t workspace_bytes,
                                     gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(M >= 0 && K >= 0 && N >= 0 && T >= 0, GNNOPS_EINVAL, "segment_matmul: negative size");
    GNNOPS_REQUIRE(dtype == GNNOPS_F16 || dtype == GNNOPS_BF16 || dtype == GNNOPS_F32, GNNOPS_EUNSUPPORTED,
                   "segment_matmul: unknown dtype code %d", dtype);
    if (M * N == 0 || T == 0) return GNNOPS_OK;
    const int64_t max_tiles = gnnops_cdiv(M, BM) + T, col_tiles = gnnops_cdiv(N, BN);
    GNNOPS_REQUIRE(T < ((int64_t)1 << 30) && max_tiles < ((int64_t)1 << 31) && col_tiles < 65536, GNNOPS_EUNSUPPORTED,
                   "segment_matmul: %lld rows in %lld segments by %lld columns is too large", (long long)M, (long long)T, (long long)N);
    GNNOPS_REQUIRE(ptr && out && (K == 0 || (x && w)), GNNOPS_EINVAL, "segment_matmul: null pointer");
    const size_t need = gnnops_segment_matmul_workspace_bytes(T);
    GNNOPS_REQUIRE(workspace && workspace_bytes >= need, GNNOPS_EWORKSPACE, "segment_matmul: workspace %zu < %zu", workspace_bytes,
                   need);
    GNNOPS_REQUIRE((uintptr_t)workspace % 4 == 0, GNNOPS_EINVAL, "segment_matmul: workspace must be 4-byte aligned");
    int32_t* tile_start = (int32_t*)workspace;
    hipLaunchKernelGGL(segment_tiles_kernel, dim3(1), dim3(256), 0, stream, ptr, tile_start, (int)T, M, max_tiles);
    int rc = gnnops_check_launch("segment_matmul tile map");
    if (rc != GNNOPS_OK) return rc;

    const dim3 grid((unsigned)max_tiles, (unsigned)col_tiles);
    if (dtype == GNNOPS_F32) {
        const bool a_vec = (K % 4 == 0) && ((uintptr_t)x % 16 == 0);
        const bool b_vec = (N % 4 == 0) && ((uintptr_t)w % 16 == 0);
        hipLaunchKernelGGL(segment_matmul_f32_kernel, grid, dim3(256), 0, stream, (const float*)x, ptr, (const float*)w,
                           (const float*)bias, (float*)out, (const int32_t*)tile_start, (int)T, M, N, K, a_vec, b_vec);
        return gnnops_check_launch("segment_matmul f32");
    }
    // the widest piece both operands' rows allow (every W[t] starts a multiple of N elements into w)
    int align = 16;
    for (; align > 2; align >>= 1)
        if ((K * 2) % align == 0 && (N * 2) % align == 0 && (uintptr_t)x % align == 0 && (uintptr_t)w % align == 0) break;
#define GNNOPS_SEGMM(AL)                                                                                                         \
    do {                                                                                                                         \
        if (dtype == GNNOPS_BF16)                                                                                                \
            hipLaunchKernelGGL((segment_matmul16_kernel<__hip_bfloat16, true, AL>), grid, dim3(256), 0, stream,                  \
                               (const uint16_t*)x, ptr, (const uint16_t*)w, (const __hip_bfloat16*)bias, (__hip_bfloat16*)out,   \
                               (const int32_t*)tile_start, (int)T, M, N, K);                                                     \
        else                                                                                                                     \
            hipLaunchKernelGGL((segment_matmul16_kernel<__half, false, AL>), grid, dim3(256), 0, stream, (const uint16_t*)x, ptr, \
                               (const uint16_t*)w, (const __half*)bias, (__half*)out, (const int32_t*)tile_start, (int)T, M, N, K); \
    } while (0)
    switch (align) {
        case 16: GNNOPS_SEGMM(16); break;
        case 8: GNNOPS_SEGMM(8); break;
        case 4: GNNOPS_SEGMM(4); break;
        default: GNNOPS_SEGMM(2); break;
    }
#undef GNNOPS_SEGMM
    return gnnops_check_launch("segment_matmul");
}
