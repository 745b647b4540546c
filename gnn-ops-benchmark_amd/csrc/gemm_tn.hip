// Transposed-left product out[P, Q] = a[R, P]^T @ b[R, Q] for tall operands (R = nodes or edges, P and Q = layer widths):
// the weight gradient of every dense layer. The ordinary GEMM tiles only the output and would walk all R rows in
// ceil(P/128) * ceil(Q/128) workgroups; here the LONG dimension is split.
//
//   stage 1  one workgroup per (P-tile, Q-tile, slab of slab_rows consecutive rows): the slab is streamed through LDS in
//            chunks of 64 (16-bit) / 32 (fp32) rows and contracted on the matrix cores (v_mfma_f32_16x16x32_{bf16,f16},
//            v_mfma_f32_16x16x4_f32) into an fp32 partial tile [128, 128] of the workspace.
//   stage 2  one thread per output element adds its `slabs` partials in ascending slab order in fp32 and rounds once.
//
// No atomics, and the geometry is a function of (R, P, Q, dtype) alone — never of the CU count — so a call gives the same bits
// on every box and every run. tiles * slabs aims at 1024 workgroups (two to three per CU resident at once on 256 CUs: 36 KiB of LDS, 162-171 VGPRs
// each) with slabs of at least 2048 rows; slabs > 1 only while tiles * slabs <= 1024, so the workspace (slabs * padded P *
// padded Q * 4 bytes) never exceeds max(64 MiB, one padded fp32 output).
//
// The contraction index is the ROW of both operands, so both fragments are k-strided reads of a row-major image:
//   16-bit  two ds_read_b64_tr_b16 per fragment. 16-lane group g reads rows 4g .. 4g+3 (elements 0-3) and 16+4g .. 16+4g+3
//           (elements 4-7) of the 32-row k-step — the same permutation of k for both operands, which is all a sum needs. With
//           an image pitch of 288 B (= 32 B mod 256 B) the 8 rows a 32-lane half touches fall on 8 disjoint 8-bank runs.
//   fp32    one ds_read_b32 per fragment (lane l: row k + (l >> 4), column l & 15); pitch 576 B = 16 banks mod 32.
// Images are filled three ways, chosen per operand by the launcher: 16-byte row pieces (rows of whole aligned 16-B pieces),
// the slab's flat byte range in 16-byte pieces after a scalar head and tail (the tile covers the operand's whole width: rows
// of 11 elements or an operand that starts at an odd element need no copy), or single elements (everything else). Cells no
// load writes (columns past the operand, rows past the slab) hold zeros.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int TN_TP = 128, TN_TQ = 128;    // output tile of a workgroup; wave w owns its columns 32w .. 32w+31
constexpr int TN_THREADS = 256;
constexpr int TN_PITCH = 144;              // image row pitch in elements, both element sizes (288 B / 576 B)
constexpr int TN_IMG_BYTES = 64 * TN_PITCH * 2;   // = 32 * TN_PITCH * 4: one operand's chunk
constexpr int64_t TN_TARGET_WGS = 1024;
constexpr int64_t TN_MIN_SLAB_ROWS = 2048;
enum { TN_LOAD_VEC = 0, TN_LOAD_FLAT = 1, TN_LOAD_ELEM = 2 };

template <typename T> struct TnCfg { static constexpr int KC = 64, KSTEP = 32; };
template <> struct TnCfg<float> { static constexpr int KC = 32, KSTEP = 4; };

// element j of a 16-byte piece (j is a constant after unrolling)
template <typename T>
__device__ inline T tn_elem(const u32x4& v, int j) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if constexpr (sizeof(T) == 4) return __uint_as_float(w[j]);
    else return (T)(w[j >> 1] >> (16 * (j & 1)));
}

// Columns c0 .. c0+tw-1 of rows r0 .. r0+rows-1 of the row-major m [*, W] -> img[row][col] (pitch TN_PITCH). rows <= KC,
// tw <= 128; at most 1024 pieces of 16 B, four per thread, all loaded before the first is stored.
template <typename T>
__device__ inline void tn_stage(const T* __restrict__ m, int64_t W, int64_t r0, int rows, int64_t c0, int tw, int mode, T* img) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int tid = threadIdx.x;
    if (mode == TN_LOAD_VEC) {
        const int ppr = tw / VEC, total = rows * ppr;
        u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + k * TN_THREADS;
            if (i < total) v[k] = load16<true>(m + (r0 + i / ppr) * W + c0 + (i % ppr) * VEC);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + k * TN_THREADS;
            if (i < total) *reinterpret_cast<u32x4*>(img + (i / ppr) * TN_PITCH + (i % ppr) * VEC) = v[k];
        }
    } else if (mode == TN_LOAD_FLAT) {     // c0 == 0 and tw == W: elements r0*W .. (r0+rows)*W of m are the whole chunk
        const T* p = m + r0 * W;
        const int n = rows * (int)W;
        int head = (int)((16 - ((uintptr_t)p & 15)) & 15) / (int)sizeof(T);
        if (head > n) head = n;
        const int body = (n - head) / VEC, tail0 = head + body * VEC;
        u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + k * TN_THREADS;
            if (i < body) v[k] = load16<true>(p + head + i * VEC);
        }
        const int edge = head + (n - tail0);                 // < 2 * VEC scalar elements before and behind the body
        if (tid < edge) {
            const int e = tid < head ? tid : tail0 + (tid - head);
            img[(e / (int)W) * TN_PITCH + e % (int)W] = p[e];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + k * TN_THREADS;
            if (i < body) {
                const int e = head + i * VEC;
                int r = e / (int)W, c = e % (int)W;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    img[r * TN_PITCH + c] = tn_elem<T>(v[k], j);
                    if (++c == (int)W) { c = 0; ++r; }
                }
            }
        }
    } else {
        const int total = rows * tw;
        for (int i = tid; i < total; i += TN_THREADS) img[(i / tw) * TN_PITCH + i % tw] = m[(r0 + i / tw) * W + c0 + i % tw];
    }
}

__device__ inline void tn_zero(unsigned char* smem) {
    for (int i = threadIdx.x; i < 2 * TN_IMG_BYTES / 16; i += TN_THREADS) reinterpret_cast<u32x4*>(smem)[i] = u32x4{0u, 0u, 0u, 0u};
}

template <bool IS_BF16>
__device__ inline f32x4 tn_mfma16(const s16x8& a, const s16x8& b, const f32x4& c) {
    if constexpr (IS_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// k-strided 16-bit fragment: `addr` = this lane's piece of rows 4g .. 4g+3 of the k-step, 16 rows further for elements 4-7
__device__ inline s16x8 tn_frag16(const unsigned char* addr) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)addr);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(addr + 16 * TN_PITCH * 2));
    return s16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

// T: float or uint16_t (the bits of either 16-bit type). Grid: slab-major, tiles of one slab adjacent (they share its rows).
template <typename T, bool IS_BF16>
__global__ __launch_bounds__(TN_THREADS, 2) void gemm_tn_partial_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                                        float* __restrict__ ws, int64_t R, int64_t P, int64_t Q,
                                                                        int n_qt, int64_t tiles, int64_t slab_rows, int mode_a,
                                                                        int mode_b) {
    constexpr int KC = TnCfg<T>::KC, KSTEP = TnCfg<T>::KSTEP;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TN_IMG_BYTES];
    T* img_a = reinterpret_cast<T*>(smem);
    T* img_b = reinterpret_cast<T*>(smem + TN_IMG_BYTES);

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t slab = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int64_t p0 = (tile / n_qt) * TN_TP, q0 = (tile % n_qt) * TN_TQ;
    const int tw_p = (int)(P - p0 < TN_TP ? P - p0 : TN_TP), tw_q = (int)(Q - q0 < TN_TQ ? Q - q0 : TN_TQ);
    const int64_t s0 = slab * slab_rows, s1 = s0 + slab_rows < R ? s0 + slab_rows : R;
    const int n_mb = (tw_p + 15) / 16;                      // 16-row blocks of the tile that hold output rows
    const bool nb_on[2] = {wave * 32 < tw_q, wave * 32 + 16 < tw_q};

    f32x4 acc[8][2];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, i16 = lane & 15;
    tn_zero(smem);
    __syncthreads();
    for (int64_t k0 = s0; k0 < s1; k0 += KC) {
        const int rows = (int)(s1 - k0 < KC ? s1 - k0 : KC);
        if (rows < KC && k0 != s0) {                        // the last, partial chunk: rows past it must not keep the previous one
            tn_zero(smem);
            __syncthreads();
        }
        tn_stage<T>(a, P, k0, rows, p0, tw_p, mode_a, img_a);
        tn_stage<T>(b, Q, k0, rows, q0, tw_q, mode_b, img_b);
        __syncthreads();
        const int n_ks = (rows + KSTEP - 1) / KSTEP;
        if constexpr (sizeof(T) == 2) {
            // lane 4q+p of a 16-lane group supplies row q, columns 4p .. 4p+3 of its 4 x 16 block and receives column (lane & 15)
            const int lane_off = ((4 * g + (i16 >> 2)) * TN_PITCH + 4 * (i16 & 3)) * 2;
            for (int ks = 0; ks < n_ks; ++ks) {
                const unsigned char* ka = smem + ks * (32 * TN_PITCH * 2) + lane_off;
                const unsigned char* kb = ka + TN_IMG_BYTES + wave * 64;
                s16x8 bf[2];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    if (nb_on[ni]) bf[ni] = tn_frag16(kb + ni * 32);
#pragma unroll
                for (int mi = 0; mi < 8; ++mi)
                    if (mi < n_mb) {
                        const s16x8 af = tn_frag16(ka + mi * 32);
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            if (nb_on[ni]) acc[mi][ni] = tn_mfma16<IS_BF16>(af, bf[ni], acc[mi][ni]);
                    }
            }
        } else {
            const float* fa = reinterpret_cast<const float*>(smem) + g * TN_PITCH + i16;
            for (int ks = 0; ks < n_ks; ++ks) {
                const float* ka = fa + ks * (4 * TN_PITCH);
                const float* kb = ka + TN_IMG_BYTES / 4 + wave * 32;
                float bf[2];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    if (nb_on[ni]) bf[ni] = kb[ni * 16];
#pragma unroll
                for (int mi = 0; mi < 8; ++mi)
                    if (mi < n_mb) {
                        const float af = ka[mi * 16];
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            if (nb_on[ni]) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[ni], acc[mi][ni], 0, 0, 0);
                    }
            }
        }
        __syncthreads();
    }

    // C/D map: column = lane & 15, row = 4 * (lane >> 4) + register. Blocks without output rows or columns are not stored
    // (stage 2 never reads them).
    float* part = ws + ((int64_t)blockIdx.x) * (TN_TP * TN_TQ);   // blockIdx.x = slab * tiles + tile
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
        if (mi < n_mb)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
                if (nb_on[ni])
#pragma unroll
                    for (int r = 0; r < 4; ++r) part[(mi * 16 + 4 * g + r) * TN_TQ + wave * 32 + ni * 16 + i16] = acc[mi][ni][r];
}

template <typename T>
__global__ __launch_bounds__(256) void gemm_tn_reduce_kernel(const float* __restrict__ ws, T* __restrict__ out, int64_t P, int64_t Q,
                                                             int n_qt, int64_t tiles, int64_t slabs) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P * Q) return;
    const int64_t p = idx / Q, q = idx % Q;
    const float* src = ws + ((p / TN_TP) * n_qt + q / TN_TQ) * (TN_TP * TN_TQ) + (p % TN_TP) * TN_TQ + q % TN_TQ;
    const int64_t stride = tiles * (TN_TP * TN_TQ);
    float s = 0.f;
#pragma unroll 16
    for (int64_t sl = 0; sl < slabs; ++sl) s += src[sl * stride];    // ascending slab order, whatever the machine
    Elem<T>::store(out + idx, s);
}

struct TnGeometry { int64_t n_pt, n_qt, tiles, slab_rows, slabs; };

TnGeometry tn_geometry(int64_t R, int64_t P, int64_t Q) {
    TnGeometry t;
    t.n_pt = gnnops_cdiv(P, TN_TP);
    t.n_qt = gnnops_cdiv(Q, TN_TQ);
    t.tiles = t.n_pt * t.n_qt;
    const int64_t want = t.tiles > 0 && t.tiles < TN_TARGET_WGS ? TN_TARGET_WGS / t.tiles : 1;   // slabs aimed at
    int64_t rows = gnnops_cdiv(gnnops_cdiv(R, want), 64) * 64;
    if (rows < TN_MIN_SLAB_ROWS) rows = TN_MIN_SLAB_ROWS;
    t.slab_rows = rows;
    t.slabs = gnnops_cdiv(R, rows);
    return t;
}

int tn_load_mode(const void* m, int64_t W, int n_tiles_w, size_t es) {
    if ((W * es) % 16 == 0 && (uintptr_t)m % 16 == 0) return TN_LOAD_VEC;
    return n_tiles_w == 1 ? TN_LOAD_FLAT : TN_LOAD_ELEM;
}

template <typename T, typename TO, bool IS_BF16>
int tn_launch(const void* a, const void* b, void* out, int64_t R, int64_t P, int64_t Q, const TnGeometry& t, void* ws, hipStream_t stream) {
    if (t.slabs > 0) {
        hipLaunchKernelGGL((gemm_tn_partial_kernel<T, IS_BF16>), dim3((unsigned)(t.tiles * t.slabs)), dim3(TN_THREADS), 0, stream,
                           (const T*)a, (const T*)b, (float*)ws, R, P, Q, (int)t.n_qt, t.tiles, t.slab_rows,
                           tn_load_mode(a, P, (int)t.n_pt, sizeof(T)), tn_load_mode(b, Q, (int)t.n_qt, sizeof(T)));
        const int rc = gnnops_check_launch("gemm_tn partial");
        if (rc != GNNOPS_OK) return rc;
    }
    hipLaunchKernelGGL((gemm_tn_reduce_kernel<TO>), dim3((unsigned)gnnops_cdiv(P * Q, 256)), dim3(256), 0, stream, (const float*)ws,
                       (TO*)out, P, Q, (int)t.n_qt, t.tiles, t.slabs);
    return gnnops_check_launch("gemm_tn reduce");
}

int tn_check_shape(int64_t R, int64_t P, int64_t Q, int dtype) {
    GNNOPS_REQUIRE(R >= 0 && P >= 0 && Q >= 0, GNNOPS_EINVAL, "gemm_tn: negative size");
    GNNOPS_REQUIRE(dtype == GNNOPS_F16 || dtype == GNNOPS_BF16 || dtype == GNNOPS_F32, GNNOPS_EUNSUPPORTED,
                   "gemm_tn: unknown dtype code %d", dtype);
    // tiles * slabs is a 1-D grid and P * Q one thread each: far beyond any layer, but never wrap
    GNNOPS_REQUIRE(gnnops_cdiv(P, TN_TP) * gnnops_cdiv(Q, TN_TQ) < ((int64_t)1 << 30) && P < ((int64_t)1 << 31) && Q < ((int64_t)1 << 31),
                   GNNOPS_EUNSUPPORTED, "gemm_tn: output %lld x %lld is too large", (long long)P, (long long)Q);
    return GNNOPS_OK;
}

}  // namespace

extern "C" int gnnops_gemm_tn_geometry(int64_t R, int64_t P, int64_t Q, int dtype, int64_t* tile_p, int64_t* tile_q,
                                       int64_t* slab_rows, int64_t* slabs) {
    const int rc = tn_check_shape(R, P, Q, dtype);
    if (rc != GNNOPS_OK) return rc;
    const TnGeometry t = tn_geometry(R, P, Q);
    if (tile_p) *tile_p = TN_TP;
    if (tile_q) *tile_q = TN_TQ;
    if (slab_rows) *slab_rows = t.slab_rows;
    if (slabs) *slabs = t.slabs;
    return GNNOPS_OK;
}

extern "C" size_t gnnops_gemm_tn_workspace_bytes(int64_t R, int64_t P, int64_t Q, int dtype) {
    if (R < 0 || P < 0 || Q < 0 || !(dtype == GNNOPS_F16 || dtype == GNNOPS_BF16 || dtype == GNNOPS_F32)) return 0;
    const TnGeometry t = tn_geometry(R, P, Q);
    return (size_t)t.slabs * (size_t)t.tiles * TN_TP * TN_TQ * sizeof(float);
}

extern "C" int gnnops_gemm_tn(const void* a, const void* b, void* out, int64_t R, int64_t P, int64_t Q, int dtype, void* workspace,
                              size_t workspace_bytes, gnnops_stream_t s) {
    const int rc = tn_check_shape(R, P, Q, dtype);
    if (rc != GNNOPS_OK) return rc;
    if (P * Q == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(out && (R == 0 || (a && b)), GNNOPS_EINVAL, "gemm_tn: null pointer");
    const TnGeometry t = tn_geometry(R, P, Q);
    const size_t need = gnnops_gemm_tn_workspace_bytes(R, P, Q, dtype);
    GNNOPS_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), GNNOPS_EWORKSPACE, "gemm_tn: workspace %zu < %zu",
                   workspace_bytes, need);
    GNNOPS_REQUIRE(need == 0 || (uintptr_t)workspace % 4 == 0, GNNOPS_EINVAL, "gemm_tn: workspace must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)s;
    if (dtype == GNNOPS_F32) return tn_launch<float, float, false>(a, b, out, R, P, Q, t, workspace, stream);
    if (dtype == GNNOPS_BF16) return tn_launch<uint16_t, __hip_bfloat16, true>(a, b, out, R, P, Q, t, workspace, stream);
    return tn_launch<uint16_t, __half, false>(a, b, out, R, P, Q, t, workspace, stream);
}
