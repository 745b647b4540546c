// spline_bw.hip — the backward of torch_spline_conv's three ops (spline.hip has the forward and the notation: b[e, s] and
// wi[e, s] = basis value / kernel index of combination s of edge e, S = (degree + 1)^D). With G = d L / d out:
//
//   d weight[k, i, o] = sum over (e, s) with wi[e, s] = k  of  b[e, s] * x[xr(e), i] * G[gr(e), o]        (bw_weight)
//   d b[e, s]         = sum over i, o  of  x[xr(e), i] * weight[wi[e, s], i, o] * G[gr(e), o]              (bw_basis)
//   d pseudo[e, d]    = sum_s d b[e, s] * (kernel_size[d] - degree * is_open[d]) * B'_m(frac_d, k_d) * prod_{d' != d} B_m(frac_d', k_d')
//   d x               = the FORWARD op on the transposed table [K, Mout, Min] (gnnops_transpose_batched): no kernel here.
//
// xr / gr are optional int64 row indices (null = row e): spline_weighting's backward passes null, spline_conv's passes
// edge_index[1] / edge_index[0], so neither x[col] nor G[row] is ever materialised.
//
// bw_weight is the contraction the forward kernel's comment asks for: the E * S (edge, combination) pairs are grouped by
// kernel index with the library's own plan (rowptr [K + 1], perm: position p -> edge p / S, combination p % S), and
//   d weight[k] = A_k^T . C_k,   A_k [n_k, Min] = rows b * x[xr],  C_k [n_k, Mout] = rows G[gr]
// runs on the matrix cores: 32-pair slabs of both gathered operands are staged in LDS (b * x formed in fp32 and rounded
// once to the storage type), fp16 / bf16 through v_mfma_f32_16x16x32, fp32 through v_mfma_f32_16x16x4_f32 (exact fp32
// products, the VALU's peak rate, and one register per operand instead of a 64-wide register tile), fp32 accumulators.
// The sorted pair list is cut at multiples of a chunk length (at most T_HUB = 8192 pairs); a workgroup owns (chunk, 64 x 64
// tile of Min x Mout) and walks the kernels whose groups meet its chunk. A group that lies inside one chunk is written
// straight to d weight; a group that crosses a cut leaves one fp32 partial per chunk in the workspace (at most two per
// chunk: the group that began before it, slot 0, and the group that runs past its end, slot 1), and the finishing pass sums
// a group's partials in ascending chunk order. That pass also writes the exact zeros of the empty kernels. No atomics:
// two calls on the same inputs give the same bits.
#include "common.h"
#include "dispatch.h"
#include "hub.h"
#include "spline_common.h"

namespace {

constexpr int BW_SLAB = 32;      // pairs per LDS slab = the k extent of one 16x16x32 MFMA (eight 16x16x4 steps in fp32)
constexpr int BW_TILE = 64;      // Min x Mout tile of a workgroup: 4 waves x (16 rows of i) x (4 column tiles of o)
constexpr int BW_RS16 = 40;      // 16-bit LDS image [channel][pair]: 32 pairs + 8 of padding, rows stay 16-byte aligned
constexpr int BW_RS32 = 80;      // fp32 LDS image [pair][channel]: 64 channels + 16 (rows r and r + 1 on different banks)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// chunk length of the sorted pair list: short lists are cut finer so that a few thousand workgroups exist
inline int64_t bw_chunk_len(int64_t P) {
    int64_t t = gnnops_cdiv(gnnops_cdiv(P, 2048), BW_SLAB) * BW_SLAB;
    if (t < 256) t = 256;
    if (t > hub::T_HUB) t = hub::T_HUB;
    return t;
}

// VEC consecutive channels [c0, c0 + VEC) of one row as floats; zero past `width`. `vec`: rows are 16-byte aligned pieces.
template <typename T>
__device__ inline void load_piece(const T* __restrict__ row, int c0, int width, bool vec, float* f) {
    constexpr int VEC = Elem<T>::VEC;
    if (vec && c0 + VEC <= width) {
        Elem<T>::unpack(load16<false>(row + c0), f);
    } else {
#pragma unroll
        for (int q = 0; q < VEC; ++q) f[q] = c0 + q < width ? Elem<T>::load(row + c0 + q) : 0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bw_weight_kernel(const T* __restrict__ g, const T* __restrict__ x, const T* __restrict__ basis,
                                                        const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
                                                        const int64_t* __restrict__ x_rows, const int64_t* __restrict__ g_rows,
                                                        T* __restrict__ grad_weight, float* __restrict__ partial, int64_t P, int K,
                                                        int Min, int Mout, int S, int64_t chunk_len, int tiles_i, int tiles_o,
                                                        int vec_x, int vec_g) {
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int VEC = Elem<T>::VEC;
    constexpr int PIECES = BW_TILE / VEC;                       // 16-byte pieces of a 64-channel tile row
    constexpr int LDS_ELEMS = F32 ? BW_SLAB * BW_RS32 : BW_TILE * BW_RS16;
    __shared__ __attribute__((aligned(16))) T sA[LDS_ELEMS];
    __shared__ __attribute__((aligned(16))) T sC[LDS_ELEMS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntiles = tiles_i * tiles_o;
    const int64_t c = blockIdx.x / ntiles;
    const int tile = (int)(blockIdx.x % ntiles);
    const int i0 = (tile / tiles_o) * BW_TILE, o0 = (tile % tiles_o) * BW_TILE;
    const int64_t c0 = c * chunk_len, c1 = c0 + chunk_len < P ? c0 + chunk_len : P;

    // the group that holds position c0: the last k with rowptr[k] <= c0 (rowptr[0] = 0 <= c0 < P = rowptr[K])
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)rowptr[mid] <= c0) lo = mid; else hi = mid;
    }

    const bool wave_rows = i0 + 16 * wave < Min;                // this wave's 16 rows of i hold anything at all
    for (int k = lo; k < K; ++k) {
        const int64_t kb = rowptr[k], ke = rowptr[k + 1];
        if (kb >= c1) break;
        const int64_t beg = kb > c0 ? kb : c0, end = ke < c1 ? ke : c1;
        if (beg >= end) continue;                               // an empty kernel inside the chunk
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int64_t slab = beg; slab < end; slab += BW_SLAB) {
            __syncthreads();                                    // the previous slab's fragments have been read
            for (int it = tid; it < BW_SLAB * PIECES; it += 256) {
                const int pair = it & (BW_SLAB - 1), piece = it / BW_SLAB;
                const int64_t p = slab + pair;
                float fa[VEC], fc[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) fa[q] = fc[q] = 0.f;
                if (p < end) {
                    const int64_t pos = perm[p];
                    const int64_t e = pos / S;
                    const float b = Elem<T>::load(basis + pos);
                    const int64_t xr = x_rows ? x_rows[e] : e, gr = g_rows ? g_rows[e] : e;
                    if (i0 + piece * VEC < Min) load_piece<T>(x + xr * Min, i0 + piece * VEC, Min, vec_x, fa);
                    if (o0 + piece * VEC < Mout) load_piece<T>(g + gr * Mout, o0 + piece * VEC, Mout, vec_g, fc);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) fa[q] *= b;
                }
                if constexpr (F32) {
                    store16<false>(sA + pair * BW_RS32 + piece * VEC, Elem<T>::pack(fa));
                    store16<false>(sC + pair * BW_RS32 + piece * VEC, Elem<T>::pack(fc));
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        Elem<T>::store(sA + (piece * VEC + q) * BW_RS16 + pair, fa[q]);
                        Elem<T>::store(sC + (piece * VEC + q) * BW_RS16 + pair, fc[q]);
                    }
                }
            }
            __syncthreads();
            if (!wave_rows) continue;
            if constexpr (F32) {
                // v_mfma_f32_16x16x4_f32: A[row lane & 15][k = lane >> 4], B[k = lane >> 4][col lane & 15]
#pragma unroll
                for (int kk = 0; kk < BW_SLAB / 4; ++kk) {
                    const int r = kk * 4 + (lane >> 4);
                    const float a = sA[r * BW_RS32 + 16 * wave + (lane & 15)];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        if (o0 + nt * 16 >= Mout) continue;
                        const float bv = sC[r * BW_RS32 + nt * 16 + (lane & 15)];
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[nt], 0, 0, 0);
                    }
                }
            } else {
                // v_mfma_f32_16x16x32: A[row lane & 15][k = 8 (lane >> 4) + j], B[k = 8 (lane >> 4) + j][col lane & 15]
                const s16x8 a = *reinterpret_cast<const s16x8*>(sA + (16 * wave + (lane & 15)) * BW_RS16 + 8 * (lane >> 4));
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    if (o0 + nt * 16 >= Mout) continue;
                    const s16x8 bv = *reinterpret_cast<const s16x8*>(sC + (nt * 16 + (lane & 15)) * BW_RS16 + 8 * (lane >> 4));
                    if constexpr (sizeof(T) == 2 && __is_same(T, __half))
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, bv), acc[nt], 0, 0, 0);
                    else
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bv), acc[nt], 0, 0, 0);
                }
            }
        }

        // C/D: column = lane & 15, row = 4 (lane >> 4) + register
        const bool head = kb < c0, tail = ke > c1;
        float* part = (head || tail) ? partial + (c * 2 + (head ? 0 : 1)) * (int64_t)Min * Mout : nullptr;
        T* dst = grad_weight + (int64_t)k * Min * Mout;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int o = o0 + nt * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 16 * wave + 4 * (lane >> 4) + r;
                if (i < Min && o < Mout) {
                    if (part) part[(int64_t)i * Mout + o] = acc[nt][r];
                    else Elem<T>::store(dst + (int64_t)i * Mout + o, acc[nt][r]);
                }
            }
        }
    }
}

// d weight[k] for the kernels the first pass did not finish: exact zeros where no pair landed, and the sum of the partials
// in ascending chunk order where the group crosses a cut. rowptr == null: no pairs at all.
template <typename T>
__global__ __launch_bounds__(256) void bw_weight_finish_kernel(const int32_t* __restrict__ rowptr, const float* __restrict__ partial,
                                                               T* __restrict__ grad_weight, int64_t K, int64_t MM, int64_t chunk_len) {
    const int64_t total = K * MM;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = t / MM, m = t % MM;
        const int64_t kb = rowptr ? rowptr[k] : 0, ke = rowptr ? rowptr[k + 1] : 0;
        if (kb == ke) {
            Elem<T>::store(grad_weight + t, 0.f);
            continue;
        }
        const int64_t cf = kb / chunk_len, cl = (ke - 1) / chunk_len;
        if (cf == cl) continue;                                 // inside one chunk: already written
        float acc = partial[(cf * 2 + 1) * MM + m];
        for (int64_t c = cf + 1; c <= cl; ++c) acc += partial[(c * 2) * MM + m];
        Elem<T>::store(grad_weight + t, acc);
    }
}

// d b[e, s] = x_e^T W_{wi[e, s]} g_e: a wave per edge, lanes over o (the kernel matrix is read as coalesced rows, like the
// forward kernel does), fp32 in the order (o chunk, i), one wave reduction per s.
template <typename T>
__global__ __launch_bounds__(256) void bw_basis_kernel(const T* __restrict__ g, const T* __restrict__ x, const T* __restrict__ weight,
                                                       const int64_t* __restrict__ weight_index, const int64_t* __restrict__ x_rows,
                                                       const int64_t* __restrict__ g_rows, T* __restrict__ grad_basis, int64_t E,
                                                       int Min, int Mout, int S) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t e = wave0; e < E; e += nwaves) {
        const T* xe = x + (x_rows ? x_rows[e] : e) * Min;
        const T* ge = g + (g_rows ? g_rows[e] : e) * Mout;
        for (int s = 0; s < S; ++s) {
            const T* wk = weight + weight_index[e * S + s] * Min * Mout;
            float tot = 0.f;
            for (int o = lane; o < Mout; o += 64) {
                float v = 0.f;
                for (int i = 0; i < Min; ++i) v += Elem<T>::load(xe + i) * Elem<T>::load(wk + (int64_t)i * Mout + o);
                tot += v * Elem<T>::load(ge + o);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
            if (lane == 0) Elem<T>::store(grad_basis + e * S + s, tot);
        }
    }
}

// d pseudo[e, d]: one thread per (e, d), the S products re-formed with B' in place of B on axis d
template <typename T, int M>
__global__ __launch_bounds__(256) void basis_bw_kernel(const T* __restrict__ grad_basis, const T* __restrict__ pseudo, SplineMeta sm,
                                                       int64_t E, T* __restrict__ grad_pseudo) {
    const int64_t total = E * sm.D;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = t / sm.D;
        const int d = (int)(t % sm.D);
        float fr[MAX_DIM];
#pragma unroll
        for (int dd = 0; dd < MAX_DIM; ++dd) {
            if (dd < sm.D) {
                const float v = Elem<T>::load(pseudo + e * sm.D + dd) * (float)(sm.kernel_size[dd] - M * sm.is_open[dd]);
                fr[dd] = v - floorf(v);
            }
        }
        float acc = 0.f;
        for (int s = 0; s < sm.S; ++s) {
            int k = s;
            float prod = 1.f;
#pragma unroll
            for (int dd = 0; dd < MAX_DIM; ++dd) {
                if (dd < sm.D) {
                    const int k_mod = k % (M + 1);
                    k /= (M + 1);
                    prod *= dd == d ? bspline_grad<M>(fr[dd], k_mod) : bspline<M>(fr[dd], k_mod);
                }
            }
            acc += Elem<T>::load(grad_basis + e * sm.S + s) * prod;
        }
        Elem<T>::store(grad_pseudo + t, acc * (float)(sm.kernel_size[d] - M * sm.is_open[d]));
    }
}

template <typename T>
int run_basis_bw(const void* grad_basis, const void* pseudo, const SplineMeta& sm, int64_t E, void* grad_pseudo, hipStream_t stream) {
    const int grid = gnnops_grid_cap(gnnops_cdiv(E * sm.D, 256));
#define GNNOPS_BB(MM)                                                                                                           \
    hipLaunchKernelGGL((basis_bw_kernel<T, MM>), dim3(grid), dim3(256), 0, stream, (const T*)grad_basis, (const T*)pseudo, sm, E, \
                       (T*)grad_pseudo)
    switch (sm.degree) {
        case 1: GNNOPS_BB(1); break;
        case 2: GNNOPS_BB(2); break;
        default: GNNOPS_BB(3); break;
    }
#undef GNNOPS_BB
    return gnnops_check_launch("spline_basis_bw");
}

template <typename T>
int run_bw_weight(const void* g, const void* x, const void* basis, const int32_t* rowptr, const int32_t* perm, const int64_t* x_rows,
                  const int64_t* g_rows, void* grad_weight, int64_t P, int64_t K, int Min, int Mout, int S, float* partial,
                  hipStream_t stream) {
    const int64_t chunk_len = bw_chunk_len(P), nchunks = gnnops_cdiv(P, chunk_len);
    const int tiles_i = (Min + BW_TILE - 1) / BW_TILE, tiles_o = (Mout + BW_TILE - 1) / BW_TILE;
    constexpr int VEC = Elem<T>::VEC;
    const int vec_x = Min % VEC == 0 && ((uintptr_t)x & 15) == 0, vec_g = Mout % VEC == 0 && ((uintptr_t)g & 15) == 0;
    if (P > 0) {
        hipLaunchKernelGGL((bw_weight_kernel<T>), dim3((unsigned)(nchunks * tiles_i * tiles_o)), dim3(256), 0, stream, (const T*)g,
                           (const T*)x, (const T*)basis, rowptr, perm, x_rows, g_rows, (T*)grad_weight, partial, P, (int)K, Min, Mout, S,
                           chunk_len, tiles_i, tiles_o, vec_x, vec_g);
        const int rc = gnnops_check_launch("spline_weighting_bw_weight");
        if (rc != GNNOPS_OK) return rc;
    }
    const int64_t MM = (int64_t)Min * Mout;
    hipLaunchKernelGGL((bw_weight_finish_kernel<T>), dim3(gnnops_grid_cap(gnnops_cdiv(K * MM, 256))), dim3(256), 0, stream,
                       P > 0 ? rowptr : nullptr, partial, (T*)grad_weight, K, MM, chunk_len);
    return gnnops_check_launch("spline_weighting_bw_weight (finish)");
}

}  // namespace

extern "C" int gnnops_spline_basis_bw(const void* grad_basis, const void* pseudo, const int64_t* kernel_size,
                                      const uint8_t* is_open_spline, int64_t E, int D, int degree, void* grad_pseudo, int dtype,
                                      gnnops_stream_t s) {
    SplineMeta sm{};
    const int rc = fill_meta(sm, kernel_size, is_open_spline, D, degree, "spline_basis_bw");
    if (rc != GNNOPS_OK) return rc;
    GNNOPS_REQUIRE(E >= 0, GNNOPS_EINVAL, "spline_basis_bw: negative size");
    if (E == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(grad_basis && pseudo && grad_pseudo, GNNOPS_EINVAL, "spline_basis_bw: null pointer");
    return gnnops_with_dtype(dtype, "spline_basis_bw", [&](auto t) {
        return run_basis_bw<typename decltype(t)::type>(grad_basis, pseudo, sm, E, grad_pseudo, (hipStream_t)s);
    });
}

extern "C" int gnnops_spline_weighting_bw_basis(const void* grad_out, const void* x, const void* weight, const int64_t* weight_index,
                                                const int64_t* x_rows, const int64_t* g_rows, void* grad_basis, int64_t E, int64_t Min,
                                                int64_t Mout, int64_t S, int dtype, gnnops_stream_t s) {
    GNNOPS_REQUIRE(E >= 0 && Min >= 0 && Mout >= 0 && S >= 0, GNNOPS_EINVAL, "spline_weighting_bw_basis: negative size");
    GNNOPS_REQUIRE(Min < (1 << 20) && Mout < (1 << 20) && S <= MAX_S, GNNOPS_EUNSUPPORTED, "spline_weighting_bw_basis: shape out of range");
    if (E * S == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(grad_basis && weight_index && (Min * Mout == 0 || (grad_out && x && weight)), GNNOPS_EINVAL,
                   "spline_weighting_bw_basis: null pointer");
    const int grid = gnnops_grid_cap(gnnops_cdiv(E, 4), 256 * 32);
    hipStream_t stream = (hipStream_t)s;
    return gnnops_with_dtype(dtype, "spline_weighting_bw_basis", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((bw_basis_kernel<T>), dim3(grid), dim3(256), 0, stream, (const T*)grad_out, (const T*)x, (const T*)weight,
                           weight_index, x_rows, g_rows, (T*)grad_basis, E, (int)Min, (int)Mout, (int)S);
        return gnnops_check_launch("spline_weighting_bw_basis");
    });
}

extern "C" size_t gnnops_spline_weighting_bw_weight_workspace_bytes(int64_t E, int64_t S, int64_t Min, int64_t Mout) {
    const int64_t P = E * S;
    if (P <= 0 || Min <= 0 || Mout <= 0) return 0;
    return (size_t)(gnnops_cdiv(P, bw_chunk_len(P)) * 2 * Min * Mout) * sizeof(float);
}

extern "C" int gnnops_spline_weighting_bw_weight(const void* grad_out, const void* x, const void* basis, const int32_t* rowptr,
                                                 const int32_t* perm, const int64_t* x_rows, const int64_t* g_rows, void* grad_weight,
                                                 int64_t E, int64_t K, int64_t Min, int64_t Mout, int64_t S, int dtype, void* workspace,
                                                 size_t workspace_bytes, gnnops_stream_t s) {
    GNNOPS_REQUIRE(E >= 0 && K >= 0 && Min >= 0 && Mout >= 0 && S >= 0, GNNOPS_EINVAL, "spline_weighting_bw_weight: negative size");
    GNNOPS_REQUIRE(Min < (1 << 20) && Mout < (1 << 20) && S <= MAX_S && K < ((int64_t)1 << 31) && E * S < ((int64_t)1 << 31),
                   GNNOPS_EUNSUPPORTED, "spline_weighting_bw_weight: shape out of range (E * S and K must stay below 2^31)");
    if (K * Min * Mout == 0) return GNNOPS_OK;
    const int64_t P = E * S;
    GNNOPS_REQUIRE(grad_weight && (P == 0 || (grad_out && x && basis && rowptr && perm)), GNNOPS_EINVAL,
                   "spline_weighting_bw_weight: null pointer");
    GNNOPS_REQUIRE(workspace_bytes >= gnnops_spline_weighting_bw_weight_workspace_bytes(E, S, Min, Mout) && (P == 0 || workspace),
                   GNNOPS_EWORKSPACE, "spline_weighting_bw_weight: workspace too small");
    GNNOPS_REQUIRE(((uintptr_t)workspace & 3) == 0, GNNOPS_EINVAL, "spline_weighting_bw_weight: workspace must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)s;
    float* partial = (float*)workspace;
    return gnnops_with_dtype(dtype, "spline_weighting_bw_weight", [&](auto t) {
        return run_bw_weight<typename decltype(t)::type>(grad_out, x, basis, rowptr, perm, x_rows, g_rows, grad_weight, P, K, (int)Min, (int)Mout,
                                                         (int)S, partial, stream);
    });
}
