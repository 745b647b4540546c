// gcn.hip — GCNConv's edge pass: symmetric normalisation with edge weights and self loops (Kipf & Welling 2017;
// torch_geometric's gcn_norm + add_remaining_self_loops + propagate), over the destination plan gnnops_edge_reduce takes.
//
//   lw[i]  = weight of the LAST self loop of i in edge order, fill_value if it has none
//   deg[i] = lw[i] + sum of w_e over the other edges into i          dis[i] = deg[i] > 0 ? rsqrt(deg[i]) : 0
//   out[i] = dis[i] * ( sum over the non-loop edges (j -> i) of w_e * dis[j] * h[j]  +  lw[i] * dis[i] * h[i] )  (+ bias)
//
// The edge list is never rewritten: a self loop is recognised where it is met (col == row) and replaced by the node's lw, so
// nothing is removed, nothing appended and the host reads nothing back. dis and lw are operands of the propagate kernel: the
// operator is symmetric, so the backward is the same kernel over the plan of the source ids with the forward's dis / lw.
//
// Lanes: a destination row belongs to a group of LPR x SLOTS lanes — LPR lanes across the row's K columns (16 B each where the
// operands allow it, one element otherwise), SLOTS edge slots that walk the row's edges side by side (fp32 accumulators,
// combined by a fixed xor tree: the same bits every run). No atomics. A destination of any in-degree is handled by the same
// loop: its group just runs longer ("GraphUNet", says what that costs).
#include "common.h"
#include "dispatch.h"

namespace {

__device__ inline int64_t cdiv_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- degree ----
constexpr int DEG_LANES = 8;   // lanes per destination

__global__ __launch_bounds__(256) void gcn_degree_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
                                                          const int64_t* __restrict__ col, const float* __restrict__ w, int64_t N,
                                                          float fill_value, float* __restrict__ dis, float* __restrict__ lw) {
    const int sub = threadIdx.x % DEG_LANES;
    const int64_t groups = (int64_t)gridDim.x * (256 / DEG_LANES);
    const int64_t rounds = cdiv_dev(N, groups);
    for (int64_t it = 0; it < rounds; ++it) {   // every lane runs every round: the shuffles below need their whole group
        const int64_t i = it * groups + (int64_t)blockIdx.x * (256 / DEG_LANES) + threadIdx.x / DEG_LANES;
        float sum = 0.f, loop_w = 0.f;
        int32_t loop_id = -1;   // original edge id of the last self loop this lane met
        if (i < N) {
            for (int32_t e = rowptr[i] + sub; e < rowptr[i + 1]; e += DEG_LANES) {
                const int32_t id = perm ? perm[e] : e;
                const float we = w ? w[id] : 1.f;
                if (col[e] == i) {
                    if (id > loop_id) { loop_id = id; loop_w = we; }
                } else {
                    sum += we;
                }
            }
        }
#pragma unroll
        for (int o = DEG_LANES / 2; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o);
            const int32_t other_id = __shfl_xor(loop_id, o);
            const float other_w = __shfl_xor(loop_w, o);
            if (other_id > loop_id) { loop_id = other_id; loop_w = other_w; }
        }
        if (i < N && sub == 0) {
            const float l = loop_id >= 0 ? loop_w : fill_value;
            const float deg = l + sum;
            lw[i] = l;
            dis[i] = deg > 0.f ? 1.f / sqrtf(deg) : 0.f;
        }
    }
}

// ---- propagate ----
struct Args {
    const void *h, *bias;
    void* out;
    const int32_t *rowptr, *perm;
    const int64_t* col;
    const float *w, *dis, *lw;
    int64_t N, K, ldh, ldo;
    int lpr_shift, slot_shift;   // LPR = 1 << lpr_shift lanes across a row, SLOTS = 1 << slot_shift edge slots
};

template <typename T, int VEC>
__device__ inline void load_row(const T* p, float* f) {
    if constexpr (VEC == 1) {
        f[0] = Elem<T>::load(p);
    } else {
        Elem<T>::unpack(load16<false>(p), f);
    }
}
template <typename T, int VEC>
__device__ inline void store_row(T* p, const float* f) {
    if constexpr (VEC == 1) {
        Elem<T>::store(p, f[0]);
    } else {
        store16<false>(p, Elem<T>::pack(f));
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void gcn_propagate_kernel(const Args a) {
    const T* __restrict__ h = (const T*)a.h;
    const T* __restrict__ bias = (const T*)a.bias;
    T* __restrict__ out = (T*)a.out;
    const int lpr = 1 << a.lpr_shift, slots = 1 << a.slot_shift;
    const int gshift = a.lpr_shift + a.slot_shift;         // lanes per destination, a power of two <= 64
    const int in_group = threadIdx.x & ((1 << gshift) - 1);
    const int kl = in_group & (lpr - 1), slot = in_group >> a.lpr_shift;
    const int64_t per_block = 256 >> gshift;
    const int64_t groups = (int64_t)gridDim.x * per_block;
    const int64_t rounds = cdiv_dev(a.N, groups);
    const int64_t kstep = (int64_t)lpr * VEC;
    for (int64_t it = 0; it < rounds; ++it) {   // every lane runs every round (shuffles)
        const int64_t i = it * groups + (int64_t)blockIdx.x * per_block + (threadIdx.x >> gshift);
        const bool row_ok = i < a.N;
        const int32_t e0 = row_ok ? a.rowptr[i] : 0, e1 = row_ok ? a.rowptr[i + 1] : 0;
        const float dis_i = row_ok ? a.dis[i] : 0.f;
        const float self = row_ok ? a.lw[i] * dis_i : 0.f;
        for (int64_t k0 = 0; k0 < a.K; k0 += kstep) {   // uniform trip count; one trip unless the row is wider than the wave
            const int64_t k = k0 + (int64_t)kl * VEC;
            const bool col_ok = k < a.K;
            float acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
            if (col_ok) {
                for (int32_t e = e0 + slot; e < e1; e += slots) {
                    const int64_t j = a.col[e];
                    if (j == i) continue;   // self loops enter through lw
                    const float we = a.w ? a.w[a.perm ? a.perm[e] : e] : 1.f;
                    const float c = we * a.dis[j];
                    float f[VEC];
                    load_row<T, VEC>(h + j * a.ldh + k, f);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] += c * f[v];
                }
            }
            for (int o = lpr; o < (1 << gshift); o <<= 1) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], o);
            }
            if (row_ok && col_ok && slot == 0) {
                float f[VEC], b[VEC];
                load_row<T, VEC>(h + i * a.ldh + k, f);
#pragma unroll
                for (int v = 0; v < VEC; ++v) b[v] = 0.f;
                if (bias) load_row<T, VEC>(bias + k, b);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = dis_i * (acc[v] + self * f[v]) + b[v];
                store_row<T, VEC>(out + i * a.ldo + k, acc);
            }
        }
    }
}

template <typename T>
int launch(Args a, hipStream_t stream) {
    constexpr int V = Elem<T>::VEC;
    const uintptr_t addr = (uintptr_t)a.h | (uintptr_t)a.out | (uintptr_t)a.bias;
    const bool wide = a.K % V == 0 && a.ldh % V == 0 && a.ldo % V == 0 && addr % 16 == 0;
    const int64_t lanes = wide ? a.K / V : a.K;
    a.lpr_shift = 0;
    while ((1 << a.lpr_shift) < lanes && a.lpr_shift < 6) ++a.lpr_shift;
    a.slot_shift = 6 - a.lpr_shift < 2 ? 6 - a.lpr_shift : 2;   // up to four edges of a row in flight per step
    const int64_t per_block = 256 >> (a.lpr_shift + a.slot_shift);
    const dim3 grid(gnnops_grid_cap(gnnops_cdiv(a.N, per_block), 256 * 32));
    if (wide) hipLaunchKernelGGL((gcn_propagate_kernel<T, V>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((gcn_propagate_kernel<T, 1>), grid, dim3(256), 0, stream, a);
    return gnnops_check_launch("gcn_propagate");
}

}  // namespace

extern "C" int gnnops_gcn_degree(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const float* w, int64_t N, int64_t E,
                                 float fill_value, float* dis, float* lw, gnnops_stream_t s) {
    GNNOPS_REQUIRE(N >= 0 && E >= 0 && N < ((int64_t)1 << 31) && E < ((int64_t)1 << 31), GNNOPS_EINVAL,
                   "gcn_degree: N = %lld, E = %lld (both below 2^31)", (long long)N, (long long)E);
    if (N == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(rowptr && dis && lw && (col || E == 0), GNNOPS_EINVAL, "gcn_degree: null pointer");
    hipLaunchKernelGGL(gcn_degree_kernel, dim3(gnnops_grid_cap(gnnops_cdiv(N, 256 / DEG_LANES), 256 * 32)), dim3(256), 0, (hipStream_t)s,
                       rowptr, perm, col, w, N, fill_value, dis, lw);
    return gnnops_check_launch("gcn_degree");
}

extern "C" int gnnops_gcn_propagate(const void* h, int64_t ldh, const int32_t* rowptr, const int32_t* perm, const int64_t* col,
                                    const float* w, const float* dis, const float* lw, const void* bias, void* out, int64_t ldo,
                                    int64_t N, int64_t E, int64_t K, int dtype, gnnops_stream_t s) {
    GNNOPS_REQUIRE(N >= 0 && E >= 0 && K >= 0 && N < ((int64_t)1 << 31) && E < ((int64_t)1 << 31), GNNOPS_EINVAL,
                   "gcn_propagate: N = %lld, E = %lld, K = %lld (N, E below 2^31)", (long long)N, (long long)E, (long long)K);
    GNNOPS_REQUIRE(dtype >= GNNOPS_F32 && dtype <= GNNOPS_BF16, GNNOPS_EUNSUPPORTED, "gcn_propagate: dtype code %d", dtype);
    if (N == 0 || K == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(h && out && rowptr && dis && lw && (col || E == 0), GNNOPS_EINVAL, "gcn_propagate: null pointer");
    GNNOPS_REQUIRE((ldh >= K || ldh == 0) && ldo >= K, GNNOPS_EINVAL, "gcn_propagate: pitches %lld, %lld below K = %lld", (long long)ldh, (long long)ldo,
                   (long long)K);
    Args a;
    a.h = h; a.bias = bias; a.out = out; a.rowptr = rowptr; a.perm = perm; a.col = col; a.w = w; a.dis = dis; a.lw = lw;
    a.N = N; a.K = K; a.ldh = ldh; a.ldo = ldo; a.lpr_shift = a.slot_shift = 0;
    hipStream_t stream = (hipStream_t)s;
    return gnnops_with_dtype(dtype, "gcn_propagate", [&](auto t) { return launch<typename decltype(t)::type>(a, stream); });
}
