// spmm_reduce.hip — sparse (CSR / plan-ordered COO) x dense with a mean, min or max over each row's nonzeros:
// torch_sparse.matmul(SparseTensor, dense, reduce=...) = spmm_mean / spmm_min / spmm_max of torch-sparse 0.6.12
// (reference pin: requirements.txt:213; the op list names torch_sparse.scatter_max / scatter_min / scatter_mean).
//
//   min / max  out[i, k] = max over the nonzeros e of row i of value[e] * mat[col[e], k]
//              arg[i, k] = the winner's position j in the ROW-ORDERED storage, rowptr[i] <= j < rowptr[i+1] (never perm[j])
//   mean       out[i, k] = (sum over e, in order, of value[e] * mat[col[e], k]) / max(rowptr[i+1] - rowptr[i], 1)
//              — torch_sparse's rule: the divisor is the number of nonzeros, not the sum of the weights.
//
// The grid, the lane groups and the three-phase fetch of U = 8 nonzeros are those of spmm_rows_kernel (spmm.hip): one lane
// group per (row, 1-KiB column chunk), 16-byte lane loads; rows of `mat` that are no multiple of 16 bytes (or misaligned
// operands) take one thread per output element. No atomics, no cross-lane step: two runs give the same bits.
//
// Arithmetic. Every product is one __fmul_rn in fp32 (exact for 16-bit inputs), never contracted. min / max compare the fp32
// products with a strict < / >, so among equal products the smallest position wins (torch_sparse's CPU kernel; its CUDA kernel
// leaves ties to a race), and round the winner once to the storage type. mean adds in the order and arithmetic of
// spmm_rows_kernel, divides in fp32 and rounds once. A row without nonzeros gives out = 0 and arg = nnz.
// NaN: a NaN product loses every comparison, so it is passed over — unless it belongs to the row's first nonzero, which is
// taken unconditionally and then never beaten (no product compares better than NaN). Not pinned by the tests.
//
// A row of more than hub::T_HUB (8192) nonzeros is walked by its one lane group like any other: correct, and slow (a
// piecewise hub pass as in spmm.hip would need a second compare over the pieces; not built).
//
// gnnops_spmm_reduce_grad_terms is the per-output-element half of the min / max backward: the three tensors that the two
// deterministic scatter-adds of gnnops/autograd.py (_SpMMReduce) then sum by destination.
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int U = 8;

template <int R>
__device__ inline bool takes(float p, float best, bool first) {
    if constexpr (R == GNNOPS_MAX) return first || p > best;
    else return first || p < best;
}

template <int N>
__device__ inline void store_args(int64_t* dst, const int32_t* a) {   // dst 16-byte aligned, N even
#pragma unroll
    for (int v = 0; v < N; v += 2) {
        u32x4 w;
        w.x = (uint32_t)a[v]; w.y = 0u; w.z = (uint32_t)a[v + 1]; w.w = 0u;   // positions are < 2^31: the high words are 0
        store16<true>(dst + v, w);
    }
}

template <typename T, int R, bool NT>
__global__ __launch_bounds__(256) void spmm_reduce_rows_kernel(const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ perm,
                                                               const int64_t* __restrict__ col, const T* __restrict__ value,
                                                               const T* __restrict__ mat, T* __restrict__ out,
                                                               int64_t* __restrict__ arg, int64_t M, int64_t D, int32_t nnz,
                                                               int gshift, int kchunks) {
    constexpr int VEC = Elem<T>::VEC;
    constexpr bool MEAN = R == GNNOPS_MEAN;
    const int G = 1 << gshift;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) >> gshift;
    const int gl = (int)(gtid & (G - 1));
    const int64_t items = (int64_t)kchunks * M;
    for (int64_t item = gtid >> gshift; item < items; item += ngroups) {
        const int64_t i = item % M;
        const int chunk = (int)(item / M);
        const int64_t c0 = ((int64_t)chunk * G + gl) * VEC;
        if (c0 >= D) continue;
        const int32_t beg = rowptr[i], end = rowptr[i + 1];
        float acc[VEC];
        int32_t at[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            acc[v] = 0.f;
            at[v] = nnz;
        }
        for (int32_t j = beg; j < end; j += U) {
            int64_t c[U];
            T wraw[U];
            u32x4 rows[U];
            int32_t e[U];
            // the three phases of spmm_rows_kernel, each with all its loads in flight together
#pragma unroll
            for (int u = 0; u < U; ++u) e[u] = (j + u < end) ? (perm ? perm[j + u] : j + u) : -1;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                c[u] = -1;
                if (e[u] >= 0) {
                    c[u] = col[e[u]];
                    if (value) wraw[u] = value[e[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (c[u] >= 0) rows[u] = load16<NT>(mat + c[u] * D + c0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (c[u] >= 0) {
                    float f[VEC];
                    Elem<T>::unpack(rows[u], f);
                    const float w = value ? Elem<T>::load(&wraw[u]) : 1.f;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float p = __fmul_rn(w, f[v]);
                        if constexpr (MEAN) {
                            acc[v] = __fadd_rn(acc[v], p);
                        } else if (takes<R>(p, acc[v], at[v] == nnz)) {   // at == nnz: nothing taken yet (j + u < nnz always)
                            acc[v] = p;
                            at[v] = j + u;
                        }
                    }
                }
            }
        }
        if constexpr (MEAN) {
            const float cnt = (float)(end - beg < 1 ? 1 : end - beg);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = __fdiv_rn(acc[v], cnt);
        }
        store16<true>(out + i * D + c0, Elem<T>::pack(acc));
        if constexpr (!MEAN) {
            if (arg) store_args<VEC>(arg + i * D + c0, at);
        }
    }
}

template <typename T, int R>
__global__ __launch_bounds__(256) void spmm_reduce_elems_kernel(const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ perm,
                                                                const int64_t* __restrict__ col, const T* __restrict__ value,
                                                                const T* __restrict__ mat, T* __restrict__ out,
                                                                int64_t* __restrict__ arg, int64_t M, int64_t D, int32_t nnz) {
    constexpr bool MEAN = R == GNNOPS_MEAN;
    const int64_t total = M * D;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = o / D, k = o % D;
        const int32_t beg = rowptr[i], end = rowptr[i + 1];
        float acc = 0.f;
        int32_t at = nnz;
        for (int32_t j = beg; j < end; ++j) {
            const int32_t e = perm ? perm[j] : j;
            const float w = value ? Elem<T>::load(value + e) : 1.f;
            const float p = __fmul_rn(w, Elem<T>::load(mat + col[e] * D + k));
            if constexpr (MEAN) {
                acc = __fadd_rn(acc, p);
            } else if (takes<R>(p, acc, j == beg)) {
                acc = p;
                at = j;
            }
        }
        if constexpr (MEAN) acc = __fdiv_rn(acc, (float)(end - beg < 1 ? 1 : end - beg));
        Elem<T>::store(out + o, acc);
        if constexpr (!MEAN) {
            if (arg) arg[o] = at;
        }
    }
}

template <typename T, int R>
int launch_reduce(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value, const void* mat, void* out,
                  int64_t* arg, int64_t M, int64_t D, int64_t nnz, int64_t mat_rows, hipStream_t stream) {
    constexpr int VEC = Elem<T>::VEC;
    if (D % VEC == 0 && (uintptr_t)mat % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)arg % 16 == 0) {
        const int64_t vecs = D / VEC;
        const int gshift = gnnops_group_shift(vecs);
        const int kchunks = (int)gnnops_cdiv(vecs, (int64_t)1 << gshift);
        const int grid = gnnops_grid_cap(gnnops_cdiv((int64_t)kchunks * M, 256 >> gshift), 256 * 64);
        // as in spmm.hip: a dense operand far beyond the Infinity Cache is streamed nontemporally
        const bool nt = (size_t)mat_rows * (size_t)D * sizeof(T) > ((size_t)2 << 30);
        if (nt)
            hipLaunchKernelGGL((spmm_reduce_rows_kernel<T, R, true>), dim3(grid), dim3(256), 0, stream, rowptr, perm, col,
                               (const T*)value, (const T*)mat, (T*)out, arg, M, D, (int32_t)nnz, gshift, kchunks);
        else
            hipLaunchKernelGGL((spmm_reduce_rows_kernel<T, R, false>), dim3(grid), dim3(256), 0, stream, rowptr, perm, col,
                               (const T*)value, (const T*)mat, (T*)out, arg, M, D, (int32_t)nnz, gshift, kchunks);
    } else {
        const int grid = gnnops_grid_cap(gnnops_cdiv(M * D, 256), 256 * 32);
        hipLaunchKernelGGL((spmm_reduce_elems_kernel<T, R>), dim3(grid), dim3(256), 0, stream, rowptr, perm, col, (const T*)value,
                           (const T*)mat, (T*)out, arg, M, D, (int32_t)nnz);
    }
    return gnnops_check_launch("spmm_reduce");
}

template <typename T>
int launch_dtype(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value, const void* mat, void* out,
                 int64_t* arg, int64_t M, int64_t D, int64_t nnz, int64_t mat_rows, int reduce, hipStream_t stream) {
    switch (reduce) {
        case GNNOPS_MEAN: return launch_reduce<T, GNNOPS_MEAN>(rowptr, perm, col, value, mat, out, nullptr, M, D, nnz, mat_rows, stream);
        case GNNOPS_MIN: return launch_reduce<T, GNNOPS_MIN>(rowptr, perm, col, value, mat, out, arg, M, D, nnz, mat_rows, stream);
        case GNNOPS_MAX: return launch_reduce<T, GNNOPS_MAX>(rowptr, perm, col, value, mat, out, arg, M, D, nnz, mat_rows, stream);
    }
    gnnops_set_error("spmm_reduce: reduce %d is not mean / min / max (the sum is gnnops_spmm)", reduce);
    return GNNOPS_EINVAL;
}

// One thread per output element (i, k) of a min / max product. With a = arg[i, k] < nnz, e = perm ? perm[a] : a:
//   dst[i, k]    = col[e]                      the row of d mat that receives the element's gradient   (mat_rows if a == nnz)
//   to_mat[i, k] = round(value[e] * g[i, k])   what it receives                                        (0 if a == nnz)
//   to_val[i, k] = round(mat[col[e], k] * g[i, k])   the element's term of d value[a]                  (0 if a == nnz)
// Products in fp32, one rounding. Coalesced in arg / g / the outputs; the reads of col, value and mat follow the winners.
template <typename T>
__global__ __launch_bounds__(256) void spmm_reduce_grad_terms_kernel(const int64_t* __restrict__ arg, const T* __restrict__ g,
                                                                     const int32_t* __restrict__ perm,
                                                                     const int64_t* __restrict__ col, const T* __restrict__ value,
                                                                     const T* __restrict__ mat, int64_t* __restrict__ dst,
                                                                     T* __restrict__ to_mat, T* __restrict__ to_val, int64_t M,
                                                                     int64_t D, int64_t nnz, int64_t mat_rows) {
    const int64_t total = M * D;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = arg[o];
        int64_t c = mat_rows;
        float tm = 0.f, tv = 0.f;
        if (a >= 0 && a < nnz) {
            const int64_t e = perm ? perm[a] : a;
            const int64_t ce = col[e];
            if (ce >= 0 && ce < mat_rows) {
                c = ce;
                const float gv = Elem<T>::load(g + o);
                tm = __fmul_rn(value ? Elem<T>::load(value + e) : 1.f, gv);
                if (to_val) tv = __fmul_rn(Elem<T>::load(mat + ce * D + o % D), gv);
            }
        }
        dst[o] = c;
        Elem<T>::store(to_mat + o, tm);
        if (to_val) Elem<T>::store(to_val + o, tv);
    }
}

template <typename T>
int launch_grad_terms(const int64_t* arg, const void* g, const int32_t* perm, const int64_t* col, const void* value,
                      const void* mat, int64_t* dst, void* to_mat, void* to_val, int64_t M, int64_t D, int64_t nnz,
                      int64_t mat_rows, hipStream_t stream) {
    const int grid = gnnops_grid_cap(gnnops_cdiv(M * D, 256), 256 * 32);
    hipLaunchKernelGGL((spmm_reduce_grad_terms_kernel<T>), dim3(grid), dim3(256), 0, stream, arg, (const T*)g, perm, col,
                       (const T*)value, (const T*)mat, dst, (T*)to_mat, (T*)to_val, M, D, nnz, mat_rows);
    return gnnops_check_launch("spmm_reduce_grad_terms");
}

}  // namespace

extern "C" int gnnops_spmm_reduce(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value,
                                  const void* mat, void* out, int64_t* arg, int64_t M, int64_t D, int64_t nnz, int64_t mat_rows,
                                  int reduce, int dtype, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(M >= 0 && D >= 0 && nnz >= 0, GNNOPS_EINVAL, "spmm_reduce: negative size");
    GNNOPS_REQUIRE(nnz < ((int64_t)1 << 31) - U, GNNOPS_EUNSUPPORTED, "spmm_reduce: nnz must be < 2^31 - 8");
    if (M * D == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(rowptr && out && (nnz == 0 || (col && mat)), GNNOPS_EINVAL, "spmm_reduce: null pointer");
    return gnnops_with_dtype(dtype, "spmm_reduce", [&](auto t) {
        return launch_dtype<typename decltype(t)::type>(rowptr, perm, col, value, mat, out, arg, M, D, nnz, mat_rows, reduce, stream);
    });
}

extern "C" int gnnops_spmm_reduce_grad_terms(const int64_t* arg, const void* g, const int32_t* perm, const int64_t* col,
                                             const void* value, const void* mat, int64_t* dst, void* to_mat, void* to_val,
                                             int64_t M, int64_t D, int64_t nnz, int64_t mat_rows, int dtype, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(M >= 0 && D >= 0 && nnz >= 0 && mat_rows >= 0, GNNOPS_EINVAL, "spmm_reduce_grad_terms: negative size");
    if (M * D == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(arg && g && dst && to_mat && (nnz == 0 || (col && mat)), GNNOPS_EINVAL, "spmm_reduce_grad_terms: null pointer");
    return gnnops_with_dtype(dtype, "spmm_reduce_grad_terms", [&](auto t) {
        return launch_grad_terms<typename decltype(t)::type>(arg, g, perm, col, value, mat, dst, to_mat, to_val, M, D, nnz, mat_rows, stream);
    });
}
