// spmm.hip — sparse (CSR / plan-ordered COO) x dense: torch_sparse.spmm(index, value, m, n, matrix) and
// torch.sparse.mm(COO, dense) (reference: op_bm_scripts/benchmark_sparse_spmm.py:12-14; BASELINE
// config 3: CSR 2M x 2M, nnz 40M, D=256 bf16).
//
// out[i, :] = sum over the nonzeros e of row i, in order, of value[e] * mat[col[e], :]
// (torch_sparse: scatter_add(matrix.index_select(-2, col) * value.unsqueeze(-1), row, dim=-2)).
//
// Row-split: one lane group per output row (and 1-KiB column chunk), 8 gathered rows of `mat` in flight,
// fp32 accumulation, one rounding on store. HBM/Infinity-Cache bound (2*nnz*D flops on ~nnz*D*s gathered
// bytes: arithmetic intensity ~1 flop/B against a ridge of ~300), so this is VALU FMA work on 16-B lane
// loads, not an MFMA tile: no two sparse rows share a dense operand tile at 20 nnz/row.
//
// Arithmetic (matches the oracle bit for bit): fp32 inputs: p = round(v*x), acc = round(acc+p) — the two
// roundings torch's `matrix[col] * value` followed by scatter_add perform; no FMA contraction.
// 16-bit inputs: v*x is exact in fp32, acc in fp32, rounded once to the storage type.
#include "common.h"
#include "dispatch.h"
#include "hub.h"

namespace {

constexpr int U = 8;

template <typename T, bool NT>
__global__ __launch_bounds__(256) void spmm_rows_kernel(const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ perm,
                                                        const int64_t* __restrict__ col, const T* __restrict__ value,
                                                        const T* __restrict__ mat, T* __restrict__ out, int64_t M,
                                                        int64_t D, int gshift, int kchunks, hub::Ws hw, int hub_on) {
    constexpr int VEC = Elem<T>::VEC;
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
        if (hub_on && end - beg > hub::T_HUB) {  // a hub row (hub.h): multiplied out piecewise by the hub pass
            if (gl == 0 && chunk == 0) hub::append(hw, (int)i, beg, end, end - beg);
            continue;
        }
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int32_t j = beg; j < end; j += U) {
            int64_t c[U];
            T wraw[U];      // the value as STORED: converting it where it is loaded would put a wait for the load right there, and
            u32x4 rows[U];  // the U (column id, value) pairs of a step would be fetched one memory latency after the other
            // three phases, each with all its loads in flight together: positions (plan order only), then (column id, value)
            // pairs, then the gathered rows. Interleaved per nonzero, every position -> column -> row chain waited on its own.
            int32_t e[U];
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
                    for (int v = 0; v < VEC; ++v) acc[v] = __fadd_rn(acc[v], __fmul_rn(w, f[v]));
                }
            }
        }
        store16<true>(out + i * D + c0, Elem<T>::pack(acc));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void spmm_elems_kernel(const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ perm,
                                                         const int64_t* __restrict__ col, const T* __restrict__ value,
                                                         const T* __restrict__ mat, T* __restrict__ out, int64_t M,
                                                         int64_t D) {
    const int64_t total = M * D;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = o / D, k = o % D;
        float acc = 0.f;
        for (int32_t j = rowptr[i]; j < rowptr[i + 1]; ++j) {
            const int32_t e = perm ? perm[j] : j;
            const float w = value ? Elem<T>::load(value + e) : 1.f;
            acc = __fadd_rn(acc, __fmul_rn(w, Elem<T>::load(mat + col[e] * D + k)));
        }
        Elem<T>::store(out + o, acc);
    }
}

// Wide dense operands whose rows are not 16-B multiples (the reference's (L, L) fp32 shapes, L = 7071): a workgroup takes
// (output row i, a run of 256 * UC columns); the row's column ids and values are the same for every lane (scalar loads),
// each lane keeps UC accumulators and sweeps the nonzeros two at a time, so 2 * UC coalesced element loads are in flight.
// Same arithmetic and order as the row kernel; no per-element division (spmm_elems_kernel pays one per output element).
template <typename T>
__global__ __launch_bounds__(256) void spmm_widerows_kernel(const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ perm,
                                                            const int64_t* __restrict__ col, const T* __restrict__ value,
                                                            const T* __restrict__ mat, T* __restrict__ out, int64_t M,
                                                            int64_t D, int chunks) {
    constexpr int UC = 4;
    const int64_t items = M * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t i = item / chunks;
        const int64_t c0 = (item - i * chunks) * (256 * UC) + threadIdx.x;
        const int32_t beg = rowptr[i], end = rowptr[i + 1];
        float acc[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u) acc[u] = 0.f;
        for (int32_t j = beg; j < end; j += 2) {
            const bool two = j + 1 < end;
            const int32_t e0 = perm ? perm[j] : j, e1 = two ? (perm ? perm[j + 1] : j + 1) : e0;
            const int64_t r0 = col[e0], r1 = col[e1];
            const float w0 = value ? Elem<T>::load(value + e0) : 1.f;
            const float w1 = two ? (value ? Elem<T>::load(value + e1) : 1.f) : 0.f;
            float x0[UC], x1[UC];
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                const int64_t k = c0 + 256 * u;
                const int64_t kc = k < D ? k : D - 1;
                x0[u] = Elem<T>::load(mat + r0 * D + kc);
                x1[u] = Elem<T>::load(mat + r1 * D + kc);
            }
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                acc[u] = __fadd_rn(acc[u], __fmul_rn(w0, x0[u]));
                if (two) acc[u] = __fadd_rn(acc[u], __fmul_rn(w1, x1[u]));
            }
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const int64_t k = c0 + 256 * u;
            if (k < D) Elem<T>::store(out + i * D + k, acc[u]);
        }
    }
}

// ---- tiled form: the rows of `mat` that a block of consecutive output rows shares are staged in LDS once ----
// A plan (include/gnnops.h, "Tiled SpMM plan"; built by gnnops.spmm_tiles) names, per block of R = 1 << rshift output rows,
// up to `slots` columns that at least two nonzeros of the block reference, and gives every nonzero its column's slot or
// 0xFFFF. A workgroup takes (row block, 128-byte column chunk): it copies the chunk of each staged row of `mat` into its
// LDS slot (16-byte loads, all of a thread's in flight together, then 16-byte LDS stores), and after one barrier runs the
// row loop of spmm_rows_kernel with 8 lanes per row: an operand row comes from LDS when the nonzero has a slot and from
// global memory otherwise. Products, their order and the single rounding are those of spmm_rows_kernel, so the bits are too.
//
// LDS image: slot s at byte 128 * s, lane gl's 16 bytes at 16 * gl — lane-linear, what the staging loop writes. A
// ds_read_b128 is served in 16-lane groups that take lanes 0-3 of two rows and lanes 4-7 of two others: two slots of equal
// parity sit on the same half of the 256-byte bank row, so such a pair reads 2-way. The slots are the data's, no swizzle of
// the image removes that; a 256-byte pitch would (one slot = one bank row) at half the staged columns per workgroup.
constexpr int TILE_THREADS = 1024;  // 16 waves on the CU beside up to 160 KiB of LDS: one workgroup per CU hides its own latency
constexpr int TILE_LANES = 8;       // lanes per row = 16-byte pieces per 128-byte chunk
constexpr int TILE_STAGE = 8;       // staging loads in flight per thread: 1024 slots x 8 pieces in one sweep
constexpr int TILE_SLOT_BYTES = TILE_LANES * 16;
constexpr int TILE_LDS_BYTES = 160 * 1024;
constexpr int TILE_NONE = 0xFFFF;

template <typename T>
__global__ __launch_bounds__(TILE_THREADS) void spmm_tiled_kernel(const int32_t* __restrict__ rowptr,
                                                                  const int64_t* __restrict__ col,
                                                                  const uint16_t* __restrict__ slot,
                                                                  const T* __restrict__ value, const T* __restrict__ mat,
                                                                  T* __restrict__ out, const int32_t* __restrict__ tile_ptr,
                                                                  const int64_t* __restrict__ tile_cols, int64_t M, int64_t D,
                                                                  int rshift, int kchunks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tile_raw[];
    u32x4* tile = reinterpret_cast<u32x4*>(tile_raw);  // [slot][TILE_LANES]
    constexpr int VEC = Elem<T>::VEC;
    // neighbouring row blocks stage overlapping columns: keep them on one XCD's L2; the chunks of one block share its CSR arrays
    const int64_t item = xcd_contiguous(blockIdx.x, gridDim.x);
    const int64_t b = item / kchunks;
    const int chunk = (int)(item - b * kchunks);
    const int tid = threadIdx.x;
    const int gl = tid & (TILE_LANES - 1);
    const int64_t c0 = ((int64_t)chunk * TILE_LANES + gl) * VEC;
    const bool live = c0 < D;  // ragged last chunk: lanes past the row neither stage nor compute
    const int32_t t0 = tile_ptr[b];
    const int pieces = (tile_ptr[b + 1] - t0) * TILE_LANES;
    for (int base = 0; base < pieces; base += TILE_THREADS * TILE_STAGE) {
        int64_t c[TILE_STAGE];
        u32x4 piece[TILE_STAGE];
#pragma unroll
        for (int u = 0; u < TILE_STAGE; ++u) {  // piece p = (slot p / 8, lane p % 8), and p % 8 == gl for every p this thread takes
            const int p = base + u * TILE_THREADS + tid;
            c[u] = (live && p < pieces) ? tile_cols[t0 + (p >> 3)] : -1;
        }
#pragma unroll
        for (int u = 0; u < TILE_STAGE; ++u)
            if (c[u] >= 0) piece[u] = load16<false>(mat + c[u] * D + c0);
#pragma unroll
        for (int u = 0; u < TILE_STAGE; ++u)
            if (c[u] >= 0) tile[base + u * TILE_THREADS + tid] = piece[u];
    }
    __syncthreads();
    if (!live) return;
    const int64_t r0 = b << rshift;
    const int nrows = (int)((M - r0) < ((int64_t)1 << rshift) ? (M - r0) : ((int64_t)1 << rshift));
    for (int r = tid / TILE_LANES; r < nrows; r += TILE_THREADS / TILE_LANES) {
        const int64_t i = r0 + r;
        const int32_t beg = rowptr[i], end = rowptr[i + 1];
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int32_t j = beg; j < end; j += U) {
            int sl[U];  // -1: past the row's end; TILE_NONE: not staged; else the LDS slot
            int64_t c[U];
            T wraw[U];
            u32x4 rows[U];
            // as in spmm_rows_kernel, each phase has all its loads in flight together: (slot, value) pairs, then the column
            // ids of the unstaged nonzeros only, then the operand rows from LDS or global memory
#pragma unroll
            for (int u = 0; u < U; ++u) {
                sl[u] = -1;
                if (j + u < end) {
                    sl[u] = slot[j + u];
                    if (value) wraw[u] = value[j + u];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (sl[u] == TILE_NONE) c[u] = col[j + u];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (sl[u] == TILE_NONE)
                    rows[u] = load16<false>(mat + c[u] * D + c0);
                else if (sl[u] >= 0)
                    rows[u] = tile[sl[u] * TILE_LANES + gl];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (sl[u] >= 0) {
                    float f[VEC];
                    Elem<T>::unpack(rows[u], f);
                    const float w = value ? Elem<T>::load(&wraw[u]) : 1.f;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = __fadd_rn(acc[v], __fmul_rn(w, f[v]));
                }
            }
        }
        store16<true>(out + i * D + c0, Elem<T>::pack(acc));
    }
}

template <typename T>
int launch_tiled(const int32_t* rowptr, const int64_t* col, const void* value, const void* mat, void* out, int64_t M, int64_t D,
                 const int32_t* tile_ptr, const int64_t* tile_cols, const uint16_t* slot, int rshift, int slots,
                 hipStream_t stream) {
    constexpr int VEC = Elem<T>::VEC;
    GNNOPS_REQUIRE(D % VEC == 0 && (uintptr_t)mat % 16 == 0 && (uintptr_t)out % 16 == 0, GNNOPS_EINVAL,
                   "spmm_tiled: D must be a multiple of %d and mat / out 16-byte aligned (use gnnops_spmm otherwise)", VEC);
    const int kchunks = (int)gnnops_cdiv(D / VEC, TILE_LANES);
    const int64_t nblocks = gnnops_cdiv(M, (int64_t)1 << rshift);
    GNNOPS_REQUIRE(nblocks * kchunks < ((int64_t)1 << 31), GNNOPS_EUNSUPPORTED, "spmm_tiled: too many (row block, chunk) items");
    static bool configured = false;
    if (!configured) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&spmm_tiled_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                TILE_LDS_BYTES) != hipSuccess)
            return gnnops_check_launch("spmm_tiled attribute");
        configured = true;
    }
    hipLaunchKernelGGL((spmm_tiled_kernel<T>), dim3((unsigned)(nblocks * kchunks)), dim3(TILE_THREADS),
                       (size_t)slots * TILE_SLOT_BYTES, stream, rowptr, col, slot, (const T*)value, (const T*)mat, (T*)out,
                       tile_ptr, tile_cols, M, D, rshift, kchunks);
    return gnnops_check_launch("spmm_tiled");
}

// CSR materialisation of a plan-ordered COO operand: out[j] = in[perm[j]] for the column ids (8 B) or the values.
template <typename U>
__global__ void permute_kernel(const U* __restrict__ in, const int32_t* __restrict__ perm, U* __restrict__ out, int64_t n) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x)
        out[j] = in[perm[j]];
}

template <typename T>
int launch(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value, const void* mat,
           void* out, int64_t M, int64_t D, int64_t mat_rows, hipStream_t stream, int64_t nnz, void* hub_ws,
           size_t hub_ws_bytes) {
    constexpr int VEC = Elem<T>::VEC;
    if (D % VEC == 0 && (uintptr_t)mat % 16 == 0 && (uintptr_t)out % 16 == 0) {
        const int64_t vecs = D / VEC;
        const int gshift = gnnops_group_shift(vecs);
        const int kchunks = (int)gnnops_cdiv(vecs, (int64_t)1 << gshift);
        const int grid = gnnops_grid_cap(gnnops_cdiv((int64_t)kchunks * M, 256 >> gshift), 256 * 64);
        // a dense operand far beyond the 256 MiB Infinity Cache is streamed nontemporally (its rows would only evict
        // the CSR arrays); a smaller one keeps normal caching so repeated rows hit on-die
        const bool nt = (size_t)mat_rows * (size_t)D * sizeof(T) > ((size_t)2 << 30);
        hub::Ws hw{};
        int hub_on = 0;
        if (hub_ws && nnz > hub::T_HUB) {
            const hub::Layout hl = hub::layout(nnz, D, false);
            if (hub_ws_bytes >= hl.total) {
                hw = hub::make_ws(hub_ws, hl, nnz, false);
                if (gnnops_memset_async(hw.counters, 0, 8, stream) != hipSuccess) return gnnops_check_launch("hub memset");
                hub_on = 1;
            }
        }
        if (nt)
            hipLaunchKernelGGL((spmm_rows_kernel<T, true>), dim3(grid), dim3(256), 0, stream, rowptr, perm, col,
                               (const T*)value, (const T*)mat, (T*)out, M, D, gshift, kchunks, hw, hub_on);
        else
            hipLaunchKernelGGL((spmm_rows_kernel<T, false>), dim3(grid), dim3(256), 0, stream, rowptr, perm, col,
                               (const T*)value, (const T*)mat, (T*)out, M, D, gshift, kchunks, hw, hub_on);
        if (hub_on)
            hub::launch_spmm_pass<T>(perm, col, (const T*)value, (const T*)mat, (T*)out, hw, nnz, D, gshift, kchunks, stream);
    } else if (D >= 256) {
        const int chunks = (int)gnnops_cdiv(D, 256 * 4);
        const int grid = gnnops_grid_cap(M * chunks, 256 * 32);
        hipLaunchKernelGGL((spmm_widerows_kernel<T>), dim3(grid), dim3(256), 0, stream, rowptr, perm, col, (const T*)value,
                           (const T*)mat, (T*)out, M, D, chunks);
    } else {
        const int grid = gnnops_grid_cap(gnnops_cdiv(M * D, 256), 256 * 32);
        hipLaunchKernelGGL((spmm_elems_kernel<T>), dim3(grid), dim3(256), 0, stream, rowptr, perm, col, (const T*)value,
                           (const T*)mat, (T*)out, M, D);
    }
    return gnnops_check_launch("spmm");
}

}  // namespace

extern "C" int gnnops_spmm(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value,
                           const void* mat, void* out, int64_t M, int64_t D, int64_t nnz, int64_t mat_rows, int dtype,
                           gnnops_stream_t s) {
    return gnnops_spmm_hubs(rowptr, perm, col, value, mat, out, M, D, nnz, mat_rows, dtype, nullptr, 0, s);
}

// The same with rows of more than 8192 nonzeros set aside and multiplied out piecewise by whole workgroups (hub.h):
// hub_workspace = gnnops_hub_workspace_bytes(nnz, D, 0) bytes, or NULL.
extern "C" int gnnops_spmm_hubs(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value,
                                const void* mat, void* out, int64_t M, int64_t D, int64_t nnz, int64_t mat_rows, int dtype,
                                void* hub_workspace, size_t hub_workspace_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(M >= 0 && D >= 0 && nnz >= 0, GNNOPS_EINVAL, "spmm: negative size");
    GNNOPS_REQUIRE(nnz < ((int64_t)1 << 31), GNNOPS_EUNSUPPORTED, "spmm: nnz must be < 2^31");
    if (M * D == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(rowptr && out && (nnz == 0 || (col && mat)), GNNOPS_EINVAL, "spmm: null pointer");
    return gnnops_with_dtype(dtype, "spmm", [&](auto t) {
        return launch<typename decltype(t)::type>(rowptr, perm, col, value, mat, out, M, D, mat_rows, stream, nnz, hub_workspace,
                                                  hub_workspace_bytes);
    });
}

// CSR x dense through a tile plan (include/gnnops.h): bit-identical to gnnops_spmm(rowptr, NULL, col, ...).
extern "C" int gnnops_spmm_tiled(const int32_t* rowptr, const int64_t* col, const void* value, const void* mat, void* out,
                                 int64_t M, int64_t D, int64_t nnz, int dtype, const int32_t* tile_ptr, const int64_t* tile_cols,
                                 const uint16_t* slot, int block_rows, int slots, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(M >= 0 && D >= 0 && nnz >= 0, GNNOPS_EINVAL, "spmm_tiled: negative size");
    GNNOPS_REQUIRE(nnz < ((int64_t)1 << 31), GNNOPS_EUNSUPPORTED, "spmm_tiled: nnz must be < 2^31");
    GNNOPS_REQUIRE(block_rows >= 1 && (block_rows & (block_rows - 1)) == 0, GNNOPS_EINVAL,
                   "spmm_tiled: block_rows %d is not a power of two", block_rows);
    GNNOPS_REQUIRE(slots >= 1 && slots <= TILE_LDS_BYTES / TILE_SLOT_BYTES, GNNOPS_EINVAL,
                   "spmm_tiled: slots %d outside [1, %d] (%d bytes of LDS each)", slots, TILE_LDS_BYTES / TILE_SLOT_BYTES,
                   TILE_SLOT_BYTES);
    if (M * D == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(rowptr && out && tile_ptr && (nnz == 0 || (col && mat && slot)), GNNOPS_EINVAL, "spmm_tiled: null pointer");
    int rshift = 0;
    while ((1 << rshift) < block_rows) ++rshift;
    return gnnops_with_dtype(dtype, "spmm_tiled", [&](auto t) {
        return launch_tiled<typename decltype(t)::type>(rowptr, col, value, mat, out, M, D, tile_ptr, tile_cols, slot, rshift, slots, stream);
    });
}

// out[j] = in[perm[j]], elements of 2, 4 or 8 bytes: turns (plan, COO columns / values) into CSR arrays once, so the
// row-split kernel streams them instead of chasing perm -> col for every nonzero.
extern "C" int gnnops_permute(const void* in, const int32_t* perm, void* out, int64_t n, int elem_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(n >= 0, GNNOPS_EINVAL, "permute: negative size");
    GNNOPS_REQUIRE(elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, GNNOPS_EUNSUPPORTED, "permute: elem_bytes %d", elem_bytes);
    if (n == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(in && perm && out, GNNOPS_EINVAL, "permute: null pointer");
    const int grid = gnnops_grid_cap(gnnops_cdiv(n, 256), 256 * 32);
    if (elem_bytes == 8)
        hipLaunchKernelGGL(permute_kernel<uint64_t>, dim3(grid), dim3(256), 0, stream, (const uint64_t*)in, perm, (uint64_t*)out, n);
    else if (elem_bytes == 4)
        hipLaunchKernelGGL(permute_kernel<uint32_t>, dim3(grid), dim3(256), 0, stream, (const uint32_t*)in, perm, (uint32_t*)out, n);
    else
        hipLaunchKernelGGL(permute_kernel<uint16_t>, dim3(grid), dim3(256), 0, stream, (const uint16_t*)in, perm, (uint16_t*)out, n);
    return gnnops_check_launch("permute");
}
