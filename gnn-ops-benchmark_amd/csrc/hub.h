// hub.h — heavy destinations ("hubs") of the row reductions (segment.hip: plan form, bucket.hip: one-shot form).
//
// Everywhere else ONE lane group walks a destination's contributions in source order — that is what makes the result
// bit-identical to the sequential oracle — which serialises a destination with 10^5 contributions into 10^4 dependent
// batches of 8 rows (measured: +13 ms for one hub of 100 000 edges, +120 ms for 1 000 000; tools/time_hub.py). A uniform
// graph (the reference's generator) has no such destination; a power-law graph does. So:
//
//   * a destination with more than T_HUB contributions is set aside by the main kernel (one record per hub, appended
//     through an atomic counter; the main kernel neither reduces nor stores it);
//   * hub_partial_kernel: the hub's contributions are cut into pieces of PART, a workgroup per piece; inside a piece the
//     lane groups take contiguous parts and their partial results are combined IN ORDER;
//   * hub_combine_kernel: one lane group per hub folds the piece partials, again in order, into the output row (starting
//     from the row already there for index_add_ / `out=`), divides a mean, writes min / max positions.
//
// min / max (and their arg: smallest position) stay exact. Sums, means and products of a hub are re-associated — piece by
// piece instead of one by one — so they are deterministic but no longer bit-identical to the sequential loop: the price
// of not serialising. Everything below T_HUB is untouched.
//
// Bucket form: the partition groups a bucket's entries in source order but does not separate its 256 destinations, so a
// piece is PART entries of the BUCKET, filtered by destination on chip (stable compaction), and at most MAX_PER_BUCKET
// hubs of one bucket (those with the smallest ids) are set aside — the others take the sequential path.
//
// The five kernels that finish a hub by pieces (hub_partial_kernel, hub_partial_spmm_kernel, hub_push_kernel here,
// chub_stat2_kernel and chub_finish_kernel of composite.hip) share ONE walk, the device helpers below:
//   npieces / piece_at   the clamped piece count and the record of piece q (false: dropped); the loop stays in the kernel
//   stage_piece          the piece's source positions into s_match, in order: perm[..] (identity without perm); the bucket
//                        form's stable compaction is HUB_STAGE_BUCKET_PIECE, one text expanded in the two kernels that have it
//   Lanes / slice        lane-group geometry of the workgroup and the contiguous part of a piece one group takes
//   for_rows             the step of U rows in flight: positions, then every load, then the rows consumed in order (the SpMM
//                        kernel keeps its own: it reads column and weight with the positions)
//   fold_groups          the groups' partials through LDS, folded by group 0 in group (= source) order
// and the host side: open (workspace -> Ws, counters cleared) and piece_grid (workgroups of a piece pass).
// What each helper does to the compiled kernels, and why two are shaped as they are: profiles/hub_walk.txt.
#pragma once
#include "common.h"

namespace hub {

constexpr int T_HUB = 8192;
constexpr int PART = 4096;
constexpr int MAX_PER_BUCKET = 4;
constexpr int THREADS = 256;
constexpr int U = 8;  // rows in flight per lane group

struct Ws {
    int32_t* counters;    // [0] hubs, [1] pieces
    int32_t* hubs;        // [cap_h][4]: destination, beg, end, degree (beg / end: perm positions, or the bucket's entry range)
    int32_t* piece_base;  // [cap_h]: first piece of the hub
    int32_t* pieces;      // [cap_p][2]: hub, piece number inside the hub
    float* partial;       // [cap_p][K]
    int32_t* parg;        // [cap_p][K] (min / max) or nullptr
    int32_t cap_h, cap_p;
};

// Every hub has more than T_HUB contributions, so there are at most E / T_HUB of them. Plan form: a hub of length L has
// ceil(L / PART) pieces, in total at most E / PART + hubs. Bucket form: at most MAX_PER_BUCKET hubs per bucket, each with
// ceil(bucket length / PART) pieces, over buckets that hold more than T_HUB entries: at most
// MAX_PER_BUCKET * (E / PART + E / T_HUB). The capacities below cover both.
inline size_t cap_hubs(int64_t E) { return (size_t)(E / T_HUB) + 1; }
inline size_t cap_pieces(int64_t E) { return (size_t)MAX_PER_BUCKET * ((size_t)(E / PART) + cap_hubs(E)) + 1; }

struct Layout { size_t counters, hubs, piece_base, pieces, partial, parg, total; };
inline Layout layout(int64_t E, int64_t K, bool want_arg) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    Layout l{};
    size_t o = 0;
    l.counters = o; o += 256;
    l.hubs = o; o += up(cap_hubs(E) * 16);
    l.piece_base = o; o += up(cap_hubs(E) * 4);
    l.pieces = o; o += up(cap_pieces(E) * 8);
    l.partial = o; o += up(cap_pieces(E) * (size_t)K * 4);
    l.parg = o; o += want_arg ? up(cap_pieces(E) * (size_t)K * 4) : 0;
    l.total = o;
    return l;
}
inline Ws make_ws(void* base, const Layout& l, int64_t E, bool want_arg) {
    char* w = (char*)base;
    Ws s{};
    s.counters = (int32_t*)(w + l.counters);
    s.hubs = (int32_t*)(w + l.hubs);
    s.piece_base = (int32_t*)(w + l.piece_base);
    s.pieces = (int32_t*)(w + l.pieces);
    s.partial = (float*)(w + l.partial);
    s.parg = want_arg ? (int32_t*)(w + l.parg) : nullptr;
    s.cap_h = (int32_t)cap_hubs(E);
    s.cap_p = (int32_t)cap_pieces(E);
    return s;
}

// Host: hubs are set aside when the caller brought a workspace (pass nullptr where the entry point's own condition rules
// them out) that is large enough for E contributions of K columns. 1: w is ready and its counters are cleared on the
// stream; 0: no hubs, w is empty; -1: the clear could not be launched.
inline int open(void* ws, size_t bytes, int64_t E, int64_t K, bool want_arg, hipStream_t stream, Ws& w) {
    w = Ws{};
    if (!ws || E <= T_HUB) return 0;
    const Layout l = layout(E, K, want_arg);
    if (bytes < l.total) return 0;
    w = make_ws(ws, l, E, want_arg);
    return gnnops_memset_async(w.counters, 0, 8, stream) == hipSuccess ? 1 : -1;
}
inline int piece_grid(const Ws& w) { return w.cap_p < 2048 ? w.cap_p : 2048; }  // workgroups of a pass over the pieces

// One thread: set a hub aside. The capacities cannot be exceeded (see above); should they be, the record is dropped and
// the counters saturate at the capacity in the readers (the hub would be lost, which the bound rules out).
__device__ inline void append(const Ws& w, int dst, int beg, int end, int deg) {
    const int np = (end - beg + PART - 1) / PART;
    const int h = atomicAdd(&w.counters[0], 1);
    if (h >= w.cap_h) return;
    const int pb = atomicAdd(&w.counters[1], np);
    w.hubs[4 * h + 0] = (pb + np <= w.cap_p) ? dst : -1;
    w.hubs[4 * h + 1] = beg;
    w.hubs[4 * h + 2] = end;
    w.hubs[4 * h + 3] = deg;
    w.piece_base[h] = pb;
    for (int p = 0; p < np && pb + p < w.cap_p; ++p) {
        w.pieces[2 * (pb + p) + 0] = (pb + np <= w.cap_p) ? h : -1;
        w.pieces[2 * (pb + p) + 1] = p;
    }
}

// ---- the shared walk of the piece passes -------------------------------------------------------------------------------
struct Piece { int h, pno, dst, beg, end, deg, pb, n; };  // hub, piece number in it, the hub's record, first entry and length of the piece

__device__ inline int npieces(const Ws& w) {  // saturates at the capacity (see append)
    const int n = w.counters[1];
    return n > w.cap_p ? w.cap_p : n;
}

__device__ inline bool piece_at(const Ws& w, int q, Piece& p) {
    p.h = w.pieces[2 * q];
    if (p.h < 0) return false;
    p.pno = w.pieces[2 * q + 1];
    p.dst = w.hubs[4 * p.h], p.beg = w.hubs[4 * p.h + 1], p.end = w.hubs[4 * p.h + 2], p.deg = w.hubs[4 * p.h + 3];
    p.pb = p.beg + p.pno * PART;
    p.n = (p.end - p.pb < PART) ? p.end - p.pb : PART;
    return true;
}

// Plan form: the piece's source positions perm[pb + i] (the entries themselves without perm) into s_match, in order; returns
// how many. The caller's barriers stand before and after.
__device__ inline int stage_piece(const Piece p, const int32_t* perm, int32_t* s_match) {
    for (int i = threadIdx.x; i < p.n; i += THREADS) s_match[i] = perm ? perm[p.pb + i] : p.pb + i;
    return p.n;
}

// Bucket form: the positions of those entries of the bucket's piece that belong to the hub, compacted into s_match —
// consecutive entries per thread and an exclusive scan of the counts keep it stable. A macro, not a function: called as a
// function it costs hub_partial_kernel<float, SUM / MUL, true> and <__half, MUL, true> a wave per SIMD
// (profiles/hub_walk.txt), expanded in place both kernels that use it compile as they did with their own copies.
#define HUB_STAGE_BUCKET_PIECE(p, keys, vals, s_match, s_tmp, m)                                         \
    {                                                                                                    \
        constexpr int IPT = PART / THREADS;                                                              \
        const uint32_t low = (uint32_t)(p).dst & 255u;                                                   \
        uint32_t pos[IPT];                                                                               \
        uint32_t c = 0;                                                                                  \
        _Pragma("unroll") for (int j = 0; j < IPT; ++j) {                                                \
            const int i = threadIdx.x * IPT + j;                                                         \
            pos[j] = 0xffffffffu;                                                                        \
            if (i < (p).n && ((keys)[(p).pb + i] & 255u) == low) { pos[j] = (vals)[(p).pb + i]; ++c; }   \
        }                                                                                                \
        uint32_t tot;                                                                                    \
        uint32_t off = block_excl_scan_u32<THREADS / 64>(c, s_tmp, &tot);                                \
        _Pragma("unroll") for (int j = 0; j < IPT; ++j)                                                  \
            if (pos[j] != 0xffffffffu) (s_match)[off++] = (int32_t)pos[j];                               \
        (m) = (int)tot;                                                                                  \
    }

struct Lanes {  // the workgroup as lane groups of G = 2^gshift lanes: lane gl of group gi
    int G, gl, gi, groups;
    __device__ explicit Lanes(int gshift)
        : G(1 << gshift), gl(threadIdx.x & (G - 1)), gi(threadIdx.x >> gshift), groups(THREADS >> gshift) {}
};

// the contiguous part [jb, je) of a piece's m positions that the lane group takes
__device__ inline void slice(int m, const Lanes l, int& jb, int& je) {
    const int part = (m + l.groups - 1) / l.groups;
    jb = l.gi * part;
    je = (jb + part < m) ? jb + part : m;
}

// U rows in flight over s_match[jb .. je): the positions are read, then every load(e) is issued, then use(e, row) runs in
// source order.
template <typename Load, typename Use>
__device__ inline void for_rows(const int32_t* s_match, int jb, int je, Load load, Use use) {
    for (int j = jb; j < je; j += U) {
        int32_t e[U];
        decltype(load(0)) rows[U];
#pragma unroll
        for (int u = 0; u < U; ++u) e[u] = (j + u < je) ? s_match[j + u] : -1;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (e[u] >= 0) rows[u] = load(e[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (e[u] >= 0) use(e[u], rows[u]);
    }
}

// Every lane's VEC partials (and, ARG, their positions) through LDS; the lanes of group 0 that are `live` fold those of
// groups 1 .. groups - 1 onto their own in group (= source) order — take(a, f) folds f into a and says whether f's position
// replaces a's — and hand each result to store(v, a, position). Ends on a barrier: s_part may be written again.
template <int VEC, bool ARG = false, typename Take, typename Store>
__device__ inline void fold_groups(const Lanes l, bool live, const float* acc, float* s_part, Take take, Store store,
                                   const int32_t* arg = nullptr, int32_t* s_parg = nullptr) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        s_part[tid * VEC + v] = acc[v];
        if constexpr (ARG) s_parg[tid * VEC + v] = arg[v];
    }
    __syncthreads();
    if (l.gi == 0 && live) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float a = s_part[l.gl * VEC + v];
            int32_t ar = ARG ? s_parg[l.gl * VEC + v] : 0;
            for (int g = 1; g < l.groups; ++g) {
                if (take(a, s_part[(g * l.G + l.gl) * VEC + v])) {
                    if constexpr (ARG) ar = s_parg[(g * l.G + l.gl) * VEC + v];
                }
            }
            store(v, a, ar);
        }
    }
    __syncthreads();
}

// A workgroup per piece: (1) the piece's source positions into LDS, in order (stage_piece); (2) the lane groups reduce
// contiguous parts of that list; (3) their partials are combined in group order into partial[piece].
template <typename T, int R, bool BUCKET>
__global__ __launch_bounds__(THREADS) void hub_partial_kernel(const T* __restrict__ src, const int32_t* __restrict__ perm,
                                                              const uint32_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ vals, Ws w, int64_t E, int64_t K,
                                                              int gshift, int kchunks) {
    constexpr int VEC = Elem<T>::VEC;
    constexpr bool IS_ARG = (R == GNNOPS_MIN || R == GNNOPS_MAX);
    __shared__ int32_t s_match[PART];
    __shared__ uint32_t s_tmp[THREADS / 64];
    __shared__ float s_part[THREADS * VEC];
    __shared__ int32_t s_parg[IS_ARG ? THREADS * VEC : 1];
    const Lanes l(gshift);
    auto take = [](float& a, float f) {  // min / max: the first of equal values keeps its position
        if constexpr (IS_ARG) {
            if (!Red<R>::better(f, a)) return false;
            a = f;
            return true;
        } else {
            a = Red<R>::apply(a, f);
            return false;
        }
    };
    const int np = npieces(w);
    for (int q = blockIdx.x; q < np; q += gridDim.x) {
        Piece p;
        if (!piece_at(w, q, p)) continue;
        __syncthreads();  // the previous piece's readers are done with the LDS arrays
        int m;
        if constexpr (BUCKET) HUB_STAGE_BUCKET_PIECE(p, keys, vals, s_match, s_tmp, m)
        else m = stage_piece(p, perm, s_match);
        __syncthreads();
        int jb, je;
        slice(m, l, jb, je);
        for (int chunk = 0; chunk < kchunks; ++chunk) {
            const int64_t col = ((int64_t)chunk * l.G + l.gl) * VEC;
            float acc[VEC];
            int32_t arg[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) { acc[v] = Red<R>::identity(); arg[v] = (int32_t)E; }
            if (col < K) {
                const T* srcb = src + col;
                for_rows(
                    s_match, jb, je, [&](int32_t e) { return load16<true>(srcb + (int64_t)e * K); },
                    [&](int32_t e, const u32x4& row) {
                        float f[VEC];
                        Elem<T>::unpack(row, f);
#pragma unroll
                        for (int v = 0; v < VEC; ++v)
                            if (take(acc[v], f[v])) arg[v] = e;
                    });
            }
            fold_groups<VEC, IS_ARG>(
                l, col < K, acc, s_part, take,
                [&](int v, float a, int32_t ar) {
                    w.partial[(int64_t)q * K + col + v] = a;
                    if constexpr (IS_ARG) {
                        if (w.parg) w.parg[(int64_t)q * K + col + v] = ar;
                    }
                },
                arg, s_parg);
        }
    }
}

// One lane group per (hub, column chunk): the piece partials folded in order into the output row.
template <typename T, int R>
__global__ __launch_bounds__(THREADS) void hub_combine_kernel(T* __restrict__ out, int64_t* __restrict__ arg_out, Ws w,
                                                              int64_t E, int64_t K, int gshift, int kchunks,
                                                              int init_from_out, int is_mean) {
    constexpr int VEC = Elem<T>::VEC;
    constexpr bool IS_ARG = (R == GNNOPS_MIN || R == GNNOPS_MAX);
    const int G = 1 << gshift;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) >> gshift;
    const int gl = (int)(gtid & (G - 1));
    int nh = w.counters[0];
    if (nh > w.cap_h) nh = w.cap_h;
    for (int64_t item = gtid >> gshift; item < (int64_t)nh * kchunks; item += ngroups) {
        const int h = (int)(item / kchunks);
        const int chunk = (int)(item - (int64_t)h * kchunks);
        const int dst = w.hubs[4 * h];
        const int64_t col = ((int64_t)chunk * G + gl) * VEC;
        if (dst < 0 || col >= K) continue;
        const int np = (w.hubs[4 * h + 2] - w.hubs[4 * h + 1] + PART - 1) / PART;
        const int pb = w.piece_base[h];
        const int64_t oidx = (int64_t)dst * K + col;
        float acc[VEC];
        int32_t arg[VEC];
        if (init_from_out) {
            Elem<T>::unpack(*reinterpret_cast<const u32x4*>(out + oidx), acc);
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = Red<R>::identity();
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) arg[v] = (int32_t)E;
        for (int p = 0; p < np; ++p) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float f = w.partial[(int64_t)(pb + p) * K + col + v];
                if constexpr (IS_ARG) {
                    if (Red<R>::better(f, acc[v])) { acc[v] = f; arg[v] = w.parg[(int64_t)(pb + p) * K + col + v]; }
                } else {
                    acc[v] = Red<R>::apply(acc[v], f);
                }
            }
        }
        if constexpr (IS_ARG) {
            if (arg_out) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) arg_out[oidx + v] = arg[v];
            }
        } else if (R == GNNOPS_SUM) {
            if (is_mean) {
                const float c = (float)w.hubs[4 * h + 3];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / c;
            }
        }
        store16<true>(out + oidx, Elem<T>::pack(acc));
    }
}

// SpMM (spmm.hip): an output row with more than T_HUB nonzeros. Same pieces; a contribution is value[e] * mat[col[e], :]
// (two roundings, as in spmm_rows_kernel), the piece partials are folded by hub_combine_kernel<T, GNNOPS_SUM>.
template <typename T>
__global__ __launch_bounds__(THREADS) void hub_partial_spmm_kernel(const int32_t* __restrict__ perm,
                                                                   const int64_t* __restrict__ col, const T* __restrict__ value,
                                                                   const T* __restrict__ mat, Ws w, int64_t D, int gshift,
                                                                   int kchunks) {
    constexpr int VEC = Elem<T>::VEC;
    __shared__ int32_t s_match[PART];
    __shared__ float s_part[THREADS * VEC];
    const Lanes l(gshift);
    const int np = npieces(w);
    for (int q = blockIdx.x; q < np; q += gridDim.x) {
        Piece p;
        if (!piece_at(w, q, p)) continue;
        __syncthreads();
        const int n = stage_piece(p, perm, s_match);
        __syncthreads();
        int jb, je;
        slice(n, l, jb, je);
        for (int chunk = 0; chunk < kchunks; ++chunk) {
            const int64_t c0 = ((int64_t)chunk * l.G + l.gl) * VEC;
            float acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
            if (c0 < D) {
                // not for_rows: column and weight of a nonzero are read with the positions, ahead of the rows of mat that hang on them
                for (int j = jb; j < je; j += U) {
                    int64_t c[U];
                    float wt[U];
                    u32x4 rows[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        c[u] = -1;
                        if (j + u < je) {
                            const int32_t e = s_match[j + u];
                            c[u] = col[e];
                            wt[u] = value ? Elem<T>::load(value + e) : 1.f;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (c[u] >= 0) rows[u] = load16<false>(mat + c[u] * D + c0);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (c[u] >= 0) {
                            float f[VEC];
                            Elem<T>::unpack(rows[u], f);
#pragma unroll
                            for (int v = 0; v < VEC; ++v) acc[v] = __fadd_rn(acc[v], __fmul_rn(wt[u], f[v]));
                        }
                    }
                }
            }
            fold_groups<VEC>(
                l, c0 < D, acc, s_part, [](float& a, float f) { a = __fadd_rn(a, f); return false; },
                [&](int v, float a, int32_t) { w.partial[(int64_t)q * D + c0 + v] = a; });
        }
    }
}

template <typename T>
inline void launch_spmm_pass(const int32_t* perm, const int64_t* col, const T* value, const T* mat, T* out, const Ws& w,
                             int64_t nnz, int64_t D, int gshift, int kchunks, hipStream_t stream) {
    hipLaunchKernelGGL((hub_partial_spmm_kernel<T>), dim3(piece_grid(w)), dim3(THREADS), 0, stream, perm, col, value, mat, w, D,
                       gshift, kchunks);
    const int64_t items = (int64_t)w.cap_h * kchunks;
    const int gb = gnnops_grid_cap(gnnops_cdiv(items, THREADS >> gshift), 1024);
    hipLaunchKernelGGL((hub_combine_kernel<T, GNNOPS_SUM>), dim3(gb), dim3(THREADS), 0, stream, out, (int64_t*)nullptr, w, nnz,
                       D, gshift, kchunks, 0, 0);
}

// Push-form index_select (gather.hip / bucket.hip): a HOT table row — selected by more than T_HUB outputs — is stored
// by one lane group, eight stores in flight, for all of its outputs (56 ms for a row selected 10^6 times, against 1.3 ms
// for the whole op without it). Set aside in the same way, its outputs are written by a workgroup per piece instead:
// every lane group loads the row once and stores it to a contiguous part of the piece's output positions.
template <bool BUCKET>
__global__ __launch_bounds__(THREADS) void hub_push_kernel(const char* __restrict__ in, const int32_t* __restrict__ perm,
                                                           const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           char* __restrict__ out, Ws w, int64_t rowbytes, int gshift,
                                                           int chunks) {
    __shared__ int32_t s_match[PART];
    __shared__ uint32_t s_tmp[THREADS / 64];
    const Lanes l(gshift);
    const int np = npieces(w);
    for (int q = blockIdx.x; q < np; q += gridDim.x) {
        Piece p;
        if (!piece_at(w, q, p)) continue;
        __syncthreads();
        int m;
        if constexpr (BUCKET) HUB_STAGE_BUCKET_PIECE(p, keys, vals, s_match, s_tmp, m)
        else m = stage_piece(p, perm, s_match);
        __syncthreads();
        for (int c = 0; c < chunks; ++c) {
            const int64_t colb = ((int64_t)c * l.G + l.gl) * 16;
            if (colb >= rowbytes) continue;
            const u32x4 v = load16<false>(in + (int64_t)p.dst * rowbytes + colb);
            char* outb = out + colb;
            for (int j0 = l.gi; j0 < m; j0 += l.groups * U) {   // groups interleave: neighbouring positions, neighbouring groups
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = j0 + u * l.groups;
                    if (j < m) store16<true>(outb + (int64_t)s_match[j] * rowbytes, v);
                }
            }
        }
    }
}

inline void launch_push_pass(bool bucket, const char* in, const int32_t* perm, const uint32_t* keys, const uint32_t* vals,
                             char* out, const Ws& w, int64_t rowbytes, int gshift, int chunks, hipStream_t stream) {
    if (bucket)
        hipLaunchKernelGGL((hub_push_kernel<true>), dim3(piece_grid(w)), dim3(THREADS), 0, stream, in, perm, keys, vals, out, w,
                           rowbytes, gshift, chunks);
    else
        hipLaunchKernelGGL((hub_push_kernel<false>), dim3(piece_grid(w)), dim3(THREADS), 0, stream, in, perm, keys, vals, out, w,
                           rowbytes, gshift, chunks);
}

// The two launches that follow a main kernel which set hubs aside (they exit at once when there are none).
template <typename T, int R, bool BUCKET>
inline void launch_pass(const T* src, const int32_t* perm, const uint32_t* keys, const uint32_t* vals, T* out,
                        int64_t* arg_out, const Ws& w, int64_t E, int64_t K, int gshift, int kchunks, int init_from_out,
                        int is_mean, hipStream_t stream) {
    hipLaunchKernelGGL((hub_partial_kernel<T, R, BUCKET>), dim3(piece_grid(w)), dim3(THREADS), 0, stream, src, perm, keys, vals,
                       w, E, K, gshift, kchunks);
    const int64_t items = (int64_t)w.cap_h * kchunks;
    const int gb = gnnops_grid_cap(gnnops_cdiv(items, THREADS >> gshift), 1024);
    hipLaunchKernelGGL((hub_combine_kernel<T, R>), dim3(gb), dim3(THREADS), 0, stream, out, arg_out, w, E, K, gshift, kchunks,
                       init_from_out, is_mean);
}

#undef HUB_STAGE_BUCKET_PIECE

}  // namespace hub
