// pool.hip — the two selection steps of a pooling level (TopKPooling / GraphUNet, the reference's GraphUNetREG,
// graph_benchmark/models/ptg_models.py): per-graph top-k of a score vector, and the stable compaction of a COO edge list
// through a node map (filter_adj / remove_self_loops).
//
// segment top-k. Every dtype is mapped to the COMPLEMENT of the sort key of sort.hip (f32_key: -0.0 folded onto +0.0, every NaN
// on top), so an ascending stable sort of the image is the descending order with ties to the lower node id and NaNs first.
//   on-chip  a graph of up to 64 nodes is ranked by one wave (each lane counts the keys that precede its own: 64 LDS
//            broadcasts, no sort at all); a graph of up to TOPK_MAX_LEN nodes by one workgroup, as four (fp16: three, bf16: two)
//            stable 8-bit passes of ldssort::sort_chunk over indices into the keys it staged once. Either way the graph is
//            read from HBM once and only its k ids are written.
//   long     one gnnops_sort of int64 keys (graph id << 32 | image) — nodes of a graph are contiguous, so graph g lands on
//            positions [graph_ptr[g], graph_ptr[g + 1]) — and a select pass that copies the first k ids of a graph. A call whose
//            longest graph exceeds TOPK_MAX_LEN runs the on-chip kernels too (they skip what is too long for them) and the select
//            pass writes the longer graphs only; a forced long route (tests) writes every graph from the sort.
// Both give the same perm: both are stable orders of the same keys.
//
// filter_edges: count the survivors per tile of FILTER_TILE edges, scan the tile counts (one workgroup), then reread the edges
// and write. Inside a tile a wave owns 256 consecutive edges as four rows of 64; ranks are popcounts of ballots in lane
// order, so survivors keep their order. 2 x 16 B read per edge and pass, 16 B (+ the value row) written per survivor.
#include <type_traits>
#include "common.h"
#include "dispatch.h"
#include "lds_sort.h"

namespace {

constexpr int TOPK_MAX_LEN = 4096;   // 3 x 16 KiB (keys, two index buffers) + 5 KiB of sort_chunk state = 53 KiB: three workgroups per CU
constexpr int TOPK_ROUNDS = TOPK_MAX_LEN / 256;
constexpr int FILTER_TILE = 1024;    // 256 threads x 4 rows

template <typename T> __device__ inline uint32_t desc_key(const T* score, int64_t i) { return ~f32_key(Elem<T>::load(score + i)); }

// ---- k per graph and its exclusive scan: one workgroup (G is a batch size) ----
__global__ __launch_bounds__(256) void topk_counts_kernel(const int32_t* __restrict__ graph_ptr, int64_t G, float ratio, int64_t k,
                                                           int32_t* __restrict__ out_ptr, int64_t* __restrict__ info) {
    __shared__ uint32_t s_tmp[4];
    __shared__ uint32_t s_max[4];
    uint32_t carry = 0, longest = 0;
    for (int64_t g0 = 0; g0 < G; g0 += 256) {
        const int64_t g = g0 + threadIdx.x;
        uint32_t kg = 0;
        if (g < G) {
            const int32_t n = graph_ptr[g + 1] - graph_ptr[g];
            longest = max(longest, (uint32_t)n);
            if (k >= 1) {
                kg = (uint32_t)(k < n ? k : n);
            } else {
                const float c = ceilf(ratio * (float)n);   // float32 product and ceil, as (ratio * num_nodes.to(torch.float)).ceil()
                kg = (uint32_t)min((int64_t)c, (int64_t)n);
            }
        }
        uint32_t total;
        const uint32_t off = block_excl_scan_u32<4>(kg, s_tmp, &total);
        if (g < G) out_ptr[g] = (int32_t)(carry + off);
        carry += total;
    }
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, o));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = longest;
    __syncthreads();
    if (threadIdx.x == 0) {
        out_ptr[G] = (int32_t)carry;
        info[0] = (int64_t)carry;
        info[1] = (int64_t)max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    }
}

// ---- on-chip, graphs of 1..64 nodes: one wave per graph ----
template <typename T>
__global__ __launch_bounds__(256) void topk_wave_kernel(const T* __restrict__ score, const int32_t* __restrict__ graph_ptr,
                                                         const int32_t* __restrict__ out_ptr, int64_t* __restrict__ perm, int64_t G) {
    __shared__ uint32_t s_key[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + wave;
    int32_t base = 0, n = 0, k = 0, obase = 0;
    if (g < G) {
        base = graph_ptr[g];
        n = graph_ptr[g + 1] - base;
        obase = out_ptr[g];
        k = out_ptr[g + 1] - obase;
    }
    if (n > 64) n = 0;   // the workgroup kernel's
    uint32_t key = 0;
    if (lane < n) key = desc_key(score, (int64_t)base + lane);
    s_key[wave][lane] = key;
    __syncthreads();
    int rank = 0;
    for (int m = 0; m < n; ++m) {
        const uint32_t other = s_key[wave][m];
        rank += (other < key || (other == key && m < lane)) ? 1 : 0;
    }
    if (lane < n && rank < k) perm[(int64_t)obase + rank] = (int64_t)base + lane;
}

// ---- on-chip, graphs of 65..TOPK_MAX_LEN nodes: one workgroup per graph ----
template <typename T>
__global__ __launch_bounds__(256) void topk_block_kernel(const T* __restrict__ score, const int32_t* __restrict__ graph_ptr,
                                                          const int32_t* __restrict__ out_ptr, int64_t* __restrict__ perm) {
    __shared__ uint32_t s_key[TOPK_MAX_LEN];
    __shared__ uint32_t s_idx[2][TOPK_MAX_LEN];
    __shared__ uint32_t s_whist[4 * 256];
    __shared__ int32_t s_rowptr[257];
    __shared__ uint32_t s_tmp[4];
    const int64_t g = blockIdx.x;
    const int32_t base = graph_ptr[g];
    const int n = graph_ptr[g + 1] - base;
    if (n <= 64 || n > TOPK_MAX_LEN) return;   // the wave kernel's / the long route's; uniform over the workgroup
    const int32_t obase = out_ptr[g];
    const int k = out_ptr[g + 1] - obase;
    for (int i = threadIdx.x; i < n; i += 256) s_key[i] = desc_key(score, (int64_t)base + i);
    __syncthreads();
    // the low bits of a widened 16-bit float are zero, so in the complemented image they are all ones for a score >= 0 and all zeros
    // for a negative one: keys of different sign differ in the top bit already and keys of one sign share their low bits, so the
    // passes over those bits would move nothing
    constexpr int FIRST = sizeof(T) == 4 ? 0 : (std::is_same<T, __half>::value ? 8 : 16);
    int cur = 0;
#pragma unroll 1
    for (int shift = FIRST; shift < 32; shift += 8) {
        const uint32_t* in = s_idx[cur];
        const bool first = shift == FIRST;
        ldssort::sort_chunk<256, TOPK_ROUNDS, false>(
            n,
            [&](int i) {
                const uint32_t id = first ? (uint32_t)i : in[i];
                return ldssort::Item{(s_key[id] >> shift) & 255u, id};
            },
            s_idx[cur ^ 1], s_whist, s_rowptr, s_tmp);
        __syncthreads();
        cur ^= 1;
    }
    for (int r = threadIdx.x; r < k; r += 256) perm[(int64_t)obase + r] = (int64_t)base + s_idx[cur][r];
}

// ---- long route ----
__device__ inline int64_t last_not_above(const int32_t* __restrict__ ptr, int64_t G, int64_t x) {   // last g in [0, G) with ptr[g] <= x
    int64_t lo = 0, hi = G;   // ptr[0] = 0 <= x
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)ptr[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}
template <typename T>
__global__ void topk_long_keys_kernel(const T* __restrict__ score, const int32_t* __restrict__ graph_ptr, int64_t G, int64_t N,
                                      int64_t* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = last_not_above(graph_ptr, G, i);
        keys[i] = (int64_t)(((uint64_t)g << 32) | (uint64_t)desc_key(score, i));
    }
}
// only_above: graphs of at most that many nodes are left to the on-chip kernels (0: this pass writes every graph)
__global__ void topk_long_select_kernel(const int64_t* __restrict__ order, const int32_t* __restrict__ graph_ptr,
                                        const int32_t* __restrict__ out_ptr, int64_t G, int only_above, int64_t* __restrict__ perm) {
    const int64_t total = out_ptr[G];
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = last_not_above(out_ptr, G, j);
        if (graph_ptr[g + 1] - graph_ptr[g] <= only_above) continue;
        perm[j] = order[(int64_t)graph_ptr[g] + (j - out_ptr[g])];
    }
}

struct LongLayout { size_t keys, sorted, order, sort_ws, sort_bytes, total; };
inline LongLayout long_layout(int64_t N) {
    LongLayout l;
    const size_t a = gnnops_align_up((size_t)N * 8, 256);
    l.keys = 0; l.sorted = a; l.order = 2 * a; l.sort_ws = 3 * a;
    l.sort_bytes = gnnops_sort_workspace_bytes(1, N, 1, 4);
    l.total = l.sort_ws + l.sort_bytes;
    return l;
}

template <typename T>
int topk_typed(const void* score, const int32_t* graph_ptr, const int32_t* out_ptr, int64_t* perm, int64_t G, int64_t N,
               int64_t max_graph_len, bool on_chip, bool mixed, void* ws, hipStream_t stream) {
    if (on_chip || mixed) {
        hipLaunchKernelGGL((topk_wave_kernel<T>), dim3((unsigned)gnnops_cdiv(G, 4)), dim3(256), 0, stream, (const T*)score, graph_ptr,
                           out_ptr, perm, G);
        if (max_graph_len > 64)
            hipLaunchKernelGGL((topk_block_kernel<T>), dim3((unsigned)G), dim3(256), 0, stream, (const T*)score, graph_ptr, out_ptr, perm);
        if (on_chip) return gnnops_check_launch("segment_topk (on-chip)");
    }
    const LongLayout l = long_layout(N);
    char* p = (char*)ws;
    int64_t* keys = (int64_t*)(p + l.keys);
    int64_t* order = (int64_t*)(p + l.order);
    hipLaunchKernelGGL((topk_long_keys_kernel<T>), dim3(gnnops_grid_cap(gnnops_cdiv(N, 256))), dim3(256), 0, stream, (const T*)score,
                       graph_ptr, G, N, keys);
    if (int rc = gnnops_sort(keys, p + l.sorted, order, 1, N, 1, 4 /* int64 */, 0, p + l.sort_ws, l.sort_bytes, (gnnops_stream_t)stream))
        return rc;
    hipLaunchKernelGGL(topk_long_select_kernel, dim3(gnnops_grid_cap(gnnops_cdiv(N, 256))), dim3(256), 0, stream, order, graph_ptr,
                       out_ptr, G, mixed ? TOPK_MAX_LEN : 0, perm);
    return gnnops_check_launch("segment_topk (long)");
}

// ---- node map ----
__global__ void node_map_kernel(const int64_t* __restrict__ perm, int64_t k, int32_t* __restrict__ node_map) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (int64_t)gridDim.x * blockDim.x)
        node_map[perm[i]] = (int32_t)i;
}

// ---- filter_edges ----
struct Endpoints { int64_t r, c; bool keep; };
__device__ inline Endpoints mapped(const int64_t* __restrict__ row, const int64_t* __restrict__ col, const int32_t* __restrict__ node_map,
                                   int64_t e, int64_t E, int drop_self_loops) {
    Endpoints p = {0, 0, false};
    if (e < E) {
        p.r = row[e]; p.c = col[e];
        if (node_map) { p.r = node_map[p.r]; p.c = node_map[p.c]; }
        p.keep = p.r >= 0 && p.c >= 0 && !(drop_self_loops && p.r == p.c);
    }
    return p;
}

__global__ __launch_bounds__(256) void filter_count_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                            const int32_t* __restrict__ node_map, int64_t E, int drop_self_loops,
                                                            uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t s_wave[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * FILTER_TILE + wave * 256;
    uint32_t n = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) n += (uint32_t)__popcll(__ballot(mapped(row, col, node_map, base + r * 64 + lane, E, drop_self_loops).keep));
    if (lane == 0) s_wave[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// exclusive scan of the tile counts in place, one workgroup; *d_count = the number of survivors
__global__ __launch_bounds__(256) void filter_scan_kernel(uint32_t* __restrict__ tile_count, int64_t tiles, int64_t* __restrict__ d_count) {
    __shared__ uint32_t s_tmp[4];
    uint32_t carry = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += 256) {
        const int64_t t = t0 + threadIdx.x;
        const uint32_t c = t < tiles ? tile_count[t] : 0u;
        uint32_t total;
        const uint32_t off = block_excl_scan_u32<4>(c, s_tmp, &total);
        if (t < tiles) tile_count[t] = carry + off;
        carry += total;
    }
    if (threadIdx.x == 0) *d_count = (int64_t)carry;
}

template <typename U>
__device__ inline void copy_row(const char* __restrict__ src, char* __restrict__ dst, int64_t bytes) {
    const U* s = reinterpret_cast<const U*>(src);
    U* d = reinterpret_cast<U*>(dst);
    for (int64_t i = 0; i < bytes / (int64_t)sizeof(U); ++i) d[i] = s[i];
}

// UNIT: bytes per access of a value row (16 where the rows allow it)
template <int UNIT>
__global__ __launch_bounds__(256) void filter_write_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                            const char* __restrict__ value, int64_t row_bytes,
                                                            const int32_t* __restrict__ node_map, int64_t E, int drop_self_loops,
                                                            const uint32_t* __restrict__ tile_offset, int64_t* __restrict__ out_row,
                                                            int64_t* __restrict__ out_col, char* __restrict__ out_value) {
    __shared__ uint32_t s_wave[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * FILTER_TILE + wave * 256;
    const uint64_t below = ldssort::lanes_below(lane);
    Endpoints p[4];
    uint32_t rank[4], n = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        p[r] = mapped(row, col, node_map, base + r * 64 + lane, E, drop_self_loops);
        const uint64_t b = __ballot(p[r].keep);
        rank[r] = n + (uint32_t)__popcll(b & below);
        n += (uint32_t)__popcll(b);
    }
    if (lane == 0) s_wave[wave] = n;
    __syncthreads();
    uint32_t off = tile_offset[blockIdx.x];
    for (int w = 0; w < wave; ++w) off += s_wave[w];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (!p[r].keep) continue;
        const int64_t o = (int64_t)off + rank[r];
        out_row[o] = p[r].r;
        out_col[o] = p[r].c;
        if (value) {
            const char* s = value + (base + r * 64 + lane) * row_bytes;
            char* d = out_value + o * row_bytes;
            if constexpr (UNIT == 16) copy_row<u32x4>(s, d, row_bytes);
            else if constexpr (UNIT == 8) copy_row<uint2>(s, d, row_bytes);
            else if constexpr (UNIT == 4) copy_row<uint32_t>(s, d, row_bytes);
            else copy_row<uint16_t>(s, d, row_bytes);
        }
    }
}

}  // namespace

extern "C" int64_t gnnops_segment_topk_max_len(void) { return TOPK_MAX_LEN; }

extern "C" int gnnops_segment_topk_counts(const int32_t* graph_ptr, int64_t G, float ratio, int64_t k, int32_t* out_ptr,
                                          int64_t* d_info, gnnops_stream_t s) {
    GNNOPS_REQUIRE(G >= 0 && G < ((int64_t)1 << 31), GNNOPS_EINVAL, "segment_topk_counts: G = %lld", (long long)G);
    GNNOPS_REQUIRE(graph_ptr && out_ptr && d_info, GNNOPS_EINVAL, "segment_topk_counts: null pointer");
    GNNOPS_REQUIRE(k >= 1 || (ratio > 0.f && ratio <= 1.f), GNNOPS_EINVAL,
                   "segment_topk_counts: needs an integer k >= 1 or a ratio in (0, 1] (got k = %lld, ratio = %g)", (long long)k, (double)ratio);
    hipLaunchKernelGGL(topk_counts_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, graph_ptr, G, ratio, k, out_ptr, d_info);
    return gnnops_check_launch("segment_topk_counts");
}

extern "C" size_t gnnops_segment_topk_workspace_bytes(int64_t N, int64_t max_graph_len, int route) {
    if (N <= 0) return 0;
    const bool on_chip = route == 1 || (route == 0 && max_graph_len <= TOPK_MAX_LEN);
    return on_chip ? 0 : long_layout(N).total;
}

extern "C" int gnnops_segment_topk(const void* score, const int32_t* graph_ptr, const int32_t* out_ptr, int64_t* perm, int64_t G,
                                   int64_t N, int64_t max_graph_len, int dtype, int route, void* workspace, size_t workspace_bytes,
                                   gnnops_stream_t s) {
    GNNOPS_REQUIRE(G >= 0 && N >= 0 && G < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), GNNOPS_EINVAL,
                   "segment_topk: G = %lld, N = %lld (both below 2^31)", (long long)G, (long long)N);
    GNNOPS_REQUIRE(route >= 0 && route <= 2, GNNOPS_EINVAL, "segment_topk: route %d (0 auto, 1 on-chip, 2 long)", route);
    GNNOPS_REQUIRE(dtype >= GNNOPS_F32 && dtype <= GNNOPS_BF16, GNNOPS_EUNSUPPORTED, "segment_topk: dtype code %d", dtype);
    GNNOPS_REQUIRE(!(route == 1 && max_graph_len > TOPK_MAX_LEN), GNNOPS_EINVAL,
                   "segment_topk: the on-chip route holds graphs of up to %d nodes (got %lld)", TOPK_MAX_LEN, (long long)max_graph_len);
    if (G == 0 || N == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(score && graph_ptr && out_ptr && perm, GNNOPS_EINVAL, "segment_topk: null pointer");
    const bool on_chip = route == 1 || (route == 0 && max_graph_len <= TOPK_MAX_LEN);
    const size_t need = gnnops_segment_topk_workspace_bytes(N, max_graph_len, route);
    GNNOPS_REQUIRE(on_chip || (workspace && workspace_bytes >= need), GNNOPS_EWORKSPACE, "segment_topk: workspace %zu < %zu",
                   workspace_bytes, need);
    hipStream_t stream = (hipStream_t)s;
    return gnnops_with_dtype(dtype, "segment_topk", [&](auto t) {
        return topk_typed<typename decltype(t)::type>(score, graph_ptr, out_ptr, perm, G, N, max_graph_len, on_chip, route == 0 && !on_chip,
                                                      workspace, stream);
    });
}

extern "C" int gnnops_node_map(const int64_t* perm, int64_t k, int64_t N, int32_t* node_map, gnnops_stream_t s) {
    GNNOPS_REQUIRE(k >= 0 && N >= 0 && N < ((int64_t)1 << 31) && k <= N, GNNOPS_EINVAL, "node_map: k = %lld, N = %lld", (long long)k, (long long)N);
    if (N == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(node_map && (perm || k == 0), GNNOPS_EINVAL, "node_map: null pointer");
    hipStream_t stream = (hipStream_t)s;
    if (gnnops_memset_async(node_map, 0xff, (size_t)N * 4, stream) != hipSuccess) return gnnops_check_launch("node_map clear");
    if (k) hipLaunchKernelGGL(node_map_kernel, dim3(gnnops_grid_cap(gnnops_cdiv(k, 256))), dim3(256), 0, stream, perm, k, node_map);
    return gnnops_check_launch("node_map");
}

extern "C" int64_t gnnops_filter_edges_tile(void) { return FILTER_TILE; }

extern "C" size_t gnnops_filter_edges_workspace_bytes(int64_t E) {
    return E <= 0 ? 0 : gnnops_align_up((size_t)gnnops_cdiv(E, FILTER_TILE) * 4, 256);
}

extern "C" int gnnops_filter_edges(const int64_t* row, const int64_t* col, const void* value, int64_t value_row_bytes,
                                   const int32_t* node_map, int64_t E, int drop_self_loops, int64_t* out_row, int64_t* out_col,
                                   void* out_value, int64_t* d_count, void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    hipStream_t stream = (hipStream_t)s;
    GNNOPS_REQUIRE(E >= 0 && E < ((int64_t)1 << 32) - FILTER_TILE, GNNOPS_EUNSUPPORTED, "filter_edges: E = %lld (below 2^32)", (long long)E);
    GNNOPS_REQUIRE(d_count, GNNOPS_EINVAL, "filter_edges: null count");
    GNNOPS_REQUIRE(!value || (value_row_bytes > 0 && value_row_bytes % 2 == 0 && out_value), GNNOPS_EINVAL,
                   "filter_edges: a value needs an output and rows of an even number of bytes (got %lld)", (long long)value_row_bytes);
    if (E == 0) {
        if (gnnops_memset_async(d_count, 0, 8, stream) != hipSuccess) return gnnops_check_launch("filter_edges clear");
        return gnnops_check_launch("filter_edges");
    }
    GNNOPS_REQUIRE(row && col && out_row && out_col, GNNOPS_EINVAL, "filter_edges: null pointer");
    GNNOPS_REQUIRE(workspace && workspace_bytes >= gnnops_filter_edges_workspace_bytes(E), GNNOPS_EWORKSPACE,
                   "filter_edges: workspace %zu < %zu", workspace_bytes, gnnops_filter_edges_workspace_bytes(E));
    const int64_t tiles = gnnops_cdiv(E, FILTER_TILE);
    uint32_t* tile_count = (uint32_t*)workspace;
    hipLaunchKernelGGL(filter_count_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, row, col, node_map, E, drop_self_loops, tile_count);
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(256), 0, stream, tile_count, tiles, d_count);
    const uintptr_t align = value ? ((uintptr_t)value | (uintptr_t)out_value | (uintptr_t)value_row_bytes) : 0;
#define FILTER_WRITE(UNIT)                                                                                                        \
    hipLaunchKernelGGL((filter_write_kernel<UNIT>), dim3((unsigned)tiles), dim3(256), 0, stream, row, col, (const char*)value,   \
                       value_row_bytes, node_map, E, drop_self_loops, tile_count, out_row, out_col, (char*)out_value)
    if (align % 16 == 0) FILTER_WRITE(16);
    else if (align % 8 == 0) FILTER_WRITE(8);
    else if (align % 4 == 0) FILTER_WRITE(4);
    else FILTER_WRITE(2);
#undef FILTER_WRITE
    return gnnops_check_launch("filter_edges");
}
