/*
 * gnnops.h — C ABI of the MI355X (gfx950) operator library behind the gnn-ops-benchmark op API.
 *
 * This is the drop-in boundary. The reference (ryienh/gnn-ops-benchmark) has no FFI of its own:
 * its hot path is the body of each `op_*` function in op_bm_scripts/benchmark_*.py, which calls a
 * third-party CUDA op (torch_scatter / torch_sparse / ATen). Each entry point below replaces ONE such
 * call; the reference call site it stands behind is cited as (file:line under the reference root).
 *
 * Conventions
 *   - Plain pointers and sizes only. Every pointer is a DEVICE pointer unless marked "host".
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream). All work is enqueued on it;
 *     nothing here synchronises the device, allocates device memory or retains a pointer after return.
 *   - Tensors are viewed around the reduced/indexed dimension as [B, E, K] (source side) and [B, N, K]
 *     (destination side): B = product of sizes before `dim`, K = product of sizes after it.
 *     A 2-D [E, D] tensor indexed along dim 0 is B=1, K=D; along dim 1 it is B=E', K=1.
 *   - `index` is int64 as in the reference (benchmark_scatter_add.py:78-84). Layout R = one index per
 *     position along E (1-D row index, broadcast over B and K). Layout F = index of the full [B,E,K]
 *     shape (what the reference scripts build).
 *   - dtype codes: GNNOPS_F32/F16/BF16. 16-bit types are accumulated in fp32 and rounded once.
 *   - Return value: 0 on success, a GNNOPS_E* code otherwise; gnnops_last_error() gives the text
 *     (thread-local). Functions never throw and never call exit().
 */
#ifndef GNNOPS_H
#define GNNOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNOPS_ABI_VERSION 3   /* 2: gnnops_narrow_index takes the id bound; round-2 exports (layers, spline, cluster)
                                * 3: one entry point per attention pass, optional operands NULL (the _u / _v1_c names are gone) */

enum gnnops_status {
    GNNOPS_OK = 0,
    GNNOPS_EINVAL = 1,    /* bad argument (shape, dtype, alignment, null pointer) */
    GNNOPS_EWORKSPACE = 2,/* workspace too small */
    GNNOPS_ELAUNCH = 3,   /* hipGetLastError() after a launch */
    GNNOPS_EUNSUPPORTED = 4
};

enum gnnops_dtype { GNNOPS_F32 = 0, GNNOPS_F16 = 1, GNNOPS_BF16 = 2 };

/* torch_scatter reduce names: scatter_add/scatter_sum, scatter_mean, scatter_min, scatter_max, scatter_mul */
enum gnnops_reduce { GNNOPS_SUM = 0, GNNOPS_MEAN = 1, GNNOPS_MIN = 2, GNNOPS_MAX = 3, GNNOPS_MUL = 4 };

typedef void* gnnops_stream_t;

int gnnops_version(void);
const char* gnnops_last_error(void);

/* Measurement aid for bench.py's roofline leg (no reference counterpart): `reads` sequential nontemporal read streams of
 * `pieces` 16-B pieces each (src holds reads * pieces pieces) combined into ONE nontemporal write stream (dst: `pieces`
 * pieces, or NULL for reads only). The rate of the 5 : 1 mix is what the memory system offers the config-2 segment
 * reduction (5 source rows and the index per output row) on the box at hand. */
int gnnops_diag_stream_mix(const void* src, void* dst, int64_t pieces, int reads, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * dim_size discovery. torch_scatter computes `int(index.max()) + 1` when dim_size is None
 * (behind benchmark_scatter_add.py:18, benchmark_scatter_min.py:17). Writes max(index) (or -1 when
 * E == 0) to *d_max (device int64). The caller decides when to read it back.
 * ------------------------------------------------------------------------------------------- */
int gnnops_index_max(const int64_t* index, int64_t E, int64_t* d_max, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Inverted index ("plan") of a destination index: a stable counting sort of index[0..E) by value.
 *   rowptr[n] .. rowptr[n+1]  = range of `perm` holding the positions e with index[e] == n,
 *   in ascending e (stable) — so a per-destination sequential reduction visits contributions in the
 *   same order as a sequential CPU loop over e.
 * rowptr: int32[N+1], perm: int32[E] (E < 2^31). index values must lie in [0, N).
 * Shared by scatter_* / index_add_ (segment reduce), index_select (push form), spmm (COO->CSR),
 * coalesce and sparse transpose.
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_plan_workspace_bytes(int64_t E, int64_t N);
int gnnops_plan_build(const int64_t* index, int64_t E, int64_t N,
                      int32_t* rowptr, int32_t* perm,
                      void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* The same plan in ONE launch for small inputs (gnnops_plan_small_fits(E, N) != 0: E <= 24576 positions, N <= 40000
 * destinations — a batch of small graphs, app_bm/benchmark_convs.py): one workgroup, counters in LDS, stable. `companion`
 * (optional, int64 [E], e.g. the edge list's source row) comes back in plan order as col [E] from the same launch. */
int gnnops_plan_small_fits(int64_t E, int64_t N);
int gnnops_plan_build_small(const int64_t* index, const int64_t* companion, int64_t E, int64_t N, int32_t* rowptr,
                            int32_t* perm, int64_t* col, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Segment reduce over a plan — the kernel behind, with layout R:
 *   torch_scatter.scatter_add / scatter_mean / scatter_min / scatter_max / scatter_mul
 *     (benchmark_scatter_add.py:15-19, benchmark_scatter_mean.py:15-18,
 *      benchmark_scatter_min.py:15-18, benchmark_scatter_max.py:15-18), and
 *   Tensor.index_add_ (benchmark_native_index_add_.py:13-16) when init_from_out != 0.
 * src [B,E,K] -> out [B,N,K].  out[b,n,k] = reduce over e in segment n of src[b,e,k].
 *   init_from_out == 0 : out is overwritten; empty segments give 0 (SUM/MEAN/MIN/MAX) or 1 (MUL).
 *   init_from_out != 0 : the reduction starts from the current out[b,n,k] (index_add_, `out=` given);
 *                        MIN/MAX keep out where no contribution beats it; MEAN is not allowed.
 * arg_out (MIN/MAX only, may be NULL): int64 [B,N,K]; position e of the first extremal contribution,
 *   E where the segment is empty (torch_scatter's convention).
 * ------------------------------------------------------------------------------------------- */
int gnnops_segment_reduce(const void* src, const int32_t* rowptr, const int32_t* perm,
                          void* out, int64_t* arg_out,
                          int64_t B, int64_t E, int64_t K, int64_t N,
                          int dtype, int reduce, int init_from_out, gnnops_stream_t stream);
/* The same with heavy destinations ("hubs": more than 8192 contributions) set aside and reduced piecewise by whole
 * workgroups instead of serially by one lane group (csrc/hub.h; B == 1, rows of whole 16-B lanes). min / max stay exact;
 * sums / means / products of a hub are re-associated (deterministic, not bit-identical to the sequential loop).
 * hub_workspace: gnnops_hub_workspace_bytes(E, K, reduce) bytes, or NULL for the plain form. */
size_t gnnops_hub_workspace_bytes(int64_t E, int64_t K, int reduce);
int gnnops_segment_reduce_hubs(const void* src, const int32_t* rowptr, const int32_t* perm,
                               void* out, int64_t* arg_out,
                               int64_t B, int64_t E, int64_t K, int64_t N,
                               int dtype, int reduce, int init_from_out,
                               void* hub_workspace, size_t hub_workspace_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One-shot row scatter — the same reference call sites as gnnops_segment_reduce (layout R, B == 1), for
 * a call that has no plan to reuse: src [E,K], index [E] int64 in [0,N), out [N,K] (arg_out as above).
 * Equivalent to gnnops_plan_build + gnnops_segment_reduce (same order of operations, bit-identical
 * results) but the last radix pass, the row-pointer kernel and the perm/rowptr round trip through HBM
 * are folded into the reduction (bucket.hip). Returns GNNOPS_EUNSUPPORTED — take the plan path — when
 * K * elem is not a whole number of 16-B lanes, pointers are not 16-B aligned, N <= 256, E == 0, or
 * E / N >= 2^31.
 * ------------------------------------------------------------------------------------------- */
int gnnops_scatter_rows_oneshot(const void* src, const int64_t* index, void* out, int64_t* arg_out,
                                int64_t E, int64_t K, int64_t N, int dtype, int reduce, int init_from_out,
                                void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* The two stages separately: gnnops_bucket_partition groups the E positions by bucket = index >> 8 (stable) into the
 * workspace — which then is a reusable, coarser plan — and gnnops_bucket_reduce runs the reduction from it (the on-chip
 * finish of the sort is repeated per call; the indices never travel through HBM as rowptr / perm). */
size_t gnnops_bucket_workspace_bytes(int64_t E, int64_t N);
int gnnops_bucket_partition(const int64_t* index, int64_t E, int64_t N, void* workspace, size_t workspace_bytes,
                            gnnops_stream_t stream);
/* Windowed partition (the per-GPU step of the destination-partitioned scatter, BASELINE config 5): positions with
 * index[e] in [lo, lo+N) are partitioned under the local id index[e]-lo; the others are set aside in position order
 * behind the last bucket (pairs bptr[NB] .. E of the layout) and are ignored by reduce / select. */
int gnnops_bucket_partition_window(const int64_t* index, int64_t E, int64_t lo, int64_t N, void* workspace,
                                   size_t workspace_bytes, gnnops_stream_t stream);
/* Byte offsets inside a partitioned workspace: keys u32[E] (local id, sentinel ceil(N/256)*256 for set-aside positions),
 * positions u32[E], bptr int32[ceil(N/256)+1]. Host-only, no device work. */
int gnnops_bucket_layout(int64_t E, int64_t N, size_t* keys_offset, size_t* vals_offset, size_t* bptr_offset);
int gnnops_bucket_reduce(const void* src, const void* workspace, void* out, int64_t* arg_out,
                         int64_t E, int64_t K, int64_t N, int dtype, int reduce, int init_from_out,
                         gnnops_stream_t stream);
/* gnnops_bucket_reduce with hubs set aside, as gnnops_segment_reduce_hubs (hub_workspace: gnnops_hub_workspace_bytes). */
int gnnops_bucket_reduce_hubs(const void* src, const void* workspace, void* out, int64_t* arg_out,
                              int64_t E, int64_t K, int64_t N, int dtype, int reduce, int init_from_out,
                              void* hub_workspace, size_t hub_workspace_bytes, gnnops_stream_t stream);
/* torch.index_select(input [N,K], 0, index [E]) -> out [E,K] (benchmark_native_index_select.py:14), push form, from a
 * workspace gnnops_bucket_partition filled for (index, E, N): each selected input row is read once and stored to every
 * output row that selects it. Rows must be a multiple of 16 bytes and 16-B aligned. */
int gnnops_bucket_select(const void* input, const void* workspace, void* out, int64_t N, int64_t K, int64_t E,
                         int elem_bytes, gnnops_stream_t stream);
/* Push-form index_select with hot rows (selected by more than 8192 outputs) set aside and written by whole workgroups
 * instead of one lane group (csrc/hub.h): hub_workspace = gnnops_hub_workspace_bytes(E, 0, 0) bytes, or NULL. */
int gnnops_bucket_select_hubs(const void* input, const void* workspace, void* out, int64_t N, int64_t K, int64_t E,
                              int elem_bytes, void* hub_workspace, size_t hub_workspace_bytes, gnnops_stream_t stream);
int gnnops_index_select_planned_hubs(const void* input, const int32_t* rowptr, const int32_t* perm, void* out,
                                     int64_t B, int64_t N, int64_t K, int64_t E, int elem_bytes,
                                     void* hub_workspace, size_t hub_workspace_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Element-wise scatter, layout F (index has the shape of src) — what the reference scripts build
 * (benchmark_scatter_add.py:67,78-84; native form `zeros_like(src).scatter_add_(dim, idx, src)`
 * benchmark_scatter_add.py:22-25; `scatter_(-1, idx, src, reduce="multiply")`
 * benchmark_scatter_multiply.py:42-45).  out[b, index[b,e,k], k] (op)= src[b,e,k].
 *   init_from_out == 0 : the call initialises out itself (0 / identity) and, for MIN/MAX, sets groups
 *                        nothing reached to 0 (needs arg_out); MEAN divides by max(count, 1).
 *   init_from_out != 0 : contributions are combined into the existing out (`out=` / in-place forms).
 * The memory-side-atomic form of SUM/MEAN/MUL on 16-bit types uses an fp32 scratch of B*N*K floats in
 * `workspace` (MEAN: one more for the counts), and its MIN/MAX is a value pass, then an arg pass choosing
 * the smallest e among ties. The LDS-strip forms use no workspace and are ONE pass: a min / max cell holds
 * the value's order image and the position together, so the extremum and its smallest position come out of
 * the same sweep. An id outside [0, N) is dropped by the LDS-strip forms; the atomic form does not look at
 * ids, so every id must lie in [0, N) there. gnnops_scatter_elementwise_route tells which form takes a call.
 * MIN/MAX in every form: the sequential loop's result — a contribution replaces on a strict improvement only, so out
 * (init_from_out) wins a tie and keeps arg = E, the smallest position wins among contributions, and a zero extremum has
 * the sign of the element arg names (-0.0 == +0.0). The atomic form needs arg_out for that last point: with
 * arg_out == NULL (init_from_out only) the sign of a zero extremum is that of any of the tied zeros.
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_scatter_elementwise_workspace_bytes(int64_t B, int64_t N, int64_t K, int dtype, int reduce);
int gnnops_scatter_elementwise(const void* src, const int64_t* index, void* out, int64_t* arg_out,
                               int64_t B, int64_t E, int64_t K, int64_t N,
                               int dtype, int reduce, int init_from_out,
                               void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* The same with the index stored in `index_bytes` bytes per element: 8 (int64, what the reference builds), 4 (int32) or 2
 * (uint16, N <= 65536) — SURVEY.md 8(f) rank 2: at the reference's layout-F shapes (benchmark_scatter_add.py:78-84) the
 * int64 index is 8 of every 10 bytes the op reads; a narrowed copy (gnnops_narrow_index) is made once per index tensor and
 * reused. A narrowed index is taken by the LDS-strip form only: GNNOPS_EUNSUPPORTED otherwise (pass the int64 index). */
int gnnops_scatter_elementwise_ix(const void* src, const void* index, int index_bytes, void* out, int64_t* arg_out,
                                  int64_t B, int64_t E, int64_t K, int64_t N, int dtype, int reduce, int init_from_out,
                                  void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* The same with the arg rows of min / max stored as int32 (arg_bytes 4; E < 2^31; the LDS-strip form only, GNNOPS_EUNSUPPORTED
 * otherwise) or int64 (arg_bytes 8 = gnnops_scatter_elementwise_ix): the dim-0 route of large full-index scatters
 * (data/scatter_max.csv:32-33, (38000, 38000)) reduces along the last dim of TRANSPOSED operands and widens the positions inside
 * the transpose back (gnnops_transpose2d_cvt), so neither the int64 index nor an int64 arg crosses a transpose. */
int gnnops_scatter_elementwise_ixa(const void* src, const void* index, int index_bytes, void* out, void* arg_out, int arg_bytes,
                                   int64_t B, int64_t E, int64_t K, int64_t N, int dtype, int reduce, int init_from_out,
                                   void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* out[i] = (int32 / uint16) index[i], i < n, for ids in [0, bound); an id outside becomes all ones (-1 / 0xFFFF — never a valid
 * id: bound <= 65535 for out_bytes 2, < 2^31 for 4), which the element kernels drop as they drop it in the int64 index. */
int gnnops_narrow_index(const int64_t* index, void* out, int64_t n, int out_bytes, int64_t bound, gnnops_stream_t stream);

/* Route query of the element-wise scatter (host only, no device is touched): the form gnnops_scatter_elementwise_ixa
 * launches for these arguments — it calls the same function and launches what it says, so the thresholds exist there only.
 * `src_addr` / `index_addr` are the base addresses (only their low four bits matter). Returns
 *   GNNOPS_ROUTE_LDS         one LDS strip of all N destinations per (b, column strip)
 *   GNNOPS_ROUTE_LDS_CHUNKS  the destinations cut into nchunks (2 .. 16) chunks of `rows`; each re-scans the strip's source
 *   GNNOPS_ROUTE_ATOMICS     memory-side atomics (int64 index and int64 arg rows only)
 *   GNNOPS_ROUTE_NONE        nothing is launched: B*N*K == 0, an argument the entry point refuses (GNNOPS_EINVAL), or a
 *                            narrowed index / int32 arg on a shape the LDS forms do not take (GNNOPS_EUNSUPPORTED)
 * and fills detail[0..7] (may be NULL):
 *   [0] tc       columns per strip                     [4] cell_bytes  LDS bytes per destination and column (4 or 8)
 *   [1] rows     destinations per chunk (N: one chunk) [5] tshift      2^tshift >= tc lanes per source row
 *   [2] nchunks                                        [6] grid        workgroups: B * ceil(K / tc) * nchunks
 *   [3] threads  per workgroup (256 / 512 / 1024)      [7] flags       bit 0: K == 1 fp32, four elements per lane and load
 * ATOMICS: threads = 256, grid = that of the launches over the source, cell_bytes as the LDS forms would have had; the rest 0.
 * NONE: all 0. */
int gnnops_scatter_elementwise_route(int64_t B, int64_t E, int64_t K, int64_t N, int dtype, int reduce, int index_bytes,
                                     int arg_bytes, uintptr_t src_addr, uintptr_t index_addr, int64_t* detail);

/* torch_scatter.scatter_min / scatter_max of a LONG 1-D tensor (benchmark_scatter_min.py:15-18 at the reference's ">= 95 % of
 * memory" shapes, data/scatter_min.csv:2: 1 472 353 280 fp32 elements): src [E], index [E] int64, out [N], arg_out [N] int64.
 * The value travels with its destination through radix passes over the destination bits above the low 15, and a workgroup
 * finishes each bucket of 32768 destinations in LDS (csrc/scatter1d.hip) — no complete sort, no random gather. Same result
 * as gnnops_segment_reduce (out 0 / arg E where nothing arrives, smallest position on ties, NaNs and the reduce's identity
 * never win). GNNOPS_EUNSUPPORTED unless 32768 < N < 2^31 - 32768 and 0 < E < 2^31 and reduce is MIN or MAX. */
size_t gnnops_scatter1d_workspace_bytes(int64_t E, int64_t N);
int gnnops_scatter1d_minmax(const void* src, const int64_t* index, void* out, int64_t* arg_out, int64_t E, int64_t N,
                            int dtype, int reduce, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* The same shapes for reduce SUM / MEAN / MUL (benchmark_scatter_mean.py:15-18 at data/scatter_mean.csv:2): three passes to buckets
 * of 256 destinations, finished by a stable on-chip sort and a sum in source position order — bit-identical to the sequential
 * loop (16-bit types: fp32 accumulator, rounded once). Same workspace and shape limits as gnnops_scatter1d_minmax. */
int gnnops_scatter1d_sum(const void* src, const int64_t* index, void* out, int64_t E, int64_t N, int dtype, int reduce,
                         void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch.index_select (benchmark_native_index_select.py:12-15; also the first half of
 * benchmark_fused_index_select_reduce.py:12-20).  input [B,N,K], index int64 [E] -> out [B,E,K],
 * out[b,e,k] = input[b,index[e],k].  Bit-exact copy of opaque elements; `elem_bytes` in {1,2,4,8}.
 * ------------------------------------------------------------------------------------------- */
int gnnops_index_select(const void* input, const int64_t* index, void* out,
                        int64_t B, int64_t N, int64_t K, int64_t E,
                        int elem_bytes, gnnops_stream_t stream);

/* Push form of the same op over a plan of `index` (each input row is read once and stored to every
 * output row that selects it). Same result, different HBM traffic; see DESIGN.md. */
int gnnops_index_select_planned(const void* input, const int32_t* rowptr, const int32_t* perm, void* out,
                                int64_t B, int64_t N, int64_t K, int64_t E,
                                int elem_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch.gather (benchmark_native_gather.py:14-17). input [B,N,K], index int64 [B,E,K] ->
 * out[b,e,k] = input[b, index[b,e,k], k]. Bit-exact copy.
 * ------------------------------------------------------------------------------------------- */
int gnnops_gather(const void* input, const int64_t* index, void* out,
                  int64_t B, int64_t N, int64_t K, int64_t E,
                  int elem_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused index_select + full sum (benchmark_fused_index_select_reduce.py:12-20):
 *   *d_sum_f32 = sum_{b,e,k} input[b,index[e],k], accumulated in fp32 (the reference's fp16 result
 *   overflows to inf at its own sizes; the fp32 accumulator is the comparable quantity).
 * The [B,E,K] intermediate is never written. Deterministic: per-block partials are combined in a
 * fixed order by a second launch. workspace: gnnops_fused_select_sum_workspace_bytes().
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_fused_select_sum_workspace_bytes(void);
int gnnops_fused_index_select_sum(const void* input, const int64_t* index, float* d_sum_f32,
                                  int64_t B, int64_t N, int64_t K, int64_t E,
                                  int dtype, void* workspace, size_t workspace_bytes,
                                  gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Route queries (host only, no device is touched): which kernel the three entry points above launch
 * for a shape and base alignment, and with what geometry. The entry points call these and switch on
 * the result, so the thresholds exist here only. `input_addr` / `out_addr` are the base addresses
 * (only their low four bits matter). Returns a gnnops_route code, GNNOPS_ROUTE_NONE when nothing is
 * launched (an empty result, an elem_bytes / dtype the entry point refuses), and fills detail[0..3]
 * (may be NULL):
 *   ROWS      gshift (2^gshift lanes per row), chunks, flags, grid.
 *             flags bit 0: a full workgroup step takes the straight-line "whole" form.
 *             flags bit 1 (fused sum only): the division-free "simple" form (one matrix, one chunk).
 *   K1        tb (rows parked per workgroup), grid.
 *   LDS       tc (columns per strip), threads, strips, tshift.
 *             Fused sum (one row parked per step): 1, 1024, grid, 0.
 *   LONGROWS  index_select: copy unit in bytes, KU (units per row, saturated at INT_MAX), grid.
 *             Fused sum: PAIR (2 = two 16-bit values per 4-byte load, else 1), K / PAIR, grid.
 *   ELEMS     index_select: copy unit in bytes, KU, grid. gather: elem_bytes, K, grid.
 *             Fused sum: 1, K, grid.
 * ------------------------------------------------------------------------------------------- */
enum gnnops_route {
    GNNOPS_ROUTE_NONE = -1,
    GNNOPS_ROUTE_ROWS = 0,
    GNNOPS_ROUTE_K1 = 1,
    GNNOPS_ROUTE_LDS = 2,
    GNNOPS_ROUTE_LONGROWS = 3,
    GNNOPS_ROUTE_ELEMS = 4,
    GNNOPS_ROUTE_LDS_CHUNKS = 5,   /* gnnops_scatter_elementwise_route only */
    GNNOPS_ROUTE_ATOMICS = 6       /* gnnops_scatter_elementwise_route only */
};
int gnnops_index_select_route(int64_t B, int64_t N, int64_t K, int64_t E, int elem_bytes, uintptr_t input_addr,
                              uintptr_t out_addr, int* detail);
int gnnops_gather_route(int64_t B, int64_t N, int64_t K, int64_t E, int elem_bytes, int* detail);
int gnnops_fused_select_sum_route(int64_t B, int64_t N, int64_t K, int64_t E, int dtype, uintptr_t input_addr,
                                  int* detail);

/* ---------------------------------------------------------------------------------------------
 * torch_sparse.spmm(index, value, m, n, matrix) / torch.sparse.mm(COO, dense)
 * (benchmark_sparse_spmm.py:12-14; BASELINE config 3). Row-split over a CSR view of the sparse operand:
 *   out[i,:] = sum_{j in [rowptr[i], rowptr[i+1])} value[e_j] * mat[col[e_j], :],  e_j = perm ? perm[j] : j
 * so a CSR matrix passes perm = NULL and a COO matrix passes the plan of its row index (rowptr, perm).
 * value == NULL means all ones. mat [mat_rows, D], out [M, D]; fp32 accumulation, one rounding.
 * ------------------------------------------------------------------------------------------- */
int gnnops_spmm(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value,
                const void* mat, void* out, int64_t M, int64_t D, int64_t nnz, int64_t mat_rows, int dtype,
                gnnops_stream_t stream);
/* The same with rows of more than 8192 nonzeros set aside and multiplied out piecewise by whole workgroups (csrc/hub.h;
 * re-associated fp32 sums for those rows only): hub_workspace = gnnops_hub_workspace_bytes(nnz, D, 0) bytes, or NULL. */
int gnnops_spmm_hubs(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value,
                     const void* mat, void* out, int64_t M, int64_t D, int64_t nnz, int64_t mat_rows, int dtype,
                     void* hub_workspace, size_t hub_workspace_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Tiled SpMM: CSR x dense with the rows of `mat` that a block of output rows shares staged in LDS once per block.
 * Same products in the same order as gnnops_spmm(rowptr, NULL, col, ...): the result is bit-identical; what changes is
 * where an operand row is fetched from. Pays on matrices whose neighbouring rows share columns (communities, bands).
 *
 * Tiled SpMM plan (what gnnops.spmm_tiles builds; any caller may build one), for R = block_rows (a power of two) and
 * S = slots (1 .. 1280: a slot holds one 128-byte column chunk of a row of `mat`, S * 128 bytes of LDS per workgroup):
 *   row block b     = rows [b * R, min((b + 1) * R, M)),  nblocks = ceil(M / R)
 *   candidate of b  = a column that at least 2 nonzeros of the block reference (repeats inside one row count)
 *   staged by b     = its S most-referenced candidates, ties to the smaller column id
 *   tile_ptr  int32 [nblocks + 1]   tile_cols[tile_ptr[b] .. tile_ptr[b + 1]) are block b's staged columns
 *   tile_cols int64 [tile_ptr[nblocks]]  staged column ids, ascending within each block
 *   slot      uint16 [nnz]          position of the nonzero's column in its block's staged list, or 0xFFFF if not staged
 * The kernel needs only: tile_ptr[b + 1] - tile_ptr[b] <= S, and slot[e] == 0xFFFF or
 * tile_cols[tile_ptr[b] + slot[e]] == col[e] for every nonzero e of block b. `col` is read for unstaged nonzeros only.
 * No row may hold more than 8192 nonzeros (those belong to gnnops_spmm_hubs). Preconditions, else GNNOPS_EINVAL:
 * D a multiple of 16 bytes / element size, mat and out 16-byte aligned. value == NULL means all ones.
 * Allocates nothing and does not synchronise; one launch on `stream`.
 * ------------------------------------------------------------------------------------------- */
int gnnops_spmm_tiled(const int32_t* rowptr, const int64_t* col, const void* value, const void* mat, void* out,
                      int64_t M, int64_t D, int64_t nnz, int dtype, const int32_t* tile_ptr, const int64_t* tile_cols,
                      const uint16_t* slot, int block_rows, int slots, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch_sparse.matmul(SparseTensor, dense, reduce = "mean" | "min" | "max") (spmm_mean / spmm_min / spmm_max of
 * torch-sparse 0.6.12). Operands as gnnops_spmm; reduce is GNNOPS_MEAN, GNNOPS_MIN or GNNOPS_MAX (the sum is gnnops_spmm).
 *   min / max  out[i,k] = max_j value[e_j] * mat[col[e_j], k] over j in [rowptr[i], rowptr[i+1]),  e_j = perm ? perm[j] : j;
 *              arg[i,k] (int64 [M, D], or NULL) = the winning j, a position in the row-ordered storage (never perm[j]).
 *              fp32 products compared strictly: of equal products the smallest j wins. The winner is rounded once.
 *   mean       the sum of gnnops_spmm (same order and arithmetic) divided in fp32 by max(rowptr[i+1] - rowptr[i], 1).
 * A row without nonzeros: out = 0, arg = nnz. NaN products: see csrc/spmm_reduce.hip. No atomics: reproducible bits.
 * Rows of more than 8192 nonzeros are walked by one lane group (correct, slow). nnz < 2^31 - 8.
 * Allocates nothing and does not synchronise; one launch on `stream`.
 * ------------------------------------------------------------------------------------------- */
int gnnops_spmm_reduce(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const void* value,
                       const void* mat, void* out, int64_t* arg, int64_t M, int64_t D, int64_t nnz, int64_t mat_rows,
                       int reduce, int dtype, gnnops_stream_t stream);
/* The per-element half of the min / max backward, for g = d out [M, D] and a = arg[i,k], e = perm ? perm[a] : a:
 *   dst[i,k] (int64) = col[e],  to_mat[i,k] = round(value[e] * g[i,k]),  to_val[i,k] = round(mat[col[e], k] * g[i,k]);
 *   a outside [0, nnz) (a row without nonzeros) or col[e] outside [0, mat_rows): dst = mat_rows and both terms 0.
 * to_val may be NULL (no value gradient wanted); value == NULL means all ones. d mat is then the scatter-add of to_mat
 * by dst over mat_rows + 1 rows and d value (row order) the scatter-add of to_val by arg over nnz + 1 slots. */
int gnnops_spmm_reduce_grad_terms(const int64_t* arg, const void* g, const int32_t* perm, const int64_t* col,
                                  const void* value, const void* mat, int64_t* dst, void* to_mat, void* to_val,
                                  int64_t M, int64_t D, int64_t nnz, int64_t mat_rows, int dtype, gnnops_stream_t stream);

/* out[j] = in[perm[j]] (elements of 2, 4 or 8 bytes): materialises the CSR column / value arrays of a plan-ordered COO
 * operand once, so gnnops_spmm can be called with perm == NULL and stream them. */
int gnnops_permute(const void* in, const int32_t* perm, void* out, int64_t n, int elem_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch.sort(input, dim, descending, stable) (benchmark_native_sort.py:28-30 times fp32). input viewed
 * [B,E,K], sorted along E; values [B,E,K] of the input dtype, indices int64 [B,E,K] (position along E).
 * Always stable. sort_dtype: 0 f32, 1 f16, 2 bf16, 3 i32, 4 i64, 5 f64 (64-bit types: B*K == 1 only).
 * -0.0 is ordered (and returned) as +0.0; NaNs last (first when descending).
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_sort_workspace_bytes(int64_t B, int64_t E, int64_t K, int sort_dtype);
int gnnops_sort(const void* input, void* values, int64_t* indices, int64_t B, int64_t E, int64_t K,
                int sort_dtype, int descending, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* On-chip form of the same op for fp32 rows that fit in LDS (E <= gnnops_sort_rows_max_len()): input / values
 * [rows, E], indices int64 [rows, E], sorted along E; one HBM read and one write per element instead of 6+ passes. */
int64_t gnnops_sort_rows_max_len(void);
int gnnops_sort_rows_f32(const float* input, float* values, int64_t* indices, int64_t rows, int64_t E,
                         int descending, gnnops_stream_t stream);
int64_t gnnops_sort_rows2_max_len(void);
/* Rows longer than gnnops_sort_rows_max_len(), up to gnnops_sort_rows2_max_len() (the reference's (28200, 28200) sort): halves sorted on chip into the caller's
 * (tmp_values, tmp_indices) — each [rows, E] — then rank-merged into (values, indices). Same ordering conventions. */
int gnnops_sort_rows2_f32(const float* input, float* values, int64_t* indices, float* tmp_values, int64_t* tmp_indices,
                          int64_t rows, int64_t E, int descending, gnnops_stream_t stream);
/* Both with the positions as int32 rows (they fit: a row is at most gnnops_sort_rows2_max_len() long), for a caller that widens
 * them in a later pass of its own (torch.sort along dim 0 of a matrix: gnnops_transpose2d_cvt mode 1 on the way back). */
int gnnops_sort_rows_f32_i32(const float* input, float* values, int32_t* indices, int64_t rows, int64_t E,
                             int descending, gnnops_stream_t stream);
int gnnops_sort_rows2_f32_i32(const float* input, float* values, int32_t* indices, float* tmp_values, int32_t* tmp_indices,
                              int64_t rows, int64_t E, int descending, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch_sparse.coalesce(index, value, m, n, op="add") / Tensor.coalesce()
 * (benchmark_sparse_coalesce.py:35-42); torch_sparse.transpose = the same call with row/col swapped
 * and (n, m). Entries are sorted row-major by (row, col); duplicates are summed in sorted (stable)
 * order. value [nnz, C] of `dtype` or NULL. Outputs are sized nnz; *d_count (device int64) receives
 * the number of distinct entries.
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_coalesce_workspace_bytes(int64_t nnz);
int gnnops_coalesce(const int64_t* row, const int64_t* col, const void* value, int64_t nnz,
                    int64_t m, int64_t n, int64_t C, int dtype,
                    int64_t* out_row, int64_t* out_col, void* out_value, int64_t* d_count,
                    void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* Dense 2-D transpose copy: torch.transpose(matA, 0, 1).contiguous() (benchmark_sparse_transpose.py:13-16).
 * in [R, C] -> out [C, R]; elem_bytes in {1, 2, 4, 8}; bit-exact. */
int gnnops_transpose2d(const void* in, void* out, int64_t R, int64_t C, int elem_bytes,
                       gnnops_stream_t stream);
/* [R, C] int64 -> [C, R] int32 (mode 0: every value must fit in 31 bits) or [R, C] int32 -> [C, R] int64 (mode 1). */
int gnnops_transpose2d_cvt(const void* in, void* out, int64_t R, int64_t C, int mode, gnnops_stream_t stream);
/* mode 0 with the largest element read left in *max_out (-1 for an empty matrix; device memory, written on the stream):
 * torch_scatter's implicit dim_size = index.max() + 1 from the index's own transpose. Values >= 2^31 make the int32 copy
 * meaningless — the caller checks *max_out before using it. */
int gnnops_transpose2d_cvt_max(const void* in, void* out, int64_t R, int64_t C, int64_t* max_out, gnnops_stream_t stream);
/* batch of independent [R, C] -> [C, R] copies (in / out [batch, R, C] / [batch, C, R]). */
int gnnops_transpose_batched(const void* in, void* out, int64_t batch, int64_t R, int64_t C, int elem_bytes,
                             gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch.addmm(input, mat1, mat2) / torch.matmul(input, other) on 16-bit operands
 * (benchmark_native_addmm.py:13-16, benchmark_native_matmul.py:13-16): out[M,N] = input[M,N] + mat1[M,K] @
 * mat2[K,N] (input == NULL: plain matmul). Row-major; dtype F16 / BF16 (fp32 MFMA accumulation, one rounding) or
 * F32 (exact-fp32 MFMA).
 * ------------------------------------------------------------------------------------------- */
/* Workspace of the 16-bit product (fp32 needs none; passing it is harmless): zero-filled copies of the last K-tile of each
 * operand when K is not a multiple of 64 or N not a multiple of 8 (a whole padded copy of a large mat1 instead), plus — when more than one round of 256 x 256 tiles leaves a last round of
 * at most half the CUs' worth — one 256 KiB fp32 slot per CU and a flag word each for the split-K tail (64 MiB on MI355X;
 * contents need not survive the call, the flags are cleared on the stream by the call itself). 0 for small aligned problems. */
size_t gnnops_addmm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int gnnops_addmm(const void* input, const void* mat1, const void* mat2, void* out,
                 int64_t M, int64_t N, int64_t K, int dtype,
                 void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* The same with a row pitch for `input` (elements): ld_input = N is gnnops_addmm; ld_input = 0 adds ONE row [N] to every
 * output row — the bias of a Linear layer (app_bm/groq_script.py:75-76 lin_f / lin_s) without materialising [M, N]. Any other
 * pitch must be >= N and a multiple of 16 bytes (EINVAL otherwise). */
int gnnops_addmm_ld(const void* input, int64_t ld_input, const void* mat1, const void* mat2, void* out, int64_t M,
                    int64_t N, int64_t K, int dtype, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Transposed-left product split along the long dimension (csrc/gemm_tn.hip): out[P,Q] = a[R,P]^T @ b[R,Q], the weight
 * gradient X^T @ G of a dense layer (R = nodes or edges, P and Q = the layer's widths). Contiguous row-major operands of one
 * dtype; products are summed in fp32 and rounded once. Stage 1: one workgroup per (128 x 128 output tile, slab of slab_rows
 * consecutive rows) writes an fp32 partial tile to the workspace; stage 2 adds each element's partials in ascending slab order.
 * No atomics; the geometry depends on (R, P, Q, dtype) alone, so the same call gives the same bits on every device.
 * slabs > 1 only while tiles * slabs <= 1024: the workspace never exceeds max(64 MiB, one fp32 output padded to whole tiles).
 * R == 0 writes zeros; P * Q == 0 returns OK at once. Operands need no alignment beyond their element size.
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_gemm_tn_workspace_bytes(int64_t R, int64_t P, int64_t Q, int dtype);   /* 0 for a negative size or an unknown dtype */
int gnnops_gemm_tn(const void* a, const void* b, void* out, int64_t R, int64_t P, int64_t Q, int dtype,
                   void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* What the launcher will do (host only): slabs == ceil(R / slab_rows); any output pointer may be NULL. */
int gnnops_gemm_tn_geometry(int64_t R, int64_t P, int64_t Q, int dtype, int64_t* tile_p, int64_t* tile_q,
                            int64_t* slab_rows, int64_t* slabs);

/* ---------------------------------------------------------------------------------------------
 * Grouped product (csrc/segment_matmul.hip), pyg_lib.ops.segment_matmul: out[ptr[t] : ptr[t+1], :] = x[ptr[t] : ptr[t+1], :] @
 * w[t] (+ bias[t]) for t < T, the per-type weight of HeteroLinear / RGCNConv. x [M, K], w [T, K, N], ptr int64 [T + 1] in
 * DEVICE memory, bias [T, N] or NULL, out [M, N]; contiguous row-major, one dtype (F32 / F16 / BF16), fp32 accumulation and
 * one rounding: a row gets the bits gnnops_addmm's register-staged kernel gives it. ptr is expected to start at 0, end at M
 * and never decrease; the kernels clamp every entry into [0, M] and take a decreasing pair as an empty segment, so no ptr
 * can make them touch a row outside [0, M) (rows no segment covers are left as they were). Two launches on the stream, no
 * host synchronisation, no atomics; the workspace holds the int32 tile map and needs no clearing.
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_segment_matmul_workspace_bytes(int64_t T);   /* 0 for a negative T */
int gnnops_segment_matmul(const void* x, const int64_t* ptr, const void* w, const void* bias, void* out, int64_t M, int64_t K,
                          int64_t N, int64_t T, int dtype, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
/* Host only: the tile of one workgroup (a segment is cut into tile_m-row tiles from its first row on) and the K-step of
 * the main loop; any output pointer may be NULL. */
int gnnops_segment_matmul_geometry(int dtype, int64_t* tile_m, int64_t* tile_n, int64_t* k_step);

/* ---------------------------------------------------------------------------------------------
 * Fused index_select(index_add(input, dim, index, other), dim, index).sum(dim)
 * (benchmark_fused_index_add_reduce.py:12-20). input [B,N,K], other [B,E,K], plan of index over N.
 * out_f32 [B,K] (fp32: the reference's fp16 result overflows at its own sizes). Nothing of size [B,N,K]
 * is materialised. workspace only when K > 1.
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_fused_index_add_select_sum_workspace_bytes(int64_t B, int64_t K);
int gnnops_fused_index_add_select_sum(const void* input, const void* other,
                                      const int32_t* rowptr, const int32_t* perm, float* out_f32,
                                      int64_t B, int64_t N, int64_t E, int64_t K, int dtype,
                                      void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch_sparse.spspmm / torch.sparse.mm(COO, COO) (benchmark_sparse_spspmm.py:12-14,94-95):
 * C = A(m x k) @ B(k x n) by expand - sort - compress. B is given as the plan (rowptrB, permB) of its row
 * index plus colB/valB. Phase 1 counts the products (*d_total, device int64) so the caller can size the
 * expansion; phase 2 writes them in (nonzero of A, nonzero of B's row) order; gnnops_coalesce over
 * (out_row, out_col, out_val, m, n) then yields the coalesced result. `workspace` is shared by both phases.
 * ------------------------------------------------------------------------------------------- */
size_t gnnops_spspmm_workspace_bytes(int64_t nnzA);
int gnnops_spspmm_count(const int64_t* colA, int64_t nnzA, const int32_t* rowptrB, int64_t* d_total,
                        void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
int gnnops_spspmm_expand(const int64_t* rowA, const int64_t* colA, const void* valA, int64_t nnzA,
                         const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, const void* valB,
                         int64_t* out_row, int64_t* out_col, void* out_val, int dtype,
                         const void* workspace, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row-wise (Gustavson) spspmm with the output row's accumulator in LDS (csrc/spgemm.hip): the same C = A @ B,
 * bit for bit, for operand pairs in which no row of B repeats a column and every output row's columns lie in a
 * window of at most gnnops_spgemm_max_span() columns. A and B are given as the plans (rowptr, perm) of their row
 * indices plus col / val; perm may be NULL when col / val are in plan (CSR) order already.
 *   row_stats  clears d_info (device int64[4]) and fills the per-row statistics of B in `workspace`
 *   symbolic   windows, sizes and row pointer of C in `workspace`; d_info = {nnz(C), some output row is too
 *              wide, some row of B repeats a column, largest window}: the caller's one host read
 *   numeric    only when neither flag is raised: out_row / out_col / out_val [nnz(C)], row-major with
 *              ascending columns; max_span = d_info[3] as read
 * One `workspace` of gnnops_spgemm_workspace_bytes(m, k) serves the three phases of a call.
 * ------------------------------------------------------------------------------------------- */
int64_t gnnops_spgemm_max_span(void);
size_t gnnops_spgemm_workspace_bytes(int64_t m, int64_t k);
int gnnops_spgemm_row_stats(const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, int64_t k, int64_t nnzB,
                            int64_t* d_info, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
int gnnops_spgemm_symbolic(const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, int64_t m, int64_t nnzA,
                           const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, int64_t k, int64_t nnzB,
                           int64_t* d_info, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
int gnnops_spgemm_numeric(const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, const void* valA, int64_t m,
                          int64_t nnzA, const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, const void* valB,
                          int64_t k, int64_t nnzC, int64_t max_span, int64_t* out_row, int64_t* out_col, void* out_val,
                          int dtype, const void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* The hashed route of the same product (spspmm(..., method="rowhash")): the output row's accumulator is an
 * open-addressing hash table in LDS keyed by column - (smallest column of the row) as 32 bits, so the columns of a
 * row may lie anywhere within 2^32 - 1 columns; an output row may hold at most gnnops_spgemm_hash_max_row() distinct
 * columns. Same phases, arguments, workspace and bits as gnnops_spgemm_*, except
 *   row_stats  rows of B of up to hash_max_row entries are checked for repeated columns and marked, the row, not the
 *              call (longer rows are not checked: the symbolic pass refuses every output row that references one)
 *   symbolic   d_info = {nnz(C), 1 * some output row has too many distinct columns + 2 * some output row spans too
 *              many columns for a key, some referenced row of B repeats a column, largest row count}
 *   numeric    only when d_info[1] and d_info[2] are zero; max_row = d_info[3] as read (it picks the table class) */
int64_t gnnops_spgemm_hash_max_row(void);
int gnnops_spgemm_hash_row_stats(const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, int64_t k, int64_t nnzB,
                                 int64_t* d_info, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
int gnnops_spgemm_hash_symbolic(const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, int64_t m, int64_t nnzA,
                                const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, int64_t k, int64_t nnzB,
                                int64_t* d_info, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
int gnnops_spgemm_hash_numeric(const int32_t* rowptrA, const int32_t* permA, const int64_t* colA, const void* valA, int64_t m,
                               int64_t nnzA, const int32_t* rowptrB, const int32_t* permB, const int64_t* colB, const void* valB,
                               int64_t k, int64_t nnzC, int64_t max_row, int64_t* out_row, int64_t* out_col, void* out_val,
                               int dtype, const void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Widening per SURVEY.md 8(f) rank 1: what PyG layers on the reference's OpProfiler path call.
 *
 * gnnops_segment_reduce with perm == NULL treats rowptr as a CSR pointer over src itself
 * (torch_scatter.segment_csr); gnnops_rowptr_from_sorted turns a sorted int64 index into that pointer
 * (torch_scatter.segment_coo's input contract).
 *
 * gnnops_segment_composite: torch_scatter.composite over a plan / CSR pointer (perm may be NULL).
 *   mode 0 softmax      out[B,E,K] = exp(x - max) / sum exp(x - max)
 *   mode 1 log_softmax  out[B,E,K] = (x - max) - log(sum + param)         param = eps (upstream 1e-12)
 *   mode 2 logsumexp    out[B,N,K] = max + log(sum + param)               param = eps
 *   mode 3 std          out[B,N,K] = sqrt(sum (x - mean)^2 / (cnt' + 1e-6)), param != 0: unbiased (cnt' = max(cnt-1,1))
 * ------------------------------------------------------------------------------------------- */
/* Backward-pass pieces (gnnops/autograd.py; the rest of every backward is one of the forward entry points above):
 *   gnnops_rowptr_expand  index[e] = n with rowptr[n] <= e < rowptr[n+1], or N where no segment holds e (E positions):
 *                         torch_scatter.gather_csr's addressing and the gather behind segment_csr's gradient.
 *   gnnops_sddmm          out[k] = sum_d a[rows_a[k], d] * b[rows_b[k], d]: d(value) of torch_sparse.spmm
 *                         (benchmark_sparse_spmm.py:12-14 under autograd); fp32 accumulation, one rounding. */
int gnnops_rowptr_expand(const int32_t* rowptr, int64_t N, int64_t E, int64_t* index, gnnops_stream_t stream);
int gnnops_sddmm(const int64_t* rows_a, const int64_t* rows_b, const void* a, const void* b, void* out,
                 int64_t nnz, int64_t D, int dtype, gnnops_stream_t stream);
/* Destination-partitioned scatter over the GPUs of a node (BASELINE config 5; gnnops/dist.py): counts[g] = number of
 * positions e with g * rows_per_owner <= index[e] < (g + 1) * rows_per_owner, g < owners <= 64 — what sizes the one
 * exchange of the step (the only value the host reads back). counts: device int64[owners], zeroed here. An id outside
 * [0, owners * rows_per_owner) is counted for no owner, so sum(counts) < E tells the caller about it. */
int gnnops_owner_counts(const int64_t* index, int64_t E, int64_t rows_per_owner, int owners, int64_t* counts,
                        gnnops_stream_t stream);
size_t gnnops_rowptr_workspace_bytes(int64_t N);
int gnnops_rowptr_from_sorted(const int64_t* sorted_index, int64_t E, int64_t N, int32_t* rowptr,
                              void* workspace, size_t workspace_bytes, gnnops_stream_t stream);
int gnnops_segment_composite(const void* src, const int32_t* rowptr, const int32_t* perm, void* out,
                             int64_t B, int64_t E, int64_t K, int64_t N, int dtype, int mode, double param,
                             gnnops_stream_t stream);
/* The same with groups of more than 8192 members set aside and processed piecewise by whole workgroups (csrc/hub.h);
 * hub_workspace = gnnops_hub_workspace_bytes(E, K, GNNOPS_MIN) bytes, or NULL. B == 1, rows of whole 16-B lanes. */
int gnnops_segment_composite_hubs(const void* src, const int32_t* rowptr, const int32_t* perm, void* out, int64_t B,
                                  int64_t E, int64_t K, int64_t N, int dtype, int mode, double param,
                                  void* hub_workspace, size_t hub_workspace_bytes, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Widening per SURVEY.md 8(f) rank 4: the message + aggregate of one message-passing layer in one pass
 * (app_bm/benchmark_convs.py:146-246 times FiLMConv, GINConv, CGConv, PNAConv, SAGEConv forward;
 * app_bm/groq_script.py:91-109 is CGConv.forward / .message). Replaces, per layer, the chain
 * x[edge_index[0]] / x[edge_index[1]] -> message -> torch_scatter.scatter(..., reduce) of MessagePassing.propagate.
 *
 *   out[i, (s * n_aggr + a) * K + k] = scaler_s(deg_i) * AGGR_a over the edges (j -> i) of f(p[i], q[j], w[e])[k]
 *
 * Edges in destination-sorted (plan) order: rowptr int32 [N+1]; col int64 [E] = source row j of sorted edge position;
 * perm int32 [E] = original edge id of that position (only read when w is given; NULL = identity).
 * functor 0 COPY    f = q                                             rows: q [K]
 *         1 ADD     f = p + q + w   (w optional)                            q, p, w [K]
 *         2 CGCONV  f = sigmoid(p_f + q_f + w_f) * softplus(p_s + q_s + w_s) q, p, w [f part K | s part K]; w optional
 *         3 FILM    f = relu(gamma * q + beta)                               q [K], p [beta K | gamma K]
 * aggr[]: 0 sum, 1 mean (divide by max(deg, 1)), 2 min, 3 max (0 for rows without edges), 4 std =
 *   sqrt(relu(mean(f^2) - mean(f)^2) + 1e-5) — PNAConv.aggregate; scalers[] (n_scalers == 0: none): 0 identity,
 *   1 amplification log(deg+1)/avg_deg_log, 2 attenuation avg_deg_log/log(deg+1), 3 linear deg/avg_deg_lin,
 *   4 inverse_linear avg_deg_lin/deg, deg clamped to >= 1 — PNAConv's degree scalers.
 * add (optional, [N, >=K]): added to the first output block (CGConv's `out += x[1]`).
 * ld* = row pitches in elements, so operands may be column blocks of one GEMM result and `out` a column block of the
 * buffer the layer would torch.cat into. fp32 arithmetic, one rounding on store.
 * ------------------------------------------------------------------------------------------- */
int gnnops_edge_reduce(int functor, const void* q, int64_t ldq, const void* p, int64_t ldp, const void* w, int64_t ldw,
                       const void* add, int64_t ldadd, const int32_t* rowptr, const int32_t* perm, const int64_t* col,
                       void* out, int64_t ldo, int64_t N, int64_t E, int64_t K, const int* aggr, int n_aggr,
                       const int* scalers, int n_scalers, float avg_deg_log, float avg_deg_lin, int dtype,
                       gnnops_stream_t stream);
/* The same with destinations of more than 8192 edges ("hubs", as csrc/hub.h) set aside by the main kernel and reduced in
 * pieces of 2048 edges by separate lane groups (fp32 partial accumulators, combined in piece order: the same result every
 * run, sums re-associated for those rows only). hub_workspace = gnnops_edge_reduce_hub_workspace_bytes(E, K) bytes, or NULL. */
size_t gnnops_edge_reduce_hub_workspace_bytes(int64_t E, int64_t K);
int gnnops_edge_reduce_hubs(int functor, const void* q, int64_t ldq, const void* p, int64_t ldp, const void* w, int64_t ldw,
                            const void* add, int64_t ldadd, const int32_t* rowptr, const int32_t* perm, const int64_t* col,
                            void* out, int64_t ldo, int64_t N, int64_t E, int64_t K, const int* aggr, int n_aggr,
                            const int* scalers, int n_scalers, float avg_deg_log, float avg_deg_lin, int dtype,
                            void* hub_workspace, size_t hub_workspace_bytes, gnnops_stream_t stream);

/* Backward of the edge pass for sum / mean aggregation — what lets GINConv / SAGEConv / CGConv / FiLMConv of gnnops.conv sit
 * in a training loop (graph_benchmark/profile/OpProfiler.py:259-292 profiles one). Per edge e = (j -> i), in EDGE order,
 * the gradient of the message with respect to the rows it was made from, given g[i] = d loss / d out[i] (for mean: already
 * divided by max(deg_i, 1)):
 *   CGCONV  z_f = p_f[i] + q_f[j] (+ w_f[e]), z_s likewise:
 *           gp[e] = [ g * softplus(z_s) * sig(z_f) (1 - sig(z_f)) | g * sig(z_f) * sig(z_s) ]   (2K; gq: pass NULL — d q and d w
 *           are the same rows)        d p[i] = sum of gp over the edges into i, d q[j] = sum over the edges out of j, d w = gp
 *   FILM    a = gamma[i] * q[j] + beta[i], m = [a > 0]:  gp[e] = [ g m | g m q[j] ]  (2K = d beta | d gamma),  gq[e] = g m gamma[i]  (K)
 * COPY / ADD messages need no call (their per-edge gradient is g[i] itself). The two sums are gnnops_segment_reduce over the
 * destination plan and over the plan of the source ids. ld* = row pitches in elements; gp [E, 2K], gq [E, K] dense. */
int gnnops_edge_grad(int functor, const void* p, int64_t ldp, const void* q, int64_t ldq, const void* w, int64_t ldw,
                     const void* g, int64_t ldg, const int64_t* src, const int64_t* dst, void* gp, void* gq, int64_t E,
                     int64_t K, int dtype, gnnops_stream_t stream);

/* Backward of the edge pass for SEVERAL aggregators and degree scalers (PNAConv in a training loop), for the messages that are
 * affine in their operands: COPY (m = q[j]) and ADD (m = p[i] + q[j] (+ w[e])); other functors: GNNOPS_EUNSUPPORTED. Operands,
 * plan (rowptr, perm, col), aggr[], scalers[] and the two averages exactly as gnnops_edge_reduce_hubs was called; nothing of the
 * forward is saved: each destination's edges are walked twice (sum, sum of squares, min and max recomputed, then the gradient).
 * g [N, max(n_scalers, 1) * n_aggr * K] = d loss / d out, blocks in the forward's order, row pitch ldg (0 = one row for all).
 *   ga_a[i] = sum over the scalers s of scaler_s(deg_i) * g[i, s, a]                       (deg clamped to >= 1)
 *   gm[e]   = ga_sum + ga_mean / deg + ga_std * [var > 0] * (m_e - mean) / (deg * std)
 *             + [e is the min's edge] ga_min + [e is the max's edge] ga_max              var, std as the forward's std block
 *   min / max: ONE edge per destination and column, the smallest edge id among those that attain the value.
 * gm [E, K] dense, row = ORIGINAL edge id (perm NULL = identity): d w = gm, d q = its segment sum over the plan of the source
 * ids (gnnops_segment_reduce). gp [N, K] dense = d p = the sum of gm over each destination's edges, accumulated in fp32 (zero
 * row for a destination without edges); COPY: not written, pass NULL. fp32 arithmetic, one rounding on store, no atomics: the
 * same bits every run. N, E, ldq, ldw < 2^31. One launch on `stream`, no workspace, no synchronisation. A destination with
 * more than 8192 edges is walked by one lane group per column chunk like any other (correct, slow). */
int gnnops_edge_multi_grad(int functor, const void* q, int64_t ldq, const void* p, int64_t ldp, const void* w, int64_t ldw,
                           const void* g, int64_t ldg, const int32_t* rowptr, const int32_t* perm, const int64_t* col,
                           void* gm, void* gp, int64_t N, int64_t E, int64_t K, const int* aggr, int n_aggr,
                           const int* scalers, int n_scalers, float avg_deg_log, float avg_deg_lin, int dtype,
                           gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Attention edge pass (csrc/attention.hip): the softmax-weighted aggregation of GATv2Conv — the reference's model zoo builds
 * GATv2REG from it (graph_benchmark/models/ptg_models.py:208-236) — in one pass with an online softmax. Operands as
 * gnnops_edge_reduce: destination-sorted plan (rowptr int32 [N+1], col int64 [E] = source row of each sorted position,
 * perm int32 [E] = original edge id of that position, NULL = identity), ld* = row pitches in elements.
 *   z[e,h,c] = p[i,h,c] + q[j,h,c] + u[e,h,c]   s[e,h] = sum_c att[h,c] * leaky_relu(z[e,h,c], negative_slope)     edge e = (j -> i)
 *   out[i,h,:] = sum_{e into i} exp(s[e,h] - lse[i,h]) * q[j,h,:],   lse[i,h] = log sum_{e into i} exp(s[e,h])
 * q [N_src, >= H*C], p [N, >= H*C], att [H*C], out [N, H*C] (pitch ldo) in `dtype`; lse fp32 [N, H], always written.
 * A destination without edges gets a zero row and lse = -inf. 1 <= H, 1 <= C, H*C <= 8192 (GNNOPS_EINVAL otherwise);
 * N, E, ldq and every value of col (so N_src) below 2^31: the kernels narrow source ids to 32 bits.
 * One launch on `stream`, no allocation, no synchronisation.
 * u, optional (GATv2Conv with edge features: u = lin_edge(edge_attr)), enters the score only — the message stays q[j,h,:].
 *   u [E, H*C] is dense, in `dtype`, its rows the ORIGINAL edge ids: the row of sorted position k is perm[k] (perm NULL =
 *   identity: the edge list is already destination-sorted), at the 64-bit element offset (int64) id * H*C. u NULL = absent
 *   (the forward then does not read perm: pass NULL); an all-zero u gives the same bits as the call without u.
 *   E == 0 or N == 0: u is not dereferenced.
 * Backward, given grad_out [N, >= H*C] (pitch ldg; 0 = one row for all), the forward's out and lse:
 *   grad_p [N, H*C] dense; gq [E, H*C] dense, row = ORIGINAL edge id: d q = its segment sum over the plan of the source ids
 *   (gnnops_segment_reduce); grad_att [H*C]. workspace = gnnops_edge_attention_backward_workspace_bytes(N, H, C) bytes of
 *   fp32 partial sums of d att, added in a fixed order. gu [E, H*C] dense, row = original edge id, = d u
 *   (gq[e] = a[e] * grad_out[i] + gu[e]): required when u is given and E > 0, ignored otherwise. No atomics: two runs give
 *   the same bits. N == 0: nothing is written.
 * ------------------------------------------------------------------------------------------- */
int gnnops_edge_attention(const void* q, int64_t ldq, const void* p, int64_t ldp, const void* att, const void* u,
                          const int32_t* rowptr, const int32_t* perm, const int64_t* col, void* out, int64_t ldo, float* lse,
                          int64_t N, int64_t E, int64_t H, int64_t C, float negative_slope, int dtype, gnnops_stream_t stream);
size_t gnnops_edge_attention_backward_workspace_bytes(int64_t N, int64_t H, int64_t C);   /* host-only; serves both families */
int gnnops_edge_attention_backward(const void* q, int64_t ldq, const void* p, int64_t ldp, const void* att, const void* u,
                                   const void* out, int64_t ldo, const float* lse, const void* grad_out, int64_t ldg,
                                   const int32_t* rowptr, const int32_t* perm, const int64_t* col, void* grad_p, void* gq,
                                   void* gu, void* grad_att, int64_t N, int64_t E, int64_t H, int64_t C, float negative_slope,
                                   int dtype, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* The second member of the family (GATConv, the original GAT, and AttentiveFP's GATEConv): the score is a per-edge scalar plus
 * a per-destination scalar, the row may carry a per-edge part u and a leaky ReLU of its own, and a per-edge, per-head scale
 * (the attention dropout mask divided by 1 - p) enters the weighted sum only, never the denominator.
 *   t[e,h,:] = q[j,h,:] + u[e,h,:]            r = has_row_slope ? leaky_relu(t, row_slope) : t              edge e = (j -> i)
 *   s[e,h] = leaky_relu(att[h,:] . r[e,h,:] + d[i,h] + c[e,h], negative_slope)   lse[i,h] = log sum_{e into i} exp(s[e,h])
 *   out[i,h,:] = sum_{e into i} exp(s[e,h] - lse[i,h]) * edge_scale[e,h] * r[e,h,:]
 * q [N_src, >= H*C] (pitch ldq), d [N, >= H] (pitch ldd), att [H*C], out [N, H*C] (pitch ldo) in `dtype`; lse fp32 [N, H].
 * u [E, H*C], c [E, H] and edge_scale [E, H] are dense, in `dtype`, their rows the ORIGINAL edge ids (read through perm,
 * offsets in 64 bits); NULL = absent (u = 0, c = 0, edge_scale = 1). row_slope is read only when has_row_slope != 0. Limits,
 * the plan operands and the empty destination as gnnops_edge_attention. One launch, no allocation, no synchronisation.
 * c (GATConv with edge features: c[e,h] = att_edge[h] . lin_edge(edge_attr)[e,h,:], one tiny product with att_edge folded
 *   into the weight) leaves the message unchanged, and an all-zero c gives the same bits as the call without c. c and u
 *   together have no kernel instance (GNNOPS_EUNSUPPORTED). E == 0 or N == 0: u, c and edge_scale are not dereferenced.
 * Backward: grad_d [N, H] dense (summed in fp32, stored once per destination); gq [E, H*C] dense, row = original edge id,
 *   = d u, and d q = its segment sum over the plan of the source ids; grad_att [H*C] through a workspace of
 *   gnnops_edge_attention_backward_workspace_bytes(N, H, C) bytes (fixed-order sum, the same bits every run). gc [E, H] dense,
 *   row = original edge id, = d c = d pre (one store per edge and head, no atomics): required when c is given and E > 0,
 *   ignored otherwise. edge_scale is not differentiated. N == 0: nothing is written. */
int gnnops_edge_attention_v1(const void* q, int64_t ldq, const void* d, int64_t ldd, const void* att, const void* u,
                             const void* c, const void* edge_scale, const int32_t* rowptr, const int32_t* perm,
                             const int64_t* col, void* out, int64_t ldo, float* lse, int64_t N, int64_t E, int64_t H, int64_t C,
                             int has_row_slope, float row_slope, float negative_slope, int dtype, gnnops_stream_t stream);
int gnnops_edge_attention_v1_backward(const void* q, int64_t ldq, const void* d, int64_t ldd, const void* att, const void* u,
                                      const void* c, const void* edge_scale, const void* out, int64_t ldo, const float* lse,
                                      const void* grad_out, int64_t ldg, const int32_t* rowptr, const int32_t* perm,
                                      const int64_t* col, void* grad_d, void* gq, void* gc, void* grad_att, int64_t N,
                                      int64_t E, int64_t H, int64_t C, int has_row_slope, float row_slope,
                                      float negative_slope, int dtype, void* workspace, size_t workspace_bytes,
                                      gnnops_stream_t stream);

/* The third member (TransformerConv, Shi et al. 2021): scaled dot-product attention. The score is the dot product of the
 * destination's query row with the edge's key row, the message a second gathered row, the value; all arithmetic in fp32.
 *   kk[e,h,:] = k[j,h,:] + u[e,h,:]           vv[e,h,:] = v[j,h,:] + u[e,h,:]                               edge e = (j -> i)
 *   s[e,h] = scale * qry[i,h,:] . kk[e,h,:]                                      lse[i,h] = log sum_{e into i} exp(s[e,h])
 *   out[i,h,:] = sum_{e into i} exp(s[e,h] - lse[i,h]) * edge_scale[e,h] * vv[e,h,:]
 * qry [N, >= H*C] (pitch ldq); k and v [N_src, >= H*C], two pointers into rows of ONE pitch ldkv (two column blocks of one
 * product); out [N, H*C] (pitch ldo) in `dtype`; lse fp32 [N, H]. u [E, H*C] and edge_scale [E, H] (the attention dropout
 * mask divided by 1 - p: in the weighted sum only, never in lse) are dense, in `dtype`, their rows the ORIGINAL edge ids (read
 * through perm, offsets in 64 bits); NULL = absent (u = 0, edge_scale = 1), and an all-ones edge_scale gives the same bits as
 * the call without it. Limits (H*C <= 8192; N, E and the pitches < 2^31), the plan operands and the empty destination (a zero
 * row, lse = -inf) as gnnops_edge_attention. E == 0 or N == 0: u and edge_scale are not dereferenced. One launch, no
 * allocation, no synchronisation, no atomics.
 * Backward (one launch, destination-ordered, no workspace: there is no att vector to sum over destinations): grad_qry [N, H*C]
 *   dense (summed in fp32, stored once per destination); gkv [E, 2*H*C] dense, row = original edge id: columns [0, H*C) =
 *   ds * scale * qry[i], columns [H*C, 2*H*C) = a * edge_scale * grad_out[i], with a = exp(s - lse) and
 *   ds = a * (edge_scale * (grad_out[i,h,:] . vv) - grad_out[i,h,:] . out[i,h,:]); [d k | d v] = its segment sum over the plan of
 *   the source ids. gu [E, H*C] dense, row = original edge id, = d u = the sum of the two halves: required when u is given and
 *   E > 0 (GNNOPS_EINVAL otherwise), ignored without u. ldg == 0: one gradient row for all destinations. edge_scale is not
 *   differentiated. N == 0: nothing is written. */
int gnnops_edge_attention_dot(const void* qry, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* u,
                              const void* edge_scale, const int32_t* rowptr, const int32_t* perm, const int64_t* col, void* out,
                              int64_t ldo, float* lse, int64_t N, int64_t E, int64_t H, int64_t C, float scale, int dtype,
                              gnnops_stream_t stream);
int gnnops_edge_attention_dot_backward(const void* qry, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* u,
                                       const void* edge_scale, const void* out, int64_t ldo, const float* lse,
                                       const void* grad_out, int64_t ldg, const int32_t* rowptr, const int32_t* perm,
                                       const int64_t* col, void* grad_qry, void* gkv, void* gu, int64_t N, int64_t E, int64_t H,
                                       int64_t C, float scale, int dtype, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The remaining ops of the reference's list (ops.txt:17-19, 29-41) - SURVEY.md 8(f) rank 4. Neither package is in the
 * reference tree (torch-spline-conv 1.2.1, torch-cluster 1.5.9: requirements.txt:214, :210) and the reference has no
 * script or output for them: the packages' published definitions, parity unpinned (oracle/spatial_oracle.py).
 *
 * torch_spline_conv  (csrc/spline.hip has the formulas)
 *   gnnops_spline_basis      pseudo [E, D] -> basis [E, S] (dtype), weight_index [E, S] int64, S = (degree + 1)^D <= 64;
 *                            kernel_size int64 [D] and is_open_spline uint8 [D] are HOST arrays
 *   gnnops_spline_weighting  out[e, o] = sum_s basis[e, s] * sum_i x[e, i] * weight[weight_index[e, s], i, o]
 *   gnnops_spline_conv       the whole layer per destination row in one pass: (rowptr, perm) = plan of edge_index[0],
 *                            src int64 [E] = edge_index[1] in plan order, pseudo [E, D] in edge order; norm != 0 divides by
 *                            the row's degree; root_weight [Min, Mout] and bias [Mout] optional
 *   Backward (csrc/spline_bw.hip; named after the package's own backward ops). x_rows / g_rows: optional int64 [E] row
 *   indices into x / grad_out (NULL = row e) - spline_conv's backward passes edge_index[1] / edge_index[0], so no gathered
 *   [E, Min] / [E, Mout] copy exists. No floating-point atomics: repeated calls give identical bits.
 *   gnnops_spline_basis_bw            grad_basis [E, S] -> grad_pseudo [E, D] (floor() carries no gradient)
 *   gnnops_spline_weighting_bw_basis  grad_basis[e, s] = x[xr(e)]^T weight[weight_index[e, s]] grad_out[gr(e)]
 *   gnnops_spline_weighting_bw_weight grad_weight [K, Min, Mout], every entry written (exact zeros for kernels no pair uses):
 *                                     (rowptr [K + 1], perm [E * S]) = gnnops_plan_build of weight_index viewed as [E * S]
 *                                     over K; per kernel an MFMA contraction of the gathered rows basis * x and grad_out.
 *                                     E * S < 2^31. Workspace: gnnops_spline_weighting_bw_weight_workspace_bytes.
 *   grad_x has no entry point of its own: it is gnnops_spline_weighting / gnnops_spline_conv on grad_out with the table
 *   transposed to [K, Mout, Min] (gnnops_transpose_batched), for the layer over the plan of edge_index[1].
 * torch_cluster  (batches as CSR pointers ptr [batches + 1] int64 over points sorted by batch; all arrays on the device)
 *   gnnops_grid_cluster  voxel id per point; size / start / end: device double [D]
 *   gnnops_knn           col [Ny, k] = the k nearest x of every y within its batch, ascending (distance, index); -1 = none
 *   gnnops_radius        col [Ny, max] = the first max x (ascending index) with |x - y|^2 < r^2; -1 = none
 *   gnnops_fps           farthest point sampling per batch: out[out_ptr[b] .. out_ptr[b+1]) starting from start[b];
 *                        dist_workspace float [N]
 *   gnnops_random_walk   out [walkers, walk_length + 1]: uniform next neighbour over a CSR adjacency (int64 rowptr, col)
 *   gnnops_graclus_rounds  `rounds` rounds of handshake matching over a CSR adjacency (weight in CSR order or NULL): cluster
 *                        int64 [N] (-1 = unmatched, initialised by the caller) gets min(n, partner) for matched pairs;
 *                        *d_active (device int) = proposals in the last round (0: the matching is maximal); finish != 0
 *                        gives every node still alone its own id. proposal: int64 [N] scratch.
 * ------------------------------------------------------------------------------------------- */
int gnnops_spline_basis(const void* pseudo, const int64_t* kernel_size, const uint8_t* is_open_spline, int64_t E, int D,
                        int degree, void* basis, int64_t* weight_index, int dtype, gnnops_stream_t stream);
int gnnops_spline_weighting(const void* x, const void* weight, const void* basis, const int64_t* weight_index, void* out,
                            int64_t E, int64_t Min, int64_t Mout, int64_t S, int dtype, gnnops_stream_t stream);
int gnnops_spline_conv(const void* x, const int32_t* rowptr, const int32_t* perm, const int64_t* src, const void* pseudo,
                       const void* weight, const int64_t* kernel_size, const uint8_t* is_open_spline, int D, int degree,
                       const void* root_weight, const void* bias, void* out, int64_t N, int64_t E, int64_t Min, int64_t Mout,
                       int norm, int dtype, gnnops_stream_t stream);
int gnnops_spline_basis_bw(const void* grad_basis, const void* pseudo, const int64_t* kernel_size, const uint8_t* is_open_spline,
                           int64_t E, int D, int degree, void* grad_pseudo, int dtype, gnnops_stream_t stream);
int gnnops_spline_weighting_bw_basis(const void* grad_out, const void* x, const void* weight, const int64_t* weight_index,
                                     const int64_t* x_rows, const int64_t* g_rows, void* grad_basis, int64_t E, int64_t Min,
                                     int64_t Mout, int64_t S, int dtype, gnnops_stream_t stream);
size_t gnnops_spline_weighting_bw_weight_workspace_bytes(int64_t E, int64_t S, int64_t Min, int64_t Mout);
int gnnops_spline_weighting_bw_weight(const void* grad_out, const void* x, const void* basis, const int32_t* rowptr,
                                      const int32_t* perm, const int64_t* x_rows, const int64_t* g_rows, void* grad_weight,
                                      int64_t E, int64_t K, int64_t Min, int64_t Mout, int64_t S, int dtype, void* workspace,
                                      size_t workspace_bytes, gnnops_stream_t stream);
int gnnops_grid_cluster(const void* pos, int64_t N, int D, const double* d_size, const double* d_start, const double* d_end,
                        int64_t* cluster, int dtype, gnnops_stream_t stream);
int gnnops_knn(const void* x, const void* y, const int64_t* ptr_x, const int64_t* ptr_y, int64_t batches, int64_t Ny, int D,
               int k, int cosine, int64_t* col, int dtype, gnnops_stream_t stream);
/* torch_cluster.knn through a uniform grid — one cloud, Euclidean, D <= 3, fp32, k <= 64; the pairs of the exhaustive kernel.
 * Step 1: bounding box (24 bytes at `box`) and cell ids of x on a G^D grid; then gnnops_plan_build(cell, Nx, G^D, rowptr, perm);
 * step 2: the queries walk the cells around their own in shells until the k-th distance is inside the block searched. */
int gnnops_knn_grid_cells(const void* x, int64_t Nx, int D, int G, void* box, int64_t* cell, gnnops_stream_t stream);
int gnnops_knn_grid_query(const void* x, const void* y, int64_t Ny, int D, int k, int G, const void* box, const int32_t* rowptr,
                          const int32_t* perm, int64_t* col, gnnops_stream_t stream);
/* torch_cluster.radius over the same cells / plan: the max_num_neighbors (<= 64) smallest indices inside the ball, ascending. */
int gnnops_radius_grid_query(const void* x, const void* y, int64_t Ny, int D, double r, int max_num_neighbors, int G, const void* box,
                             const int32_t* rowptr, const int32_t* perm, int64_t* col, gnnops_stream_t stream);
int gnnops_radius(const void* x, const void* y, const int64_t* ptr_x, const int64_t* ptr_y, int64_t batches, int64_t Ny, int D,
                  double r, int max_num_neighbors, int64_t* col, int dtype, gnnops_stream_t stream);
int gnnops_fps(const void* x, const int64_t* ptr, const int64_t* out_ptr, const int64_t* start, int64_t batches, int D,
               float* dist_workspace, int64_t* out, int dtype, gnnops_stream_t stream);
int gnnops_random_walk(const int64_t* rowptr, const int64_t* col, const int64_t* start, int64_t walkers, int walk_length,
                       uint64_t seed, int64_t* out, gnnops_stream_t stream);
/* torch_cluster.random_walk with node2vec's bias (p: return, q: in-out; ops.txt:41): after a uniform first step, a candidate drawn
 * uniformly from the current node's neighbours is accepted with probability (1/p, 1, 1/q) / max(1/p, 1, 1/q) when it is the
 * previous node / a neighbour of the previous node / neither (rejection sampling, as the package). Every row of the CSR
 * adjacency must be sorted ascending (the neighbour test is a binary search). */
int gnnops_random_walk_node2vec(const int64_t* rowptr, const int64_t* col, const int64_t* start, int64_t walkers, int walk_length,
                                double p, double q, uint64_t seed, int64_t* out, gnnops_stream_t stream);
int gnnops_graclus_rounds(const int64_t* rowptr, const int64_t* col, const void* weight, int64_t N, uint64_t seed, int rounds,
                          int64_t* cluster, int64_t* proposal, int* d_active, int finish, int dtype, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GraphUNet's pieces (the reference's GraphUNetREG, graph_benchmark/models/ptg_models.py; torch_geometric 2.0.2 TopKPooling,
 * filter_adj, GCNConv — the packages' published definitions, parity unpinned): csrc/pool.hip, csrc/gcn.hip.
 *
 * Per-graph top-k of a score vector. graph_ptr int32 [G+1]: the nodes of one graph are contiguous (a sorted `batch`).
 *   gnnops_segment_topk_counts  k_g = min(k, n_g) for an integer k >= 1; with k < 1, k_g = ceil(ratio * float32(n_g)) in
 *       float32 for a ratio in (0, 1], as (ratio * num_nodes.to(torch.float)).ceil(). out_ptr int32 [G+1] = exclusive scan
 *       of k_g; d_info (device int64 [2]) = { sum of k_g, the longest graph } — the one host read the caller needs: the
 *       first sizes perm, the second picks the route. One workgroup.
 *   gnnops_segment_topk  perm int64 [out_ptr[G]]: global node ids, graph after graph, each graph's in descending score.
 *       Ties go to the lower node id, -0.0 orders as +0.0, a NaN ranks above every number (gnnops_sort, descending).
 *       score [N] in `dtype`. max_graph_len: at least the longest graph (d_info[1]).
 *       route 0: on-chip when max_graph_len <= gnnops_segment_topk_max_len(), else long; 1: on-chip (GNNOPS_EINVAL if a
 *       graph cannot fit); 2: long. On-chip: one wave per graph of up to 64 nodes, one workgroup per longer one, the graph
 *       read once, only its k ids written. Long: one gnnops_sort of int64 keys (graph id << 32 | score image) and a select
 *       pass, in `workspace` of gnnops_segment_topk_workspace_bytes(N, max_graph_len, route) bytes (host-only; 0 on-chip).
 *       Both routes give the same perm. G, N below 2^31. No allocation, no synchronisation.
 * ------------------------------------------------------------------------------------------- */
int64_t gnnops_segment_topk_max_len(void);
int gnnops_segment_topk_counts(const int32_t* graph_ptr, int64_t G, float ratio, int64_t k, int32_t* out_ptr, int64_t* d_info,
                               gnnops_stream_t stream);
size_t gnnops_segment_topk_workspace_bytes(int64_t N, int64_t max_graph_len, int route);
int gnnops_segment_topk(const void* score, const int32_t* graph_ptr, const int32_t* out_ptr, int64_t* perm, int64_t G, int64_t N,
                        int64_t max_graph_len, int dtype, int route, void* workspace, size_t workspace_bytes,
                        gnnops_stream_t stream);

/* node_map int32 [N] = -1 everywhere, then node_map[perm[i]] = i for i < k: the `mask[perm] = arange(k)` of filter_adj.
 * perm: distinct ids in [0, N). */
int gnnops_node_map(const int64_t* perm, int64_t k, int64_t N, int32_t* node_map, gnnops_stream_t stream);

/* Stable compaction of a COO edge list. row, col int64 [E]; node_map (optional) int32 [>= every id + 1], -1 = node gone;
 * value (optional) [E] rows of value_row_bytes bytes each (an even number). An edge survives if both mapped endpoints are
 * >= 0 and, with drop_self_loops, they differ. Survivors keep their order; out_row / out_col (int64, room for E) get the
 * mapped ids, out_value the rows, *d_count (device int64) their number. Count per tile of gnnops_filter_edges_tile()
 * edges, scan of the tile counts, write: two passes over the edges. workspace = gnnops_filter_edges_workspace_bytes(E)
 * bytes (host-only). E below 2^32 - tile. */
int64_t gnnops_filter_edges_tile(void);
size_t gnnops_filter_edges_workspace_bytes(int64_t E);
int gnnops_filter_edges(const int64_t* row, const int64_t* col, const void* value, int64_t value_row_bytes,
                        const int32_t* node_map, int64_t E, int drop_self_loops, int64_t* out_row, int64_t* out_col,
                        void* out_value, int64_t* d_count, void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

/* GCNConv's edge pass over the destination plan of gnnops_edge_reduce (rowptr int32 [N+1], perm int32 [E] = original edge id
 * of a sorted position, NULL = identity; col int64 [E] = source row of a sorted position). w fp32 [E] in EDGE order (read
 * through perm), NULL = every weight 1.
 *   gnnops_gcn_degree     lw[i] = the weight of the last self loop of i in edge order, fill_value without one;
 *                         deg[i] = lw[i] + sum of w_e over the non-loop edges into i; dis[i] = deg[i] > 0 ? rsqrt(deg[i]) : 0.
 *                         dis, lw fp32 [N]. (add_remaining_self_loops + gcn_norm; the edge list is not rewritten.)
 *   gnnops_gcn_propagate  out[i] = dis[i] * (sum over the non-loop edges (j -> i) of w_e * dis[j] * h[j] + lw[i] * dis[i] * h[i])
 *                         (+ bias [K]). h [N_src, >= K] (pitch ldh; 0 = one row for all), out [N, >= K] (pitch ldo), bias in
 *                         `dtype`; fp32 arithmetic, one rounding on store, no atomics, the same bits every run. The operator
 *                         is symmetric: the backward is this call over the plan of the SOURCE ids with the same dis / lw.
 * A destination of any in-degree is reduced by its own lane group. N, E below 2^31. One launch each. */
int gnnops_gcn_degree(const int32_t* rowptr, const int32_t* perm, const int64_t* col, const float* w, int64_t N, int64_t E,
                      float fill_value, float* dis, float* lw, gnnops_stream_t stream);
int gnnops_gcn_propagate(const void* h, int64_t ldh, const int32_t* rowptr, const int32_t* perm, const int64_t* col,
                         const float* w, const float* dis, const float* lw, const void* bias, void* out, int64_t ldo,
                         int64_t N, int64_t E, int64_t K, int dtype, gnnops_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * What the GATv2 model (the reference's GATv2REG, graph_benchmark/models/ptg_models.py) runs between two attention passes, as
 * one row pass (csrc/norm.hip): the mean over heads, the bias, ReLU, the feature-dropout mask and LayerNorm.
 *   y[c] = (a[i,0,c] + ... + a[i,H-1,c]) / H (+ bias[c])    r[c] = relu ? max(y[c], 0) : y[c]    d[c] = r[c] * scale[i,c]
 *   gamma given: mu = mean_c d, var = mean_c (d - mu)^2 (biased, two passes), out[i,c] = (d[c] - mu) * rsqrt(var + eps) * gamma[c] (+ beta[c])
 *   gamma NULL:  out[i,c] = d[c]
 * a [N, >= H*C] (pitch lda in elements, so a column block of a wider matrix is fine), bias / gamma / beta [C], scale [N, C]
 * dense (the mask already divided by 1 - p), out [N, C] dense, all in `dtype`; NULL bias / scale / beta = absent (beta needs
 * gamma). fp32 arithmetic, heads added in ascending order, one rounding on store. stats (optional, read by the backward):
 * fp32 [N, 2] = (mu, rstd), written only with gamma. 1 <= H, 1 <= C, H*C <= 8192 (GNNOPS_EINVAL otherwise); N, lda < 2^31.
 * One launch on `stream`, no allocation, no synchronisation.
 * Backward, given grad_out [N, >= C] (pitch ldg; 0 = one row for all) and the forward's operands and stats (nothing else is
 * saved: y, the gate and xhat are recomputed): grad_a [N, H*C] dense (d y / H in every head), and where the pointer is not
 * NULL grad_bias = sum_i d y, grad_gamma = sum_i grad_out * xhat, grad_beta = sum_i grad_out, each [C] (the last two need
 * gamma). scale is not differentiated. workspace = gnnops_head_act_norm_backward_workspace_bytes(N, H, C) bytes (host-only)
 * of fp32 partial column sums, added in a fixed order by a second kernel: no atomics, the same bits every run. N == 0:
 * nothing is written.
 * ------------------------------------------------------------------------------------------- */
int gnnops_head_act_norm(const void* a, int64_t lda, const void* bias, const void* scale, const void* gamma, const void* beta,
                         void* out, float* stats, int64_t N, int64_t H, int64_t C, int relu, float eps, int dtype,
                         gnnops_stream_t stream);
size_t gnnops_head_act_norm_backward_workspace_bytes(int64_t N, int64_t H, int64_t C);
int gnnops_head_act_norm_backward(const void* a, int64_t lda, const void* bias, const void* scale, const void* gamma,
                                  const float* stats, const void* grad_out, int64_t ldg, void* grad_a, void* grad_bias,
                                  void* grad_gamma, void* grad_beta, int64_t N, int64_t H, int64_t C, int relu, int dtype,
                                  void* workspace, size_t workspace_bytes, gnnops_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNOPS_H */
