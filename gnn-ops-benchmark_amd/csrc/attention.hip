// attention.hip — softmax-weighted aggregation over the destination-sorted edge list in ONE pass, and its backward, for three ways
// of scoring an edge e = (j -> i) per head h. Common to all three:
//   a[e,h]     = exp(s[e,h] - lse[i,h]),   lse[i,h] = log sum_{e into i} exp(s[e,h])
//   out[i,h,:] = sum_{e into i} a[e,h] * message[e,h,:]
// The weight of an edge depends on ALL the edges of its destination, which the elementwise messages of conv.hip cannot say.
//
// THE WALK (its helpers stand once, next to Place; a kernel adds its score, message and gradient arithmetic).
// Layout: ONE WAVE per (destination, block of 64 / G heads) = one item (item_of), one group of G = 2^gshift lanes per head, lane gl of
// a group on the columns (k * G + gl) * VEC .. + VEC of its head, k < NCH (Place). The whole wave walks the same edges, so the edge
// loop, its bounds and the row base addresses are scalar: the ids of a run of 64 edges are one coalesced load (run_ids) handed out
// by v_readlane (run_id, as conv.hip's WAVE_ROW form), every row base of a step is taken and pinned ahead of its row loads, and
// every raw row of a step is in flight before the first is consumed (fetch_row). The per-head dot product is a butterfly of DPP moves
// inside the group with every lane active (group_sum of lane_group.h: quad_perm, row_half_mirror, row_mirror; groups of 32 / 64
// lanes add the four row sums read by v_readlane). Per-edge operands (u, edge_scale, c) and per-edge results are rows of the ORIGINAL
// edge id, read and written through perm (perm == NULL = identity) with int64 offsets.
// Forward: per (destination, head) a running maximum m, a denominator l and the accumulators (online softmax): a step of U edges may
// raise the maximum, l and the accumulators are then rescaled by exp(m_old - m_new) (softmax_raise); the end of a destination
// writes acc / l and lse (store_destination). Each gathered row is read once and serves the score and the weighted sum; no [E, H]
// score and no [E, H, C] message is written.
// Backward (destination-ordered too, no atomics): delta = sum_c g * out per head, s recomputed from the same rows,
// a = exp(s - lse), ds = a * (g . message - delta); per-edge gradient rows are written once, per-destination sums stay in registers.
// A family with an att vector sums d att per wave in fp32 across its destinations and a second small kernel adds the [waves, H * C]
// partials in a fixed order. The three backward kernels share run_ids (attention_bwd_kernel and dot_bwd_kernel also item_of and
// run_id) with the forward ones and keep the rest of their walk inline (the delta sweep, the row fetch, the zeroing and the
// partial-row store): as helpers those changed the register allocation of single instances enough to cost a wave per SIMD. The two
// gate kernels take wave_of_grid and run_ids only and compile to the instructions they had: with more, the plain instances of
// gate_fwd_kernel ran about 1 % slower and GATConv's forward + backward read above its earlier time (profiles/attention_walk.txt).
// Rows of more than 256 pieces per head (C > 256 * VEC) take the NCH = 128, VEC = 1 instance: correct at any C <= 8192, its
// operand rows re-read per edge (cache hits) and its accumulators wherever the compiler finds room.
// Heavy destinations are walked by their one wave (no piecewise pass yet: the (m, l, accumulator) triple merges across
// pieces, so the cure of hub.h applies).
// No atomics anywhere: two runs give the same bits.
//
// FIRST FAMILY, GATv2 (gnnops.conv.edge_attention / GATv2Conv; the reference's model zoo builds GATv2REG from GATv2Conv,
// graph_benchmark/models/ptg_models.py:208-236, and trains it, OpProfiler.py:97-112):
//   z[e,h,c] = p[i,h,c] + q[j,h,c] (+ u[e,h,c])      s[e,h] = sum_c att[h,c] * leaky_relu(z[e,h,c], slope)      message = q[j,h,:]
// Algorithmic bytes per launch, forward: E * H * (C * elem + 8 / heads-per-wave-block) gathered + N * (p row + out row + 4 H);
// the unfused chain on this package's ops moves at least three [E, H, C] tensors and two [E, H] ones, each written and read.
// Backward: one [E, H * C] tensor gq is written (d q = its segment sum over the source plan), d p is summed in registers and
// stored once per destination. HASU (u = lin_edge(edge_attr), GATv2Conv with edge_dim; compile-time instances beside the ones
// without, which compile as before): forward, the online softmax keeps its steps of Unroll<NCH>::U edges — the same maxima and
// rescalings, so u = 0 gives the bits of the pass without u — and fetches the raw rows of a step in two halves (AttUnroll::FWL),
// holding the first half's q rows for the weighted sum. Backward, where an edge stands alone, the step halves (2 / 1 / 1 / 1);
// t = ds * att * leaky'(z) is stored twice: inside gq[e] = a * g[i] + t[e], and alone as gu[e] = d u.
//
// SECOND FAMILY, GAT (v1) and GATE (gnnops.conv.edge_attention_v1: GATConv, the original GAT, and AttentiveFP's GATEConv): the score
// comes from a per-edge scalar and a per-destination scalar, with an optional per-edge row u and per-edge, per-head scale k (the
// attention dropout mask, in the weighted sum only):
//   t[e,h,:] = q[j,h,:] + u[e,h,:]      r = t, or leaky_relu(t, row_slope)      message = k[e,h] * r[e,h,:]
//   s[e,h] = leaky_relu(att[h,:] . r[e,h,:] + d[i,h] (+ c[e,h]), slope)
// With u a step holds two raw rows per edge, so its unroll halves. HASC (c = att_edge . lin_edge(edge_attr), [E, H], GATConv with
// edge_dim; read exactly as edge_scale is): backward writes gc[e,h] = d pre, one store per edge and head. Instantiated without u only.
//
// THIRD FAMILY, scaled dot product (gnnops.conv.edge_attention_dot: TransformerConv): see the comment above DotArgs.
#include "common.h"
#include "lane_group.h"
#include "dispatch.h"

namespace {

struct AttArgs {
    const void *q, *p, *att, *g, *o;    // o, g: the stored forward output and its gradient (backward only)
    const void* u;                      // [E, H * C], rows = ORIGINAL edge ids (read through perm), or null
    void* gu;                           // d u [E, H * C], rows = original edge ids (backward with u only)
    const int32_t *rowptr, *perm;
    const int64_t* col;
    void *out, *dp, *gq;
    float *lse, *partial;
    int64_t N, ldq, ldp, ldo, ldg;
    int H, C, gshift, hblocks, nwaves;
    float slope;
};

template <typename T, int VEC>
__device__ inline u32x4 att_load_raw(const T* p) {
    constexpr int BYTES = VEC * (int)sizeof(T);
    u32x4 r = {0u, 0u, 0u, 0u};
    if constexpr (BYTES == 16) {
        r = load16<false>(p);
    } else if constexpr (BYTES == 8) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        r.x = t.x; r.y = t.y;
    } else if constexpr (BYTES == 4) {
        r.x = *reinterpret_cast<const uint32_t*>(p);
    } else {
        r.x = *reinterpret_cast<const uint16_t*>(p);
    }
    return r;
}
template <typename T, int VEC>
__device__ inline void att_unpack(const u32x4& r, float* f) {
    float g[Elem<T>::VEC];
    Elem<T>::unpack(r, g);
#pragma unroll
    for (int v = 0; v < VEC; ++v) f[v] = g[v];
}
template <typename T, int VEC>
__device__ inline void att_store(T* p, const float* f) {
    constexpr int BYTES = VEC * (int)sizeof(T);
    if constexpr (VEC == 1) {
        Elem<T>::store(p, f[0]);
    } else {
        float g[Elem<T>::VEC];
#pragma unroll
        for (int v = 0; v < Elem<T>::VEC; ++v) g[v] = v < VEC ? f[v] : 0.f;
        const u32x4 r = Elem<T>::pack(g);
        if constexpr (BYTES == 16) store16<false>(p, r);
        else if constexpr (BYTES == 8) *reinterpret_cast<uint2*>(p) = uint2{r.x, r.y};
        else *reinterpret_cast<uint32_t*>(p) = r.x;
    }
}

template <int NCH> struct Unroll { static constexpr int U = NCH == 1 ? 8 : NCH == 2 ? 4 : NCH <= 4 ? 2 : 1; };

// With a per-edge row u an edge brings two raw rows, so the rows in flight together are those of half as many edges: forward,
// the online softmax keeps its steps of Unroll<NCH>::U edges (the same maxima and rescalings as without u, so u = 0 gives the same
// bits) and fetches a step's rows in two halves of FWL edges, the q rows of the first half held for the weighted sum; backward,
// where every edge stands alone, the step itself halves.
template <int NCH, bool HASU> struct AttUnroll {
    static constexpr int FWL = HASU && Unroll<NCH>::U > 1 ? Unroll<NCH>::U / 2 : Unroll<NCH>::U;
    static constexpr int BW = HASU ? (NCH == 1 ? 2 : 1) : (NCH == 1 ? 4 : NCH == 2 ? 2 : 1);
};

// where a lane stands: its head, and per piece k its element offset inside a row of H * C (0 and !ok past the head's end)
struct Place {
    int lane, gl, G, h, C;
    bool head_ok;
    __device__ inline Place(int gshift, int H, int C_, int hb) {
        lane = threadIdx.x & 63;
        G = 1 << gshift;
        gl = lane & (G - 1);
        h = hb * (64 >> gshift) + (lane >> gshift);
        C = C_;
        head_ok = h < H;
    }
    template <int VEC> __device__ inline bool live(int k) const { return k * G * VEC < C; }   // wave-uniform: some lane has piece k
    template <int VEC> __device__ inline bool ok(int k) const { return head_ok && (k * G + gl) * VEC < C; }
    template <int VEC> __device__ inline int off(int k) const { return ok<VEC>(k) ? h * C + (k * G + gl) * VEC : 0; }
};

// ---- the walk, once: what the kernels below do alike, whatever they score. wave_of_grid and run_ids serve all six, item_of and run_id
// the attention_* and dot_* kernels, the helpers after them attention_fwd_kernel and dot_fwd_kernel (why: see the head comment) --
__device__ inline int wave_of_grid() {
    return __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
}

// item it = (destination i, head block hb) and the scalar bounds [jb, je) of the edges into i
struct Item { int i, hb; int32_t jb, je; };
__device__ inline Item item_of(int64_t it, int hblocks, const int32_t* rowptr) {
    Item t;
    t.i = __builtin_amdgcn_readfirstlane((int)(it / hblocks));
    t.hb = __builtin_amdgcn_readfirstlane((int)(it % hblocks));
    t.jb = __builtin_amdgcn_readfirstlane(rowptr[t.i]);
    t.je = __builtin_amdgcn_readfirstlane(rowptr[t.i + 1]);
    return t;
}

// the ids of the run of (at most) 64 edges from jrun: one coalesced load each, lane l holds id l of the run. cl = the source,
// el = the ORIGINAL edge id (perm == NULL = identity), fetched only where something is read or written by it
struct RunIds { int cl, el; };
__device__ inline RunIds run_ids(const int64_t* col, const int32_t* perm, int32_t jrun, int32_t je, int lane, bool by_edge) {
    RunIds r{0, 0};
    if (jrun + lane < je) {
        r.cl = (int)col[jrun + lane];
        if (by_edge) r.el = perm ? perm[jrun + lane] : jrun + lane;
    }
    return r;
}
// id k of the run as a scalar (v_readlane). A kernel multiplies it into the row bases of a step and pins them (asm volatile, "+s") at
// the top of the step, ahead of every row load (conv.hip:209-224)
__device__ inline int64_t run_id(int ids, int32_t k) { return __builtin_amdgcn_readlane(ids, k & 63); }

// the NCH raw pieces of one row (q, k, v, u); a kernel puts every row of a step in flight before it consumes the first
template <typename T, int VEC, int NCH>
__device__ inline void fetch_row(const T* row, const Place& pl, u32x4 (&r)[NCH]) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (!pl.live<VEC>(k)) continue;
        r[k] = att_load_raw<T, VEC>(row + pl.off<VEC>(k));
    }
}
// a row that stays in registers (HOLD), unpacked; a piece that no lane has reads offset 0
template <typename T, int VEC, int NCH>
__device__ inline void hold_row(const T* row, const Place& pl, float (&f)[NCH][VEC]) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) att_unpack<T, VEC>(att_load_raw<T, VEC>(row + pl.off<VEC>(k)), f[k]);
}

template <int NCH, int VEC>
__device__ inline void zero_pieces(float (&x)[NCH][VEC]) {
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) x[k][v] = 0.f;
}

// Online softmax, the raise: the step's scores s[u] (of the edges j + u < end) may lift the running maximum m; the denominator l and
// the accumulators are rescaled by exp(m_old - m_new). The kernel then adds the step's exp(s[u] - m) to l and its messages to acc.
template <int U, int NCH, int VEC>
__device__ inline void softmax_raise(const float (&s)[U], int32_t j, int32_t end, float& m, float& l, float (&acc)[NCH][VEC]) {
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (j + u < end) mn = fmaxf(mn, s[u]);
    const float scale = expf(m - mn);   // 0 on the first step (m = -inf): nothing to rescale yet
    m = mn;
    l = l * scale;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[k][v] = acc[k][v] * scale;
}

// the end of a destination: out = acc / l and lse = m + log l; a destination without an edge (any == false) gets a zero row and -inf
template <typename T, int VEC, int NCH>
__device__ inline void store_destination(const Place& pl, bool any, float m, float l, const float (&acc)[NCH][VEC], T* out_row, float* lse_row,
                                         float neg_inf) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (!pl.live<VEC>(k)) continue;
        float o[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = any ? acc[k][v] / l : 0.f;
        if (pl.ok<VEC>(k)) att_store<T, VEC>(out_row + pl.off<VEC>(k), o);
    }
    if (pl.head_ok && pl.gl == 0) lse_row[pl.h] = any ? m + logf(l) : neg_inf;
}

template <typename T, int VEC, int NCH, bool HASU>
__global__ __launch_bounds__(256) void attention_fwd_kernel(const AttArgs a) {
    constexpr int U = Unroll<NCH>::U;
    constexpr int UL = AttUnroll<NCH, HASU>::FWL;   // edges whose raw rows are fetched together (U without u)
    constexpr bool HOLD = NCH <= 4;   // p and att pieces stay in registers
    const T* __restrict__ q = (const T*)a.q;
    const T* __restrict__ p = (const T*)a.p;
    const T* __restrict__ att = (const T*)a.att;
    const T* __restrict__ ue = (const T*)a.u;
    const int wave = wave_of_grid();
    const int64_t items = a.N * a.hblocks;
    const int ldq = (int)a.ldq;
    const int HC = a.H * a.C;
    const float slope = a.slope;
    const float NEG_INF = -__builtin_huge_valf();
    for (int64_t it = wave; it < items; it += a.nwaves) {
        const Item t = item_of(it, a.hblocks, a.rowptr);
        const int i = t.i;
        const Place pl(a.gshift, a.H, a.C, t.hb);
        const int lane = pl.lane;
        float pv[HOLD ? NCH : 1][VEC], av[HOLD ? NCH : 1][VEC];
        if constexpr (HOLD) {
            hold_row<T, VEC>(p + (int64_t)i * a.ldp, pl, pv);
            hold_row<T, VEC>(att, pl, av);
        }
        float acc[NCH][VEC];
        zero_pieces(acc);
        float m = NEG_INF, l = 0.f;
        for (int32_t jrun = t.jb; jrun < t.je; jrun += 64) {
            const int32_t jrun_end = min(jrun + 64, t.je);
            const RunIds ids = run_ids(a.col, a.perm, jrun, t.je, lane, HASU);
            for (int32_t j = jrun; j < jrun_end; j += U) {
                int64_t qrow[U], erow[HASU ? U : 1];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    qrow[u] = run_id(ids.cl, j - jrun + u) * ldq;
                    asm volatile("" : "+s"(qrow[u]));   // the row bases are computed HERE, ahead of every row load (conv.hip:209-224)
                    if constexpr (HASU) {
                        erow[u] = run_id(ids.el, j - jrun + u) * HC;
                        asm volatile("" : "+s"(erow[u]));
                    }
                }
                u32x4 qr[U][NCH];
                float s[U];
#pragma unroll
                for (int u0 = 0; u0 < U; u0 += UL) {        // one round without u, two halves with it
                    u32x4 ur[HASU ? UL : 1][HASU ? NCH : 1];
#pragma unroll
                    for (int u = u0; u < u0 + UL; ++u) {    // every row load of the round in flight before the first is consumed
                        if (j + u < jrun_end) {
                            fetch_row<T, VEC>(q + qrow[u], pl, qr[u]);
                            if constexpr (HASU) fetch_row<T, VEC>(ue + erow[u], pl, ur[u - u0]);
                        }
                    }
#pragma unroll
                    for (int u = u0; u < u0 + UL; ++u) {
                        s[u] = 0.f;
                        if (j + u < jrun_end) {
                            float part = 0.f;
#pragma unroll
                            for (int k = 0; k < NCH; ++k) {
                                if (!pl.live<VEC>(k)) continue;
                                float qv[VEC], pk[VEC], ak[VEC], uv[VEC];
                                att_unpack<T, VEC>(qr[u][k], qv);
                                if constexpr (HASU) att_unpack<T, VEC>(ur[u - u0][k], uv);
                                if constexpr (!HOLD) {
                                    att_unpack<T, VEC>(att_load_raw<T, VEC>(p + (int64_t)i * a.ldp + pl.off<VEC>(k)), pk);
                                    att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), ak);
                                }
                                float sub = 0.f;
#pragma unroll
                                for (int v = 0; v < VEC; ++v) {
                                    float z = (HOLD ? pv[k][v] : pk[v]) + qv[v];
                                    if constexpr (HASU) z = z + uv[v];
                                    sub += (HOLD ? av[k][v] : ak[v]) * (z > 0.f ? z : z * slope);
                                }
                                part += pl.ok<VEC>(k) ? sub : 0.f;
                            }
                            s[u] = group_sum(part, a.gshift, lane);
                        }
                    }
                }
                softmax_raise(s, j, jrun_end, m, l, acc);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < jrun_end) {
                        const float w = expf(s[u] - m);
                        l = l + w;
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            float qv[VEC];
                            att_unpack<T, VEC>(qr[u][k], qv);
#pragma unroll
                            for (int v = 0; v < VEC; ++v) acc[k][v] = acc[k][v] + w * qv[v];
                        }
                    }
                }
            }
        }
        store_destination<T, VEC>(pl, t.je > t.jb, m, l, acc, (T*)a.out + (int64_t)i * a.ldo, a.lse + (int64_t)i * a.H, NEG_INF);
    }
}

// Backward. The wave's head block is the same for all its destinations (nwaves is a multiple of hblocks), so the d att sums
// of its lanes stay in registers across destinations and are written once, to row wave / hblocks of the partials.
template <typename T, int VEC, int NCH, bool HASU>
__global__ __launch_bounds__(256) void attention_bwd_kernel(const AttArgs a) {
    constexpr int U = AttUnroll<NCH, HASU>::BW;
    constexpr bool HOLD = NCH <= 4;
    const T* __restrict__ q = (const T*)a.q;
    const T* __restrict__ p = (const T*)a.p;
    const T* __restrict__ att = (const T*)a.att;
    const T* __restrict__ g = (const T*)a.g;
    const T* __restrict__ o = (const T*)a.o;
    const T* __restrict__ ue = (const T*)a.u;
    const int64_t* __restrict__ col = a.col;
    const int32_t* __restrict__ perm = a.perm;
    const int wave = wave_of_grid();
    if (wave >= a.nwaves) return;
    const int64_t items = a.N * a.hblocks;
    const int ldq = (int)a.ldq;
    const int HC = a.H * a.C;
    const float slope = a.slope;
    const int hb = __builtin_amdgcn_readfirstlane(wave % a.hblocks);
    const Place pl(a.gshift, a.H, a.C, hb);
    const int lane = pl.lane;
    float datt[NCH][VEC];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) datt[k][v] = 0.f;
    float av[HOLD ? NCH : 1][VEC];
    if constexpr (HOLD) {
#pragma unroll
        for (int k = 0; k < NCH; ++k) att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), av[k]);
    }
    for (int64_t it = wave; it < items; it += a.nwaves) {
        const Item t = item_of(it, a.hblocks, a.rowptr);
        const int i = t.i;
        const int32_t jb = t.jb, je = t.je;
        float pv[HOLD ? NCH : 1][VEC], gv[HOLD ? NCH : 1][VEC], dp[NCH][VEC];
        float dpart = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) dp[k][v] = 0.f;
            if (!pl.live<VEC>(k)) continue;
            float gk[VEC], ok_[VEC];
            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
            att_unpack<T, VEC>(att_load_raw<T, VEC>(o + (int64_t)i * a.ldo + pl.off<VEC>(k)), ok_);
            float sub = 0.f;
#pragma unroll
            for (int v = 0; v < VEC; ++v) sub += gk[v] * ok_[v];
            dpart += pl.ok<VEC>(k) ? sub : 0.f;
            if constexpr (HOLD) {
                att_unpack<T, VEC>(att_load_raw<T, VEC>(p + (int64_t)i * a.ldp + pl.off<VEC>(k)), pv[k]);
#pragma unroll
                for (int v = 0; v < VEC; ++v) gv[k][v] = gk[v];
            }
        }
        const float delta = group_sum(dpart, a.gshift, lane);                    // sum_c g * out of this head
        const float lse = pl.head_ok ? a.lse[(int64_t)i * a.H + pl.h] : 0.f;
        for (int32_t jrun = jb; jrun < je; jrun += 64) {
            const int32_t jrun_end = min(jrun + 64, je);
            const RunIds ids = run_ids(col, perm, jrun, je, lane, true);
            const int cl = ids.cl, el = ids.el;   // under the names the inline steps below use: their text, and so their schedule, stays as it was
            for (int32_t j = jrun; j < jrun_end; j += U) {
                int64_t qrow[U], erow[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    qrow[u] = run_id(cl, j - jrun + u) * ldq;
                    erow[u] = run_id(el, j - jrun + u) * HC;
                    asm volatile("" : "+s"(qrow[u]));
                    asm volatile("" : "+s"(erow[u]));
                }
                u32x4 qr[U][NCH], ur[HASU ? U : 1][HASU ? NCH : 1];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < jrun_end) {
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            qr[u][k] = att_load_raw<T, VEC>(q + qrow[u] + pl.off<VEC>(k));
                            if constexpr (HASU) ur[u][k] = att_load_raw<T, VEC>(ue + erow[u] + pl.off<VEC>(k));
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u >= jrun_end) continue;
                    float spart = 0.f, dapart = 0.f;
#pragma unroll
                    for (int k = 0; k < NCH; ++k) {
                        if (!pl.live<VEC>(k)) continue;
                        float qv[VEC], pk[VEC], ak[VEC], gk[VEC], uv[VEC];
                        att_unpack<T, VEC>(qr[u][k], qv);
                        if constexpr (HASU) att_unpack<T, VEC>(ur[u][k], uv);
                        if constexpr (!HOLD) {
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(p + (int64_t)i * a.ldp + pl.off<VEC>(k)), pk);
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), ak);
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
                        }
                        float s1 = 0.f, s2 = 0.f;
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            float z = (HOLD ? pv[k][v] : pk[v]) + qv[v];
                            if constexpr (HASU) z = z + uv[v];
                            s1 += (HOLD ? av[k][v] : ak[v]) * (z > 0.f ? z : z * slope);
                            s2 += (HOLD ? gv[k][v] : gk[v]) * qv[v];
                        }
                        const bool ok = pl.ok<VEC>(k);
                        spart += ok ? s1 : 0.f;
                        dapart += ok ? s2 : 0.f;
                    }
                    const float s = group_sum(spart, a.gshift, lane), da = group_sum(dapart, a.gshift, lane);
                    const float w = expf(s - lse);
                    const float ds = w * (da - delta);
#pragma unroll
                    for (int k = 0; k < NCH; ++k) {
                        if (!pl.live<VEC>(k)) continue;
                        float qv[VEC], pk[VEC], ak[VEC], gk[VEC], row[VEC], uv[VEC], trow[VEC];
                        att_unpack<T, VEC>(qr[u][k], qv);
                        if constexpr (HASU) att_unpack<T, VEC>(ur[u][k], uv);
                        if constexpr (!HOLD) {
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(p + (int64_t)i * a.ldp + pl.off<VEC>(k)), pk);
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), ak);
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
                        }
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            float z = (HOLD ? pv[k][v] : pk[v]) + qv[v];
                            if constexpr (HASU) z = z + uv[v];
                            const float t = ds * (HOLD ? av[k][v] : ak[v]) * (z > 0.f ? 1.f : slope);
                            dp[k][v] = dp[k][v] + t;
                            datt[k][v] = datt[k][v] + ds * (z > 0.f ? z : z * slope);
                            row[v] = w * (HOLD ? gv[k][v] : gk[v]) + t;
                            if constexpr (HASU) trow[v] = t;
                        }
                        if (pl.ok<VEC>(k)) att_store<T, VEC>((T*)a.gq + erow[u] + pl.off<VEC>(k), row);
                        if constexpr (HASU) {
                            if (pl.ok<VEC>(k)) att_store<T, VEC>((T*)a.gu + erow[u] + pl.off<VEC>(k), trow);   // d u = t, row = original edge id
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            if (pl.live<VEC>(k) && pl.ok<VEC>(k)) att_store<T, VEC>((T*)a.dp + (int64_t)i * HC + pl.off<VEC>(k), dp[k]);
    }
    float* prow = a.partial + (int64_t)(wave / a.hblocks) * HC;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (!pl.live<VEC>(k) || !pl.ok<VEC>(k)) continue;
#pragma unroll
        for (int v = 0; v < VEC; ++v) prow[pl.off<VEC>(k) + v] = datt[k][v];
    }
}

// d att[c] = the partial rows added top to bottom: the same bits every run
template <typename T>
__global__ __launch_bounds__(256) void attention_datt_kernel(const float* __restrict__ partial, int rows, int HC, T* __restrict__ datt) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= HC) return;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s = s + partial[(int64_t)r * HC + c];
    Elem<T>::store(datt + c, s);
}

// ---- GATConv (v1) / GATEConv ---------------------------------------------------------------------------------------------------
struct GateArgs {
    const void *q, *d, *att, *u, *ks, *g, *o;   // u [E, H * C], ks [E, H] (edge_scale): rows = ORIGINAL edge ids, either may be null
    const void* c;                              // [E, H], a per-edge term of the pre-activation: rows = original edge ids, or null
    void* gc;                                   // d c [E, H] = d pre, rows = original edge ids (backward with c only)
    const int32_t *rowptr, *perm;
    const int64_t* col;
    void *out, *dd, *gq;
    float *lse, *partial;
    int64_t N, ldq, ldd, ldo, ldg;
    int H, C, gshift, hblocks, nwaves;
    float slope, row_slope;   // row_slope = 1 where the row is taken as it is: t * 1 = t and the derivative is 1, exactly
};

// edges per step: every raw row of a step is in flight before the first is consumed, and with u there are two per edge
template <int NCH, bool HASU> struct GateUnroll {
    static constexpr int FW = HASU ? (NCH == 1 ? 4 : NCH == 2 ? 2 : 1) : Unroll<NCH>::U;
    static constexpr int BW = HASU ? (NCH == 1 ? 2 : 1) : (NCH == 1 ? 4 : NCH == 2 ? 2 : 1);
};

template <typename T> __device__ inline float gate_scalar(const T* p) {
    float f[1];
    att_unpack<T, 1>(att_load_raw<T, 1>(p), f);
    return f[0];
}

// t = q[j] + u[e] of one piece
template <typename T, int VEC, bool HASU>
__device__ inline void gate_row(const u32x4& qr, const u32x4& ur, float* t) {
    att_unpack<T, VEC>(qr, t);
    if constexpr (HASU) {
        float uv[VEC];
        att_unpack<T, VEC>(ur, uv);
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[v] = t[v] + uv[v];
    }
}

// This kernel takes wave_of_grid and run_ids only, and keeps the rest of its walk and its softmax step inline: with them it compiles
// to the instructions it had, and with the forward helpers its plain instances (GATConv without u and c) ran about 1 % slower
// (profiles/attention_walk.txt).
template <typename T, int VEC, int NCH, bool HASU, bool HASC>
__global__ __launch_bounds__(256) void gate_fwd_kernel(const GateArgs a) {
    constexpr int U = GateUnroll<NCH, HASU>::FW;
    constexpr bool HOLD = NCH <= 4;   // att pieces stay in registers
    const T* __restrict__ q = (const T*)a.q;
    const T* __restrict__ d = (const T*)a.d;
    const T* __restrict__ att = (const T*)a.att;
    const T* __restrict__ ue = (const T*)a.u;
    const T* __restrict__ ks = (const T*)a.ks;
    const T* __restrict__ ce = (const T*)a.c;
    const int64_t* __restrict__ col = a.col;
    const int32_t* __restrict__ perm = a.perm;
    const int wave = wave_of_grid();
    const int64_t items = a.N * a.hblocks;
    const int ldq = (int)a.ldq;
    const int HC = a.H * a.C;
    const float slope = a.slope, rs = a.row_slope;
    const bool by_edge = HASU || HASC || ks != nullptr;   // something is read by original edge id
    const float NEG_INF = -__builtin_huge_valf();
    for (int64_t it = wave; it < items; it += a.nwaves) {
        const int i = __builtin_amdgcn_readfirstlane((int)(it / a.hblocks));
        const int hb = __builtin_amdgcn_readfirstlane((int)(it % a.hblocks));
        const Place pl(a.gshift, a.H, a.C, hb);
        const int lane = pl.lane;
        const int hk = pl.head_ok ? pl.h : 0;
        const int32_t jb = __builtin_amdgcn_readfirstlane(a.rowptr[i]), je = __builtin_amdgcn_readfirstlane(a.rowptr[i + 1]);
        float av[HOLD ? NCH : 1][VEC];
        if constexpr (HOLD) {
#pragma unroll
            for (int k = 0; k < NCH; ++k) att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), av[k]);
        }
        const float dv = gate_scalar<T>(d + (int64_t)i * a.ldd + hk);
        float acc[NCH][VEC];
#pragma unroll
        for (int k = 0; k < NCH; ++k)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[k][v] = 0.f;
        float m = NEG_INF, l = 0.f;
        for (int32_t jrun = jb; jrun < je; jrun += 64) {
            const int32_t jrun_end = min(jrun + 64, je);
            const RunIds ids = run_ids(col, perm, jrun, je, lane, by_edge);
            const int cl = ids.cl, el = ids.el;   // under the names the inline steps below use: their text, and so their schedule, stays as it was
            for (int32_t j = jrun; j < jrun_end; j += U) {
                int64_t qrow[U], erow[HASU ? U : 1], krow[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    qrow[u] = (int64_t)__builtin_amdgcn_readlane(cl, (j - jrun + u) & 63) * ldq;
                    asm volatile("" : "+s"(qrow[u]));   // the row bases are computed HERE, ahead of every row load
                    krow[u] = 0;
                    if (by_edge) {                      // pure GAT without a mask: no per-edge base at all
                        const int64_t e = __builtin_amdgcn_readlane(el, (j - jrun + u) & 63);
                        krow[u] = e * a.H;
                        if constexpr (HASU) {
                            erow[u] = e * HC;
                            asm volatile("" : "+s"(erow[u]));
                        }
                    }
                }
                u32x4 qr[U][NCH], ur[HASU ? U : 1][HASU ? NCH : 1];
                float kv[U], cv[HASC ? U : 1];
#pragma unroll
                for (int u = 0; u < U; ++u) {           // every row load of the step in flight before the first is consumed
                    kv[u] = 1.f;
                    if (j + u < jrun_end) {
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            qr[u][k] = att_load_raw<T, VEC>(q + qrow[u] + pl.off<VEC>(k));
                            if constexpr (HASU) ur[u][k] = att_load_raw<T, VEC>(ue + erow[HASU ? u : 0] + pl.off<VEC>(k));
                        }
                        if (ks) kv[u] = gate_scalar<T>(ks + krow[u] + hk);
                        if constexpr (HASC) cv[u] = gate_scalar<T>(ce + krow[u] + hk);
                    }
                }
                float s[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    s[u] = 0.f;
                    if (j + u < jrun_end) {
                        float part = 0.f;
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            float t[VEC], ak[VEC];
                            gate_row<T, VEC, HASU>(qr[u][k], ur[HASU ? u : 0][HASU ? k : 0], t);
                            if constexpr (!HOLD) att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), ak);
                            float sub = 0.f;
#pragma unroll
                            for (int v = 0; v < VEC; ++v) sub += (HOLD ? av[k][v] : ak[v]) * (t[v] > 0.f ? t[v] : t[v] * rs);
                            part += pl.ok<VEC>(k) ? sub : 0.f;
                        }
                        float pre = group_sum(part, a.gshift, lane) + dv;
                        if constexpr (HASC) pre = pre + cv[u];
                        s[u] = pre > 0.f ? pre : pre * slope;
                    }
                }
                float mn = m;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j + u < jrun_end) mn = fmaxf(mn, s[u]);
                const float scale = expf(m - mn);   // 0 on the first step (m = -inf): nothing to rescale yet
                m = mn;
                l = l * scale;
#pragma unroll
                for (int k = 0; k < NCH; ++k)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[k][v] = acc[k][v] * scale;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < jrun_end) {
                        const float w = expf(s[u] - mn);
                        l = l + w;                      // the denominator never sees the scale: dropout comes after the softmax
                        const float wk = w * kv[u];
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            float t[VEC];
                            gate_row<T, VEC, HASU>(qr[u][k], ur[HASU ? u : 0][HASU ? k : 0], t);
#pragma unroll
                            for (int v = 0; v < VEC; ++v) acc[k][v] = acc[k][v] + wk * (t[v] > 0.f ? t[v] : t[v] * rs);
                        }
                    }
                }
            }
        }
        const bool any = je > jb;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            if (!pl.live<VEC>(k)) continue;
            float o[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) o[v] = any ? acc[k][v] / l : 0.f;
            if (pl.ok<VEC>(k)) att_store<T, VEC>((T*)a.out + (int64_t)i * a.ldo + pl.off<VEC>(k), o);
        }
        if (pl.head_ok && pl.gl == 0) a.lse[(int64_t)i * a.H + pl.h] = any ? m + logf(l) : NEG_INF;
    }
}

// Backward: as attention_bwd_kernel (one head block per wave, d att in registers across its destinations); d d[i, h] is the sum
// of dpre over the edges of i, in a register, stored once.
// As gate_fwd_kernel, this kernel takes wave_of_grid and run_ids only: so it compiles to the instructions it had.
template <typename T, int VEC, int NCH, bool HASU, bool HASC>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const GateArgs a) {
    constexpr int U = GateUnroll<NCH, HASU>::BW;
    constexpr bool HOLD = NCH <= 4;
    const T* __restrict__ q = (const T*)a.q;
    const T* __restrict__ d = (const T*)a.d;
    const T* __restrict__ att = (const T*)a.att;
    const T* __restrict__ ue = (const T*)a.u;
    const T* __restrict__ ks = (const T*)a.ks;
    const T* __restrict__ ce = (const T*)a.c;
    const T* __restrict__ g = (const T*)a.g;
    const T* __restrict__ o = (const T*)a.o;
    const int64_t* __restrict__ col = a.col;
    const int32_t* __restrict__ perm = a.perm;
    const int wave = wave_of_grid();
    if (wave >= a.nwaves) return;
    const int64_t items = a.N * a.hblocks;
    const int ldq = (int)a.ldq;
    const int HC = a.H * a.C;
    const float slope = a.slope, rs = a.row_slope;
    const int hb = __builtin_amdgcn_readfirstlane(wave % a.hblocks);
    const Place pl(a.gshift, a.H, a.C, hb);
    const int lane = pl.lane;
    const int hk = pl.head_ok ? pl.h : 0;
    float datt[NCH][VEC];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) datt[k][v] = 0.f;
    float av[HOLD ? NCH : 1][VEC];
    if constexpr (HOLD) {
#pragma unroll
        for (int k = 0; k < NCH; ++k) att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), av[k]);
    }
    for (int64_t it = wave; it < items; it += a.nwaves) {
        const int i = __builtin_amdgcn_readfirstlane((int)(it / a.hblocks));
        const int32_t jb = __builtin_amdgcn_readfirstlane(a.rowptr[i]), je = __builtin_amdgcn_readfirstlane(a.rowptr[i + 1]);
        float gv[HOLD ? NCH : 1][VEC];
        float dpart = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            if (!pl.live<VEC>(k)) continue;
            float gk[VEC], ok_[VEC];
            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
            att_unpack<T, VEC>(att_load_raw<T, VEC>(o + (int64_t)i * a.ldo + pl.off<VEC>(k)), ok_);
            float sub = 0.f;
#pragma unroll
            for (int v = 0; v < VEC; ++v) sub += gk[v] * ok_[v];
            dpart += pl.ok<VEC>(k) ? sub : 0.f;
            if constexpr (HOLD) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) gv[k][v] = gk[v];
            }
        }
        const float delta = group_sum(dpart, a.gshift, lane);                    // sum_c g * out of this head
        const float lse = pl.head_ok ? a.lse[(int64_t)i * a.H + pl.h] : 0.f;
        const float dv = gate_scalar<T>(d + (int64_t)i * a.ldd + hk);
        float dd = 0.f;
        for (int32_t jrun = jb; jrun < je; jrun += 64) {
            const int32_t jrun_end = min(jrun + 64, je);
            const RunIds ids = run_ids(col, perm, jrun, je, lane, true);   // always: erow is the row of gq
            const int cl = ids.cl, el = ids.el;   // under the names the inline steps below use: their text, and so their schedule, stays as it was
            for (int32_t j = jrun; j < jrun_end; j += U) {
                int64_t qrow[U], erow[U], krow[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    qrow[u] = (int64_t)__builtin_amdgcn_readlane(cl, (j - jrun + u) & 63) * ldq;
                    const int64_t e = __builtin_amdgcn_readlane(el, (j - jrun + u) & 63);
                    erow[u] = e * HC;                   // always: the row of gq
                    krow[u] = (HASC || ks) ? e * a.H : 0;
                    asm volatile("" : "+s"(qrow[u]));
                    asm volatile("" : "+s"(erow[u]));
                }
                u32x4 qr[U][NCH], ur[HASU ? U : 1][HASU ? NCH : 1];
                float kv[U], cv[HASC ? U : 1];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    kv[u] = 1.f;
                    if (j + u < jrun_end) {
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            qr[u][k] = att_load_raw<T, VEC>(q + qrow[u] + pl.off<VEC>(k));
                            if constexpr (HASU) ur[u][k] = att_load_raw<T, VEC>(ue + erow[u] + pl.off<VEC>(k));
                        }
                        if (ks) kv[u] = gate_scalar<T>(ks + krow[u] + hk);
                        if constexpr (HASC) cv[u] = gate_scalar<T>(ce + krow[u] + hk);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u >= jrun_end) continue;
                    float spart = 0.f, dapart = 0.f;
#pragma unroll
                    for (int k = 0; k < NCH; ++k) {
                        if (!pl.live<VEC>(k)) continue;
                        float t[VEC], ak[VEC], gk[VEC];
                        gate_row<T, VEC, HASU>(qr[u][k], ur[HASU ? u : 0][HASU ? k : 0], t);
                        if constexpr (!HOLD) {
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), ak);
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
                        }
                        float s1 = 0.f, s2 = 0.f;
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            const float r = t[v] > 0.f ? t[v] : t[v] * rs;
                            s1 += (HOLD ? av[k][v] : ak[v]) * r;
                            s2 += (HOLD ? gv[k][v] : gk[v]) * r;
                        }
                        const bool ok = pl.ok<VEC>(k);
                        spart += ok ? s1 : 0.f;
                        dapart += ok ? s2 : 0.f;
                    }
                    float pre = group_sum(spart, a.gshift, lane) + dv;
                    if constexpr (HASC) pre = pre + cv[u];
                    const float da = kv[u] * group_sum(dapart, a.gshift, lane);
                    const float w = expf((pre > 0.f ? pre : pre * slope) - lse);
                    const float ds = w * (da - delta);
                    const float dpre = ds * (pre > 0.f ? 1.f : slope);
                    const float wk = w * kv[u];
                    dd = dd + dpre;
                    if constexpr (HASC) {
                        if (pl.head_ok && pl.gl == 0) att_store<T, 1>((T*)a.gc + krow[u] + pl.h, &dpre);   // d c = d pre, row = original edge id
                    }
#pragma unroll
                    for (int k = 0; k < NCH; ++k) {
                        if (!pl.live<VEC>(k)) continue;
                        float t[VEC], ak[VEC], gk[VEC], row[VEC];
                        gate_row<T, VEC, HASU>(qr[u][k], ur[HASU ? u : 0][HASU ? k : 0], t);
                        if constexpr (!HOLD) {
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(att + pl.off<VEC>(k)), ak);
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
                        }
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            datt[k][v] = datt[k][v] + dpre * (t[v] > 0.f ? t[v] : t[v] * rs);
                            row[v] = (wk * (HOLD ? gv[k][v] : gk[v]) + dpre * (HOLD ? av[k][v] : ak[v])) * (t[v] > 0.f ? 1.f : rs);
                        }
                        if (pl.ok<VEC>(k)) att_store<T, VEC>((T*)a.gq + erow[u] + pl.off<VEC>(k), row);
                    }
                }
            }
        }
        if (pl.head_ok && pl.gl == 0) att_store<T, 1>((T*)a.dd + (int64_t)i * a.H + pl.h, &dd);
    }
    float* prow = a.partial + (int64_t)(wave / a.hblocks) * HC;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (!pl.live<VEC>(k) || !pl.ok<VEC>(k)) continue;
#pragma unroll
        for (int v = 0; v < VEC; ++v) prow[pl.off<VEC>(k) + v] = datt[k][v];
    }
}

// ---- TransformerConv: scaled dot-product attention ---------------------------------------------------------------------------
// The third member (gnnops.conv.edge_attention_dot: TransformerConv, Shi et al. 2021). The score is a dot product of the destination's
// query row with the edge's key row, and the message is a second gathered row, the value:
//   kk[e,h,:] = k[j,h,:] (+ u[e,h,:])      vv[e,h,:] = v[j,h,:] (+ u[e,h,:])      s[e,h] = scale * qry[i,h,:] . kk[e,h,:]
//   out[i,h,:] = sum_{e into i} exp(s[e,h] - lse[i,h]) * ks[e,h] * vv[e,h,:]
// k and v are two pointers into rows of one pitch (two column blocks of one product), so an edge has one row base for both; u
// [E, H * C] and ks [E, H] (the attention dropout scale, in the weighted sum only) are read through perm as the gate kernels' are.
// The same layout, id hand-out, group sums and online softmax as above; the qry row of the destination is held as p is. There is
// no att vector: the backward has no partial sums across destinations, no second kernel and no workspace, and takes the forward's
// grid. It writes ONE [E, 2 * H * C] tensor gkv, row = original edge id: the k half ds * scale * qry[i], the v half a * ks * g[i]
// (d k and d v = one segment sum over the source plan), with u also gu = the sum of the halves; d qry is summed in registers.
struct DotArgs {
    const void *qry, *k, *v, *u, *ks, *g, *o;   // u [E, H * C], ks [E, H] (edge_scale): rows = ORIGINAL edge ids, either may be null
    void* gu;                                   // d u [E, H * C], rows = original edge ids (backward with u only)
    const int32_t *rowptr, *perm;
    const int64_t* col;
    void *out, *dq, *gkv;                       // dq: d qry [N, H * C]; gkv [E, 2 * H * C], rows = original edge ids
    float* lse;
    int64_t N, ldq, ldkv, ldo, ldg;
    int H, C, gshift, hblocks, nwaves;
    float scale;
};

// edges per step: an edge brings two raw rows, three with u, and every raw row of a step is in flight before the first is consumed.
// Forward 8 / 12 pieces per lane in flight (AttUnroll holds 8 / 8 + 4); backward, where an edge also stores two or three rows, half.
template <int NCH, bool HASU> struct DotUnroll {
    static constexpr int FW = NCH == 1 ? 4 : NCH == 2 ? 2 : 1;
    static constexpr int BW = HASU ? 1 : (NCH == 1 ? 2 : 1);
};

template <typename T, int VEC, int NCH, bool HASU>
__global__ __launch_bounds__(256) void dot_fwd_kernel(const DotArgs a) {
    constexpr int U = DotUnroll<NCH, HASU>::FW;
    constexpr bool HOLD = NCH <= 4;   // the qry pieces stay in registers
    const T* __restrict__ qry = (const T*)a.qry;
    const T* __restrict__ kp = (const T*)a.k;
    const T* __restrict__ vp = (const T*)a.v;
    const T* __restrict__ ue = (const T*)a.u;
    const T* __restrict__ ks = (const T*)a.ks;
    const int wave = wave_of_grid();
    const int64_t items = a.N * a.hblocks;
    const int ldkv = (int)a.ldkv;
    const int HC = a.H * a.C;
    const float sc = a.scale;
    const bool by_edge = HASU || ks != nullptr;   // something is read by original edge id
    const float NEG_INF = -__builtin_huge_valf();
    for (int64_t it = wave; it < items; it += a.nwaves) {
        const Item t = item_of(it, a.hblocks, a.rowptr);
        const int i = t.i;
        const Place pl(a.gshift, a.H, a.C, t.hb);
        const int lane = pl.lane;
        const int hk = pl.head_ok ? pl.h : 0;
        float qv[HOLD ? NCH : 1][VEC];
        if constexpr (HOLD) hold_row<T, VEC>(qry + (int64_t)i * a.ldq, pl, qv);
        float acc[NCH][VEC];
        zero_pieces(acc);
        float m = NEG_INF, l = 0.f;
        for (int32_t jrun = t.jb; jrun < t.je; jrun += 64) {
            const int32_t jrun_end = min(jrun + 64, t.je);
            const RunIds ids = run_ids(a.col, a.perm, jrun, t.je, lane, by_edge);
            for (int32_t j = jrun; j < jrun_end; j += U) {
                int64_t srow[U], erow[HASU ? U : 1], krow[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    srow[u] = run_id(ids.cl, j - jrun + u) * ldkv;   // one base for the k and the v row
                    asm volatile("" : "+s"(srow[u]));   // the row bases are computed HERE, ahead of every row load
                    krow[u] = 0;
                    if (by_edge) {
                        const int64_t e = run_id(ids.el, j - jrun + u);
                        krow[u] = e * a.H;
                        if constexpr (HASU) {
                            erow[u] = e * HC;
                            asm volatile("" : "+s"(erow[u]));
                        }
                    }
                }
                u32x4 kr[U][NCH], vr[U][NCH], ur[HASU ? U : 1][HASU ? NCH : 1];
                float kv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {           // every row load of the step in flight before the first is consumed
                    kv[u] = 1.f;
                    if (j + u < jrun_end) {
                        fetch_row<T, VEC>(kp + srow[u], pl, kr[u]);
                        fetch_row<T, VEC>(vp + srow[u], pl, vr[u]);
                        if constexpr (HASU) fetch_row<T, VEC>(ue + erow[u], pl, ur[u]);
                        if (ks) kv[u] = gate_scalar<T>(ks + krow[u] + hk);
                    }
                }
                float s[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    s[u] = 0.f;
                    if (j + u < jrun_end) {
                        float part = 0.f;
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            float t[VEC], qk[VEC];
                            gate_row<T, VEC, HASU>(kr[u][k], ur[HASU ? u : 0][HASU ? k : 0], t);
                            if constexpr (!HOLD) att_unpack<T, VEC>(att_load_raw<T, VEC>(qry + (int64_t)i * a.ldq + pl.off<VEC>(k)), qk);
                            float sub = 0.f;
#pragma unroll
                            for (int v = 0; v < VEC; ++v) sub += (HOLD ? qv[k][v] : qk[v]) * t[v];
                            part += pl.ok<VEC>(k) ? sub : 0.f;
                        }
                        s[u] = sc * group_sum(part, a.gshift, lane);
                    }
                }
                softmax_raise(s, j, jrun_end, m, l, acc);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < jrun_end) {
                        const float w = expf(s[u] - m);
                        l = l + w;                      // the denominator never sees the scale: dropout comes after the softmax
                        const float wk = w * kv[u];
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            float t[VEC];
                            gate_row<T, VEC, HASU>(vr[u][k], ur[HASU ? u : 0][HASU ? k : 0], t);
#pragma unroll
                            for (int v = 0; v < VEC; ++v) acc[k][v] = acc[k][v] + wk * t[v];
                        }
                    }
                }
            }
        }
        store_destination<T, VEC>(pl, t.je > t.jb, m, l, acc, (T*)a.out + (int64_t)i * a.ldo, a.lse + (int64_t)i * a.H, NEG_INF);
    }
}

// Backward: the forward's walk (one wave per destination and head block, any wave any head block: nothing is carried from one
// destination to the next). Every edge stands alone: s is recomputed, a = exp(s - lse), ds = a * (ks * (g . vv) - D).
template <typename T, int VEC, int NCH, bool HASU>
__global__ __launch_bounds__(256) void dot_bwd_kernel(const DotArgs a) {
    constexpr int U = DotUnroll<NCH, HASU>::BW;
    constexpr bool HOLD = NCH <= 4;   // the qry and g pieces stay in registers
    const T* __restrict__ qry = (const T*)a.qry;
    const T* __restrict__ kp = (const T*)a.k;
    const T* __restrict__ vp = (const T*)a.v;
    const T* __restrict__ ue = (const T*)a.u;
    const T* __restrict__ ks = (const T*)a.ks;
    const T* __restrict__ g = (const T*)a.g;
    const T* __restrict__ o = (const T*)a.o;
    const int64_t* __restrict__ col = a.col;
    const int32_t* __restrict__ perm = a.perm;
    const int wave = wave_of_grid();
    const int64_t items = a.N * a.hblocks;
    const int ldkv = (int)a.ldkv;
    const int HC = a.H * a.C;
    const float sc = a.scale;
    for (int64_t it = wave; it < items; it += a.nwaves) {
        const Item t = item_of(it, a.hblocks, a.rowptr);
        const int i = t.i, hb = t.hb;
        const Place pl(a.gshift, a.H, a.C, hb);
        const int lane = pl.lane;
        const int hk = pl.head_ok ? pl.h : 0;
        const int32_t jb = t.jb, je = t.je;
        float qv[HOLD ? NCH : 1][VEC], gv[HOLD ? NCH : 1][VEC], dq[NCH][VEC];
        float dpart = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) dq[k][v] = 0.f;
            if (!pl.live<VEC>(k)) continue;
            float gk[VEC], ok_[VEC];
            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
            att_unpack<T, VEC>(att_load_raw<T, VEC>(o + (int64_t)i * a.ldo + pl.off<VEC>(k)), ok_);
            float sub = 0.f;
#pragma unroll
            for (int v = 0; v < VEC; ++v) sub += gk[v] * ok_[v];
            dpart += pl.ok<VEC>(k) ? sub : 0.f;
            if constexpr (HOLD) {
                att_unpack<T, VEC>(att_load_raw<T, VEC>(qry + (int64_t)i * a.ldq + pl.off<VEC>(k)), qv[k]);
#pragma unroll
                for (int v = 0; v < VEC; ++v) gv[k][v] = gk[v];
            }
        }
        const float delta = group_sum(dpart, a.gshift, lane);                    // D = sum_c g * out of this head
        const float lse = pl.head_ok ? a.lse[(int64_t)i * a.H + pl.h] : 0.f;
        for (int32_t jrun = jb; jrun < je; jrun += 64) {
            const int32_t jrun_end = min(jrun + 64, je);
            const RunIds ids = run_ids(col, perm, jrun, je, lane, true);
            const int cl = ids.cl, el = ids.el;   // under the names the inline steps below use: their text, and so their schedule, stays as it was
            for (int32_t j = jrun; j < jrun_end; j += U) {
                int64_t srow[U], erow[U], krow[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    srow[u] = run_id(cl, j - jrun + u) * ldkv;
                    const int64_t e = run_id(el, j - jrun + u);
                    erow[u] = e * HC;                   // always: the row of gkv is 2 * erow
                    krow[u] = ks ? e * a.H : 0;
                    asm volatile("" : "+s"(srow[u]));
                    asm volatile("" : "+s"(erow[u]));
                }
                u32x4 kr[U][NCH], vr[U][NCH], ur[HASU ? U : 1][HASU ? NCH : 1];
                float kv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    kv[u] = 1.f;
                    if (j + u < jrun_end) {
#pragma unroll
                        for (int k = 0; k < NCH; ++k) {
                            if (!pl.live<VEC>(k)) continue;
                            kr[u][k] = att_load_raw<T, VEC>(kp + srow[u] + pl.off<VEC>(k));
                            vr[u][k] = att_load_raw<T, VEC>(vp + srow[u] + pl.off<VEC>(k));
                            if constexpr (HASU) ur[u][k] = att_load_raw<T, VEC>(ue + erow[u] + pl.off<VEC>(k));
                        }
                        if (ks) kv[u] = gate_scalar<T>(ks + krow[u] + hk);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u >= jrun_end) continue;
                    float spart = 0.f, dapart = 0.f;
#pragma unroll
                    for (int k = 0; k < NCH; ++k) {
                        if (!pl.live<VEC>(k)) continue;
                        float tk[VEC], tv[VEC], qk[VEC], gk[VEC];
                        gate_row<T, VEC, HASU>(kr[u][k], ur[HASU ? u : 0][HASU ? k : 0], tk);
                        gate_row<T, VEC, HASU>(vr[u][k], ur[HASU ? u : 0][HASU ? k : 0], tv);
                        if constexpr (!HOLD) {
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(qry + (int64_t)i * a.ldq + pl.off<VEC>(k)), qk);
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
                        }
                        float s1 = 0.f, s2 = 0.f;
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            s1 += (HOLD ? qv[k][v] : qk[v]) * tk[v];
                            s2 += (HOLD ? gv[k][v] : gk[v]) * tv[v];
                        }
                        const bool ok = pl.ok<VEC>(k);
                        spart += ok ? s1 : 0.f;
                        dapart += ok ? s2 : 0.f;
                    }
                    const float s = sc * group_sum(spart, a.gshift, lane);
                    const float da = kv[u] * group_sum(dapart, a.gshift, lane);
                    const float w = expf(s - lse);
                    const float ds = w * (da - delta);
                    const float dss = ds * sc, wk = w * kv[u];
#pragma unroll
                    for (int k = 0; k < NCH; ++k) {
                        if (!pl.live<VEC>(k)) continue;
                        float tk[VEC], qk[VEC], gk[VEC], rk[VEC], rv[VEC], ru[VEC];
                        gate_row<T, VEC, HASU>(kr[u][k], ur[HASU ? u : 0][HASU ? k : 0], tk);
                        if constexpr (!HOLD) {
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(qry + (int64_t)i * a.ldq + pl.off<VEC>(k)), qk);
                            att_unpack<T, VEC>(att_load_raw<T, VEC>(g + (int64_t)i * a.ldg + pl.off<VEC>(k)), gk);
                        }
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            dq[k][v] = dq[k][v] + ds * tk[v];
                            rk[v] = dss * (HOLD ? qv[k][v] : qk[v]);
                            rv[v] = wk * (HOLD ? gv[k][v] : gk[v]);
                            ru[v] = rk[v] + rv[v];
                        }
                        if (pl.ok<VEC>(k)) {
                            att_store<T, VEC>((T*)a.gkv + 2 * erow[u] + pl.off<VEC>(k), rk);
                            att_store<T, VEC>((T*)a.gkv + 2 * erow[u] + HC + pl.off<VEC>(k), rv);
                            if constexpr (HASU) att_store<T, VEC>((T*)a.gu + erow[u] + pl.off<VEC>(k), ru);   // d u, row = original edge id
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            if (!pl.live<VEC>(k) || !pl.ok<VEC>(k)) continue;
            float r[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) r[v] = sc * dq[k][v];
            att_store<T, VEC>((T*)a.dq + (int64_t)i * HC + pl.off<VEC>(k), r);
        }
    }
}

struct Geometry { int vec, nch, gshift, hblocks; };

// widest piece the operands allow, narrowed while the heads of a row leave half the wave idle; NCH pieces per lane
inline Geometry geometry(int H, int C, int max_vec, int es) {
    int vec = max_vec;
    while (vec > 1 && C % vec != 0) vec >>= 1;
    auto gshift_of = [&](int v) { int s = 0; while ((1 << s) < C / v && s < 6) ++s; return s; };
    while (vec > 1 && vec * es > 4 && (int64_t)H << gshift_of(vec) <= 32 && C / vec <= 32) vec >>= 1;
    Geometry g{};
    const int pieces = C / vec;
    g.vec = vec;
    g.gshift = gshift_of(vec);
    g.nch = pieces <= 64 ? 1 : pieces <= 128 ? 2 : pieces <= 256 ? 4 : 128;
    if (g.nch == 128) { g.vec = 1; g.gshift = 6; }   // 64 lanes x 128 single elements: any C <= 8192
    const int hp = 64 >> g.gshift;
    g.hblocks = (H + hp - 1) / hp;
    return g;
}

inline int rows_of_partials(int64_t N, int H, int C) {
    const int64_t HC = (int64_t)H * C;
    int64_t rows = ((int64_t)1 << 22) / HC;            // 16 MiB of fp32 partials at the most
    rows = rows < 256 ? 256 : rows > 2048 ? 2048 : rows;
    if (rows > N) rows = N;
    return (int)(rows < 1 ? 1 : rows);
}

// the forward or the backward kernel of one instance, whatever the family
template <bool BW, typename Args>
void run(void (*fwd)(Args), void (*bwd)(Args), const Args& a, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(BW ? bwd : fwd, dim3(grid), dim3(256), 0, stream, a);
}

// A family names its Args and, for one <T, VEC, NCH>, the instance an operand turns on: the only choice a family makes itself.
struct AttFamily {
    using Args = AttArgs;
    template <typename T, bool BW, int VEC, int NCH>
    static void launch(const Args& a, int grid, hipStream_t stream) {
        if (a.u) run<BW>(attention_fwd_kernel<T, VEC, NCH, true>, attention_bwd_kernel<T, VEC, NCH, true>, a, grid, stream);
        else run<BW>(attention_fwd_kernel<T, VEC, NCH, false>, attention_bwd_kernel<T, VEC, NCH, false>, a, grid, stream);
    }
};

struct GateFamily {
    using Args = GateArgs;
    // the instances with the per-edge score term c are those of GATConv(edge_dim): no per-edge row beside it
    template <typename T, bool BW, int VEC, int NCH>
    static void launch(const Args& a, int grid, hipStream_t stream) {
        if (a.c) run<BW>(gate_fwd_kernel<T, VEC, NCH, false, true>, gate_bwd_kernel<T, VEC, NCH, false, true>, a, grid, stream);
        else if (a.u) run<BW>(gate_fwd_kernel<T, VEC, NCH, true, false>, gate_bwd_kernel<T, VEC, NCH, true, false>, a, grid, stream);
        else run<BW>(gate_fwd_kernel<T, VEC, NCH, false, false>, gate_bwd_kernel<T, VEC, NCH, false, false>, a, grid, stream);
    }
};

struct DotFamily {
    using Args = DotArgs;
    template <typename T, bool BW, int VEC, int NCH>
    static void launch(const Args& a, int grid, hipStream_t stream) {
        if (a.u) run<BW>(dot_fwd_kernel<T, VEC, NCH, true>, dot_bwd_kernel<T, VEC, NCH, true>, a, grid, stream);
        else run<BW>(dot_fwd_kernel<T, VEC, NCH, false>, dot_bwd_kernel<T, VEC, NCH, false>, a, grid, stream);
    }
};

template <typename F, typename T, bool BW, int VEC>
void launch_pieces(const typename F::Args& a, int nch, int grid, hipStream_t stream) {
    if (nch == 1) F::template launch<T, BW, VEC, 1>(a, grid, stream);
    else if (nch == 2) F::template launch<T, BW, VEC, 2>(a, grid, stream);
    else F::template launch<T, BW, VEC, 4>(a, grid, stream);
}

template <typename F, typename T, bool BW>
void launch_typed(const typename F::Args& a, const Geometry& geo, int grid, hipStream_t stream) {
    if (geo.nch == 128) return F::template launch<T, BW, 1, 128>(a, grid, stream);
    gnnops_with_piece_width<T>(geo.vec, [&](auto v) { launch_pieces<F, T, BW, decltype(v)::value>(a, geo.nch, grid, stream); });
}

// what: the entry point's name, for the refusal of a dtype code check_sizes has already refused
template <typename F, bool BW>
int launch(const char* what, const typename F::Args& a, const Geometry& geo, int grid, int dtype, hipStream_t stream) {
    return gnnops_with_dtype(dtype, what, [&](auto t) {
        launch_typed<F, typename decltype(t)::type, BW>(a, geo, grid, stream);
        return (int)GNNOPS_OK;
    });
}

template <typename T>
void launch_datt_typed(const float* partial, int rows, int HC, void* grad_att, hipStream_t stream) {
    hipLaunchKernelGGL(attention_datt_kernel<T>, dim3((unsigned)gnnops_cdiv(HC, 256)), dim3(256), 0, stream, partial, rows, HC, (T*)grad_att);
}

int launch_datt(const char* what, const float* partial, int rows, int HC, void* grad_att, int dtype, hipStream_t stream) {
    return gnnops_with_dtype(dtype, what, [&](auto t) {
        launch_datt_typed<typename decltype(t)::type>(partial, rows, HC, grad_att, stream);
        return (int)GNNOPS_OK;
    });
}

int check_sizes(const char* what, int64_t N, int64_t E, int64_t H, int64_t C, int64_t ldq, int64_t ldp, int dtype, int* es) {
    GNNOPS_REQUIRE(N >= 0 && E >= 0, GNNOPS_EINVAL, "%s: negative size", what);
    GNNOPS_REQUIRE(H >= 1 && C >= 1 && H * C <= 8192, GNNOPS_EINVAL, "%s: needs heads >= 1, channels >= 1 and heads * channels <= 8192 (got %lld x %lld)",
                   what, (long long)H, (long long)C);
    GNNOPS_REQUIRE(N < ((int64_t)1 << 31) && E < ((int64_t)1 << 31) && ldq < ((int64_t)1 << 31), GNNOPS_EUNSUPPORTED,
                   "%s: N, E and the row pitch must be < 2^31", what);
    GNNOPS_REQUIRE(ldq >= H * C && ldp >= H * C, GNNOPS_EINVAL, "%s: a row pitch is shorter than the row", what);
    *es = gnnops_elem_bytes(dtype);
    GNNOPS_REQUIRE(*es, GNNOPS_EINVAL, "%s: unknown dtype %d", what, dtype);
    return GNNOPS_OK;
}

struct Launch { Geometry geo; int rows, grid, nwaves; };   // grid == 0: a valid call with nothing to launch

template <typename Args>
void set_geometry(Args& a, const Launch& l) {
    a.gshift = l.geo.gshift;
    a.hblocks = l.geo.hblocks;
    a.nwaves = l.nwaves;
}

// What the two forward entry points check and choose before they launch. The caller says what only it knows: its name, whether
// its other pitches hold a row, whether it was given the u and c that no instance takes together, whether the pointers it needs
// are there, and the operands that bound the piece width. ldp: the pitch of p, or H * C for the family without p.
int forward_prologue(const char* what, int64_t N, int64_t E, int64_t H, int64_t C, int64_t ldq, int64_t ldp, bool pitches, bool u_and_c,
                     bool pointers, int dtype, Operands operands, Launch* l) {
    int es = 0;
    const int rc = check_sizes(what, N, E, H, C, ldq, ldp, dtype, &es);
    if (rc != GNNOPS_OK) return rc;
    GNNOPS_REQUIRE(pitches, GNNOPS_EINVAL, "%s: a row pitch is shorter than the row", what);
    GNNOPS_REQUIRE(!u_and_c, GNNOPS_EUNSUPPORTED, "%s: a per-edge row u and a per-edge score term c together have no kernel instance", what);
    if (N == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(pointers, GNNOPS_EINVAL, "%s: null pointer", what);
    l->geo = geometry((int)H, (int)C, gnnops_widest_piece(es, operands), es);
    l->grid = gnnops_grid_cap(gnnops_cdiv(N * l->geo.hblocks, 4), 256 * 32);
    l->nwaves = l->grid * 4;
    return GNNOPS_OK;
}

// The same for the two backward entry points. orphan: the name of a per-edge operand given without a place for its gradient, or
// null. One wave per (row of d att partials, head block).
int backward_prologue(const char* what, int64_t N, int64_t E, int64_t H, int64_t C, int64_t ldq, int64_t ldp, bool pitches, bool u_and_c,
                      const void* grad_att, bool pointers, const char* orphan, const void* workspace, size_t workspace_bytes, int dtype,
                      Operands operands, Launch* l) {
    int es = 0;
    const int rc = check_sizes(what, N, E, H, C, ldq, ldp, dtype, &es);
    if (rc != GNNOPS_OK) return rc;
    GNNOPS_REQUIRE(pitches, GNNOPS_EINVAL, "%s: a row pitch is shorter than the row", what);
    GNNOPS_REQUIRE(grad_att, GNNOPS_EINVAL, "%s: null pointer", what);
    GNNOPS_REQUIRE(!u_and_c, GNNOPS_EUNSUPPORTED, "%s: a per-edge row u and a per-edge score term c together have no kernel instance", what);
    if (N == 0) return GNNOPS_OK;   // no destination: nothing is written
    GNNOPS_REQUIRE(pointers, GNNOPS_EINVAL, "%s: null pointer", what);
    GNNOPS_REQUIRE(!orphan, GNNOPS_EINVAL, "%s: %s without a place for its gradient", what, orphan);
    const size_t need = gnnops_edge_attention_backward_workspace_bytes(N, H, C);
    GNNOPS_REQUIRE(workspace && workspace_bytes >= need && (uintptr_t)workspace % 16 == 0, GNNOPS_EWORKSPACE, "%s: workspace %zu < %zu",
                   what, workspace_bytes, need);
    l->geo = geometry((int)H, (int)C, gnnops_widest_piece(es, operands), es);
    l->rows = rows_of_partials(N, (int)H, (int)C);
    l->nwaves = l->rows * l->geo.hblocks;
    l->grid = (int)gnnops_cdiv(l->nwaves, 4);
    return GNNOPS_OK;
}

}  // namespace

extern "C" size_t gnnops_edge_attention_backward_workspace_bytes(int64_t N, int64_t H, int64_t C) {
    if (N <= 0 || H < 1 || C < 1 || H * C > 8192) return 0;
    return (size_t)rows_of_partials(N, (int)H, (int)C) * (size_t)(H * C) * sizeof(float);
}

extern "C" int gnnops_edge_attention(const void* q, int64_t ldq, const void* p, int64_t ldp, const void* att, const void* u,
                                     const int32_t* rowptr, const int32_t* perm, const int64_t* col, void* out, int64_t ldo, float* lse,
                                     int64_t N, int64_t E, int64_t H, int64_t C, float negative_slope, int dtype, gnnops_stream_t s) {
    if (E == 0) u = nullptr;   // no edge: u is never read
    Launch l{};
    const int rc = forward_prologue("edge_attention", N, E, H, C, ldq, ldp, ldo >= H * C, false,
                                    rowptr && out && lse && p && att && (E == 0 || (q && col)), dtype,
                                    {{q, ldq}, {p, ldp}, {att, 0}, {u, H * C}, {out, ldo}}, &l);
    if (rc != GNNOPS_OK || !l.grid) return rc;
    AttArgs a{};
    a.q = q; a.p = p; a.att = att; a.u = u; a.rowptr = rowptr; a.perm = perm; a.col = col; a.out = out; a.lse = lse;
    a.N = N; a.ldq = ldq; a.ldp = ldp; a.ldo = ldo; a.H = (int)H; a.C = (int)C; a.slope = negative_slope;
    set_geometry(a, l);
    if (const int rc = launch<AttFamily, false>("edge_attention", a, l.geo, l.grid, dtype, (hipStream_t)s)) return rc;
    return gnnops_check_launch("edge_attention");
}

extern "C" int gnnops_edge_attention_backward(const void* q, int64_t ldq, const void* p, int64_t ldp, const void* att, const void* u,
                                              const void* out, int64_t ldo, const float* lse, const void* grad_out, int64_t ldg,
                                              const int32_t* rowptr, const int32_t* perm, const int64_t* col, void* grad_p, void* gq,
                                              void* gu, void* grad_att, int64_t N, int64_t E, int64_t H, int64_t C, float negative_slope,
                                              int dtype, void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    if (E == 0) u = nullptr;   // no edge: u is never read, gu never written
    Launch l{};
    const int rc = backward_prologue("edge_attention_backward", N, E, H, C, ldq, ldp, ldo >= H * C && (ldg >= H * C || ldg == 0), false, grad_att,
                                     rowptr && out && lse && p && att && grad_out && grad_p && (E == 0 || (q && col && gq)),
                                     u && !gu ? "u" : nullptr, workspace, workspace_bytes, dtype,
                                     {{q, ldq}, {p, ldp}, {att, 0}, {out, ldo}, {grad_out, ldg}, {grad_p, H * C}, {gq, H * C}, {u, H * C},
                                      {u ? gu : nullptr, H * C}}, &l);
    if (rc != GNNOPS_OK || !l.grid) return rc;
    AttArgs a{};
    a.q = q; a.p = p; a.att = att; a.u = u; a.g = grad_out; a.o = out; a.rowptr = rowptr; a.perm = perm; a.col = col;
    a.dp = grad_p; a.gq = gq; a.gu = gu; a.lse = const_cast<float*>(lse); a.partial = (float*)workspace;
    a.N = N; a.ldq = ldq; a.ldp = ldp; a.ldo = ldo; a.ldg = ldg; a.H = (int)H; a.C = (int)C; a.slope = negative_slope;
    set_geometry(a, l);
    if (const int rc = launch<AttFamily, true>("edge_attention_backward", a, l.geo, l.grid, dtype, (hipStream_t)s)) return rc;
    if (const int rc = launch_datt("edge_attention_backward", a.partial, l.rows, (int)(H * C), grad_att, dtype, (hipStream_t)s)) return rc;
    return gnnops_check_launch("edge_attention_backward");
}

extern "C" int gnnops_edge_attention_v1(const void* q, int64_t ldq, const void* d, int64_t ldd, const void* att, const void* u,
                                        const void* c, const void* edge_scale, const int32_t* rowptr, const int32_t* perm,
                                        const int64_t* col, void* out, int64_t ldo, float* lse, int64_t N, int64_t E, int64_t H, int64_t C,
                                        int has_row_slope, float row_slope, float negative_slope, int dtype, gnnops_stream_t s) {
    Launch l{};
    const int rc = forward_prologue("edge_attention_v1", N, E, H, C, ldq, H * C, ldo >= H * C && ldd >= H, u && c,
                                    rowptr && out && lse && d && att && (E == 0 || (q && col)), dtype,
                                    {{q, ldq}, {att, 0}, {u, H * C}, {out, ldo}}, &l);
    if (rc != GNNOPS_OK || !l.grid) return rc;
    GateArgs a{};
    a.q = q; a.d = d; a.att = att; a.u = E ? u : nullptr; a.c = E ? c : nullptr; a.ks = E ? edge_scale : nullptr;
    a.rowptr = rowptr; a.perm = perm; a.col = col;
    a.out = out; a.lse = lse;
    a.N = N; a.ldq = ldq; a.ldd = ldd; a.ldo = ldo; a.H = (int)H; a.C = (int)C;
    a.slope = negative_slope; a.row_slope = has_row_slope ? row_slope : 1.f;
    set_geometry(a, l);
    if (const int rc = launch<GateFamily, false>("edge_attention_v1", a, l.geo, l.grid, dtype, (hipStream_t)s)) return rc;
    return gnnops_check_launch("edge_attention_v1");
}

extern "C" int gnnops_edge_attention_v1_backward(const void* q, int64_t ldq, const void* d, int64_t ldd, const void* att, const void* u,
                                                 const void* c, const void* edge_scale, const void* out, int64_t ldo, const float* lse,
                                                 const void* grad_out, int64_t ldg, const int32_t* rowptr, const int32_t* perm,
                                                 const int64_t* col, void* grad_d, void* gq, void* gc, void* grad_att, int64_t N,
                                                 int64_t E, int64_t H, int64_t C, int has_row_slope, float row_slope,
                                                 float negative_slope, int dtype, void* workspace, size_t workspace_bytes,
                                                 gnnops_stream_t s) {
    Launch l{};
    const int rc = backward_prologue("edge_attention_v1_backward", N, E, H, C, ldq, H * C,
                                     ldo >= H * C && ldd >= H && (ldg >= H * C || ldg == 0), u && c, grad_att,
                                     rowptr && out && lse && d && att && grad_out && grad_d && (E == 0 || (q && col && gq)),
                                     E != 0 && c && !gc ? "c" : nullptr, workspace, workspace_bytes, dtype,
                                     {{q, ldq}, {att, 0}, {u, H * C}, {out, ldo}, {grad_out, ldg}, {gq, H * C}}, &l);
    if (rc != GNNOPS_OK || !l.grid) return rc;
    GateArgs a{};
    a.q = q; a.d = d; a.att = att; a.u = E ? u : nullptr; a.c = E ? c : nullptr; a.ks = E ? edge_scale : nullptr; a.g = grad_out; a.o = out;
    a.rowptr = rowptr; a.perm = perm; a.col = col;
    a.dd = grad_d; a.gq = gq; a.gc = gc; a.lse = const_cast<float*>(lse); a.partial = (float*)workspace;
    a.N = N; a.ldq = ldq; a.ldd = ldd; a.ldo = ldo; a.ldg = ldg; a.H = (int)H; a.C = (int)C;
    a.slope = negative_slope; a.row_slope = has_row_slope ? row_slope : 1.f;
    set_geometry(a, l);
    if (const int rc = launch<GateFamily, true>("edge_attention_v1_backward", a, l.geo, l.grid, dtype, (hipStream_t)s)) return rc;
    if (const int rc = launch_datt("edge_attention_v1_backward", a.partial, l.rows, (int)(H * C), grad_att, dtype, (hipStream_t)s)) return rc;
    return gnnops_check_launch("edge_attention_v1_backward");
}

// The third family has no att vector, hence no d att partials and no workspace: its backward walks the forward's grid, one wave
// per (destination, head block), and both directions take forward_prologue (the gathered pitch ldkv where the others pass ldq, the
// pitch of qry where the first family passes ldp). orphan as in backward_prologue.
namespace {
int dot_prologue(const char* what, int64_t N, int64_t E, int64_t H, int64_t C, int64_t ldq, int64_t ldkv, bool pitches, bool pointers,
                 const char* orphan, int dtype, Operands operands, Launch* l) {
    const int rc = forward_prologue(what, N, E, H, C, ldkv, ldq, pitches, false, pointers, dtype, operands, l);
    if (rc != GNNOPS_OK || !l->grid) return rc;
    GNNOPS_REQUIRE(ldq < ((int64_t)1 << 31), GNNOPS_EUNSUPPORTED, "%s: N, E and the row pitch must be < 2^31", what);
    GNNOPS_REQUIRE(!orphan, GNNOPS_EINVAL, "%s: %s without a place for its gradient", what, orphan);
    return GNNOPS_OK;
}
}  // namespace

extern "C" int gnnops_edge_attention_dot(const void* qry, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* u,
                                         const void* edge_scale, const int32_t* rowptr, const int32_t* perm, const int64_t* col,
                                         void* out, int64_t ldo, float* lse, int64_t N, int64_t E, int64_t H, int64_t C, float scale,
                                         int dtype, gnnops_stream_t s) {
    if (E == 0) u = edge_scale = nullptr;   // no edge: neither is read
    Launch l{};
    const int rc = dot_prologue("edge_attention_dot", N, E, H, C, ldq, ldkv, ldo >= H * C,
                                rowptr && out && lse && qry && (E == 0 || (k && v && col)), nullptr, dtype,
                                {{qry, ldq}, {k, ldkv}, {v, ldkv}, {u, H * C}, {out, ldo}}, &l);
    if (rc != GNNOPS_OK || !l.grid) return rc;
    DotArgs a{};
    a.qry = qry; a.k = k; a.v = v; a.u = u; a.ks = edge_scale; a.rowptr = rowptr; a.perm = perm; a.col = col; a.out = out; a.lse = lse;
    a.N = N; a.ldq = ldq; a.ldkv = ldkv; a.ldo = ldo; a.H = (int)H; a.C = (int)C; a.scale = scale;
    set_geometry(a, l);
    if (const int rc = launch<DotFamily, false>("edge_attention_dot", a, l.geo, l.grid, dtype, (hipStream_t)s)) return rc;
    return gnnops_check_launch("edge_attention_dot");
}

extern "C" int gnnops_edge_attention_dot_backward(const void* qry, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* u,
                                                  const void* edge_scale, const void* out, int64_t ldo, const float* lse,
                                                  const void* grad_out, int64_t ldg, const int32_t* rowptr, const int32_t* perm,
                                                  const int64_t* col, void* grad_qry, void* gkv, void* gu, int64_t N, int64_t E, int64_t H,
                                                  int64_t C, float scale, int dtype, gnnops_stream_t s) {
    if (E == 0) u = edge_scale = nullptr;   // no edge: neither is read, gu never written
    Launch l{};
    const int rc = dot_prologue("edge_attention_dot_backward", N, E, H, C, ldq, ldkv, ldo >= H * C && (ldg >= H * C || ldg == 0),
                                rowptr && out && lse && qry && grad_out && grad_qry && (E == 0 || (k && v && col && gkv)),
                                u && !gu ? "u" : nullptr, dtype,
                                {{qry, ldq}, {k, ldkv}, {v, ldkv}, {u, H * C}, {out, ldo}, {grad_out, ldg}, {grad_qry, H * C}, {gkv, 2 * H * C},
                                 {u ? gu : nullptr, H * C}}, &l);
    if (rc != GNNOPS_OK || !l.grid) return rc;
    DotArgs a{};
    a.qry = qry; a.k = k; a.v = v; a.u = u; a.ks = edge_scale; a.g = grad_out; a.o = out; a.rowptr = rowptr; a.perm = perm; a.col = col;
    a.dq = grad_qry; a.gkv = gkv; a.gu = gu; a.lse = const_cast<float*>(lse);
    a.N = N; a.ldq = ldq; a.ldkv = ldkv; a.ldo = ldo; a.ldg = ldg; a.H = (int)H; a.C = (int)C; a.scale = scale;
    set_geometry(a, l);
    if (const int rc = launch<DotFamily, true>("edge_attention_dot_backward", a, l.geo, l.grid, dtype, (hipStream_t)s)) return rc;
    return gnnops_check_launch("edge_attention_dot_backward");
}
