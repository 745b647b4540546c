// norm.hip — what sits between two attention passes of the GATv2 model, in ONE pass over the rows, and its backward
// (gnnops.conv.head_act_norm; gnnops.conv.GATv2): the mean over heads, the bias, ReLU, the feature-dropout mask and LayerNorm.
//
//   y[c]  = (a[i,0,c] + a[i,1,c] + ... + a[i,H-1,c]) / H (+ bias[c])     fp32, heads in ascending order, a true division
//   r[c]  = relu ? max(y[c], 0) : y[c]
//   d[c]  = r[c] * k[i,c]                                                 k optional: the mask, already divided by 1 - p
//   norm: mu = mean_c d, var = mean_c (d - mu)^2 (two passes over the held row), out = (d - mu) * rstd * gamma[c] (+ beta[c])
//   else: out = d
//
// Layout (attention.hip's): one group of G = 2^gshift lanes per ROW, 64 / G rows per wave, lane gl of a group on the columns
// (k * G + gl) * VEC .. + VEC, k < NCH, 16-byte loads where the operands allow; the two row sums are group_sum's DPP butterfly
// with every lane active (a group past the last row works on zeros). Rows of more than 256 pieces take the NCH = 0 instance:
// 64 lanes x single elements, the row recomputed from a (cache hits) in each pass instead of held.
//
// Algorithmic bytes, forward: N * C * (H + 1 [+ 1 for k]) elements + 8 N for (mu, rstd) when a gradient is wanted. Nothing else
// is saved: the backward re-reads a, bias and k and recomputes y, the gate and xhat: N * C * (H [+ 1] + 1 for g) read and
// N * C * H written. d bias / d gamma / d beta: every lane group keeps fp32 partials over its rows (registers; the wide
// instance keeps them in its own row of the workspace), writes one row of [groups, 3, C], and a second small kernel adds the
// rows in a fixed order: no atomics, the same bits every run.
#include "common.h"
#include "lane_group.h"
#include "dispatch.h"

namespace {

struct NormArgs {
    const void *a, *bias, *k, *gamma, *beta, *g;
    void *out, *da;
    float *stats, *partial;      // stats [N, 2] = (mu, rstd); partial [groups, 3, C]
    int64_t N, lda, ldg;
    int H, C, gshift, nwaves, nk;
    int relu, norm;
    float eps;
};

template <typename T, int VEC>
__device__ inline void row_load(const T* p, float* f) {
    constexpr int BYTES = VEC * (int)sizeof(T);
    if constexpr (VEC == 1) {
        f[0] = Elem<T>::load(p);
    } else {
        u32x4 r = {0u, 0u, 0u, 0u};
        if constexpr (BYTES == 16) {
            r = load16<false>(p);
        } else if constexpr (BYTES == 8) {
            const uint2 t = *reinterpret_cast<const uint2*>(p);
            r.x = t.x; r.y = t.y;
        } else {
            r.x = *reinterpret_cast<const uint32_t*>(p);
        }
        float g[Elem<T>::VEC];
        Elem<T>::unpack(r, g);
#pragma unroll
        for (int v = 0; v < VEC; ++v) f[v] = g[v];
    }
}
template <typename T, int VEC>
__device__ inline void row_store(T* p, const float* f) {
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

// One piece of row i at column c0: d (the value the norm sees) and m = d d / d y (the ReLU gate times the mask). A lane
// without a piece (!ok) gets zeros and reads nothing.
template <typename T, int VEC>
__device__ inline void piece(const NormArgs& a, int64_t i, int c0, bool ok, float* d, float* m) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) { d[v] = 0.f; m[v] = 0.f; }
    if (!ok) return;
    const T* row = (const T*)a.a + i * a.lda + c0;
    float y[VEC], t[VEC];
    row_load<T, VEC>(row, y);
    for (int h = 1; h < a.H; ++h) {
        row_load<T, VEC>(row + (int64_t)h * a.C, t);
#pragma unroll
        for (int v = 0; v < VEC; ++v) y[v] = y[v] + t[v];
    }
    const float Hf = (float)a.H;
#pragma unroll
    for (int v = 0; v < VEC; ++v) y[v] = y[v] / Hf;
    if (a.bias) {
        row_load<T, VEC>((const T*)a.bias + c0, t);
#pragma unroll
        for (int v = 0; v < VEC; ++v) y[v] = y[v] + t[v];
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) t[v] = 1.f;
    if (a.k) row_load<T, VEC>((const T*)a.k + i * a.C + c0, t);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const bool open = !a.relu || y[v] > 0.f;
        const float r = a.relu && y[v] < 0.f ? 0.f : y[v];
        d[v] = r * t[v];
        m[v] = open ? t[v] : 0.f;
    }
}

template <typename T, int VEC, int NCH>
__global__ __launch_bounds__(256) void head_act_norm_fwd_kernel(const NormArgs a) {
    constexpr bool HOLD = NCH > 0;
    constexpr int NH = HOLD ? NCH : 1, UNR = NH;      // the held pieces unroll; the wide instance loops
    const int wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int lane = threadIdx.x & 63, G = 1 << a.gshift, gl = lane & (G - 1), sub = lane >> a.gshift, R = 64 >> a.gshift;
    const int nk = HOLD ? NCH : a.nk, C = a.C;
    const float Cf = (float)C;
    T* __restrict__ out = (T*)a.out;
    for (int64_t base = (int64_t)wave * R; base < a.N; base += (int64_t)a.nwaves * R) {   // wave-uniform: every lane stays in
        const int64_t i = base + sub;
        const bool row_ok = i < a.N;
        float d[NH][VEC], m[VEC];
        float part = 0.f;
#pragma unroll UNR
        for (int k = 0; k < nk; ++k) {
            const int c0 = (k * G + gl) * VEC;
            const bool ok = row_ok && c0 < C;
            float* dk = d[HOLD ? k : 0];
            piece<T, VEC>(a, i, c0, ok, dk, m);
#pragma unroll
            for (int v = 0; v < VEC; ++v) part = part + dk[v];
            if (!a.norm && ok) row_store<T, VEC>(out + i * C + c0, dk);
        }
        if (!a.norm) continue;
        const float mu = group_sum(part, a.gshift, lane) / Cf;
        part = 0.f;
#pragma unroll UNR
        for (int k = 0; k < nk; ++k) {
            const int c0 = (k * G + gl) * VEC;
            const bool ok = row_ok && c0 < C;
            float* dk = d[HOLD ? k : 0];
            if constexpr (!HOLD) piece<T, VEC>(a, i, c0, ok, dk, m);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float e = dk[v] - mu;
                part = part + (ok ? e * e : 0.f);
            }
        }
        const float var = group_sum(part, a.gshift, lane) / Cf;
        const float rstd = 1.f / sqrtf(var + a.eps);
#pragma unroll UNR
        for (int k = 0; k < nk; ++k) {
            const int c0 = (k * G + gl) * VEC;
            const bool ok = row_ok && c0 < C;
            float* dk = d[HOLD ? k : 0];
            if constexpr (!HOLD) piece<T, VEC>(a, i, c0, ok, dk, m);
            if (!ok) continue;
            float ga[VEC], be[VEC], o[VEC];
            row_load<T, VEC>((const T*)a.gamma + c0, ga);
#pragma unroll
            for (int v = 0; v < VEC; ++v) be[v] = 0.f;
            if (a.beta) row_load<T, VEC>((const T*)a.beta + c0, be);
#pragma unroll
            for (int v = 0; v < VEC; ++v) o[v] = (dk[v] - mu) * rstd * ga[v] + be[v];
            row_store<T, VEC>(out + i * C + c0, o);
        }
        if (a.stats && row_ok && gl == 0) {
            a.stats[2 * i] = mu;
            a.stats[2 * i + 1] = rstd;
        }
    }
}

// Backward. Group `gid` of the launch owns row gid of the partials and the rows gid, gid + groups, ... of the input.
template <typename T, int VEC, int NCH>
__global__ __launch_bounds__(256) void head_act_norm_bwd_kernel(const NormArgs a) {
    constexpr bool HOLD = NCH > 0;
    constexpr int NH = HOLD ? NCH : 1, UNR = NH;      // the held pieces unroll; the wide instance loops
    const int wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wave >= a.nwaves) return;
    const int lane = threadIdx.x & 63, G = 1 << a.gshift, gl = lane & (G - 1), sub = lane >> a.gshift, R = 64 >> a.gshift;
    const int nk = HOLD ? NCH : a.nk, C = a.C;
    const int64_t HC = (int64_t)a.H * C;
    const float Cf = (float)C, Hf = (float)a.H;
    const T* __restrict__ g = (const T*)a.g;
    T* __restrict__ da = (T*)a.da;
    float* __restrict__ prow = a.partial + ((int64_t)wave * R + sub) * 3 * C;
    float sb[NH][VEC], sg[NH][VEC], se[NH][VEC];      // d bias, d gamma, d beta of this group's rows (HOLD)
#pragma unroll
    for (int k = 0; k < NH; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) sb[k][v] = sg[k][v] = se[k][v] = 0.f;
    if constexpr (!HOLD) {
        for (int c = gl; c < C; c += G) prow[c] = prow[C + c] = prow[2 * C + c] = 0.f;      // the SAME lane adds to these words below
    }
    for (int64_t base = (int64_t)wave * R; base < a.N; base += (int64_t)a.nwaves * R) {
        const int64_t i = base + sub;
        const bool row_ok = i < a.N;
        float mu = 0.f, rstd = 1.f;
        if (a.norm && row_ok) {
            mu = a.stats[2 * i];
            rstd = a.stats[2 * i + 1];
        }
        float xh[NH][VEC], gv[NH][VEC], mv[NH][VEC];
        float s1 = 0.f, s2 = 0.f;
        if (a.norm) {
#pragma unroll UNR
            for (int k = 0; k < nk; ++k) {
                const int c0 = (k * G + gl) * VEC;
                const bool ok = row_ok && c0 < C;
                const int kk = HOLD ? k : 0;
                float d[VEC], ga[VEC];
                piece<T, VEC>(a, i, c0, ok, d, mv[kk]);
#pragma unroll
                for (int v = 0; v < VEC; ++v) { gv[kk][v] = 0.f; ga[v] = 0.f; }
                if (ok) {
                    row_load<T, VEC>(g + i * a.ldg + c0, gv[kk]);
                    row_load<T, VEC>((const T*)a.gamma + c0, ga);
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    xh[kk][v] = ok ? (d[v] - mu) * rstd : 0.f;
                    const float gx = gv[kk][v] * ga[v];
                    s1 = s1 + gx;
                    s2 = s2 + gx * xh[kk][v];
                }
            }
            s1 = group_sum(s1, a.gshift, lane) / Cf;
            s2 = group_sum(s2, a.gshift, lane) / Cf;
        }
#pragma unroll UNR
        for (int k = 0; k < nk; ++k) {
            const int c0 = (k * G + gl) * VEC;
            const bool ok = row_ok && c0 < C;
            const int kk = HOLD ? k : 0;
            float ga[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) ga[v] = 0.f;
            if (!HOLD || !a.norm) {
                float d[VEC];
                piece<T, VEC>(a, i, c0, ok, d, mv[kk]);
#pragma unroll
                for (int v = 0; v < VEC; ++v) { gv[kk][v] = 0.f; xh[kk][v] = ok && a.norm ? (d[v] - mu) * rstd : 0.f; }
                if (ok) row_load<T, VEC>(g + i * a.ldg + c0, gv[kk]);
            }
            if (!ok) continue;
            if (a.norm) row_load<T, VEC>((const T*)a.gamma + c0, ga);
            float dy[VEC], dh[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float dd = a.norm ? rstd * (gv[kk][v] * ga[v] - s1 - xh[kk][v] * s2) : gv[kk][v];
                dy[v] = dd * mv[kk][v];
                dh[v] = dy[v] / Hf;
            }
            for (int h = 0; h < a.H; ++h) row_store<T, VEC>(da + i * HC + (int64_t)h * C + c0, dh);
            if constexpr (HOLD) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    sb[k][v] = sb[k][v] + dy[v];
                    sg[k][v] = sg[k][v] + gv[k][v] * xh[k][v];
                    se[k][v] = se[k][v] + gv[k][v];
                }
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    prow[c0 + v] = prow[c0 + v] + dy[v];
                    prow[C + c0 + v] = prow[C + c0 + v] + gv[0][v] * xh[0][v];
                    prow[2 * C + c0 + v] = prow[2 * C + c0 + v] + gv[0][v];
                }
            }
        }
    }
    if constexpr (HOLD) {
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c0 = (k * G + gl) * VEC;
            if (c0 >= C) continue;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                prow[c0 + v] = sb[k][v];
                prow[C + c0 + v] = sg[k][v];
                prow[2 * C + c0 + v] = se[k][v];
            }
        }
    }
}

// The [rows, 3 * C] partials added per column: 8 threads take every 8th row top to bottom, their 8 sums are added in order.
// The same bits every run. A null output is skipped.
template <typename T>
__global__ __launch_bounds__(256) void head_act_norm_colsum_kernel(const float* __restrict__ partial, int rows, int C, T* __restrict__ dbias,
                                                                   T* __restrict__ dgamma, T* __restrict__ dbeta) {
    __shared__ float s[8][32];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + cx, W = 3 * C;
    float acc = 0.f;
    if (col < W)
        for (int r = ry; r < rows; r += 8) acc = acc + partial[(int64_t)r * W + col];
    s[ry][cx] = acc;
    __syncthreads();
    if (ry != 0 || col >= W) return;
    float t = s[0][cx];
#pragma unroll
    for (int j = 1; j < 8; ++j) t = t + s[j][cx];
    const int which = col / C, c = col % C;
    T* dst = which == 0 ? dbias : which == 1 ? dgamma : dbeta;
    if (dst) Elem<T>::store(dst + c, t);
}

struct Geometry { int vec, nch, gshift, nk; };

// widest piece the operands allow; G = the pieces of a row rounded up to a power of two, NCH pieces per lane past 64
inline Geometry geometry(int C, int max_vec) {
    int vec = max_vec;
    while (vec > 1 && C % vec != 0) vec >>= 1;
    const int pieces = C / vec;
    Geometry g{};
    g.vec = vec;
    g.gshift = gnnops_group_shift(pieces);
    g.nch = pieces <= 64 ? 1 : pieces <= 128 ? 2 : pieces <= 256 ? 4 : 0;
    if (g.nch == 0) { g.vec = 1; g.gshift = 6; }      // 64 lanes x single elements, the row re-read per pass: any C <= 8192
    g.nk = (int)gnnops_cdiv(C, (int64_t)g.vec << g.gshift);
    return g;
}

// waves of the backward: 4 Mi fp32 words of partials at the most, at least 64 waves where the rows allow
inline int backward_waves(int64_t N, int C, int gshift) {
    const int R = 64 >> gshift;
    int64_t waves = ((int64_t)1 << 22) / ((int64_t)3 * C * R);
    waves = waves < 64 ? 64 : waves > 2048 ? 2048 : waves;
    const int64_t need = gnnops_cdiv(N, R);
    return (int)(waves < need ? waves : need < 1 ? 1 : need);
}

template <typename T, bool BW, int VEC, int NCH>
void launch_kernel(const NormArgs& a, int grid, hipStream_t stream) {
    if constexpr (BW) hipLaunchKernelGGL((head_act_norm_bwd_kernel<T, VEC, NCH>), dim3(grid), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((head_act_norm_fwd_kernel<T, VEC, NCH>), dim3(grid), dim3(256), 0, stream, a);
}

template <typename T, bool BW, int VEC>
void launch_pieces(const NormArgs& a, int nch, int grid, hipStream_t stream) {
    if (nch == 1) launch_kernel<T, BW, VEC, 1>(a, grid, stream);
    else if (nch == 2) launch_kernel<T, BW, VEC, 2>(a, grid, stream);
    else launch_kernel<T, BW, VEC, 4>(a, grid, stream);
}

template <typename T, bool BW>
void launch(const NormArgs& a, const Geometry& geo, int grid, hipStream_t stream) {
    if (geo.nch == 0) return launch_kernel<T, BW, 1, 0>(a, grid, stream);
    gnnops_with_piece_width<T>(geo.vec, [&](auto v) { launch_pieces<T, BW, decltype(v)::value>(a, geo.nch, grid, stream); });
}

int check_sizes(const char* what, int64_t N, int64_t H, int64_t C, int64_t lda, int dtype, int* es) {
    GNNOPS_REQUIRE(N >= 0, GNNOPS_EINVAL, "%s: negative size", what);
    GNNOPS_REQUIRE(H >= 1 && C >= 1 && H * C <= 8192, GNNOPS_EINVAL,
                   "%s: needs heads >= 1, channels >= 1 and heads * channels <= 8192 (got %lld x %lld)", what, (long long)H, (long long)C);
    GNNOPS_REQUIRE(N < ((int64_t)1 << 31) && lda < ((int64_t)1 << 31), GNNOPS_EUNSUPPORTED, "%s: N and the row pitch must be < 2^31", what);
    GNNOPS_REQUIRE(lda >= H * C, GNNOPS_EINVAL, "%s: a row pitch is shorter than the row", what);
    *es = gnnops_elem_bytes(dtype);
    GNNOPS_REQUIRE(*es, GNNOPS_EINVAL, "%s: unknown dtype %d", what, dtype);
    return GNNOPS_OK;
}

}  // namespace

extern "C" int gnnops_head_act_norm(const void* a, int64_t lda, const void* bias, const void* scale, const void* gamma, const void* beta,
                                    void* out, float* stats, int64_t N, int64_t H, int64_t C, int relu, float eps, int dtype,
                                    gnnops_stream_t s) {
    int es = 0;
    const int rc = check_sizes("head_act_norm", N, H, C, lda, dtype, &es);
    if (rc != GNNOPS_OK) return rc;
    GNNOPS_REQUIRE(gamma || !beta, GNNOPS_EINVAL, "head_act_norm: beta without gamma");
    if (N == 0) return GNNOPS_OK;
    GNNOPS_REQUIRE(a && out, GNNOPS_EINVAL, "head_act_norm: null pointer");
    const int max_vec = gnnops_widest_piece(es, {{a, lda}, {bias, 0}, {scale, C}, {gamma, 0}, {beta, 0}, {out, C}});
    const Geometry geo = geometry((int)C, max_vec);
    NormArgs args{};
    args.a = a; args.bias = bias; args.k = scale; args.gamma = gamma; args.beta = beta; args.out = out; args.stats = gamma ? stats : nullptr;
    args.N = N; args.lda = lda; args.H = (int)H; args.C = (int)C; args.gshift = geo.gshift; args.nk = geo.nk;
    args.relu = relu != 0; args.norm = gamma != nullptr; args.eps = eps;
    const int grid = gnnops_grid_cap(gnnops_cdiv(gnnops_cdiv(N, 64 >> geo.gshift), 4), 256 * 32);
    args.nwaves = grid * 4;
    hipStream_t stream = (hipStream_t)s;
    return gnnops_with_dtype(dtype, "head_act_norm", [&](auto t) {
        launch<typename decltype(t)::type, false>(args, geo, grid, stream);
        return gnnops_check_launch("head_act_norm");
    });
}

extern "C" size_t gnnops_head_act_norm_backward_workspace_bytes(int64_t N, int64_t H, int64_t C) {
    if (N <= 0 || H < 1 || C < 1 || H * C > 8192) return 0;
    size_t need = 0;      // the piece width follows the operands' alignment: the largest need of the widths that can occur
    for (int vec = 1; vec <= 8; vec <<= 1) {
        const Geometry geo = geometry((int)C, vec);
        const size_t rows = (size_t)backward_waves(N, (int)C, geo.gshift) * (size_t)(64 >> geo.gshift);
        const size_t bytes = rows * 3 * (size_t)C * sizeof(float);
        need = bytes > need ? bytes : need;
    }
    return need;
}

extern "C" int gnnops_head_act_norm_backward(const void* a, int64_t lda, const void* bias, const void* scale, const void* gamma,
                                             const float* stats, const void* grad_out, int64_t ldg, void* grad_a, void* grad_bias,
                                             void* grad_gamma, void* grad_beta, int64_t N, int64_t H, int64_t C, int relu, int dtype,
                                             void* workspace, size_t workspace_bytes, gnnops_stream_t s) {
    int es = 0;
    const int rc = check_sizes("head_act_norm_backward", N, H, C, lda, dtype, &es);
    if (rc != GNNOPS_OK) return rc;
    GNNOPS_REQUIRE(ldg >= C || ldg == 0, GNNOPS_EINVAL, "head_act_norm_backward: a row pitch is shorter than the row");
    GNNOPS_REQUIRE(gamma || (!grad_gamma && !grad_beta), GNNOPS_EINVAL, "head_act_norm_backward: a norm gradient without gamma");
    if (N == 0) return GNNOPS_OK;   // no row: nothing is written
    GNNOPS_REQUIRE(a && grad_out && grad_a && (!gamma || stats), GNNOPS_EINVAL, "head_act_norm_backward: null pointer");
    const size_t need = gnnops_head_act_norm_backward_workspace_bytes(N, H, C);
    GNNOPS_REQUIRE(workspace && workspace_bytes >= need && (uintptr_t)workspace % 16 == 0, GNNOPS_EWORKSPACE,
                   "head_act_norm_backward: workspace %zu < %zu", workspace_bytes, need);
    const int max_vec = gnnops_widest_piece(es, {{a, lda}, {bias, 0}, {scale, C}, {gamma, 0}, {grad_out, ldg}, {grad_a, H * C}});
    const Geometry geo = geometry((int)C, max_vec);
    NormArgs args{};
    args.a = a; args.bias = bias; args.k = scale; args.gamma = gamma; args.g = grad_out; args.da = grad_a;
    args.stats = const_cast<float*>(stats); args.partial = (float*)workspace;
    args.N = N; args.lda = lda; args.ldg = ldg; args.H = (int)H; args.C = (int)C; args.gshift = geo.gshift; args.nk = geo.nk;
    args.relu = relu != 0; args.norm = gamma != nullptr;
    args.nwaves = backward_waves(N, (int)C, geo.gshift);
    const int grid = (int)gnnops_cdiv(args.nwaves, 4);
    hipStream_t stream = (hipStream_t)s;
    return gnnops_with_dtype(dtype, "head_act_norm_backward", [&](auto t) {
        using T = typename decltype(t)::type;
        launch<T, true>(args, geo, grid, stream);
        if (grad_bias || grad_gamma || grad_beta) {
            const int rows = args.nwaves * (64 >> geo.gshift);
            const dim3 cgrid((unsigned)gnnops_cdiv(3 * C, 32));
            hipLaunchKernelGGL(head_act_norm_colsum_kernel<T>, cgrid, dim3(256), 0, stream, args.partial, rows, (int)C, (T*)grad_bias,
                               (T*)grad_gamma, (T*)grad_beta);
        }
        return gnnops_check_launch("head_act_norm_backward");
    });
}
