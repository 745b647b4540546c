// spline_common.h: what the forward (spline.hip) and backward (spline_bw.hip) B-spline kernels share: the per-launch
// description of the basis, B_m and its derivative, and the (basis value, kernel index) of one combination of one edge.
#pragma once
#include "common.h"

namespace {

constexpr int MAX_DIM = 8;
constexpr int MAX_S = 64;

struct SplineMeta {
    int D, degree, S;
    int64_t kernel_size[MAX_DIM];
    int is_open[MAX_DIM];
};

template <int M>
__device__ inline float bspline(float v, int k) {
    if constexpr (M == 1) {
        return k == 0 ? 1.f - v : v;
    } else if constexpr (M == 2) {
        if (k == 0) return 0.5f * v * v - v + 0.5f;
        if (k == 1) return -v * v + v + 0.5f;
        return 0.5f * v * v;
    } else {
        if (k == 0) return (1.f - v) * (1.f - v) * (1.f - v) / 6.f;
        if (k == 1) return (3.f * v * v * v - 6.f * v * v + 4.f) / 6.f;
        if (k == 2) return (-3.f * v * v * v + 3.f * v * v + 3.f * v + 1.f) / 6.f;
        return v * v * v / 6.f;
    }
}

// basis value and weight index of combination s for one edge's pseudo-coordinates (fp32 arithmetic for every storage type)
template <typename T, int M>
__device__ inline void basis_of(const T* __restrict__ pseudo_e, const SplineMeta& sm, int s, float& b, int64_t& wi) {
    int k = s;
    int64_t off = 1;
    wi = 0;
    b = 1.f;
    for (int d = 0; d < sm.D; ++d) {
        const int k_mod = k % (M + 1);
        k /= (M + 1);
        float v = Elem<T>::load(pseudo_e + d) * (float)(sm.kernel_size[d] - M * sm.is_open[d]);
        const float fl = floorf(v);
        wi += (((int64_t)fl + k_mod) % sm.kernel_size[d]) * off;
        off *= sm.kernel_size[d];
        v -= fl;
        b *= bspline<M>(v, k_mod);
    }
}

// d B_m(v, k) / d v (the derivative the backward of spline_basis needs; at a knot it is the right-hand one, because
// floor() carries no gradient)
template <int M>
__device__ inline float bspline_grad(float v, int k) {
    if constexpr (M == 1) {
        return k == 0 ? -1.f : 1.f;
    } else if constexpr (M == 2) {
        if (k == 0) return v - 1.f;
        if (k == 1) return -2.f * v + 1.f;
        return v;
    } else {
        if (k == 0) return -0.5f * (1.f - v) * (1.f - v);
        if (k == 1) return 1.5f * v * v - 2.f * v;
        if (k == 2) return -1.5f * v * v + v + 0.5f;
        return 0.5f * v * v;
    }
}

inline int fill_meta(SplineMeta& sm, const int64_t* kernel_size, const uint8_t* is_open_spline, int D, int degree, const char* what) {
    GNNOPS_REQUIRE(D >= 1 && D <= MAX_DIM, GNNOPS_EUNSUPPORTED, "%s: 1..%d pseudo-coordinate dimensions", what, MAX_DIM);
    GNNOPS_REQUIRE(degree >= 1 && degree <= 3, GNNOPS_EUNSUPPORTED, "%s: B-spline degree must be 1, 2 or 3", what);
    GNNOPS_REQUIRE(kernel_size && is_open_spline, GNNOPS_EINVAL, "%s: null kernel_size / is_open_spline", what);
    sm.D = D;
    sm.degree = degree;
    int64_t S = 1;
    for (int d = 0; d < D; ++d) {
        S *= degree + 1;
        GNNOPS_REQUIRE(kernel_size[d] >= 1, GNNOPS_EINVAL, "%s: kernel_size must be positive", what);
        sm.kernel_size[d] = kernel_size[d];
        sm.is_open[d] = is_open_spline[d] ? 1 : 0;
    }
    GNNOPS_REQUIRE(S <= MAX_S, GNNOPS_EUNSUPPORTED, "%s: (degree + 1)^D = %lld basis products per edge, at most %d", what, (long long)S,
                   MAX_S);
    sm.S = (int)S;
    return GNNOPS_OK;
}

}  // namespace
