// Host-side launch plumbing, once: runtime dtype -> element type, widest aligned piece, piece width -> template argument, and the
// lane-group size of a row. Host code only: nothing here is called from a kernel.
#pragma once
#include <initializer_list>
#include <type_traits>
#include <utility>
#include "common.h"

template <typename T> struct gnnops_type_tag { using type = T; };

// fn(tag) with typename decltype(tag)::type = the element type of `dtype`; what fn returns. Any other code is refused here.
template <typename Fn>
inline int gnnops_with_dtype(int dtype, const char* what, Fn&& fn) {
    switch (dtype) {
        case GNNOPS_F32: return fn(gnnops_type_tag<float>{});
        case GNNOPS_F16: return fn(gnnops_type_tag<__half>{});
        case GNNOPS_BF16: return fn(gnnops_type_tag<__hip_bfloat16>{});
    }
    gnnops_set_error("%s: unknown dtype %d", what, dtype);
    return GNNOPS_EINVAL;
}

// bytes per element; 0 for an unknown code
inline int gnnops_elem_bytes(int dtype) { return dtype == GNNOPS_F32 ? 4 : dtype == GNNOPS_F16 || dtype == GNNOPS_BF16 ? 2 : 0; }

// lanes that share a row of `pieces` pieces: the smallest g in 0..6 with 2^g >= pieces
inline int gnnops_group_shift(int64_t pieces) {
    int g = 0;
    while (g < 6 && ((int64_t)1 << g) < pieces) ++g;
    return g;
}

using Operands = std::initializer_list<std::pair<const void*, int64_t>>;   // (pointer, row pitch in elements) of what a kernel reads or writes in pieces

// widest piece (elements, from 16 bytes down) that every non-null pointer and every pitch is a multiple of
inline int gnnops_widest_piece(int es, Operands operands) {
    int vec = 16 / es;
    for (const auto& op : operands) {
        if (!op.first) continue;
        while (vec > 1 && ((uintptr_t)op.first % (vec * es) != 0 || (op.second * es) % (vec * es) != 0)) vec >>= 1;
    }
    return vec;
}

// fn(std::integral_constant<int, V>{}) for V = vec in {8, 4, 2, 1}; 8 only where T has 8 elements in 16 bytes, anything else goes to 1
template <typename T, typename Fn>
inline auto gnnops_with_piece_width(int vec, Fn&& fn) {
    if constexpr (Elem<T>::VEC == 8) {
        if (vec == 8) return fn(std::integral_constant<int, 8>{});
    }
    if (vec == 4) return fn(std::integral_constant<int, 4>{});
    if (vec == 2) return fn(std::integral_constant<int, 2>{});
    return fn(std::integral_constant<int, 1>{});
}
