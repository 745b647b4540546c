// gemm_tile.h — the register-staged, fully bounds-checked 128 x 128 output tile of the dense products, as device functions:
// gemm_tile16 (fp16 / bf16 operands, v_mfma_f32_16x16x32) and gemm_tile_f32 (fp32, v_mfma_f32_16x16x4). One workgroup of 256
// threads computes C[m0 : m0+128, n0 : n0+128] = addend + A @ B, rows at or past `m_end` and columns at or past N neither
// read nor written. Callers: gemm.hip (one tile per (blockIdx.y, blockIdx.x), m_end = M) and segment_matmul.hip (a tile
// of one segment: m_end = the segment's end, B = that segment's weight). The order of every sum depends on K alone, so a
// row gets the same bits from either caller.
//
// Layout (row-major operands, as torch hands them over):
//   A tile [128][64] in LDS, 128-B rows, 16-B chunks XOR-swizzled by (row & 7); a lane's A fragment (row l&15,
//     k = 8*(l>>4)..+7) is one conflict-free ds_read_b128.
//   B tile [64][128] stays ROW-major in LDS (coalesced 16-B global loads, no transposing writes) in the
//     guide's swizzled 256-B-row image; the k-strided B fragment comes from two ds_read_b64_tr_b16
//     hardware-transpose reads (4 k-rows x 16 columns per 16-lane group each).
//   4 waves as 2 x 2, each 64 x 64 = 4 x 4 MFMA tiles (64 accumulator VGPRs). The epilogue parks each wave's fp32
//     tile in LDS and writes 16-B row pieces.
#pragma once
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int A_TILE_BYTES = BM * BK * 2;              // 16 KiB, 128-B rows, 8 chunks of 16 B
constexpr int B_TILE_BYTES = BK * BN * 2;              // 16 KiB, 256-B rows, 16 chunks of 16 B
constexpr int STAGE_BYTES = A_TILE_BYTES + B_TILE_BYTES;
constexpr int CS = 68;                                  // epilogue row stride in floats (64 + 4)

template <bool IS_BF16>
__device__ inline f32x4 mfma16(const s16x8& a, const s16x8& b, const f32x4& c) {
    if constexpr (IS_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// XOR swizzles (byte offsets inside a tile). A: chunk ^ (row & 7) makes the ds_read_b128 of 16 rows x one
// k-chunk conflict-free; B: the guide's 256-B-row image (cdna_hip_programming.md T10 (b)), conflict-free for
// ds_read_b64_tr_b16.
__device__ inline int a_off(int row, int ch) { return row * 128 + ((ch ^ (row & 7)) << 4); }
__device__ inline int b_off(int row, int ch) { return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4); }

// Eight consecutive outputs of one row, columns col..col+7: += addend, one rounding, stored as wide as the row
// alignment allows (16 B when N % 8 == 0, 8 B when N % 4 == 0, else per element); rows >= M and columns >= N are dropped.
template <typename T>
__device__ inline void epi_store8(T* __restrict__ C, const T* __restrict__ addend, int64_t row, int64_t col, int64_t M,
                                  int64_t N, float (&f)[8], bool vec_c, bool half_c, int64_t ldadd) {
    if (row >= M || col >= N) return;
    if (vec_c && col + 8 <= N) {
        if (addend) {
            float g[8];
            Elem<T>::unpack(*reinterpret_cast<const u32x4*>(addend + row * ldadd + col), g);
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] += g[i];
        }
        *reinterpret_cast<u32x4*>(C + row * N + col) = Elem<T>::pack(f);
    } else if (half_c) {  // rows 8-B aligned (N % 4 == 0): two 4-element pieces, each whole or absent
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (col + 4 * h < N) {
                float* fh = f + 4 * h;
                if (addend) {
                    const uint2 g2 = *reinterpret_cast<const uint2*>(addend + row * ldadd + col + 4 * h);
                    float g[8];
                    Elem<T>::unpack(u32x4{g2.x, g2.y, 0u, 0u}, g);
#pragma unroll
                    for (int i = 0; i < 4; ++i) fh[i] += g[i];
                }
                float tmp[8] = {fh[0], fh[1], fh[2], fh[3], 0.f, 0.f, 0.f, 0.f};
                const u32x4 pk = Elem<T>::pack(tmp);
                *reinterpret_cast<uint2*>(C + row * N + col + 4 * h) = uint2{pk.x, pk.y};
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (col + i < N) {
                float v = f[i];
                if (addend) v += Elem<T>::load(addend + row * ldadd + col + i);
                Elem<T>::store(C + row * N + col + i, v);
            }
        }
    }
}

// 8 consecutive 16-bit elements of row `r`, columns c..c+7 of a [rows][cols] row-major matrix whose rows start
// ALIGN-byte aligned (cols * 2 % ALIGN == 0): ALIGN = 16 -> one dwordx4, 8 -> two dwordx2, 4 -> four dwords, 2 -> elements.
// A piece never straddles the row end; pieces beyond it, and rows beyond `rows`, read as 0.
template <int ALIGN>
__device__ inline u32x4 load8(const uint16_t* __restrict__ base, int64_t r, int64_t c, int64_t rows, int64_t cols) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (r >= rows || c >= cols) return v;
    const uint16_t* p = base + r * cols + c;
    if constexpr (ALIGN == 16) {
        v = *reinterpret_cast<const u32x4*>(p);
    } else if constexpr (ALIGN == 8) {
        const uint2 lo = *reinterpret_cast<const uint2*>(p);
        v.x = lo.x; v.y = lo.y;
        if (c + 4 < cols) { const uint2 hi = *reinterpret_cast<const uint2*>(p + 4); v.z = hi.x; v.w = hi.y; }
    } else if constexpr (ALIGN == 4) {
        v.x = *reinterpret_cast<const uint32_t*>(p);
        if (c + 2 < cols) v.y = *reinterpret_cast<const uint32_t*>(p + 2);
        if (c + 4 < cols) v.z = *reinterpret_cast<const uint32_t*>(p + 4);
        if (c + 6 < cols) v.w = *reinterpret_cast<const uint32_t*>(p + 6);
    } else {   // odd row lengths (K = 11 node features): element loads
        uint16_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = (c + j < cols) ? p[j] : (uint16_t)0;
        v.x = e[0] | ((uint32_t)e[1] << 16); v.y = e[2] | ((uint32_t)e[3] << 16);
        v.z = e[4] | ((uint32_t)e[5] << 16); v.w = e[6] | ((uint32_t)e[7] << 16);
    }
    return v;
}

// LDS of one workgroup of gemm_tile16: two stages; the epilogue (four waves' fp32 tiles, 68 KiB) reuses them
constexpr int TILE16_EPI_BYTES = 4 * 64 * CS * 4;
constexpr int TILE16_SMEM_BYTES = (2 * STAGE_BYTES > TILE16_EPI_BYTES) ? 2 * STAGE_BYTES : TILE16_EPI_BYTES;

// C[m0.., n0..] = addend + A @ B for one 128 x 128 tile. A [.., K] and B [K, N] row-major with ALIGN-byte aligned rows;
// lda / ldb = row lengths as stored (== K / N unless the host padded them); they bound the column reads. `m_end` bounds
// the rows: A rows at or past it read as 0 and C rows at or past it are not written. `smem`: TILE16_SMEM_BYTES, 16-B
// aligned. Every thread of the 256 must call it (it holds __syncthreads()).
template <typename T, bool IS_BF16, int ALIGN>
__device__ __forceinline__ void gemm_tile16(unsigned char* smem, const uint16_t* __restrict__ A,
                                            const uint16_t* __restrict__ Bm, const T* __restrict__ addend,
                                            T* __restrict__ C, int64_t m0, int64_t n0, int64_t m_end, int64_t N, int64_t K,
                                            int64_t lda, int64_t ldb, int64_t ldadd) {
    const int64_t M = m_end;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging: 4 chunks of A and 4 of B per thread and K-step; chunk id = tid + 256*p
    int a_st[4], b_st[4];          // swizzled LDS byte offsets (within a stage)
    int64_t a_gr[4], b_gr[4];      // global row of each chunk
    int a_gc[4], b_gc[4];          // global column (elements) inside the tile
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int id = tid + 256 * p;
        const int ar = id >> 3, ac = id & 7;     // A: 128 rows x 8 chunks
        a_st[p] = a_off(ar, ac);
        a_gr[p] = m0 + ar;
        a_gc[p] = ac * 8;
        const int br = id >> 4, bc = id & 15;    // B: 64 rows x 16 chunks
        b_st[p] = A_TILE_BYTES + b_off(br, bc);
        b_gr[p] = br;
        b_gc[p] = bc * 8;
    }
    u32x4 ra[4], rb[4];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            ra[p] = load8<ALIGN>(A, a_gr[p], k0 + a_gc[p], M, lda);
            rb[p] = load8<ALIGN>(Bm, k0 + b_gr[p], n0 + b_gc[p], K, ldb);
        }
    };
    auto sstore = [&](int stage) {
        unsigned char* base = smem + stage * STAGE_BYTES;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<u32x4*>(base + a_st[p]) = ra[p];
            *reinterpret_cast<u32x4*>(base + b_st[p]) = rb[p];
        }
    };

    // fragment addresses. A: row = wr*64 + mi*16 + (lane&15), chunk = ks*4 + (lane>>4).
    // B (transposed read): 16-lane group g = lane>>4 owns k rows ks*32 + 8g (+4 for the second read); lane 4q+p
    // supplies row +q, chunk c0 + (p>>1), +8 bytes for odd p; c0 = 2 * (16-column block) = wc*8 + ni*2.
    const int a_row = wr * 64 + (lane & 15);
    const int a_kc = lane >> 4;
    const int b_q = (lane & 15) >> 2, b_p = lane & 3;
    const int b_row = 8 * (lane >> 4) + b_q;

    const int64_t ksteps = (K + BK - 1) / BK;
    gload(0);
    sstore(0);
    __syncthreads();
    for (int64_t kt = 0; kt < ksteps; ++kt) {
        const int cur = (int)(kt & 1);
        const bool more = kt + 1 < ksteps;
        if (more) gload((kt + 1) * BK);
        const unsigned char* sA = smem + cur * STAGE_BYTES;
        const unsigned char* sB = sA + A_TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            s16x8 af[4], bf[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                af[mi] = *reinterpret_cast<const s16x8*>(sA + a_off(a_row + mi * 16, ks * 4 + a_kc));
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int ch = wc * 8 + ni * 2 + (b_p >> 1);
                const int r_lo = ks * 32 + b_row;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (s16x4 __attribute__((address_space(3)))*)(sB + b_off(r_lo, ch) + 8 * (b_p & 1)));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (s16x4 __attribute__((address_space(3)))*)(sB + b_off(r_lo + 4, ch) + 8 * (b_p & 1)));
                bf[ni] = s16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma16<IS_BF16>(af[mi], bf[ni], acc[mi][ni]);
        }
        if (more) sstore(cur ^ 1);
        __syncthreads();
    }

    // Epilogue through LDS: each wave parks its 64 x 64 fp32 tile (C/D map: col = lane & 15, row = (lane >> 4)*4 + reg),
    // then reads whole row pieces back: 8 lanes x 8 columns per row, so the addend load and the store are 16-B
    // accesses on 128-B row segments. One rounding, after the add.
    float* ctile = reinterpret_cast<float*>(smem) + wave * (64 * CS);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ctile[(mi * 16 + (lane >> 4) * 4 + r) * CS + ni * 16 + (lane & 15)] = acc[mi][ni][r];
    __builtin_amdgcn_wave_barrier();  // the tile is private to this wave; LDS ops of one wave complete in order
    const bool vec_c = (N % 8 == 0) && ((uintptr_t)C % 16 == 0) && (addend == nullptr || (uintptr_t)addend % 16 == 0);
    const bool half_c = (N % 4 == 0) && ((uintptr_t)C % 8 == 0) && (addend == nullptr || (uintptr_t)addend % 8 == 0);
    const int pr = lane >> 3, pc = (lane & 7) * 8;
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        const int rr = pass * 8 + pr;
        const int64_t row = m0 + wr * 64 + rr;
        const int64_t col = n0 + wc * 64 + pc;
        float f[8];
        const f32x4 lo = *reinterpret_cast<const f32x4*>(&ctile[rr * CS + pc]);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(&ctile[rr * CS + pc + 4]);
        f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3]; f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
        epi_store8<T>(C, addend, row, col, M, N, f, vec_c, half_c, ldadd);
    }
}

// ---- fp32 operands: v_mfma_f32_16x16x4_f32 (exact fp32 products and sums, 1/16 of the bf16 MFMA rate = the fp32
// vector peak, MI355X_MICROARCH.md "Matrix cores"). Same 128 x 128 block / 2 x 2 waves / 4 x 4 MFMA tiles; BK = 16.
// A tile [128][16] with 20-float rows and B tile [16][128] with 144-float rows: both fragment reads (one ds_read_b32
// per lane: A[row l&15][k l>>4], B[k l>>4][col l&15]) are bank-conflict-free, and B needs no transpose at all.
constexpr int FBK = 16, FAS = 20, FBS = 144;

__device__ inline f32x4 load4f(const float* __restrict__ base, int64_t r, int64_t c, int64_t rows, int64_t cols, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r >= rows || c >= cols) return v;
    const float* p = base + r * cols + c;
    if (vec && c + 4 <= cols) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (c + i < cols) v[i] = p[i];
    return v;
}

// LDS of one workgroup of gemm_tile_f32, in floats: two stages (2560 + 2304 floats each); the epilogue's staging area fits
constexpr int TILE_F32_STAGE_F = BM * FAS + FBK * FBS;
constexpr int TILE_F32_EPI_F = 4 * 32 * CS;
constexpr int TILE_F32_SMEM_F = (2 * TILE_F32_STAGE_F > TILE_F32_EPI_F) ? 2 * TILE_F32_STAGE_F : TILE_F32_EPI_F;

// The fp32 twin of gemm_tile16: contiguous A [.., K] and B [K, N]; a_vec / b_vec = 16-B row pieces allowed. `smem`:
// TILE_F32_SMEM_F floats, 16-B aligned.
__device__ __forceinline__ void gemm_tile_f32(float* smem, const float* __restrict__ A, const float* __restrict__ Bm,
                                              const float* __restrict__ addend, float* __restrict__ C, int64_t m0,
                                              int64_t n0, int64_t m_end, int64_t N, int64_t K, bool a_vec, bool b_vec,
                                              int64_t ldadd) {
    constexpr int STAGE_F = TILE_F32_STAGE_F;
    const int64_t M = m_end;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging: A 128 x 16 floats = 512 float4 chunks (2 per thread), B 16 x 128 = 512 chunks (2 per thread)
    f32x4 ra[2], rb[2];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int id = tid + 256 * p;
            ra[p] = load4f(A, m0 + (id >> 2), k0 + (id & 3) * 4, M, K, a_vec);
            rb[p] = load4f(Bm, k0 + (id >> 5), n0 + (id & 31) * 4, K, N, b_vec);
        }
    };
    auto sstore = [&](int stage) {
        float* sA = smem + stage * STAGE_F;
        float* sB = sA + BM * FAS;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int id = tid + 256 * p;
            *reinterpret_cast<f32x4*>(&sA[(id >> 2) * FAS + (id & 3) * 4]) = ra[p];
            *reinterpret_cast<f32x4*>(&sB[(id >> 5) * FBS + (id & 31) * 4]) = rb[p];
        }
    };

    const int64_t ksteps = (K + FBK - 1) / FBK;
    gload(0);
    sstore(0);
    __syncthreads();
    for (int64_t kt = 0; kt < ksteps; ++kt) {
        const int cur = (int)(kt & 1);
        const bool more = kt + 1 < ksteps;
        if (more) gload((kt + 1) * FBK);
        const float* sA = smem + cur * STAGE_F;
        const float* sB = sA + BM * FAS;
#pragma unroll
        for (int ks = 0; ks < FBK / 4; ++ks) {
            float af[4], bf[4];
            const int kk = ks * 4 + (lane >> 4);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) af[mi] = sA[(wr * 64 + mi * 16 + (lane & 15)) * FAS + kk];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) bf[ni] = sB[kk * FBS + wc * 64 + ni * 16 + (lane & 15)];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
        }
        if (more) sstore(cur ^ 1);
        __syncthreads();
    }

    // epilogue: each wave stages its 64 x 64 tile through LDS in two rounds of 32 rows, so the staging area (34 KiB) stays
    // below the main loop's two stages (38 KiB) and three workgroups share a CU (one round of 64 rows: 68 KiB, two).
    // The K loop ended on a barrier: every wave is done with the stages.
    float* ctile = smem + wave * (32 * CS);
    const bool vec_c = (N % 4 == 0) && ((uintptr_t)C % 16 == 0) && (addend == nullptr || (uintptr_t)addend % 16 == 0);
    const int pr = lane >> 4, pc = (lane & 15) * 4;  // 16 lanes x 4 columns per row, 4 rows per pass
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    ctile[(h * 16 + (lane >> 4) * 4 + r) * CS + ni * 16 + (lane & 15)] = acc[c * 2 + h][ni][r];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int pass = 0; pass < 8; ++pass) {
            const int rr = pass * 4 + pr;
            const int64_t row = m0 + wr * 64 + c * 32 + rr;
            const int64_t col = n0 + wc * 64 + pc;
            f32x4 v = *reinterpret_cast<const f32x4*>(&ctile[rr * CS + pc]);
            if (row >= M || col >= N) continue;
            if (vec_c && col + 4 <= N) {
                if (addend) {
                    const f32x4 g = *reinterpret_cast<const f32x4*>(addend + row * ldadd + col);
                    v[0] += g[0]; v[1] += g[1]; v[2] += g[2]; v[3] += g[3];
                }
                *reinterpret_cast<f32x4*>(C + row * N + col) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (col + i < N) C[row * N + col + i] = v[i] + (addend ? addend[row * ldadd + col + i] : 0.f);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace
