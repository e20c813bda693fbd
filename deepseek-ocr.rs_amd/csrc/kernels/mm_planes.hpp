// Token rows as three 16-bit planes in LDS, the B operand of v_mfma_f32_16x16x32_{f16,bf16}: shared by the decode
// matrix-core units (decode_mm.hip, decode_f8mm.hip).  Numerics: decode_mm.hip header, DESIGN.md section 2.
#pragma once
#include "decode_common.hpp"

namespace dsocr {

typedef _Float16 mm_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 mm_b16x8 __attribute__((ext_vector_type(8)));

constexpr int MM_MT = 8;  // token rows staged (M <= 8)

template <typename WT>
struct MmT;
template <>
struct MmT<f16_t> {
    typedef mm_f16x8 frag;
    static constexpr bool scaled = true;
    __device__ static uint16_t to_bits(float v, float& back) {
        const _Float16 h = (_Float16)v;
        back = (float)h;
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
    }
    __device__ static f32x4 mfma(const frag& a, const frag& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <>
struct MmT<bf16_t> {
    typedef mm_b16x8 frag;
    static constexpr bool scaled = false;
    __device__ static uint16_t to_bits(float v, float& back) {
        const __bf16 h = (__bf16)v;
        back = (float)h;
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
    }
    __device__ static f32x4 mfma(const frag& a, const frag& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

// LDS row pitch of a plane row (16-bit elements): K + 16 puts consecutive rows 8 banks apart, which
// makes the B-operand ds_read_b128 (rows l&7, k groups l>>4) conflict-free.
__host__ __device__ inline int mm_pitch(int K) { return K + 16; }

// Wave-level staging of token row m of x (f32, K <= 1536) as 3 planes in LDS (xp[(p * MT + m) * KP +
// k]) with its inverse scale scl[m], in two halves so that the row's loads can be issued BEFORE the
// weight stream (vmcnt retires in issue order: loads issued after a weight batch wait for it).
// NORM: RMS-normalised first — the lane's chunks (lane, lane+64, lane+128; 8 floats each) squared and
// summed u-major then j, one wave sum, x * (1 / den) * w.
template <int U>
struct MmRowU {
    float v[U][8];
    float w[U][8];
};
typedef MmRowU<3> MmRow;  // K <= 1536

template <bool NORM, int U = 3>
__device__ __forceinline__ void mm_row_load(MmRowU<U>& r, const float* xr, int K, const float* nw) {
    const int lane = threadIdx.x & 63;
    const int chunks = K >> 3;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int cc = min(u * 64 + lane, chunks - 1);
        const float4 lo = *reinterpret_cast<const float4*>(xr + (cc << 3));
        const float4 hi = *reinterpret_cast<const float4*>(xr + (cc << 3) + 4);
        r.v[u][0] = lo.x; r.v[u][1] = lo.y; r.v[u][2] = lo.z; r.v[u][3] = lo.w;
        r.v[u][4] = hi.x; r.v[u][5] = hi.y; r.v[u][6] = hi.z; r.v[u][7] = hi.w;
        if (NORM) {
            const float4 wl = *reinterpret_cast<const float4*>(nw + (cc << 3));
            const float4 wh = *reinterpret_cast<const float4*>(nw + (cc << 3) + 4);
            r.w[u][0] = wl.x; r.w[u][1] = wl.y; r.w[u][2] = wl.z; r.w[u][3] = wl.w;
            r.w[u][4] = wh.x; r.w[u][5] = wh.y; r.w[u][6] = wh.z; r.w[u][7] = wh.w;
        }
    }
}

template <typename WT, bool NORM, int U = 3, bool DIVNORM = false>
__device__ __forceinline__ void mm_row_store(MmRowU<U>& r, int K, float eps, uint16_t* xp, int KP, float* scl, int m) {
    const int lane = threadIdx.x & 63;
    const int chunks = K >> 3;
    if (NORM) {
        float q = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u * 64 + lane < chunks)
#pragma unroll
                for (int j = 0; j < 8; ++j) q += r.v[u][j] * r.v[u][j];
        // one division per row: x * (1 / den) is within an ulp of the reference's x / den (the planes
        // below are exact, the GEMM sums in its own order: this path is tolerance-pinned, not bitwise)
        if (DIVNORM) {  // x / den * w: dec_route_grp's (and the reference's) form, bit for bit
            const float den = sqrtf(wave_sum(q) / (float)K + eps);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 8; ++j) r.v[u][j] = (r.v[u][j] / den) * r.w[u][j];
        } else {
            const float inv = 1.0f / sqrtf(wave_sum(q) / (float)K + eps);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 8; ++j) r.v[u][j] = (r.v[u][j] * inv) * r.w[u][j];
        }
    }
    float s_inv = 1.f;
    if (MmT<WT>::scaled) {
        float mx = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u * 64 + lane < chunks)
#pragma unroll
                for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(r.v[u][j]));
        mx = wave_max(mx);
        int s = 0;
        if (mx > 0.f) {
            int e;
            (void)frexpf(mx, &e);  // mx < 2^e
            s = 15 - e;            // mx * 2^s < 2^15
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) r.v[u][j] = ldexpf(r.v[u][j], s);
        s_inv = ldexpf(1.f, -s);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = u * 64 + lane;
        if (c < chunks) {
            uint16_t pb[3][8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float b0, b1, b2;
                pb[0][j] = MmT<WT>::to_bits(r.v[u][j], b0);
                const float r1 = r.v[u][j] - b0;
                pb[1][j] = MmT<WT>::to_bits(r1, b1);
                const float r2 = r1 - b1;
                pb[2][j] = MmT<WT>::to_bits(r2, b2);
            }
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                uint4 q;
                q.x = pb[p][0] | ((uint32_t)pb[p][1] << 16);
                q.y = pb[p][2] | ((uint32_t)pb[p][3] << 16);
                q.z = pb[p][4] | ((uint32_t)pb[p][5] << 16);
                q.w = pb[p][6] | ((uint32_t)pb[p][7] << 16);
                *reinterpret_cast<uint4*>(xp + ((long)(p * MM_MT + m) * KP + (c << 3))) = q;
            }
        }
    }
    if (lane == 0) scl[m] = s_inv;
}

}  // namespace dsocr
