// DSQ block decoding on the device: the one decoder shared by the load-time dequantiser (dsq.hip) and the
// packed decode kernels (decode_q.hip).  Every value follows Candle's k-quants to_float in the source's
// operation order: one f32 multiply per factor (and for Q4_K one subtract), never contracted into an
// FMA, then rounded to fp16 (RNE) — bit-identical to oracle/dsq.py.  The packed kernels use that fp16
// value widened to f32, so they differ from dequant-on-load only in the order of their sums.
#pragma once
#include <hip/hip_fp16.h>

#include <cstdint>

#include "dev_common.hpp"

// no contraction of a multiply and the following add / subtract into an FMA anywhere below (the pragma holds to
// the end of the including file: the kernels that want an FMA call fmaf)
#pragma clang fp contract(off)

namespace dsocr {

__device__ __forceinline__ float f16_at(const uint8_t* p) {
    const uint16_t bits = (uint16_t)p[0] | ((uint16_t)p[1] << 8);
    return f16_bits_to_f32(bits);
}

// the f32 value is pinned in a register first: otherwise the backend folds the last multiply and
// the conversion into v_fma_mix(a, b, +0) — one rounding straight to f16 (not f32 then f16) and
// -0 * x + 0 = +0 — which is not the reference's arithmetic
__device__ __forceinline__ uint16_t to_f16_rne(float v) {
    asm volatile("" : "+v"(v));
    return __half_as_ushort(__float2half_rn(v));
}

// get_scale_min_k4 (GGML k-quants): 6-bit scale / min codes of sub-block j from the 12 packed bytes
__device__ __forceinline__ void scale_min_k4(int j, const uint8_t* q, int& d, int& m) {
    if (j < 4) {
        d = q[j] & 63;
        m = q[j + 4] & 63;
    } else {
        d = (q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4);
        m = (q[j + 4] >> 4) | ((q[j] >> 6) << 4);
    }
}
// the same from the 12 bytes held as three little-endian words (a block header loaded as one dwordx4:
// word 0 = d | dmin, words 1..3 = scales)
__device__ __forceinline__ void scale_min_k4_words(int j, uint32_t s0, uint32_t s1, uint32_t s2, int& d, int& m) {
    auto byte = [&](int i) { return (int)(((i < 4 ? s0 : (i < 8 ? s1 : s2)) >> (8 * (i & 3))) & 0xFF); };
    if (j < 4) {
        d = byte(j) & 63;
        m = byte(j + 4) & 63;
    } else {
        d = (byte(j + 4) & 0xF) | ((byte(j - 4) >> 6) << 4);
        m = (byte(j + 4) >> 4) | ((byte(j) >> 6) << 4);
    }
}

// Q4_K sub-block factors: d1 = d * scale code, m1 = dmin * min code (each one f32 multiply)
__device__ __forceinline__ void q4k_sub(float d, float dmin, int sc, int m, float& d1, float& m1) {
    d1 = __fmul_rn(d, (float)sc);
    m1 = __fmul_rn(dmin, (float)m);
}
// Q4_K value of nibble `nib` in a sub-block: fp16 bits of d1 * nib - m1
__device__ __forceinline__ uint16_t q4k_f16(float d1, float m1, int nib) {
    return to_f16_rne(__fsub_rn(__fmul_rn(d1, (float)nib), m1));
}
// Q8_0 value: fp16 bits of d * q
__device__ __forceinline__ uint16_t q8_0_f16(float d, int q) { return to_f16_rne(__fmul_rn(d, (float)q)); }

// ---- the decode kernels' unpack: 8 weights per lane as f32 (the fp16 values widened)
// Q4_K: one lane of a 32-lane group holds the dword at qs[32c + 4j .. +3] of chunk c = l32 >> 3, j = l32 & 7:
// o[0..3] = values 64c + 4j + {0..3} (low nibbles, sub-block 2c), o[4..7] = values 64c + 32 + 4j + {0..3}
// (high nibbles, sub-block 2c + 1).  hdr: the block's first 16 bytes.
__device__ __forceinline__ void q4k_unpack8(const uint4 hdr, uint32_t qs, int l32, float* o) {
    const float d = f16_bits_to_f32(hdr.x & 0xffffu), dmin = f16_bits_to_f32(hdr.x >> 16);
    const int c = l32 >> 3;
    int s0, m0, s1, m1;
    scale_min_k4_words(2 * c, hdr.y, hdr.z, hdr.w, s0, m0);
    scale_min_k4_words(2 * c + 1, hdr.y, hdr.z, hdr.w, s1, m1);
    float d0, n0, d1, n1;
    q4k_sub(d, dmin, s0, m0, d0, n0);
    q4k_sub(d, dmin, s1, m1, d1, n1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = (qs >> (8 * k)) & 0xFF;
        o[k] = f16_bits_to_f32(q4k_f16(d0, n0, b & 0xF));
        o[4 + k] = f16_bits_to_f32(q4k_f16(d1, n1, b >> 4));
    }
}
// element offset (within the 256-value super-block) of o[0] and o[4] above
__device__ __forceinline__ int q4k_lane_off(int l32) { return 64 * (l32 >> 3) + 4 * (l32 & 7); }

// Q8_0: 8 consecutive int8 codes (two dwords) of one block with scale d
__device__ __forceinline__ void q8_0_unpack8(float d, uint32_t q0, uint32_t q1, float* o) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[k] = f16_bits_to_f32(q8_0_f16(d, (int)(int8_t)((q0 >> (8 * k)) & 0xFF)));
        o[4 + k] = f16_bits_to_f32(q8_0_f16(d, (int)(int8_t)((q1 >> (8 * k)) & 0xFF)));
    }
}

}  // namespace dsocr
