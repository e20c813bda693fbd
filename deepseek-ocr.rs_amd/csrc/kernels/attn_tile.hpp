// One 32-query x 32-key tile of exact-f32 flash attention on v_mfma_f32_32x32x2_f32, shared by attention_fwd2
// (attention.hip), attention_prefix (attention_prefix.hip) and attention_past / attention_chunk (attention_past.hip).
//
// A wave owns 32 queries: lanes l32 and l32 + 32 share query l32 and split the head dims (lane half h feeds dims
// [h HD/2, (h + 1) HD/2)).  S^T = K.Q^T puts the lane's own query in the accumulator column, so the online softmax
// needs no cross-lane traffic beyond one exchange between the two halves, and P feeds O^T += V^T.P^T straight from
// the score accumulator, the keys in its permuted order (attn_tile_key; cdna_hip_programming.md §3 "An accumulator
// tile as the next MFMA's operand").
//
// What lives here: the register-to-key map, the query load, the two MFMA products, the online-softmax step and the
// unnormalised (m, l, O[hd]) record of a key piece with its combine.  What stays in each kernel: the grid decode, the
// staging of K / V and its double buffering, the scale / bias / mask loop over the sixteen scores, every barrier and
// fence, and the epilogue.
//
// Every piece is a force-inlined function that takes the register arrays by reference: a register array captured by
// a lambda (or handed to a function that is not inlined) is demoted to scratch.
#pragma once
#include "dev_common.hpp"

namespace dsocr {

constexpr int ATTN_TILE = 32;  // queries per wave and keys per tile: the MFMA's 32 x 32 accumulator

// accumulator register r of lane (half, l32) holds row attn_tile_key(r, half) of the tile, column l32
__device__ __forceinline__ int attn_tile_key(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// the lane's half of its query row (16-byte loads)
template <int HD>
__device__ __forceinline__ void attn_tile_load_q(const float* qrow, int half, float (&qreg)[HD / 2]) {
    const float* qr = qrow + half * (HD / 2);
#pragma unroll
    for (int i = 0; i < HD / 2; i += 4) {
        const float4 v4 = *reinterpret_cast<const float4*>(qr + i);
        qreg[i] = v4.x; qreg[i + 1] = v4.y; qreg[i + 2] = v4.z; qreg[i + 3] = v4.w;
    }
}

// S^T = K . Q^T of one tile: krow is the lane's key row (l32) of a K tile in LDS at row pitch HD + 4 floats (the
// 16-byte fragment reads of 32 rows fall on distinct banks)
template <int HD>
__device__ __forceinline__ void attn_tile_scores(const float* krow, int half, const float (&qreg)[HD / 2], f32x16& sc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < HD / 2; i += 4) {
        const float4 k4 = *reinterpret_cast<const float4*>(krow + half * (HD / 2) + i);
        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qreg[i], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qreg[i + 1], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qreg[i + 2], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qreg[i + 3], sc, 0, 0, 0);
    }
}

// max of the lane's query over the tile's 32 keys (sc: scaled, biased, masked scores; -inf = masked)
__device__ __forceinline__ float attn_tile_max(const f32x16& sc) {
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, sc[r]);
    return fmaxf(m, __shfl_xor(m, 32, 64));
}

// sc -> p = e^(sc - m) in place (all zeros when m == -inf: no visible key), returns the sum over the 32 keys
__device__ __forceinline__ float attn_tile_exp(f32x16& sc, float m) {
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float p = (m == -INFINITY) ? 0.f : __expf(sc[r] - m);
        sc[r] = p;
        sum += p;
    }
    return sum + __shfl_xor(sum, 32, 64);
}

// One online-softmax step: folds the tile's scores into the running (m, l), rescales O^T and leaves p in sc.
// alpha where m_new == -inf (the query has seen no key yet) multiplies an l and an O that are still zero; 1 there.
// A kernel with a single tile per wave calls attn_tile_max / attn_tile_exp itself: its (m, l) are the tile's.
template <int HD>
__device__ __forceinline__ void attn_tile_softmax(f32x16& sc, float& m_run, float& l_run, f32x16 (&o)[HD / 32]) {
    const float m_new = fmaxf(m_run, attn_tile_max(sc));
    const float alpha = (m_new == -INFINITY) ? 1.f : __expf(m_run - m_new);
    const float psum = attn_tile_exp(sc, m_new);
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int t = 0; t < HD / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
}

// O^T += V^T . P^T from a transposed V tile in LDS: vt[d][key] at row pitch ATTN_TILE + 4 floats, 16-byte reads of
// the 4 adjacent keys that registers 4 g4 .. 4 g4 + 3 of p hold
template <int HD>
__device__ __forceinline__ void attn_tile_pv_lds(const float* vt, int half, int l32, const f32x16& p, f32x16 (&o)[HD / 32]) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        const int kb = 8 * g4 + 4 * half;
#pragma unroll
        for (int t = 0; t < HD / 32; ++t) {
            const float4 v4 = *reinterpret_cast<const float4*>(vt + (t * 32 + l32) * (ATTN_TILE + 4) + kb);
            o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(v4.x, p[4 * g4 + 0], o[t], 0, 0, 0);
            o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(v4.y, p[4 * g4 + 1], o[t], 0, 0, 0);
            o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(v4.z, p[4 * g4 + 2], o[t], 0, 0, 0);
            o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(v4.w, p[4 * g4 + 3], o[t], 0, 0, 0);
        }
    }
}

// O^T += V^T . P^T with the V rows read from memory as they are (32 lanes, 32 consecutive floats of one row): keys
// k0 + attn_tile_key(r, half) clamped to last_row; a masked key carries p = 0 and reads a clamped (written) row
template <int HD>
__device__ __forceinline__ void attn_tile_pv_rows(const float* V, long row_stride, int k0, int last_row, int half,
                                                  int l32, const f32x16& p, f32x16 (&o)[HD / 32]) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int key = min(k0 + 8 * g4 + 4 * half + j, last_row);
            const float* vr = V + (long)key * row_stride + l32;
#pragma unroll
            for (int t = 0; t < HD / 32; ++t)
                o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[t * 32], p[4 * g4 + j], o[t], 0, 0, 0);
        }
    }
}

// The unnormalised partial of one key piece for the lane's query: rec[0] = m, rec[1] = l, rec[HDR + d] = O[d].
// HDR is 2 in memory and 4 in LDS (16-byte aligned O slices).
template <int HD>
__device__ __forceinline__ void attn_rec_write(float* rec, int hdr, int half, float m, float l, const f32x16 (&o)[HD / 32]) {
    if (half == 0) { rec[0] = m; rec[1] = l; }
#pragma unroll
    for (int t = 0; t < HD / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) rec[hdr + t * 32 + attn_tile_key(r, half)] = o[t][r];
}

// Flash-decoding combine of one query's n records (rec0 + i * stride) for output dim d, in record order:
// m = max m_i, l = sum l_i e^(m_i - m), o = sum o_i e^(m_i - m); returns o / l.  A piece that saw no key of the
// query left m_i = -inf and weighs nothing.
__device__ __forceinline__ float attn_rec_combine(const float* rec0, long stride, int n, int hdr, int d) {
    float m = -INFINITY;
    for (int i = 0; i < n; ++i) m = fmaxf(m, rec0[i * stride]);
    float l = 0.f, acc = 0.f;
    for (int i = 0; i < n; ++i) {
        const float* r = rec0 + i * stride;
        const float w = r[0] == -INFINITY ? 0.f : __expf(r[0] - m);
        l += r[1] * w;
        acc += r[hdr + d] * w;
    }
    return acc / l;
}

}  // namespace dsocr
