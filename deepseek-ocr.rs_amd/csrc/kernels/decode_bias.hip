// Per-request logit bias and token allow / deny sets: a per-row term on the exact head's f32 logits.
//   logit_bias_fill / _scatter  at admission, outside the step graph: the request's sparse (id, value) list, a few
//                               KB over PCIe, becomes the slot's dense f32 row
//   dec_logit_bias              grid (chunks of V, B), in the step, after the lm_head and before dec_lp_partial /
//                               the repetition penalty: l' = l + b for the rows whose flag is set
// A latency-bound stream (two rows read, one written, per constrained page): no LDS, no matrix cores; 16-byte
// accesses where both rows are aligned, a scalar path for unaligned rows and the tail (as dec_lp_partial).
#include "decode_common.hpp"

namespace dsocr {

constexpr int LB_BLOCK = 256;
constexpr int LB_PER_BLOCK = 2048;  // 8 logits per thread as two 16-byte loads of each row, all in flight before the first add
constexpr int LB_PER = LB_PER_BLOCK / LB_BLOCK;

__global__ __launch_bounds__(LB_BLOCK) void logit_bias_fill_kernel(LogitBiasBuildArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.on = a.on_value;
    if (!a.on_value) return;
    const float f = a.allow_only ? -INFINITY : 0.f;
    // ld % 4 == 0 and the row is 16-byte aligned (checked by the launcher): whole float4s, the pad [V, ld) as 0
    const long v = 4 * ((long)blockIdx.x * LB_BLOCK + threadIdx.x);
    if (v >= a.ld) return;
    float4 q;
    q.x = v < a.V ? f : 0.f; q.y = v + 1 < a.V ? f : 0.f; q.z = v + 2 < a.V ? f : 0.f; q.w = v + 3 < a.V ? f : 0.f;
    *reinterpret_cast<float4*>(a.row + v) = q;
}

// ids are unique (checked on the host), so no two threads store to one column
__global__ __launch_bounds__(LB_BLOCK) void logit_bias_scatter_kernel(LogitBiasBuildArgs a) {
    const int i = blockIdx.x * LB_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int t = a.ids[i];
    if (t >= 0 && t < a.V) a.row[t] = a.values[i];
}

__global__ __launch_bounds__(LB_BLOCK) void dec_logit_bias_kernel(DecBiasArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    // block-uniform (one scalar load): an unconstrained row of a mixed batch is neither read nor written
    if (!a.on[b]) return;
    float* lg = a.logits + (long)b * a.ld;
    const float* bs = a.bias + (long)b * a.bias_ld;
    const int v0 = blockIdx.x * LB_PER_BLOCK, v1 = min(a.V, v0 + LB_PER_BLOCK);
    const bool vec = ((reinterpret_cast<uintptr_t>(lg) | reinterpret_cast<uintptr_t>(bs)) & 15) == 0;
    float x[LB_PER], y[LB_PER];
#pragma unroll
    for (int j = 0; j < LB_PER / 4; ++j) {
        const int v = v0 + 4 * (tid + j * LB_BLOCK);
        if (vec && v + 3 < v1) {
            const float4 q = *reinterpret_cast<const float4*>(lg + v);
            const float4 r = *reinterpret_cast<const float4*>(bs + v);
            x[4 * j] = q.x; x[4 * j + 1] = q.y; x[4 * j + 2] = q.z; x[4 * j + 3] = q.w;
            y[4 * j] = r.x; y[4 * j + 1] = r.y; y[4 * j + 2] = r.z; y[4 * j + 3] = r.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {  // (the scalar path: an unaligned row, or the tail of V)
                x[4 * j + c] = v + c < v1 ? lg[v + c] : 0.f;
                y[4 * j + c] = v + c < v1 ? bs[v + c] : 0.f;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < LB_PER / 4; ++j) {
        const int v = v0 + 4 * (tid + j * LB_BLOCK);
        if (vec && v + 3 < v1) {
            float4 q;
            q.x = x[4 * j] + y[4 * j]; q.y = x[4 * j + 1] + y[4 * j + 1];
            q.z = x[4 * j + 2] + y[4 * j + 2]; q.w = x[4 * j + 3] + y[4 * j + 3];
            *reinterpret_cast<float4*>(lg + v) = q;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (v + c < v1) lg[v + c] = x[4 * j + c] + y[4 * j + c];  // never a column in [V, ld)
        }
    }
}

void launch_logit_bias_build(const LogitBiasBuildArgs& a, hipStream_t s) {
    if (!a.row || !a.on || a.V <= 0 || a.ld < a.V || a.ld % 4 || (reinterpret_cast<uintptr_t>(a.row) & 15))
        throw std::runtime_error("EINVAL: logit bias row (16-byte aligned, ld % 4 == 0, ld >= V)");
    if (a.n < 0 || a.n > a.V || (a.n && (!a.ids || !a.values))) throw std::runtime_error("EINVAL: logit bias list");
    const unsigned fill = a.on_value ? (unsigned)((a.ld / 4 + LB_BLOCK - 1) / LB_BLOCK) : 1u;
    DSOCR_LAUNCH(logit_bias_fill_kernel, dim3(fill), dim3(LB_BLOCK), 0, s, a);
    if (a.on_value && a.n)
        DSOCR_LAUNCH(logit_bias_scatter_kernel, dim3((unsigned)((a.n + LB_BLOCK - 1) / LB_BLOCK)), dim3(LB_BLOCK), 0, s, a);
}

void launch_dec_logit_bias(const DecBiasArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.V <= 0 || a.ld < a.V || a.bias_ld < a.V || !a.logits || !a.bias || !a.on)
        throw std::runtime_error("EINVAL: logit bias add needs B, V > 0, rows of at least V floats and the row flags");
    DSOCR_LAUNCH(dec_logit_bias_kernel, dim3((unsigned)((a.V + LB_PER_BLOCK - 1) / LB_PER_BLOCK), a.B), dim3(LB_BLOCK), 0, s, a);
}

}  // namespace dsocr
