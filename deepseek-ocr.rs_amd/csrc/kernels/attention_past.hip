// Prefill attention behind a cached past, f32 end to end like attention.hip: every sequence brings n_q new rows
// (already rotated, their K / V rows already appended) and attends them causally to the past + n_q rows its cache
// now holds.  Query row i sits at position past + i and sees keys [0, past + i].
//
// The new rows are few (a prompt suffix behind a cached page is a handful of rows against ~700 keys), so the
// parallelism comes from the keys, not from the queries:
//   * attention_past_kernel: one workgroup per (128-key piece, head, sequence x 32-query tile), four waves, wave w
//     owning keys [32 w, 32 w + 32) of the piece.  A wave stages its K tile in its own slice of LDS (row pitch
//     hd + 4 floats: the 16-byte fragment reads of 32 rows fall on distinct banks), computes S^T = K.Q^T on
//     v_mfma_f32_32x32x2_f32 with the lane's own query in the accumulator column, takes the softmax of its 32 keys
//     and feeds P straight from that accumulator into O^T = V^T.P^T (keys in the accumulator's permuted order; V
//     rows are read from the cache as they are: 32 lanes, 32 consecutive floats of one row).  It writes its
//     unnormalised (m, l, O[hd]) per query to the workspace.  Products are exact f32, as in attention_fwd2.
//   * attention_past_merge_kernel, a second launch: thread (query, d) combines the query's records in key order
//     (m = max m_i, l = sum l_i e^(m_i - m), o = sum o_i e^(m_i - m), out = o / l).
// Nothing is handed over inside a launch: a wave reads only the caches and writes only its own records; the kernel
// boundary orders the records before the combine.
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dev_common.hpp"
#include "kernels.hpp"

namespace dsocr {

constexpr int PA_Q = 32;      // queries per tile (one accumulator column per lane pair)
constexpr int PA_KT = 32;     // keys per wave
constexpr int PA_WAVES = 4;   // waves per workgroup: a piece of 128 keys

template <int HD>
__global__ __launch_bounds__(64 * PA_WAVES) void attention_past_kernel(AttnPastArgs a) {
    constexpr int KP = HD + 4;
    extern __shared__ __attribute__((aligned(16))) float pa_lds[];
    const int nqt = (a.max_q + PA_Q - 1) / PA_Q, nkt = (a.max_total + PA_KT - 1) / PA_KT;
    const int s = blockIdx.z / nqt, qt = blockIdx.z % nqt, h = blockIdx.y;
    const int past = a.past[s], nq = a.n_q[s];
    const int q0 = qt * PA_Q;
    if (q0 >= nq) return;
    const int kend = past + min(nq, q0 + PA_Q);  // keys [0, kend): what the tile's last query sees
    if ((int)blockIdx.x * PA_WAVES * PA_KT >= kend) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int kvh = h / (a.heads / a.kv_heads);
    const int ktile = blockIdx.x * PA_WAVES + wave, k0 = ktile * PA_KT;
    const float* Q = a.q.ptr + a.q.seq_off[s] + (long)h * a.q.head_stride;
    const float* K = a.k.ptr + a.k.seq_off[s] + (long)kvh * a.k.head_stride;
    const float* V = a.v.ptr + a.v.seq_off[s] + (long)kvh * a.v.head_stride;
    // this wave's K tile: rows clamped to the last visible key (a clamped row's scores are masked below)
    float* Ks = pa_lds + wave * PA_KT * KP;
#pragma unroll
    for (int j = 0; j < HD / 8; ++j) {
        const int f = lane + 64 * j;
        const int row = f / (HD / 4), c4 = (f % (HD / 4)) * 4;
        const int key = min(k0 + row, kend - 1);
        *reinterpret_cast<float4*>(&Ks[row * KP + c4]) = *reinterpret_cast<const float4*>(K + (long)key * a.k.row_stride + c4);
    }
    __syncthreads();
    if (k0 >= kend) return;  // (wave-uniform; no barrier follows)
    const int q_lane = q0 + l32;  // lanes l and l + 32 share a query and split the head dims
    const bool q_valid = q_lane < nq;
    float qreg[HD / 2];
    {
        const float* qr = Q + (long)(q_valid ? q_lane : 0) * a.q.row_stride + half * (HD / 2);
#pragma unroll
        for (int i = 0; i < HD / 2; i += 4) {
            const float4 v4 = *reinterpret_cast<const float4*>(qr + i);
            qreg[i] = v4.x; qreg[i + 1] = v4.y; qreg[i + 2] = v4.z; qreg[i + 3] = v4.w;
        }
    }
    f32x16 sc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < HD / 2; i += 4) {
        const float4 k4 = *reinterpret_cast<const float4*>(&Ks[l32 * KP + half * (HD / 2) + i]);
        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qreg[i], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qreg[i + 1], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qreg[i + 2], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qreg[i + 3], sc, 0, 0, 0);
    }
    // accumulator register r of lane (half, l32): key k0 + kappa(r, half), query l32
    const int last_key = past + q_lane;
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float v = key > last_key ? -INFINITY : sc[r] * a.scale;
        sc[r] = v;
        m = fmaxf(m, v);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float p = (m == -INFINITY) ? 0.f : __expf(sc[r] - m);
        sc[r] = p;
        l += p;
    }
    l += __shfl_xor(l, 32, 64);
    // O^T = V^T . P^T over the tile's keys in the accumulator's order; masked keys carry p = 0 and read a clamped
    // (written) row
    f32x16 o[HD / 32];
#pragma unroll
    for (int t = 0; t < HD / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int key = min(k0 + 8 * g4 + 4 * half + j, kend - 1);
            const float* vr = V + (long)key * a.v.row_stride + l32;
#pragma unroll
            for (int t = 0; t < HD / 32; ++t)
                o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[t * 32], sc[4 * g4 + j], o[t], 0, 0, 0);
        }
    }
    if (!q_valid) return;
    float* rec = a.part + (((((long)s * a.heads + h) * nqt + qt) * nkt + ktile) * PA_Q + l32) * (HD + 2);
    if (half == 0) { rec[0] = m; rec[1] = l; }
#pragma unroll
    for (int t = 0; t < HD / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) rec[2 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half] = o[t][r];
}

// thread (query, d): the query's key tiles [0, ceil((past + q + 1) / 32)) were all written by the launch before
template <int HD>
__global__ __launch_bounds__(256) void attention_past_merge_kernel(AttnPastArgs a) {
    const int s = blockIdx.z, h = blockIdx.y;
    const int past = a.past[s], nq = a.n_q[s];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(idx / HD), d = (int)(idx % HD);
    if (q >= nq) return;
    const int nqt = (a.max_q + PA_Q - 1) / PA_Q, nkt = (a.max_total + PA_KT - 1) / PA_KT;
    const int qt = q / PA_Q, ql = q % PA_Q;
    const int n = (past + q + PA_KT) / PA_KT;
    const float* rec0 = a.part + (((((long)s * a.heads + h) * nqt + qt) * nkt) * PA_Q + ql) * (HD + 2);
    const long pstride = (long)PA_Q * (HD + 2);
    float m = -INFINITY;
    for (int i = 0; i < n; ++i) m = fmaxf(m, rec0[i * pstride]);
    float l = 0.f, acc = 0.f;
    for (int i = 0; i < n; ++i) {
        const float* r = rec0 + i * pstride;
        const float w = r[0] == -INFINITY ? 0.f : __expf(r[0] - m);
        l += r[1] * w;
        acc += r[2 + d] * w;
    }
    a.o[a.o_seq_off[s] + (long)q * a.o_row_stride + (long)h * a.o_head_stride + d] = acc / l;
}

size_t attention_past_part_floats(int n_seq, int heads, int max_q, int max_total, int hd) {
    const size_t nqt = (size_t)(max_q + PA_Q - 1) / PA_Q, nkt = (size_t)(max_total + PA_KT - 1) / PA_KT;
    return (size_t)n_seq * heads * nqt * nkt * PA_Q * (hd + 2);
}

bool attention_past_ok(const AttnPastArgs& a) {
    if (a.hd != 32 && a.hd != 64 && a.hd != 128) return false;
    if (a.n_seq <= 0 || a.heads <= 0 || a.kv_heads <= 0 || a.heads % a.kv_heads) return false;
    if (a.max_q < 1 || a.max_total < a.max_q) return false;
    if (!a.q.ptr || !a.k.ptr || !a.v.ptr || !a.o || !a.past || !a.n_q) return false;
    if (!a.q.seq_off || !a.k.seq_off || !a.v.seq_off || !a.o_seq_off) return false;
    // 16-byte loads of q and k rows
    if (a.q.row_stride % 4 || a.q.head_stride % 4 || a.k.row_stride % 4 || a.k.head_stride % 4) return false;
    if (a.q.row_stride < a.hd || a.k.row_stride < a.hd || a.v.row_stride < a.hd) return false;
    if ((reinterpret_cast<uintptr_t>(a.q.ptr) | reinterpret_cast<uintptr_t>(a.k.ptr)) & 15) return false;
    const long nqt = (a.max_q + PA_Q - 1) / PA_Q;
    if (a.heads > 65535 || (long)a.n_seq * nqt > 65535) return false;
    if (!a.part || a.part_floats < attention_past_part_floats(a.n_seq, a.heads, a.max_q, a.max_total, a.hd)) return false;
    return true;
}

template <int HD>
static void launch_past_hd(const AttnPastArgs& a, hipStream_t s) {
    const size_t lds = (size_t)PA_WAVES * PA_KT * (HD + 4) * sizeof(float);
    if (lds > 64 * 1024) {  // hd 128: 66 KB of dynamic LDS (set at every launch: cheap, and right on every device)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_past_kernel<HD>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("EDEVICE: attention_past: dynamic LDS limit: ") + hipGetErrorString(e));
    }
    const int nqt = (a.max_q + PA_Q - 1) / PA_Q;
    const dim3 g1((a.max_total + PA_WAVES * PA_KT - 1) / (PA_WAVES * PA_KT), a.heads, a.n_seq * nqt);
    const dim3 g2((unsigned)(((long)a.max_q * HD + 255) / 256), a.heads, a.n_seq);
    DSOCR_LAUNCH(attention_past_kernel<HD>, g1, dim3(64 * PA_WAVES), lds, s, a);
    DSOCR_LAUNCH(attention_past_merge_kernel<HD>, g2, dim3(256), 0, s, a);
}

void launch_attention_past(const AttnPastArgs& a, hipStream_t s) {
    if (!attention_past_ok(a)) throw std::runtime_error("EINVAL: attention_past: shape outside the kernel's contract");
    if (a.hd == 128) launch_past_hd<128>(a, s);
    else if (a.hd == 64) launch_past_hd<64>(a, s);
    else launch_past_hd<32>(a, s);
}

}  // namespace dsocr
