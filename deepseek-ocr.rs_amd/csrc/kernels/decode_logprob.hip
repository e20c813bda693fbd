// Per-token log-probabilities of the decode step: the raw logits of the exact head reduced, on the device and
// inside the captured step, to one log-sum-exp, the chosen token's log-probability and the K most likely
// alternatives per emitted token.
//   dec_lp_partial  grid (chunks of V, B), after the lm_head and before the repetition penalty
//   dec_lp_final    grid (1, B), after the selection kernels
// Every reduction runs in a fixed order (DPP butterflies inside a wave, then waves / chunks by index), so an
// entry depends on the row's logits alone: not on B, the slot or timing.
#include "decode_common.hpp"

namespace dsocr {

constexpr int LP_BLOCK = 256;
constexpr int LP_PER_BLOCK = 2048;  // 8 logits per thread as two 16-byte loads, all in flight before the first compare
constexpr int LP_PER = LP_PER_BLOCK / LP_BLOCK;
constexpr int LP_CPL = 4;           // chunks per lane of the final merge: V <= 64 * LP_CPL * LP_PER_BLOCK
constexpr int LP_NONE = 0x7fffffff;
size_t dec_lp_chunks(int V) { return (size_t)(V + LP_PER_BLOCK - 1) / LP_PER_BLOCK; }

__device__ __forceinline__ bool lp_finite(float x) { return (x > -INFINITY) && (x < INFINITY); }
__device__ __forceinline__ bool lp_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// The wave's K best of the N (value, id) pairs every lane holds, descending, lower id first on equal values (the
// order of argmax_first), to outv / outi[0..K) (LDS or global; lane 0 writes).  A taken pair becomes (-inf, NONE);
// when fewer than K ids exist the rest are (-inf, -1).  No barrier: K wave reductions.
template <int N>
__device__ __forceinline__ void wave_topk(float (&v)[N], int (&id)[N], int K, float* outv, int* outi) {
    const int lane = threadIdx.x & 63;
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = LP_NONE;
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (id[j] != LP_NONE && lp_better(v[j], id[j], bv, bi)) { bv = v[j]; bi = id[j]; }
        wave_argmax(bv, bi);
        if (bi != LP_NONE) {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (id[j] == bi) { id[j] = LP_NONE; v[j] = -INFINITY; }
        }
        if (lane == 0) { outv[k] = bv; outi[k] = bi == LP_NONE ? -1 : bi; }
    }
}

__global__ __launch_bounds__(LP_BLOCK) void dec_lp_partial_kernel(DecLpArgs a) {
    __shared__ float red[LP_BLOCK / 64];
    __shared__ float wv[(LP_BLOCK / 64) * LP_MAX_TOP];
    __shared__ int wi[(LP_BLOCK / 64) * LP_MAX_TOP];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchunk = gridDim.x;
    const float* lg = a.logits + (long)b * a.ld;
    const int v0 = blockIdx.x * LP_PER_BLOCK, v1 = min(a.V, v0 + LP_PER_BLOCK);
    float x[LP_PER];
    int id[LP_PER];
    const bool vec = (reinterpret_cast<uintptr_t>(lg) & 15) == 0;
#pragma unroll
    for (int j = 0; j < LP_PER / 4; ++j) {
        const int v = v0 + 4 * (tid + j * LP_BLOCK);
        if (vec && v + 3 < v1) {
            const float4 q = *reinterpret_cast<const float4*>(lg + v);
            x[4 * j] = q.x; x[4 * j + 1] = q.y; x[4 * j + 2] = q.z; x[4 * j + 3] = q.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) x[4 * j + c] = v + c < v1 ? lg[v + c] : -INFINITY;  // (the scalar tail)
        }
    }
    // the step's bookkeeping as it is before the selection, and the raw logits at the row's context ids (the
    // penalty rewrites exactly those): read here, before either kernel that changes them runs
    const int n = a.ctx_len ? a.ctx_len[b] : 0;
    if (blockIdx.x == 0 && tid == 0) {
        a.rec[2 * b] = a.out_len[b];
        a.rec[2 * b + 1] = a.side ? min(n, (int)a.ctx_cap) : 0;
    }
    if (a.side) {
        const int* cx = a.ctx + (long)b * a.ctx_cap;
        for (int i = blockIdx.x * LP_BLOCK + tid; i < n && i < a.ctx_cap; i += nchunk * LP_BLOCK) {
            const int t = cx[i];
            a.side[(long)b * a.ctx_cap + i] = (t >= 0 && t < a.V) ? lg[t] : 0.f;
        }
    }
    // local maximum over the finite entries
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < LP_PER; ++j) {
        const int v = v0 + 4 * (tid + (j / 4) * LP_BLOCK) + (j & 3);
        const bool ok = v < v1 && lp_finite(x[j]);
        id[j] = ok ? v : LP_NONE;
        if (!ok) x[j] = -INFINITY;
        m = fmaxf(m, x[j]);
    }
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < LP_BLOCK / 64; ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    // local sum of exp(l - local max): lane order inside the wave, then the waves by index
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LP_PER; ++j)
        if (id[j] != LP_NONE) s += expf(x[j] - m);
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    // local top-K: every wave's own K, then wave 0 merges the four lists
    const int K = a.K;
    wave_topk<LP_PER>(x, id, K, wv + wave * LP_MAX_TOP, wi + wave * LP_MAX_TOP);
    __syncthreads();
    const long pb = (long)b * nchunk + blockIdx.x;
    if (tid == 0) {
        float t = red[0];
#pragma unroll
        for (int w = 1; w < LP_BLOCK / 64; ++w) t += red[w];
        a.part_max[pb] = m;
        a.part_sum[pb] = t;
    }
    if (wave == 0 && K > 0) {
        // (LP_BLOCK / 64) * K <= 80 candidates: two per lane
        float cv[2];
        int ci[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = lane + 64 * j, w = c / K, k = c - w * K;
            const bool ok = w < LP_BLOCK / 64 && wi[w * LP_MAX_TOP + k] >= 0;
            cv[j] = ok ? wv[w * LP_MAX_TOP + k] : -INFINITY;
            ci[j] = ok ? wi[w * LP_MAX_TOP + k] : LP_NONE;
        }
        wave_topk<2>(cv, ci, K, a.part_tv + pb * K, a.part_ti + pb * K);
    }
}

__global__ __launch_bounds__(LP_BLOCK) void dec_lp_final_kernel(DecLpArgs a, int nchunk) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];  // [nchunk * K] values | [nchunk * K] ids
    __shared__ float pm[64 * LP_CPL], ps[64 * LP_CPL];
    __shared__ float lse_s[2];
    __shared__ int hit;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len0 = a.rec[2 * b], n0 = a.rec[2 * b + 1];
    // an entry exactly where the selection emitted an id: out_len grew (an EOS or a done row leaves it)
    if (a.out_len[b] <= len0 || len0 >= a.out_cap) return;
    const int K = a.K;
    float* cv = dyn;
    int* ci = reinterpret_cast<int*>(dyn + (size_t)nchunk * K);
    const long pb = (long)b * nchunk;
    for (int i = tid; i < nchunk * K; i += LP_BLOCK) { cv[i] = a.part_tv[pb * K + i]; ci[i] = a.part_ti[pb * K + i]; }
    for (int i = tid; i < nchunk; i += LP_BLOCK) { pm[i] = a.part_max[pb + i]; ps[i] = a.part_sum[pb + i]; }
    if (tid == 0) hit = LP_NONE;
    __syncthreads();
    // the emitted token's raw logit: from the side row where the token occurs in the context (first match: the
    // penalty may have rewritten logits[tok]), else the logits row, which nothing has touched at tok
    const int tok = a.tok[b];
    const int* cx = a.ctx + (long)b * a.ctx_cap;
    int first = LP_NONE;
    for (int i = tid; i < n0; i += LP_BLOCK)
        if (cx[i] == tok) { first = i; break; }
    if (first != LP_NONE) atomicMin(&hit, first);
    // log-sum-exp: the chunks in index order, rescaled to the global maximum (one thread: a fixed order)
    if (tid == 64) {
        float M = -INFINITY;
        for (int j = 0; j < nchunk; ++j) M = fmaxf(M, pm[j]);
        float S = 0.f;
        for (int j = 0; j < nchunk; ++j)
            if (pm[j] > -INFINITY) S += ps[j] * expf(pm[j] - M);
        lse_s[0] = M;
        lse_s[1] = logf(S);
    }
    __syncthreads();
    const float M = lse_s[0], logS = lse_s[1];
    const bool any = M > -INFINITY;
    const long e = (long)b * a.out_cap + len0;
    if (tid == 0) {
        const float lt = (tok >= 0 && tok < a.V) ? (hit != LP_NONE ? a.side[(long)b * a.ctx_cap + hit] : a.logits[(long)b * a.ld + tok])
                                                 : -INFINITY;
        a.lp[e] = (any && lp_finite(lt)) ? lt - M - logS : -INFINITY;
    }
    if (wave != 0 || K == 0) return;
    // K-way merge of the chunks' sorted lists: every lane holds the heads of its chunks
    int head[LP_CPL];
#pragma unroll
    for (int c = 0; c < LP_CPL; ++c) head[c] = 0;
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = LP_NONE;
#pragma unroll
        for (int c = 0; c < LP_CPL; ++c) {
            const int j = lane + 64 * c;
            if (j < nchunk && head[c] < K) {
                const int i = ci[j * K + head[c]];
                const float v = cv[j * K + head[c]];
                if (i >= 0 && lp_better(v, i, bv, bi)) { bv = v; bi = i; }
            }
        }
        wave_argmax(bv, bi);
#pragma unroll
        for (int c = 0; c < LP_CPL; ++c) {
            const int j = lane + 64 * c;
            if (j < nchunk && head[c] < K && bi != LP_NONE && ci[j * K + head[c]] == bi) ++head[c];
        }
        if (lane == 0) {
            a.top_id[e * K + k] = bi == LP_NONE ? -1 : bi;
            a.top_lp[e * K + k] = bi == LP_NONE ? -INFINITY : bv - M - logS;
        }
    }
}

static void lp_check(const DecLpArgs& a) {
    if (a.B <= 0 || a.V <= 0 || a.K < 0 || a.K > LP_MAX_TOP) throw std::runtime_error("EINVAL: log-probabilities need B, V > 0 and 0 <= K <= 20");
    if (dec_lp_chunks(a.V) > 64 * LP_CPL) throw std::runtime_error("EINVAL: log-probabilities: vocabulary above 524288");
    if (!a.logits || !a.tok || !a.out_len || !a.rec || !a.part_max || !a.part_sum || !a.lp || a.out_cap <= 0 ||
        (a.K && (!a.part_tv || !a.part_ti || !a.top_id || !a.top_lp)) || (a.side && (!a.ctx || !a.ctx_len || a.ctx_cap <= 0)))
        throw std::runtime_error("EINVAL: log-probability workspaces");
}

void launch_dec_lp_partial(const DecLpArgs& a, hipStream_t s) {
    lp_check(a);
    DSOCR_LAUNCH(dec_lp_partial_kernel, dim3((unsigned)dec_lp_chunks(a.V), a.B), dim3(LP_BLOCK), 0, s, a);
}

void launch_dec_lp_final(const DecLpArgs& a, hipStream_t s) {
    lp_check(a);
    const int nchunk = (int)dec_lp_chunks(a.V);
    const size_t lds = (size_t)nchunk * a.K * 8;  // <= 256 * 20 * 8 = 40 KB
    DSOCR_LAUNCH(dec_lp_final_kernel, dim3(1, a.B), dim3(LP_BLOCK), lds, s, a, nchunk);
}

}  // namespace dsocr
