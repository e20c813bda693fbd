// Windowed no-repeat n-gram ban with a token whitelist: with n = ctx_len and the (g-1)-token suffix
// s = ctx[n-g+1 .. n), every start i in [max(0, n-w), n-g] whose ctx[i .. i+g-1) equals s makes t = ctx[i+g-1] a
// candidate; a candidate inside [0, V) and outside the whitelist gets l[t] = -inf, unless that would leave the row
// without a finite logit (then the row is left as it is).  Stateless: nothing but the record follows a slot.
//   dec_ngram_window   grid (B), one block per row: the row's decision is made inside the block.  After the
//                      frequency / presence launch, in the plain ban's place; the selection then runs with ngram 0.
//                      A row whose record is off (and a.plain < 2) is left after one block-uniform load of it.
// Phases, each block-uniform:
//   1. count: thread `tid` owns the starts lo + tid, lo + tid + NW_BLOCK, ...; a start is compared backwards from the
//      last suffix token with early exit (nearly every start fails on the first compare).  The suffix is read
//      through LDS when g - 1 <= NW_SUF, else from the context row itself (L1).  m = matches that are candidates.
//      m == 0: return.
//   2. finite logits are counted chunk by chunk, stopping once more than m were seen (usually in the first chunk,
//      so the row is not read): more than m finite logits cannot all be banned by m candidates.
//   3. only a row with at most m finite logits is decided exactly: a thread that holds a finite logit looks its
//      column up among the candidates (a window scan that tests the continuation first).  No survivor: return.
//   4. write: the starts are matched again and every candidate stores -inf.  Duplicates store the same value: no
//      atomics, no read-modify-write.
// Four waves and 4.2 KB of LDS per block: latency-bound work on a window of tens to a few thousand ids.
#include <climits>

#include "decode_common.hpp"

namespace dsocr {

constexpr int NW_BLOCK = 256;
constexpr int NW_SUF = 1024;             // suffix ids kept in LDS
constexpr int NW_CHUNK = NW_BLOCK * 8;   // logits per counting step

__device__ __forceinline__ bool nw_finite(float x) { return fabsf(x) < INFINITY; }  // (NaN: false)

// the block's sum of v, in every thread (red: NW_BLOCK / 64 ints; the leading barrier frees it from its last use)
__device__ __forceinline__ int nw_block_sum(int v, int* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < NW_BLOCK / 64; ++w) t += red[w];
    return t;
}

__global__ __launch_bounds__(NW_BLOCK) void dec_ngram_window_kernel(DecNgramWindowArgs a) {
    __shared__ int suf[NW_SUF];
    __shared__ int white[NGRAM_MAX_WHITELIST];
    __shared__ int red[NW_BLOCK / 64];
    __shared__ int survivor;
    const int b = blockIdx.x, tid = threadIdx.x;
    const NgramWindowRec* rec = a.rec + b;
    int g = rec->g, w = rec->w, nw = min(max(rec->n_white, 0), NGRAM_MAX_WHITELIST);
    if (g < 2) {  // no record of its own: the plain ban as the record {plain, unbounded, no whitelist}, or nothing
        g = a.plain; w = INT_MAX; nw = 0;
        if (g < 2) return;
    }
    const int n = min(max(a.ctx_len[b], 0), (int)a.ctx_cap);
    if (w < 1 || n < g) return;
    const int lo = max(0, n - w), hi = n - g;  // the admissible starts, both ends included
    if (lo > hi) return;
    const int V = a.V;
    const int* cx = a.ctx + (long)b * a.ctx_cap;
    float* lg = a.logits + (long)b * a.ld;
    const int* tail = cx + (n - g + 1);  // the suffix: g - 1 ids
    const bool in_lds = g - 1 <= NW_SUF;
    if (in_lds)
        for (int j = tid; j < g - 1; j += NW_BLOCK) suf[j] = tail[j];
    if (tid < nw) white[tid] = rec->white[tid];
    if (tid == 0) survivor = 0;
    __syncthreads();
    const int* sfx = in_lds ? suf : tail;
    // ctx[i .. i+g-1) == suffix, compared from the last id backwards (i + g - 1 <= n - 1: inside the row)
    auto prefix_matches = [&](int i) {
        for (int k = g - 2; k >= 0; --k)
            if (cx[i + k] != sfx[k]) return false;
        return true;
    };
    auto whitelisted = [&](int t) {
        for (int q = 0; q < nw; ++q)
            if (white[q] == t) return true;  // (every lane reads the same address: a broadcast)
        return false;
    };
    // the id start i bans, or -1
    auto candidate = [&](int i) {
        if (!prefix_matches(i)) return -1;
        const int t = cx[i + g - 1];
        return (t < 0 || t >= V || whitelisted(t)) ? -1 : t;
    };
    // ---- 1. the number of candidates (repeats counted)
    int mine = 0;
    for (int i = lo + tid; i <= hi; i += NW_BLOCK) mine += candidate(i) >= 0 ? 1 : 0;
    const int m = nw_block_sum(mine, red);
    if (m == 0) return;
    // ---- 2. more than m finite logits?
    int finite = 0;
    for (int v0 = 0; v0 < V && finite <= m; v0 += NW_CHUNK) {
        int c = 0;
        for (int j = 0; j < NW_CHUNK / NW_BLOCK; ++j) {
            const int v = v0 + j * NW_BLOCK + tid;
            if (v < V && nw_finite(lg[v])) ++c;
        }
        finite += nw_block_sum(c, red);
    }
    // ---- 3. at most m finite logits: does one of them survive the ban?
    if (finite <= m) {
        bool alive = false;
        for (int v = tid; v < V && !alive; v += NW_BLOCK) {
            if (!nw_finite(lg[v])) continue;
            bool banned = false;
            if (!whitelisted(v))
                for (int i = lo; i <= hi && !banned; ++i) banned = cx[i + g - 1] == v && prefix_matches(i);
            alive = !banned;
        }
        if (alive) survivor = 1;  // (every writer stores the same value)
        __syncthreads();
        if (!survivor) return;
    }
    // ---- 4. the ban
    for (int i = lo + tid; i <= hi; i += NW_BLOCK) {
        const int t = candidate(i);
        if (t >= 0) lg[t] = -INFINITY;
    }
}

void launch_dec_ngram_window(const DecNgramWindowArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.V <= 0 || a.ld < a.V || a.ctx_cap <= 0 || !a.logits || !a.ctx || !a.ctx_len || !a.rec)
        throw std::runtime_error("EINVAL: n-gram window needs B, V, ctx_cap > 0, rows of at least V floats, the context rows and the records");
    DSOCR_LAUNCH(dec_ngram_window_kernel, dim3(a.B), dim3(NW_BLOCK), 0, s, a);
}

}  // namespace dsocr
