// Frequency / presence penalties over a page's generated tokens: l[t] -= frequency * c[t] + presence
// for every id t that occurs c[t] > 0 times in out_ids[0 .. out_len).  Stateless: no per-slot count table; the
// counts are formed from the output row itself every step.
//   dec_out_penalty   grid (PN_GRID(out_cap), B), in the step after launch_rep_penalty and before the selection.
//                     A row whose record is off is left after one block-uniform load of the record.
// Position i of the row belongs to one thread (grid-stride over blocks of PN_BLOCK positions).  The whole row
// passes through LDS in tiles of PN_TILE ids (once per block when it fits one tile); every thread compares its id
// with the tile (all lanes read the same LDS address: a broadcast, no bank conflict), counting the occurrences and
// those before its own position.  The
// thread that holds the first occurrence does the one read-modify-write of l[t]: no two threads write one
// column, so no atomics.  Two waves per block, 8 KB of LDS: the work is O(n^2) compares on a row of a few hundred
// ids, latency-bound, and many small blocks spread it over the CUs.
#include <algorithm>

#include "decode_common.hpp"

namespace dsocr {

constexpr int PN_BLOCK = 128;
constexpr int PN_TILE = 2048;  // ids per LDS tile (a multiple of 4: the compare loop reads 16 bytes at a time)
static_assert(PN_TILE % 4 == 0 && PN_TILE % PN_BLOCK == 0, "tile of whole int4s, filled by whole blocks");

static unsigned pn_grid(long out_cap) { return (unsigned)std::min<long>(8, std::max<long>(1, (out_cap + 255) / 256)); }

__global__ __launch_bounds__(PN_BLOCK) void dec_out_penalty_kernel(DecPenaltyArgs a) {
    __shared__ __attribute__((aligned(16))) int tile[PN_TILE];
    const int b = blockIdx.y, tid = threadIdx.x;
    const PenaltyRec rec = a.rec[b];
    if (rec.frequency == 0.f && rec.presence == 0.f) return;  // block-uniform: the row is neither read nor written
    const int n = min(max(a.out_len[b], 0), (int)a.out_cap);
    const int* out = a.out_ids + (long)b * a.out_cap;
    float* lg = a.logits + (long)b * a.ld;
    // (base, the tile loop and its barriers are block-uniform; a thread past n or with an id outside [0, V) carries
    // -2, which no tile entry equals: ids are >= -1 after the pad)
    auto stage = [&](int j0, int len, int len4) {
        for (int j = tid; j < len4; j += PN_BLOCK) {
            const int u = j < len ? out[j0 + j] : -1;
            tile[j] = u < -1 ? -1 : u;
        }
    };
    // a row of at most one tile (the usual case) is staged once, ahead of the grid-stride loop
    const bool one_tile = n <= PN_TILE;
    if (one_tile) {
        stage(0, n, (n + 3) & ~3);
        __syncthreads();
    }
    for (int base = blockIdx.x * PN_BLOCK; base < n; base += gridDim.x * PN_BLOCK) {
        const int i = base + tid;
        int t = i < n ? out[i] : -2;
        if (t < 0 || t >= a.V) t = -2;
        int cnt = 0, before = 0;
        for (int j0 = 0; j0 < n; j0 += PN_TILE) {
            const int len = min(PN_TILE, n - j0), len4 = (len + 3) & ~3;
            if (!one_tile) {
                __syncthreads();  // the previous tile has been read by every thread
                stage(j0, len, len4);
                __syncthreads();
            }
            for (int j = 0; j < len4; j += 4) {
                const int4 q = *reinterpret_cast<const int4*>(tile + j);
                const int g = j0 + j;
                const int e0 = q.x == t, e1 = q.y == t, e2 = q.z == t, e3 = q.w == t;
                cnt += e0 + e1 + e2 + e3;
                before += (e0 & (g < i)) + (e1 & (g + 1 < i)) + (e2 & (g + 2 < i)) + (e3 & (g + 3 < i));
            }
        }
        if (t >= 0 && before == 0) {  // the first occurrence of t: cnt >= 1 (its own position)
            // one multiply, one add, one subtract, each rounded.  HIP's __fmul_rn / __fadd_rn are plain operators that
            // the default -ffp-contract=fast fuses into one fma (seen as a last-bit difference against NumPy where
            // frequency * c is inexact and presence != 0), so contraction is switched off for this block
#pragma clang fp contract(off)
            const float m = rec.frequency * (float)cnt;
            const float p = m + rec.presence;
            lg[t] = lg[t] - p;
        }
    }
}

void launch_dec_out_penalty(const DecPenaltyArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.V <= 0 || a.ld < a.V || a.out_cap <= 0 || !a.logits || !a.out_ids || !a.out_len || !a.rec)
        throw std::runtime_error("EINVAL: output penalty needs B, V, out_cap > 0, rows of at least V floats, the output rows and the records");
    DSOCR_LAUNCH(dec_out_penalty_kernel, dim3(pn_grid(a.out_cap), a.B), dim3(PN_BLOCK), 0, s, a);
}

}  // namespace dsocr
