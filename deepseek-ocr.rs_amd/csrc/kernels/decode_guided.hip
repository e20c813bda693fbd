// Guided decoding: a request's token automaton constrains what it may emit, inside the decode step.
//   guided_fill / _scatter  at admission, outside the step graph: the staged automaton becomes the row's dense
//                           bitmask [n_states][mask_ld] (bit t of state s: id t has an edge from s; the EOS bit iff s
//                           accepts) and its CSR, and state / seen / status / on are reset
//   dec_guided_mask         grid (chunks of V, B), in the step, after the logit bias and before dec_lp_partial: every
//                           id whose bit is clear in the row's state gets -inf
//   dec_guided_advance      grid (B), one wave per row, right after the final selection kernel: the appended token is
//                           searched among the state's edges
//   guided_slot_move        the used part of the tables and the scalars, row src -> dst (a session's compaction)
// The mask is a store-only stream (one mask byte per 8 logits read, -inf written where a bit is clear, no logit
// read: a kept logit is never touched, so it stays bit for bit); the advance is a few dependent loads behind a launch
// boundary.  No LDS; every early exit sits on scalar loads of the block's own row.
//
// The scatter uses atomicOr, one thread per edge.  The alternative, one thread per mask word searching the state's
// edge range, does n_states x mask_ld searches (4 M at the caps) for automata that typically have a few hundred
// edges; the atomics only meet where two edges of one state fall into one word, and the build runs once per
// admission, outside the step.
#include "decode_common.hpp"

namespace dsocr {

constexpr int GD_BLOCK = 256;
constexpr int GD_PER_BLOCK = 2048;  // 8 logits per thread: one mask byte
constexpr int GD_MAX_GRID = 2048;   // the build and the move are grid-stride loops

__global__ __launch_bounds__(GD_BLOCK) void guided_fill_kernel(GuidedBuildArgs a) {
    const GuidedTables& t = a.t;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *t.on = a.stage ? 1 : 0;
        if (a.stage) { *t.state = a.start; *t.seen = 0; *t.status = 0; }
    }
    if (!a.stage) return;
    const long i0 = (long)blockIdx.x * GD_BLOCK + threadIdx.x, step = (long)gridDim.x * GD_BLOCK;
    const int n = a.n_states;
    const int* acc = a.stage;
    const int* rp = a.stage + n;
    const int* tk = rp + n + 1;
    const int* nx = tk + a.E;
    // the bitmask: whole uint4s (mask_ld % 4 == 0, 16-byte aligned rows), zero but for an accepting state's EOS bit
    const long q_ld = t.mask_ld / 4, nq = (long)n * q_ld;
    const bool eos_on = a.eos >= 0 && a.eos < a.V;
    const long eos_q = eos_on ? (a.eos >> 5) / 4 : -1;
    for (long i = i0; i < nq; i += step) {
        const long s = i / q_ld, q = i - s * q_ld;
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (q == eos_q && acc[s]) {
            const unsigned bit = 1u << (a.eos & 31);
            const int c = (a.eos >> 5) & 3;
            if (c == 0) w.x = bit; else if (c == 1) w.y = bit; else if (c == 2) w.z = bit; else w.w = bit;
        }
        reinterpret_cast<uint4*>(t.mask)[i] = w;
    }
    for (long i = i0; i <= n; i += step) t.rowptr[i] = rp[i];
    for (long i = i0; i < a.E; i += step) { t.tok[i] = tk[i]; t.next[i] = nx[i]; }
}

// one thread per edge: its state is the last s with row_ptr[s] <= e (row_ptr is non-decreasing from 0 to E)
__global__ __launch_bounds__(GD_BLOCK) void guided_scatter_kernel(GuidedBuildArgs a) {
    const long e = (long)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (e >= a.E) return;
    const int n = a.n_states;
    const int* rp = a.stage + n;
    const int* tk = rp + n + 1;
    int lo = 0, hi = n;  // invariant: rp[lo] <= e < rp[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rp[mid] <= e) lo = mid; else hi = mid;
    }
    const int tkn = tk[e];
    if (tkn < 0 || tkn >= a.V) return;
    atomicOr(a.t.mask + (long)lo * a.t.mask_ld + (tkn >> 5), 1u << (tkn & 31));
}

__global__ __launch_bounds__(GD_BLOCK) void dec_guided_mask_kernel(DecGuidedMaskArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    // block-uniform (scalar loads of the row's own words): a row without an automaton, a violated one and a finished
    // one are neither read further nor written
    if (!a.t.on[b]) return;
    const int s = a.t.state[b];
    if (s < 0 || s >= a.t.cap_states) return;
    if (a.done[b]) return;
    const int v = blockIdx.x * GD_PER_BLOCK + 8 * tid;
    if (v >= a.V) return;
    float* lg = a.logits + (long)b * a.ld;
    // little-endian words: byte v / 8 of the state's row holds bits v .. v + 7 (v / 8 < 4 * mask_ld)
    const unsigned char* mrow = reinterpret_cast<const unsigned char*>(a.t.mask + ((long)b * a.t.cap_states + s) * a.t.mask_ld);
    const unsigned m = mrow[v >> 3];
    if (m == 0xffu) return;
    const bool vec = (reinterpret_cast<uintptr_t>(lg) & 15) == 0;  // (v % 8 == 0: lg + v is aligned iff lg is)
    if (vec && m == 0u && v + 7 < a.V) {
        const float4 q = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        *reinterpret_cast<float4*>(lg + v) = q;
        *reinterpret_cast<float4*>(lg + v + 4) = q;
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c)  // (the scalar path: an unaligned row, a byte with a kept id, the tail of V)
            if (v + c < a.V && !((m >> c) & 1u)) lg[v + c] = -INFINITY;  // never a column in [V, ld)
    }
}

__global__ __launch_bounds__(64) void dec_guided_advance_kernel(DecGuidedAdvanceArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    // block-uniform: the row's own words
    if (!a.t.on[b]) return;
    const int s = a.t.state[b];
    if (s < 0 || s >= a.t.cap_states) return;
    const int L = a.out_len[b];
    if (L == a.t.seen[b]) return;  // nothing was appended: EOS selected, or the row is done
    if (L < 1 || L > a.out_cap) return;
    const int tkn = a.out[(long)b * a.out_cap + (L - 1)];
    const int* rp = a.t.rowptr + (long)b * (a.t.cap_states + 1);
    const int* tk = a.t.tok + (long)b * a.t.cap_edges;
    const int r0 = rp[s], r1 = rp[s + 1], n = r1 - r0;
    int at = -1;
    if (r0 >= 0 && n > 0 && r1 <= a.t.cap_edges) {
        if (n <= 64) {  // one compare per lane
            const bool hit = lane < n && tk[r0 + lane] == tkn;
            const unsigned long long bal = __ballot(hit);
            if (bal) at = r0 + __ffsll((long long)bal) - 1;
        } else if (lane == 0) {  // ids ascend within a state
            int lo = r0, hi = r1;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (tk[mid] < tkn) lo = mid + 1; else hi = mid;
            }
            if (lo < r1 && tk[lo] == tkn) at = lo;
        }
    }
    if (lane != 0) return;
    a.t.seen[b] = L;
    const int ns = at >= 0 ? a.t.next[(long)b * a.t.cap_edges + at] : -1;
    if (ns >= 0 && ns < a.t.cap_states) {
        a.t.state[b] = ns;
        if (rp[ns] == rp[ns + 1]) { a.t.status[b] = 1; a.done[b] = 1; }  // terminal: complete
    } else {  // no edge (the id-0 last resort): violated
        a.t.state[b] = -1; a.t.status[b] = 2; a.done[b] = 1;
    }
}

__global__ __launch_bounds__(GD_BLOCK) void guided_slot_move_kernel(GuidedTables t, int src, int dst, int n_states, long E) {
    const int on = t.on[src];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        t.on[dst] = on; t.state[dst] = t.state[src]; t.seen[dst] = t.seen[src]; t.status[dst] = t.status[src];
    }
    if (!on) return;
    const long i0 = (long)blockIdx.x * GD_BLOCK + threadIdx.x, step = (long)gridDim.x * GD_BLOCK;
    const long row_q = (long)t.cap_states * t.mask_ld / 4, nq = (long)n_states * t.mask_ld / 4;
    const uint4* ms = reinterpret_cast<const uint4*>(t.mask) + src * row_q;
    uint4* md = reinterpret_cast<uint4*>(t.mask) + dst * row_q;
    for (long i = i0; i < nq; i += step) md[i] = ms[i];
    const long rs = (long)src * (t.cap_states + 1), rd = (long)dst * (t.cap_states + 1);
    for (long i = i0; i <= n_states; i += step) t.rowptr[rd + i] = t.rowptr[rs + i];
    const long es = (long)src * t.cap_edges, ed = (long)dst * t.cap_edges;
    for (long i = i0; i < E; i += step) { t.tok[ed + i] = t.tok[es + i]; t.next[ed + i] = t.next[es + i]; }
}

static void check_tables(const GuidedTables& t, const char* what) {
    if (!t.mask || !t.rowptr || !t.tok || !t.next || !t.state || !t.seen || !t.status || !t.on || t.mask_ld <= 0 ||
        t.mask_ld % 4 || (reinterpret_cast<uintptr_t>(t.mask) & 15) || t.cap_states < 1 || t.cap_states > GUIDED_MAX_STATES ||
        t.cap_edges < 1 || t.cap_edges > GUIDED_MAX_EDGES)
        throw std::runtime_error(std::string("EINVAL: ") + what + " needs the guided tables (16-byte aligned mask, mask_ld % 4 == 0)");
}

static unsigned stride_grid(long items) {
    return (unsigned)std::min<long>(std::max<long>((items + GD_BLOCK - 1) / GD_BLOCK, 1), GD_MAX_GRID);
}

void launch_guided_build(const GuidedBuildArgs& a, hipStream_t s) {
    check_tables(a.t, "guided build");
    if (!a.stage) {
        DSOCR_LAUNCH(guided_fill_kernel, dim3(1), dim3(GD_BLOCK), 0, s, a);
        return;
    }
    if (a.V <= 0 || a.t.mask_ld * 32 < a.V || a.n_states < 1 || a.n_states > a.t.cap_states || a.E < 0 ||
        a.E > a.t.cap_edges || a.start < 0 || a.start >= a.n_states)
        throw std::runtime_error("EINVAL: guided build: the automaton does not fit the row's tables");
    const long items = std::max<long>((long)a.n_states * a.t.mask_ld / 4, std::max<long>(a.E, a.n_states + 1));
    DSOCR_LAUNCH(guided_fill_kernel, dim3(stride_grid(items)), dim3(GD_BLOCK), 0, s, a);
    if (a.E) DSOCR_LAUNCH(guided_scatter_kernel, dim3((unsigned)((a.E + GD_BLOCK - 1) / GD_BLOCK)), dim3(GD_BLOCK), 0, s, a);
}

void launch_dec_guided_mask(const DecGuidedMaskArgs& a, hipStream_t s) {
    check_tables(a.t, "guided mask");
    if (a.B <= 0 || a.V <= 0 || a.ld < a.V || a.t.mask_ld * 32 < a.V || !a.logits || !a.done)
        throw std::runtime_error("EINVAL: guided mask needs B, V > 0, rows of at least V floats, mask rows of V bits and the done flags");
    DSOCR_LAUNCH(dec_guided_mask_kernel, dim3((unsigned)((a.V + GD_PER_BLOCK - 1) / GD_PER_BLOCK), a.B), dim3(GD_BLOCK), 0, s, a);
}

void launch_dec_guided_advance(const DecGuidedAdvanceArgs& a, hipStream_t s) {
    check_tables(a.t, "guided advance");
    if (a.B <= 0 || a.out_cap <= 0 || !a.out || !a.out_len || !a.done)
        throw std::runtime_error("EINVAL: guided advance needs B > 0 and the output rows");
    DSOCR_LAUNCH(dec_guided_advance_kernel, dim3(a.B), dim3(64), 0, s, a);
}

void launch_guided_slot_move(const GuidedTables& t, int src, int dst, int n_states, long E, hipStream_t s) {
    check_tables(t, "guided slot move");
    if (src < 0 || dst < 0 || src == dst || n_states < 0 || n_states > t.cap_states || E < 0 || E > t.cap_edges)
        throw std::runtime_error("EINVAL: guided slot move needs src != dst and the source's sizes within the tables");
    const long items = std::max<long>((long)n_states * t.mask_ld / 4, std::max<long>(E, n_states + 1));
    DSOCR_LAUNCH(guided_slot_move_kernel, dim3(stride_grid(items)), dim3(GD_BLOCK), 0, s, t, src, dst, n_states, E);
}

}  // namespace dsocr
