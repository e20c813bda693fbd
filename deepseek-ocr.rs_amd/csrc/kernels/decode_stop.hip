// Stop sequences matched inside the decode step: a request's stop set ends its page on the device,
// in the step that completes a sequence, through the same done[b] word EOS writes.
//   stop_table_build       at admission, outside the step graph: the request's staged list becomes the row's table
//                          [STOP_MAX_SEQS][1 + STOP_MAX_LEN] (a length, then the ids), and seen / hit are reset
//   dec_stop_match         grid (B), one wave per row, in the step right after the final selection kernel: the tail
//                          of the row's output against every sequence
//   stop_slot_move         the four arrays' row src -> dst (a session's compaction)
// One token arrives per step, so only the tail is looked at: 16 x 32 compares at most, 8 per lane.  Latency-bound
// (a few dependent loads behind a launch boundary): no LDS, every early exit on scalar loads of the block's own row.
#include "decode_common.hpp"

namespace dsocr {

static_assert(STOP_MAX_SEQS * 4 == 64 && STOP_MAX_LEN == 32, "dec_stop_match: 4 lanes of 8 ids per sequence, one wave");

__global__ __launch_bounds__(64) void dec_stop_match_kernel(DecStopArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    // block-uniform (scalar loads of the row's own words): a row without a stop set is neither read further nor written
    const int n = a.n_seq[b];
    if (n == 0) return;
    const int L = a.out_len[b];
    if (L == a.seen[b]) return;  // nothing was appended: EOS selected, or the row is done
    const int s = lane >> 2, q = lane & 3;  // sequence s, ids [8 q, 8 q + 8) of it
    const int* row = a.tab + (long)b * STOP_ROW_INTS + s * (1 + STOP_MAX_LEN);
    const int m = s < n ? row[0] : 0;
    // m <= L: a sequence longer than the output cannot match, and out[L - m] is never below out[0]
    bool ok = m >= 1 && m <= STOP_MAX_LEN && m <= L && L <= a.out_cap;
    if (ok) {
        const int* tail = a.out + (long)b * a.out_cap + (L - m);
        const int j1 = min(8 * q + 8, m);
        for (int j = 8 * q; j < j1; ++j) ok = ok && tail[j] == row[1 + j];
    }
    // wave reduction: a sequence matches when its four lanes do; the lowest set group is the lowest index
    const unsigned long long bal = __ballot(ok);
    const unsigned long long grp = bal & (bal >> 1) & (bal >> 2) & (bal >> 3) & 0x1111111111111111ull;
    if (lane != 0) return;
    a.seen[b] = L;
    if (grp) {
        const int sq = (__ffsll((long long)grp) - 1) >> 2;
        a.hit[2 * b] = sq;
        a.hit[2 * b + 1] = a.tab[(long)b * STOP_ROW_INTS + sq * (1 + STOP_MAX_LEN)];
        a.done[b] = 1;
    }
}

__global__ __launch_bounds__(256) void stop_table_build_kernel(StopBuildArgs a) {
    const int tid = threadIdx.x;
    const int n = a.stage ? min(max(a.stage[0], 0), STOP_MAX_SEQS) : 0;
    if (tid == 0) { *a.n_seq = n; *a.seen = 0; a.hit[0] = -1; a.hit[1] = 0; }
    if (n == 0) return;
    const int* lens = a.stage + 1;
    const int* ids = a.stage + 1 + STOP_MAX_SEQS;
    for (int e = tid; e < STOP_ROW_INTS; e += 256) {
        const int s = e / (1 + STOP_MAX_LEN), c = e % (1 + STOP_MAX_LEN);
        int off = 0;
        for (int i = 0; i < s && i < n; ++i) off += min(max(lens[i], 0), STOP_MAX_LEN);
        const int m = s < n ? min(max(lens[s], 0), STOP_MAX_LEN) : 0;
        a.tab[e] = c == 0 ? m : (c - 1 < m ? ids[off + c - 1] : -1);  // off + m <= STOP_MAX_SEQS * STOP_MAX_LEN
    }
}

__global__ __launch_bounds__(256) void stop_slot_move_kernel(int* tab, int* n_seq, int* seen, int* hit, int src, int dst) {
    const int tid = threadIdx.x;
    const int n = n_seq[src];
    if (tid == 0) { n_seq[dst] = n; seen[dst] = seen[src]; hit[2 * dst] = hit[2 * src]; hit[2 * dst + 1] = hit[2 * src + 1]; }
    if (n == 0) return;
    for (int e = tid; e < STOP_ROW_INTS; e += 256) tab[(long)dst * STOP_ROW_INTS + e] = tab[(long)src * STOP_ROW_INTS + e];
}

void launch_dec_stop_match(const DecStopArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.out_cap <= 0 || !a.out || !a.out_len || !a.done || !a.tab || !a.n_seq || !a.seen || !a.hit)
        throw std::runtime_error("EINVAL: stop match needs B > 0, the output rows and the four stop arrays");
    DSOCR_LAUNCH(dec_stop_match_kernel, dim3(a.B), dim3(64), 0, s, a);
}

void launch_stop_table_build(const StopBuildArgs& a, hipStream_t s) {
    if (!a.tab || !a.n_seq || !a.seen || !a.hit) throw std::runtime_error("EINVAL: stop table build needs the row's four cells");
    DSOCR_LAUNCH(stop_table_build_kernel, dim3(1), dim3(256), 0, s, a);
}

void launch_stop_slot_move(int* tab, int* n_seq, int* seen, int* hit, int src, int dst, hipStream_t s) {
    if (!tab || !n_seq || !seen || !hit || src < 0 || dst < 0 || src == dst)
        throw std::runtime_error("EINVAL: stop slot move needs the four arrays and src != dst");
    DSOCR_LAUNCH(stop_slot_move_kernel, dim3(1), dim3(256), 0, s, tab, n_seq, seen, hit, src, dst);
}

}  // namespace dsocr
