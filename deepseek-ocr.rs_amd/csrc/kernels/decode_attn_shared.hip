// Decode attention of B rows that share a prompt (Engine::generate_n).
//
// Contract: the f32 cache in its [page][kv_head][max_len][hd] layout.  Keys [0, P) (P = shared_len >= 1) of every row
// are read from PAGE 0 ONLY; rows [0, P) of pages 1 .. B - 1 are never read or written.  Keys [P, kv_pos[b]) come from
// page b (kv_pos[b] >= P for every row).  The step's own key / value come from qkv, are rotated at kv_pos[b] unless
// prerot, appended to page b at row kv_pos[b] and used from LDS, not from the load.  Everything is f32 and every
// product exact (f32 MFMA or fmaf).  hd 32 / 64 / 128, heads % kv_heads == 0, 1 <= B <= 16, max_len <= 512 * 128.
//
// Two launches.  The first holds two kinds of blocks, grid (nsc + noc B, heads), 256 threads:
//   shared block (c < nsc = ceil(P / 128), h): loads its 128-key K and V chunk of page 0 ONCE and serves the B query
//     rows of head h as the columns of v_mfma_f32_16x16x4_f32 (columns >= B are zero).  Wave w owns keys 32 w .. + 31
//     as two 16-key tiles.  S^T = K.Q^T: lane (key l % 16, group g = l / 16) feeds dims 16 u + 4 g + e in instruction
//     (u, e) - one float4 of its own key row per u, the four groups of a key 64 contiguous bytes - and Q matches from
//     LDS.  The accumulator holds keys 4 g + r of column l % 16, which is the B operand of O^T += V^T.P^T with the
//     keys in that permuted order (attn_tile.hpp's pattern at 16 x 16); the A operand is V[key 4 g + r][dim], lane
//     j = l % 16 owning dims VEC (j + 16 u) + e so that its V operand too is 16-byte runs of key rows read straight
//     from memory (16 lanes 256 contiguous bytes).  No LDS staging of K or V.  Softmax per column over the block's
//     128 keys (keys >= P score -inf by a select, loads clamped to row P - 1); the four waves' O are summed in wave
//     order through LDS.  One record (m, l, O[hd]) per (row, head, chunk).
//   own block (c < noc = ceil((max_len - P) / 128), h, b): keys P + 128 c .. of page b for the single query (b, h):
//     dec_attn_kv16_kernel's fmaf + DPP-butterfly form on f32 rows (a key is hd / 8 lanes of 8 dims, every load
//     instruction 2 KiB contiguous).  One query is 1 of 16 matrix columns, so no MFMA here.  A chunk that starts past
//     kv_pos[b] returns before issuing anything; the block that owns kv_pos[b] appends (one writer per kv head).
// The second launch merges: thread (row, head, d) combines the query's records in key order, shared chunks then own
// chunks (attn_rec_combine's sums, with expf).  Nothing is handed from block to block inside a launch: the kernel
// boundary orders the records.  No counter, no sentinel, no polling.
#include "decode_common.hpp"

namespace dsocr {

namespace {
constexpr int SH_CH = 128;    // keys per block
constexpr int SH_COLS = 16;   // query columns of the 16 x 16 MFMA
constexpr int SH_HDR = 4;     // record: [m, l, -, -, o[HD]]

template <int N>
__device__ __forceinline__ void ld_nt(const float* p, float* o) {
    if constexpr (N == 4) {
        const float4 v = ldg_nt_f4(p);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 v = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p));
        o[0] = v[0]; o[1] = v[1];
    }
}

// element td of a q or k head row, rotated at pos (x cos + sign partner sin, as dec_attn_body)
template <bool PREROT>
__device__ __forceinline__ float rope_elem(const DecAttnSharedArgs& a, const float* hrow, int td, int pos) {
    if (PREROT || td >= a.rope_dim) return hrow[td];
    const int half = a.rope_dim / 2;
    auto map = [&](int i) { return !a.use_mla ? i : (i < half ? 2 * i : 2 * (i - half) + 1); };
    const float x = hrow[map(td)], r = hrow[td < half ? map(td + half) : map(td - half)];
    const float sg = td < half ? -1.f : 1.f;
    return x * a.cos[(long)pos * a.rope_dim + td] + (sg * r) * a.sin[(long)pos * a.rope_dim + td];
}

// max / sum of a value over the four lane groups of a column (lanes l, l ^ 16, l ^ 32, l ^ 48)
__device__ __forceinline__ float col_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float col_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

template <int HD>
__device__ __forceinline__ float* rec_of(const DecAttnSharedArgs& a, int nrec, int b, int h, int rec) {
    return a.part + (((long)b * a.heads + h) * nrec + rec) * (HD + SH_HDR);
}

// ---------------------------------------------------------------- shared block: chunk c of [0, P), head h, all rows
template <int HD, bool PREROT>
__device__ __forceinline__ void shared_block(const DecAttnSharedArgs& a, float* lds, int nrec, int c, int h) {
    constexpr int QP = HD + 4;             // q row pitch (16-byte aligned rows)
    constexpr int OP = HD + 1;             // O pitch: the 64 lanes of a store fall on 64 banks
    constexpr int KU = HD / 16;            // float4 of its key row per lane and tile
    constexpr int DT = HD / 16;            // O^T tiles of 16 dims; dims per lane of the V operand
    constexpr int VEC = DT >= 4 ? 4 : DT;  // floats per V load
    constexpr int VU = DT / VEC;
    float* qs = lds;                           // [16][QP]
    float* red_m = qs + SH_COLS * QP;          // [4 waves][16]
    float* red_l = red_m + 4 * SH_COLS;        // [4 waves][16]
    float* o_s = red_l + 4 * SH_COLS;          // [4 waves][16][OP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int P = a.shared_len, B = a.B;
    const int gq = a.heads / a.kv_heads, kvh = h / gq;
    const float* Kc = a.kc + (long)kvh * a.head_stride;  // page 0
    const float* Vc = a.vc + (long)kvh * a.head_stride;
    const int k0 = c * SH_CH + wave * 32;
    // 1. every K and V load of the wave's 32 keys (clamped to row P - 1: a key past it is masked at use)
    float kreg[2][KU][4], vreg[2][4][DT];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float* kr = Kc + (long)min(k0 + t * 16 + col, P - 1) * HD + 4 * g;
#pragma unroll
        for (int u = 0; u < KU; ++u) ld_nt<4>(kr + 16 * u, kreg[t][u]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* vr = Vc + (long)min(k0 + t * 16 + 4 * g + r, P - 1) * HD + VEC * col;
#pragma unroll
            for (int u = 0; u < VU; ++u) ld_nt<VEC>(vr + VEC * 16 * u, vreg[t][r] + VEC * u);
        }
    // 2. the B query rows of head h, rotated at their own positions; columns >= B are zero
    for (int i = tid; i < SH_COLS * HD; i += 256) {
        const int b = i / HD, d = i % HD;
        qs[b * QP + d] = b < B ? rope_elem<PREROT>(a, a.qkv + (long)b * a.ld + h * HD, d, a.kv_pos[b]) : 0.f;
    }
    __syncthreads();
    // 3. S^T = K.Q^T: s[t][r] = key 16 t + 4 g + r of column col.  One accumulator per 16 dims (four MFMA), the KU
    //    accumulators then added pairwise: one serial chain over all of hd carried partial sums of ~sqrt(hd) through
    //    hd / 4 roundings and put the scores' error past 4 x the f32 kernel's (whose dot is 8 fmaf + a lane tree);
    //    the independent chains also keep the matrix pipe full
    f32x4 sp[2][KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        const float4 q4 = *reinterpret_cast<const float4*>(qs + col * QP + 16 * u + 4 * g);
        const float qe[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            sp[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) sp[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kreg[t][u][e], qe[e], sp[t][u], 0, 0, 0);
        }
    }
#pragma unroll
    for (int st = 1; st < KU; st *= 2)
#pragma unroll
        for (int u = 0; u + st < KU; u += 2 * st)
#pragma unroll
            for (int t = 0; t < 2; ++t) sp[t][u] += sp[t][u + st];
    f32x4 s[2] = {sp[0][0], sp[1][0]};
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[t][r] = k0 + t * 16 + 4 * g + r < P ? s[t][r] * a.scale : -INFINITY;
            mx = fmaxf(mx, s[t][r]);
        }
    mx = col_max(mx);
    if (g == 0) red_m[wave * SH_COLS + col] = mx;
    __syncthreads();
    // 4. softmax over the block's 128 keys (key 128 c < P is in every column: m is finite)
    const float m = fmaxf(fmaxf(red_m[col], red_m[SH_COLS + col]), fmaxf(red_m[2 * SH_COLS + col], red_m[3 * SH_COLS + col]));
    float lsum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[t][r] = expf(s[t][r] - m);
            lsum += s[t][r];
        }
    lsum = col_sum(lsum);
    if (g == 0) red_l[wave * SH_COLS + col] = lsum;
    // 5. O^T += V^T.P^T: instruction (t, r) takes keys 16 t + 4 g + r, P from the score accumulator
    f32x4 o[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < DT; ++j) o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vreg[t][r][j], s[t][r], o[j], 0, 0, 0);
    // o[VEC u + e][r] = O[col][dim VEC (4 g + r + 16 u) + e] over the wave's keys
#pragma unroll
    for (int u = 0; u < VU; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                o_s[(wave * SH_COLS + col) * OP + VEC * (4 * g + r + 16 * u) + e] = o[VEC * u + e][r];
    __syncthreads();
    // 6. the four waves in wave order -> one record per row
    for (int i = tid; i < B * HD; i += 256) {
        const int b = i / HD, d = i % HD;
        float t = o_s[b * OP + d];
#pragma unroll
        for (int w = 1; w < 4; ++w) t += o_s[(w * SH_COLS + b) * OP + d];
        rec_of<HD>(a, nrec, b, h, c)[SH_HDR + d] = t;
    }
    if (tid < B) {
        float* rec = rec_of<HD>(a, nrec, tid, h, c);
        rec[0] = fmaxf(fmaxf(red_m[tid], red_m[SH_COLS + tid]), fmaxf(red_m[2 * SH_COLS + tid], red_m[3 * SH_COLS + tid]));
        rec[1] = (red_l[tid] + red_l[SH_COLS + tid]) + (red_l[2 * SH_COLS + tid] + red_l[3 * SH_COLS + tid]);
    }
}

// ---------------------------------------------------------------- own block: chunk c of [P, max_len), head h, row b
template <int HD, bool PREROT>
__device__ __forceinline__ void own_block(const DecAttnSharedArgs& a, float* lds, int nrec, int nsc, int c, int h, int b) {
    constexpr int CH = SH_CH;
    constexpr int LPK = HD / 8, KPI = 64 / LPK, NI = 32 / KPI;
    float* qs = lds;            // [HD]
    float* knew = qs + HD;      // [HD]
    float* vnew = knew + HD;    // [HD]
    float* p_s = vnew + HD;     // [CH]
    float* red = p_s + CH;      // [8]
    float* o_s = red + 8;       // [256 / LPK][HD] = 2048
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pos = a.kv_pos[b];
    const int k0 = a.shared_len + c * CH;
    if (k0 > pos) return;
    const int len = pos + 1;
    const int gq = a.heads / a.kv_heads, kvh = h / gq;
    const long cbase = (long)b * a.page_stride + (long)kvh * a.head_stride;
    float* Kc = a.kc + cbase;
    float* Vc = a.vc + cbase;
    const int sub = lane % LPK, kslot = lane / LPK;
    auto key_of = [&](int i) { return wave * 32 + i * KPI + kslot; };
    // 1. the chunk's K / V loads (keys clamped to the position: keys at and past it are masked at use)
    const int klim = min(k0 + CH, len) - 1;
    float4 kreg[NI][2], vreg[NI][2];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const float* p = Kc + (long)min(k0 + key_of(i), klim) * HD + sub * 8;
        kreg[i][0] = ldg_nt_f4(p);
        kreg[i][1] = ldg_nt_f4(p + 4);
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const float* p = Vc + (long)min(k0 + key_of(i), klim) * HD + sub * 8;
        vreg[i][0] = ldg_nt_f4(p);
        vreg[i][1] = ldg_nt_f4(p + 4);
    }
    const bool own = pos < k0 + CH;
    // 2. rotated q (and the new k, v in the owning chunk)
    const float* row = a.qkv + (long)b * a.ld;
    if (tid < HD) {
        qs[tid] = rope_elem<PREROT>(a, row + h * HD, tid, pos);
        if (own) {
            knew[tid] = rope_elem<PREROT>(a, row + (a.heads + kvh) * HD, tid, pos);
            vnew[tid] = row[(a.heads + a.kv_heads + kvh) * HD + tid];
        }
    }
    __syncthreads();
    // append: one writer per kv head (the attention below uses the LDS rows)
    if (own && h == kvh * gq && tid < HD) {
        Kc[(long)pos * HD + tid] = knew[tid];
        Vc[(long)pos * HD + tid] = vnew[tid];
    }
    const int kn = min(CH, len - k0);
    // 3. scores: eight fmaf per key and lane, then the transposing butterfly inside the key's LPK lanes: after it
    //    lane l holds key i = (l % LPK) >> 1 summed over all of the key's lanes
    float q8[8], kn8[8];
    ld_x8(qs + sub * 8, q8);
    ld_x8(knew + sub * 8, kn8);
    float v[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const float kf[8] = {kreg[i][0].x, kreg[i][0].y, kreg[i][0].z, kreg[i][0].w,
                             kreg[i][1].x, kreg[i][1].y, kreg[i][1].z, kreg[i][1].w};
        const bool mine = k0 + key_of(i) == pos;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(q8[j], mine ? kn8[j] : kf[j], acc);
        v[i] = acc;
    }
    if constexpr (NI >= 8) bfly<DPP_ROW_ROR8, 8, 8>(v, lane);
    if constexpr (NI >= 4) bfly<DPP_ROW_HALF_MIRROR, 4, 4>(v, lane);
    bfly<DPP_QUAD_XOR2, 2, 2>(v, lane);
    const float r = v[0] + dpp_f<DPP_QUAD_XOR1>(0.f, v[0]);
    {
        const int kk = key_of(sub >> 1);
        const float sc = kk < kn ? r * a.scale : -INFINITY;
        if ((sub & 1) == 0) p_s[kk] = sc;
        const float mw = wave_max(sc);
        if (lane == 0) red[wave] = mw;
    }
    __syncthreads();
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (wave < 2) {  // whole waves active for the DPP reduction
        const float p = tid < kn ? expf(p_s[tid] - m) : 0.f;
        p_s[tid] = p;
        const float l = wave_sum(p);
        if (lane == 0) red[4 + wave] = l;
    }
    __syncthreads();
    // 4. P.V over this lane's NI keys (same lane <-> (key, dims) map as K)
    float vn8[8];
    ld_x8(vnew + sub * 8, vn8);
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int key = key_of(i);
        const float vf[8] = {vreg[i][0].x, vreg[i][0].y, vreg[i][0].z, vreg[i][0].w,
                             vreg[i][1].x, vreg[i][1].y, vreg[i][1].z, vreg[i][1].w};
        const bool mine = k0 + key == pos, past = key >= kn;
        const float p = p_s[key];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = past ? 0.f : (mine ? vn8[j] : vf[j]);  // never 0 * (stale cache bits)
            o[j] = fmaf(p, x, o[j]);
        }
    }
    *reinterpret_cast<float4*>(o_s + tid * 8) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(o_s + tid * 8 + 4) = make_float4(o[4], o[5], o[6], o[7]);
    __syncthreads();
    float* rec = rec_of<HD>(a, nrec, b, h, nsc + c);
    if (tid < HD) {
        float t = o_s[tid];
#pragma unroll 8
        for (int gI = 1; gI < 2048 / HD; ++gI) t += o_s[gI * HD + tid];
        rec[SH_HDR + tid] = t;
    }
    if (tid == 0) {
        rec[0] = m;
        rec[1] = red[4] + red[5];
    }
}

constexpr int shared_lds_floats(int hd) {
    const int sh = SH_COLS * (hd + 4) + 8 * SH_COLS + 4 * SH_COLS * (hd + 1);
    const int own = 3 * hd + SH_CH + 8 + 2048;
    return sh > own ? sh : own;
}
}  // namespace

template <int HD, bool PREROT>
__global__ __launch_bounds__(256) void dec_attn_shared_kernel(DecAttnSharedArgs a) {
    static_assert(HD == 128 || HD == 64 || HD == 32, "unsupported head_dim");
    __shared__ __attribute__((aligned(16))) float lds[shared_lds_floats(HD)];
    const int nsc = (a.shared_len + SH_CH - 1) / SH_CH, noc = (a.max_len - a.shared_len + SH_CH - 1) / SH_CH;
    const int x = blockIdx.x, h = blockIdx.y;
    if (x < nsc) shared_block<HD, PREROT>(a, lds, nsc + noc, x, h);
    else own_block<HD, PREROT>(a, lds, nsc + noc, nsc, (x - nsc) % noc, h, (x - nsc) / noc);
}

// thread (row, head, d): the query's records in key order - the shared chunks, then its own chunks up to kv_pos
template <int HD>
__global__ __launch_bounds__(HD) void dec_attn_shared_merge_kernel(DecAttnSharedArgs a) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const int nsc = (a.shared_len + SH_CH - 1) / SH_CH, noc = (a.max_len - a.shared_len + SH_CH - 1) / SH_CH;
    const int n = nsc + (a.kv_pos[b] - a.shared_len) / SH_CH + 1;
    // attn_rec_combine's sums with expf for its __expf, as the decode merges of dec_attn / dec_attn_kv16: the fast
    // form scales its argument in f32, about |m_i - m| 2^-24 relative error in a record's weight, which is the size of
    // the whole error budget here.  Every record saw at least one key, so every m_i is finite.
    const float* rec0 = rec_of<HD>(a, nsc + noc, b, h, 0);
    constexpr int PR = HD + SH_HDR;
    float m = -INFINITY;
    for (int i = 0; i < n; ++i) m = fmaxf(m, rec0[i * PR]);
    float l = 0.f, acc = 0.f;
    for (int i = 0; i < n; ++i) {
        const float w = expf(rec0[i * PR] - m);
        l += rec0[i * PR + 1] * w;
        acc += rec0[i * PR + SH_HDR + d] * w;
    }
    a.o[(long)b * a.o_ld + (long)h * HD + d] = acc / l;
}

bool dec_attn_shared_ok(const DecAttnSharedArgs& a) {
    return (a.hd == 128 || a.hd == 64 || a.hd == 32) && a.kv_heads > 0 && a.heads % a.kv_heads == 0 && a.B >= 1 &&
           a.B <= SH_COLS && a.shared_len >= 1 && a.shared_len < a.max_len && a.max_len <= 512 * SH_CH &&
           a.rope_dim <= a.hd && a.rope_dim % 2 == 0 && (!a.prerot || a.rope_dim == a.hd);
}

size_t dec_attn_shared_workspace(int B, int heads, int hd, int max_len, int shared_len) {
    const size_t nrec = (size_t)(shared_len + SH_CH - 1) / SH_CH + (size_t)(max_len - shared_len + SH_CH - 1) / SH_CH;
    return sizeof(float) * nrec * heads * B * (hd + SH_HDR);
}

void launch_dec_attn_shared(const DecAttnSharedArgs& a, hipStream_t s) {
    if (!dec_attn_shared_ok(a))
        throw std::runtime_error("EINVAL: shared-prompt decode attention: head_dim 32 / 64 / 128, heads a multiple of "
                                 "kv_heads, 1..16 rows, 1 <= shared_len < max_len <= 65536");
    if (!a.part || !a.kc || !a.vc) throw std::runtime_error("EINTERNAL: dec_attn_shared needs the cache and a record buffer");
    const int nsc = (a.shared_len + SH_CH - 1) / SH_CH, noc = (a.max_len - a.shared_len + SH_CH - 1) / SH_CH;
    const dim3 g1(nsc + noc * a.B, a.heads), g2(a.heads, a.B);
    const bool prerot = a.prerot != 0;
    with_rows<128, 64, 32>(a.hd, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        if (prerot) DSOCR_LAUNCH((dec_attn_shared_kernel<HD, true>), g1, dim3(256), 0, s, a);
        else DSOCR_LAUNCH((dec_attn_shared_kernel<HD, false>), g1, dim3(256), 0, s, a);
        DSOCR_LAUNCH((dec_attn_shared_merge_kernel<HD>), g2, dim3(HD), 0, s, a);
    });
}

}  // namespace dsocr
