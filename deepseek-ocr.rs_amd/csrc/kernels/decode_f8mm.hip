// FP8 (E4M3) expert weights on the matrix cores for decode steps of 3..8 tokens (DSOCR_LOAD_FP8_EXPERTS_MM; the
// kernels take T = 1..8).  Contract: DESIGN.md sections 4.4.3 / 4.4.4 — W8[r][k] = 2^e_r * e4m3(code[r][k]); the
// codes are widened to f16 (exact: every E4M3 value is an f16 normal) straight into the A operand of
// v_mfma_f32_16x16x32_f16, the f32 token rows are the B operand as three f16 planes behind a power-of-two row scale
// (mm_planes.hpp, as decode_mm.hip), so every product is exact in the f32 accumulator; 2^e_r and the token's inverse
// plane scale multiply the C tile once each in the epilogue.  Sums are in a fixed order: no float atomics.
//
// Layout (fp8_tile_order): a second copy of each code table as [N/16 tiles][K/64 steps][64 lanes][16 B].  Lane
// l = (r = l & 15, g = l >> 4) of block (n, s) holds row 16n + r's codes k = 64s + 8g .. +7 in bytes 0..7 and
// k = 64s + 32 + 8g .. +7 in bytes 8..15: one wave-wide nontemporal dwordx4 is one contiguous 1 KiB block of 16 rows
// x 64 k, and it feeds two MFMA k-steps, half h of the lane's bytes being the A fragment of k-step 2s + h in
// decode_mm.hip's k order.  The B fragment of that step is then plane row l & 7, elements 32 (2s + h) + 8g .. +7: the
// 16-byte-per-g read mm_pitch was chosen for (conflict-free; a lane holding 16 consecutive k would read at 32-byte
// steps per g, which no linear pitch serves without a two-way conflict: DESIGN.md 4.4.4).
//
// Kernels:
//   fp8_tile_order        the relayout (rows past the table's end become zero codes)
//   moe_gateup_f8mm       units of 16 intermediate rows (shared expert first, then (record, tile)); KS waves split a
//                         unit's K and meet in LDS in piece order; persistent grid, token planes staged once a block
//   moe_down_f8mm         block = 64 output rows (16 per wave) x a contiguous group of segments (records, then the
//                         shared expert in pieces of I columns); G groups meet through a workspace, summed in group
//                         order by the block that completes the row tile's ticket
//   fp8_mm_rows_dot       parity hook: y[T][rows] = x . W8^T through the same blocks, converts, planes and scales
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "decode_common.hpp"
#include "mm_codes.hpp"

namespace dsocr {

namespace {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef MmT<f16_t>::frag frag;


// eight E4M3 codes (two dwords) -> the f16 A fragment: v_cvt_scalef32_pk_f16_fp8, scale 1.0, low / high word
__device__ __forceinline__ frag f8_frag(uint32_t w0, uint32_t w1) {
    const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w0, 1.0f, false);
    const f16x2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w0, 1.0f, true);
    const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w1, 1.0f, false);
    const f16x2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w1, 1.0f, true);
    return frag{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}

// One 1 KiB block of each of NM matrices (the same k range) against the planes: bb = the lane's plane-0 fragment
// pointer at the block's first k (row l & 7, + 8g).  The B fragments are read once for all NM matrices.
template <int NM>
__device__ __forceinline__ void f8mm_block(const uint4 (&q)[NM], const uint16_t* bb, int KP, f32x4 (&acc)[NM]) {
    frag a0[NM], a1[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        a0[m] = f8_frag(q[m].x, q[m].y);
        a1[m] = f8_frag(q[m].z, q[m].w);
    }
#pragma unroll
    for (int p = 2; p >= 0; --p) {
        const frag b0 = *reinterpret_cast<const frag*>(bb + (long)p * MM_MT * KP);
        const frag b1 = *reinterpret_cast<const frag*>(bb + (long)p * MM_MT * KP + 32);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            acc[m] = MmT<f16_t>::mfma(a0[m], b0, acc[m]);
            acc[m] = MmT<f16_t>::mfma(a1[m], b1, acc[m]);
        }
    }
}

// A wave's stream over n consecutive blocks of NM matrices (p[m]: the lane's granule of the first block), PF blocks of
// each per register batch, double-buffered.  start() issues the first batch (before the planes are staged), run()
// consumes the stream; n is wave-uniform.
template <int NM, int PF>
struct F8mmStream {
    uint4 qa[PF][NM], qb[PF][NM];
    const uint8_t* p[NM];
    int n;
    __device__ __forceinline__ void load(uint4 (&q)[PF][NM], int c) {
#pragma unroll
        for (int i = 0; i < PF; ++i)
            if (c + i < n)
#pragma unroll
                for (int m = 0; m < NM; ++m) q[i][m] = ldg_nt16(p[m] + (long)(c + i) * 1024);
    }
    __device__ __forceinline__ void start() { load(qa, 0); }
    __device__ __forceinline__ void compute(const uint4 (&q)[PF][NM], int c, const uint16_t* bb, int KP, f32x4 (&acc)[NM]) const {
#pragma unroll
        for (int i = 0; i < PF; ++i)
            if (c + i < n) f8mm_block<NM>(q[i], bb + 64 * (c + i), KP, acc);
    }
    __device__ __forceinline__ void run(const uint16_t* bb, int KP, f32x4 (&acc)[NM]) {
        for (int c = 0; c < n; c += 2 * PF) {
            if (c + PF < n) load(qb, c + PF);
            compute(qa, c, bb, KP, acc);
            if (c + PF >= n) break;
            if (c + 2 * PF < n) load(qa, c + 2 * PF);
            compute(qb, c + PF, bb, KP, acc);
        }
    }
};

// ------------------------------------------------------------------ the relayout
__global__ __launch_bounds__(256) void fp8_tile_order_kernel(long rows, int cols, const uint8_t* codes, uint8_t* out) {
    const int steps = cols >> 6;
    const long total = ((rows + 15) >> 4) * steps * 64;
    for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < total; f += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(f & 63);
        const long ts = f >> 6;
        const int s = (int)(ts % steps);
        const long r = ts / steps * 16 + (lane & 15);
        uint2 lo = make_uint2(0u, 0u), hi = make_uint2(0u, 0u);
        if (r < rows) {
            const uint8_t* src = codes + r * cols + 64 * s + 8 * (lane >> 4);
            lo = *reinterpret_cast<const uint2*>(src);
            hi = *reinterpret_cast<const uint2*>(src + 32);
        }
        *reinterpret_cast<uint4*>(out + f * 16) = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
}

// ------------------------------------------------------------------ y = x . W8^T (parity hook)
// One block per 16-row tile; its 4 waves split the K steps (the last wave takes the short piece) and meet in LDS.
__global__ __launch_bounds__(256) void fp8_mm_rows_dot_kernel(const uint8_t* tq, const int8_t* exps, long rows, int cols, int T,
                                                              const float* x, float* y) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xp[];  // [3][MT][KP]
    __shared__ float scl[MM_MT];
    __shared__ f32x4 red[3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int KP = mm_pitch(cols), steps = cols >> 6, per = (steps + 3) >> 2;
    const int s0 = min(wave * per, steps), s1 = min(s0 + per, steps);
    F8mmStream<1, 5> st;
    st.p[0] = tq + (((long)blockIdx.x * steps + s0) * 64 + lane) * 16;
    st.n = s1 - s0;
    st.start();
    for (int m = wave; m < T; m += 4) {
        MmRow r;
        mm_row_load<false>(r, x + (long)m * cols, cols, nullptr);
        mm_row_store<f16_t, false>(r, cols, 0.f, xp, KP, scl, m);
    }
    __syncthreads();
    f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    st.run(xp + (long)(col & 7) * KP + 8 * g + 64 * s0, KP, acc);
    if (wave > 0) red[wave - 1][lane] = acc[0];
    __syncthreads();
    if (wave == 0 && col < T) {
        f32x4 v = acc[0];
#pragma unroll
        for (int q = 0; q < 3; ++q) v += red[q][lane];
        const float sc = scl[col];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long r = (long)blockIdx.x * 16 + 4 * g + i;
            if (r < rows) y[(long)col * rows + r] = (v[i] * sc) * pow2i(exps[r]);
        }
    }
}

// ------------------------------------------------------------------ gate/up
constexpr int GU_REC = 18;  // the words of a router record the launch reads: expert, picks, 8 h rows, 8 weights

template <int KS>
__global__ __launch_bounds__(512, 4) void moe_gateup_f8mm_kernel(MoeF8Args a) {
    WaveSpan span_(a.span);
    constexpr int NU = 8 / KS, PF = 3;
    extern __shared__ __attribute__((aligned(16))) uint16_t xp[];  // [3][MT][KP], then the pieces' partial tiles
    __shared__ float scl[MM_MT];
    __shared__ int rec_s[64 * GU_REC];  // every record word the unit loop reads comes from LDS, not behind the stream
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4, piece = wave % KS, us = wave / KS;
    const int KP = mm_pitch(a.H);
    f32x4(*red)[2][64] = reinterpret_cast<f32x4(*)[2][64]>(xp + 3 * MM_MT * (long)KP);  // [NU (KS - 1)][gate, up][lane]
    if (wave < a.T) {
        MmRow xr;
        mm_row_load<false>(xr, a.x + (long)wave * a.H, a.H, nullptr);
        mm_row_store<f16_t, false>(xr, a.H, 0.f, xp, KP, scl, wave);
    }
    const int ng = min(min(a.grp[0], a.slots), 64);
    for (int i = tid; i < ng * GU_REC; i += 512) rec_s[i] = a.grp[MOE_GRP_REC * (1 + i / GU_REC) + i % GU_REC];
    __syncthreads();
    const int tiles_r = a.I >> 4, tiles_s = a.Is >> 4, n_units = tiles_s + ng * tiles_r;
    const int steps = a.H >> 6, per = steps / KS, s0 = piece * per;
    const uint16_t* bb = xp + (long)(col & 7) * KP + 8 * g + 64 * s0;
    for (int base = blockIdx.x * NU; base < n_units; base += gridDim.x * NU) {  // block-uniform
        const int unit = base + us;
        const bool valid = unit < n_units;  // wave-uniform
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        bool sh = true;
        int rs = 0, i0 = 0;
        uint32_t eg4 = 0, eu4 = 0;
        if (valid) {
            sh = unit < tiles_s;
            int t = unit;
            if (!sh) { rs = (unit - tiles_s) / tiles_r; t = (unit - tiles_s) % tiles_r; }
            i0 = 16 * t;
            const int rows_I = sh ? a.Is : a.I;
            const F8Mat& m = sh ? a.sWgu : a.Wgu;
            const long r0 = (sh ? 0L : (long)rec_s[rs * GU_REC] * 2 * a.I) + i0;  // the unit's first gate row
            if (piece == 0) {  // issued ahead of the stream: they retire first
                eg4 = *reinterpret_cast<const uint32_t*>(m.e + r0 + 4 * g);
                eu4 = *reinterpret_cast<const uint32_t*>(m.e + r0 + rows_I + 4 * g);
            }
            F8mmStream<2, PF> st;
            st.p[0] = m.t + (((r0 >> 4) * steps + s0) * 64 + lane) * 16;
            st.p[1] = st.p[0] + (long)(rows_I >> 4) * steps * 1024;
            st.n = per;
            st.start();
            st.run(bb, KP, acc);
        }
        if (KS > 1) {  // the pieces of a unit meet in LDS, summed in piece order by piece 0
            if (valid && piece > 0) {
                red[us * (KS - 1) + piece - 1][0][lane] = acc[0];
                red[us * (KS - 1) + piece - 1][1][lane] = acc[1];
            }
            __syncthreads();
            if (valid && piece == 0) {
#pragma unroll
                for (int q = 0; q < KS - 1; ++q) {
                    acc[0] += red[us * (KS - 1) + q][0][lane];
                    acc[1] += red[us * (KS - 1) + q][1][lane];
                }
            }
            __syncthreads();  // read before the next units' pieces land
        }
        if (valid && piece == 0) {
            // token col's slot row (routed: -1 when the token did not pick this expert) and routing weight
            int slot = -1;
            float wk = 1.f;
            if (sh) {
                slot = col < a.T ? col : -1;
            } else {
                const int* rec = rec_s + rs * GU_REC;
                const int cnt = min(rec[1], 8);
                for (int q = 0; q < cnt; ++q) {
                    const int r = rec[2 + q];
                    if (r / a.topk == col) { slot = r; wk = __int_as_float(rec[10 + q]); }
                }
            }
            if (slot >= 0) {
                const float sc = scl[col];
                float hv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float gs = (acc[0][i] * sc) * pow2b(eg4, i), uv = (acc[1][i] * sc) * pow2b(eu4, i);
                    const float h = (gs / (1.0f + expf(-gs))) * uv;  // silu (candle: x / (1 + exp(-x)))
                    hv[i] = sh ? h : h * wk;
                }
                float* dst = sh ? a.hs + (long)slot * a.Is : a.h + (long)slot * a.I;
                *reinterpret_cast<float4*>(dst + i0 + 4 * g) = make_float4(hv[0], hv[1], hv[2], hv[3]);
            }
        }
    }
}

// ------------------------------------------------------------------ down + combine + residual
constexpr int DN_RT = MMC_DN_RT;  // output rows per block: 16 per wave

__global__ __launch_bounds__(256) void moe_down_f8mm_kernel(MoeF8Args a, int G) {
    WaveSpan span_(a.span);
    constexpr int U = 2, PF = 7;  // chunks of 8 floats per lane of a token column (I <= 1024); blocks per batch
    extern __shared__ __attribute__((aligned(16))) uint16_t xp[];  // [3][MT][KP]
    __shared__ float scl[MM_MT];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const int tiles = a.H / DN_RT, tile = blockIdx.x % tiles, gi = blockIdx.x / tiles;
    const int ng = min(a.grp[0], a.slots), np = a.Is > 0 ? (a.Is + a.I - 1) / a.I : 0, n_seg = ng + np;
    const int spg = (n_seg + G - 1) / G, sb = min(gi * spg, n_seg), se = min(sb + spg, n_seg);  // this group's segments
    const int j0 = tile * DN_RT + 16 * wave;
    const int KP = mm_pitch(a.I);
    const uint16_t* bb = xp + (long)(col & 7) * KP + 8 * g;
    f32x4 tot = {0.f, 0.f, 0.f, 0.f};
    for (int seg = sb; seg < se; ++seg) {  // block-uniform
        const bool shared = seg >= ng;
        const int* rec = a.grp + MOE_GRP_REC * (1 + (shared ? 0 : seg));
        const int c0 = shared ? (seg - ng) * a.I : 0, in_dim = shared ? min(a.I, a.Is - c0) : a.I;
        F8mmStream<1, PF> st;
        uint32_t e4;
        if (shared) {
            st.p[0] = a.sWd.t + (((long)(j0 >> 4) * (a.Is >> 6) + (c0 >> 6)) * 64 + lane) * 16;
            e4 = *reinterpret_cast<const uint32_t*>(a.sWd.e + j0 + 4 * g);
        } else {
            const long r0 = (long)rec[0] * a.H + j0;
            st.p[0] = a.Wd.t + ((r0 >> 4) * (a.I >> 6) * 64 + lane) * 16;
            e4 = *reinterpret_cast<const uint32_t*>(a.Wd.e + r0 + 4 * g);
        }
        st.n = in_dim >> 6;
        st.start();
        // wave w stages token columns w and w + 4: the h~ row of the token's pick of this expert (shared: the piece
        // of hs[t]), zeros when the token did not pick it
        for (int t = wave; t < MM_MT; t += 4) {
            const float* src = nullptr;
            if (t < a.T) {
                if (shared) {
                    src = a.hs + (long)t * a.Is + c0;
                } else {
                    const int cnt = min(rec[1], 8);
                    for (int q = 0; q < cnt; ++q)
                        if (rec[2 + q] / a.topk == t) src = a.h + (long)rec[2 + q] * a.I;
                }
            }
            MmRowU<U> xr;
            if (src) {
                mm_row_load<false, U>(xr, src, in_dim, nullptr);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < 8; ++j) xr.v[u][j] = 0.f;
            }
            mm_row_store<f16_t, false, U>(xr, in_dim, 0.f, xp, KP, scl, t);
        }
        __syncthreads();
        f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
        st.run(bb, KP, acc);
        const float sc = scl[col & 7];
#pragma unroll
        for (int i = 0; i < 4; ++i) tot[i] += (acc[0][i] * sc) * pow2b(e4, i);
        __syncthreads();  // the planes are restaged by the next segment
    }
    mmc_down_finish(tot, G, gi, tile, j0, a.T, a.H, a.out, a.dn_part, a.dn_tick, &last_s);
}


}  // namespace

// ------------------------------------------------------------------ host side
bool fp8_tile_ok(long cols) { return cols > 0 && cols % 64 == 0; }

size_t fp8_tile_bytes(long rows, long cols) { return (size_t)((rows + 15) / 16) * 16 * (size_t)cols; }

void launch_fp8_tile_order(long rows, long cols, const uint8_t* codes, uint8_t* out, hipStream_t s) {
    if (rows <= 0 || !fp8_tile_ok(cols) || cols > (1L << 30) || !codes || !out)
        throw std::runtime_error("EINVAL: fp8_tile_order takes rows of a multiple of 64 codes");
    const long granules = (rows + 15) / 16 * cols;  // 16 rows x cols / 16
    hipLaunchKernelGGL(fp8_tile_order_kernel, dim3((unsigned)std::min<long>((granules + 255) / 256, 4096)), dim3(256), 0, s, rows,
                       (int)cols, codes, out);
}

void launch_fp8_mm_rows_dot(const uint8_t* tiles, const int8_t* exps, long rows, long cols, int T, const float* x, float* y,
                            hipStream_t s) {
    if (rows <= 0 || !fp8_tile_ok(cols) || cols > 1536 || !tiles || !exps || !x || !y)
        throw std::runtime_error("EINVAL: fp8_mm_rows_dot takes rows of a multiple of 64 codes, at most 1536");
    if (T < 1 || T > MM_MT) throw std::runtime_error("EINVAL: fp8_mm_rows_dot takes 1..8 token rows");
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)fp8_mm_rows_dot_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        attr = true;
    }
    hipLaunchKernelGGL(fp8_mm_rows_dot_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), mmc_plane_bytes((int)cols), s, tiles, exps,
                       rows, (int)cols, T, x, y);
}

bool moe_f8mm_ok(const MoeF8Args& a) {
    if (!moe_f8_ok(a) || a.H % 64 || a.I % 64 || a.Is % 64 || a.H > 1536 || a.I > 1024) return false;
    if (!a.Wgu.t || !a.Wd.t || (a.Is > 0 && (!a.sWgu.t || !a.sWd.t))) return false;
    return (long)MM_MT * a.H * 4 * std::max(a.slots, 1) < (1L << 31);
}

void launch_moe_gateup_f8mm(const MoeF8Args& a, hipStream_t s) {
    if (!moe_f8mm_ok(a)) throw std::runtime_error("EINVAL: FP8 decode MoE (matrix cores) outside its range");
    const int steps = a.H / 64, ks = steps % 4 == 0 ? 4 : steps % 2 == 0 ? 2 : 1;
    const int max_units = a.Is / 16 + a.slots * (a.I / 16);
    const size_t lds = mmc_plane_bytes(a.H) + (ks > 1 ? (size_t)(8 / ks) * (ks - 1) * 2 * 64 * sizeof(f32x4) : 0);
#define DSOCR_GF(KS)                                                                                                    \
    do {                                                                                                                \
        static int resident = 0;                                                                                        \
        if (!resident) {                                                                                                \
            (void)hipFuncSetAttribute((const void*)moe_gateup_f8mm_kernel<KS>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                      96 * 1024);                                                                       \
            resident = mmc_resident_blocks((const void*)moe_gateup_f8mm_kernel<KS>, 512, lds);                               \
        }                                                                                                               \
        const int nu = 8 / KS, blocks = std::max(1, std::min(resident, (max_units + nu - 1) / nu));                      \
        DSOCR_LAUNCH(moe_gateup_f8mm_kernel<KS>, dim3(blocks), dim3(512), lds, s, a);                                    \
    } while (0)
    if (ks == 4) DSOCR_GF(4);
    else if (ks == 2) DSOCR_GF(2);
    else DSOCR_GF(1);
#undef DSOCR_GF
}

int moe_down_f8mm_groups(const MoeF8Args& a) { return mmc_down_groups(a); }

void launch_moe_down_f8mm(const MoeF8Args& a, hipStream_t s) {
    if (!moe_f8mm_ok(a)) throw std::runtime_error("EINVAL: FP8 decode MoE (matrix cores) outside its range");
    const int G = moe_down_f8mm_groups(a);
    DSOCR_LAUNCH(moe_down_f8mm_kernel, dim3((unsigned)(G * (a.H / DN_RT))), dim3(256), mmc_plane_bytes(a.I), s, a, G);
}

}  // namespace dsocr
