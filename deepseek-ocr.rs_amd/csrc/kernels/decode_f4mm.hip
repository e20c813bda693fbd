// MXFP4 expert weights on the matrix cores for decode steps of 1..8 tokens (DSOCR_LOAD_MXFP4_EXPERTS).  Contract:
// DESIGN.md section 4.4.5 — per output row r one exponent e_r, per block of 32 consecutive k one down-shift d_b
// (0..12) and per weight one OCP E2M1 code: W4[r][k] = 2^(e_r - d_b) e2m1(code[r][k]), an fp16 value by construction.
// One v_cvt_scalef32_pk_f16_fp4 per two weights widens a byte of codes to f16 with 2^-d_b in its scale operand (the
// result is e2m1 2^-d_b >= 2^-13: an f16 normal), four of them fill the A operand of v_mfma_f32_16x16x32_f16; the f32
// token rows are the B operand as three f16 planes behind a power-of-two row scale (mm_planes.hpp), so every product
// is exact in the f32 accumulator; 2^e_r and the token's inverse plane scale multiply the C tile once each in the
// epilogue.  Sums are in a fixed order: no float atomics.
//
// Layout (mxfp4_tile_order).  Codes: [N/16 tiles][K/128 blocks][64 lanes][16 B]: lane l = (r = l & 15, g = l >> 4) of
// block (n, s) holds in dword j the eight codes k = 128 s + 32 j + 8 g .. +7 of row 16 n + r (low nibble = even k), so
// one wave-wide nontemporal dwordx4 is one contiguous 1 KiB = 16 rows x 128 k = four MFMA k-steps, dword j being the
// A fragment of k-step 4 s + j in decode_mm.hip's k order; the B fragment of that step is plane row l & 7, elements
// 32 (4 s + j) + 8 g .. +7 (the conflict-free 16-byte-per-g read of DESIGN.md 4.4.4).  Shifts: a plane
// [N/16][K/128][16 rows][4 B]: a k-step is one 32-block, so the lane's four shift bytes of a 1 KiB block are one dword
// (64 B per block beside the 1 KiB of codes; the four lanes of a row read the same dword).  Exponents: int8 [N].
//
// Kernels:
//   mxfp4_quantize_rows   load time, one wave per row, four lanes per 32-block: block exponents from the float's
//                         exponent and significand, the row's largest, the shifts, the codes by comparison against
//                         the seven midpoints of the E2M1 grid (ties to the even code)
//   mxfp4_dequant_rows    load time: W4 written over the fp16 rows (prefill and batches above 8 stream it)
//   mxfp4_tile_order      the relayout of codes and shifts (rows past the table's end: zero codes)
//   moe_gateup_f4mm       units of 16 intermediate rows (shared expert first, then (record, tile)); KS waves split a
//                         unit's K and meet in LDS in piece order; persistent grid, token planes staged once a block
//   moe_down_f4mm         block = 64 output rows (16 per wave) x a contiguous group of segments (records, then the
//                         shared expert in pieces of I columns); G groups meet through a workspace, summed in group
//                         order by the block that completes the row tile's ticket
//   mxfp4_mm_rows_dot     parity hook: y[T][rows] = x . W4^T through the same blocks, converts, planes and scales
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

constexpr int F4_DMAX = 12;   // largest block down-shift
constexpr int F4_EMIN = -11;  // smallest row exponent: the smallest non-zero W4 is 2^(-11 - 12) 0.5 = 2^-24

// 2^-d for shift byte i of a dword
__device__ __forceinline__ float shiftb(uint32_t d4, int i) { return pow2i(-(int)((d4 >> (8 * i)) & 0xffu)); }

// the E2M1 value of code magnitude c (0..7): 0, 1/2, 1, 3/2, 2, 3, 4, 6
__device__ __forceinline__ float e2m1_mag(int c) { return c < 2 ? 0.5f * (float)c : pow2i((c >> 1) - 1) * (1.0f + 0.5f * (float)(c & 1)); }

// eight E2M1 codes (one dword) -> the f16 A fragment e2m1 * sc: v_cvt_scalef32_pk_f16_fp4, byte select 0..3
__device__ __forceinline__ frag f4_frag(uint32_t w, float sc) {
    const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 0);
    const f16x2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 1);
    const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 2);
    const f16x2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 3);
    return frag{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}

// One 1 KiB block (four k-steps) of each of NM matrices (the same k range) against the planes: bb = the lane's plane-0
// fragment pointer at the block's first k (row l & 7, + 8 g).  Step-major: the NM fragments of a step live only over
// its three plane reads, and the B fragments are read once for all NM matrices.
template <int NM>
__device__ __forceinline__ void f4mm_block(const uint4 (&q)[NM], const uint32_t (&d)[NM], const uint16_t* bb, int KP,
                                           f32x4 (&acc)[NM]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        frag a[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const uint32_t w = j == 0 ? q[m].x : j == 1 ? q[m].y : j == 2 ? q[m].z : q[m].w;
            a[m] = f4_frag(w, shiftb(d[m], j));
        }
#pragma unroll
        for (int p = 2; p >= 0; --p) {
            const frag b = *reinterpret_cast<const frag*>(bb + (long)p * MM_MT * KP + 32 * j);
#pragma unroll
            for (int m = 0; m < NM; ++m) acc[m] = MmT<f16_t>::mfma(a[m], b, acc[m]);
        }
    }
}

// A wave's stream over n consecutive blocks of NM matrices (p[m]: the lane's code granule of the first block, ps[m]:
// its shift dword), PF blocks of each per register batch, double-buffered: 5 VGPRs per block in flight.  start()
// issues the first batch (before the planes are staged), run() consumes the stream; n is wave-uniform.
template <int NM, int PF>
struct F4mmStream {
    uint4 qa[PF][NM], qb[PF][NM];
    uint32_t da[PF][NM], db[PF][NM];
    const uint8_t* p[NM];
    const uint8_t* ps[NM];
    int n;
    __device__ __forceinline__ void load(uint4 (&q)[PF][NM], uint32_t (&d)[PF][NM], int c) {
#pragma unroll
        for (int i = 0; i < PF; ++i)
            if (c + i < n)
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    q[i][m] = ldg_nt16(p[m] + (long)(c + i) * 1024);
                    d[i][m] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ps[m] + (long)(c + i) * 64));
                }
    }
    __device__ __forceinline__ void start() { load(qa, da, 0); }
    __device__ __forceinline__ void compute(const uint4 (&q)[PF][NM], const uint32_t (&d)[PF][NM], int c, const uint16_t* bb,
                                            int KP, f32x4 (&acc)[NM]) const {
#pragma unroll
        for (int i = 0; i < PF; ++i)
            if (c + i < n) f4mm_block<NM>(q[i], d[i], bb + 128 * (c + i), KP, acc);
    }
    __device__ __forceinline__ void run(const uint16_t* bb, int KP, f32x4 (&acc)[NM]) {
        for (int c = 0; c < n; c += 2 * PF) {
            if (c + PF < n) load(qb, db, c + PF);
            compute(qa, da, c, bb, KP, acc);
            if (c + PF >= n) break;
            if (c + 2 * PF < n) load(qa, da, c + 2 * PF);
            compute(qb, db, c + PF, bb, KP, acc);
        }
    }
};

// ------------------------------------------------------------------ load-time quantiser
// smallest e with amax 2^-e <= 6 (= 1.5 * 2^2): amax = m 2^ex, m in [1, 2) -> ex - 2 + [m > 1.5]
__device__ __forceinline__ int block_exponent(float amax) {
    const uint32_t b = __float_as_uint(amax);  // (an fp16 value widened: always a normal f32)
    return (int)(b >> 23) - 127 - 2 + ((b & 0x7fffffu) > 0x400000u ? 1 : 0);
}

// the code of v (already scaled onto the grid, |v| <= 6): nearest grid value, ties to the even code; sign = v's
__device__ __forceinline__ int e2m1_code(float v) {
    const float a = fabsf(v);
    const int c = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
    return c | ((__float_as_uint(v) >> 31) << 3);
}

constexpr int F4_NOBLK = -1000;  // block exponent of an all-zero block

// One wave per row; lane l owns the 8 weights of chunk c = l, l + 64, ...; the four lanes of a quad own one 32-block.
__global__ __launch_bounds__(256) void mxfp4_quantize_rows_kernel(long rows, int cols, const uint16_t* w, uint8_t* codes,
                                                                   uint8_t* shifts, int8_t* exps) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;  // wave-uniform
    const uint16_t* wr = w + r * cols;
    const int chunks = cols >> 3;  // a multiple of 4: the loops below are quad-uniform
    auto block_amax = [&](int c, float* v) {
        unpack8<f16_t>(*reinterpret_cast<const uint4*>(wr + 8 * c), v);
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
        m = fmaxf(m, __shfl_xor(m, 1));
        return fmaxf(m, __shfl_xor(m, 2));
    };
    float v[8];
    int er = F4_NOBLK;
    for (int c = lane; c < chunks; c += 64) {
        const float am = block_amax(c, v);
        if (am > 0.f) er = max(er, block_exponent(am));
    }
    er = (int)wave_max((float)er);
    er = er == F4_NOBLK ? 0 : max(er, F4_EMIN);
    for (int c = lane; c < chunks; c += 64) {
        const float am = block_amax(c, v);
        const int d = am > 0.f ? min(er - block_exponent(am), F4_DMAX) : F4_DMAX;
        const int s = er - d;  // the block's scale 2^s: -23 <= s <= 14
        const float inv = pow2i(-s);
        uint32_t q = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int code = e2m1_code(v[j] * inv);  // exact scaling: the comparison is the only rounding
            // top of the range: a code whose value is past the largest fp16 takes the next code down (4 2^14 -> 3 2^14)
            if (e2m1_mag(code & 7) * pow2i(s) > 65504.f) --code;
            q |= (uint32_t)code << (4 * j);
        }
        *reinterpret_cast<uint32_t*>(codes + r * (cols >> 1) + 4 * c) = q;
        if ((lane & 3) == 0) shifts[r * (cols >> 5) + (c >> 2)] = (uint8_t)d;
    }
    if (lane == 0) exps[r] = (int8_t)er;
}

// W4 as fp16 (exact) from the row-major codes and shifts
__global__ __launch_bounds__(256) void mxfp4_dequant_rows_kernel(long rows, int cols, const uint8_t* codes, const uint8_t* shifts,
                                                                  const int8_t* exps, uint16_t* out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int er = exps[r];
    for (int c = lane; c < (cols >> 3); c += 64) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(codes + r * (cols >> 1) + 4 * c);
        const float sc = pow2i(er - (int)shifts[r * (cols >> 5) + (c >> 2)]);
        uint32_t h[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int code = (q >> (4 * j)) & 15;
            const float mag = e2m1_mag(code & 7) * sc;
            const _Float16 f = (_Float16)((code & 8) ? -mag : mag);
            uint16_t b;
            __builtin_memcpy(&b, &f, 2);
            h[j >> 1] = (j & 1) ? (h[j >> 1] | ((uint32_t)b << 16)) : (uint32_t)b;
        }
        *reinterpret_cast<uint4*>(out + r * cols + 8 * c) = make_uint4(h[0], h[1], h[2], h[3]);
    }
}

// ------------------------------------------------------------------ the relayout
__global__ __launch_bounds__(256) void mxfp4_tile_order_kernel(long rows, int cols, const uint8_t* codes, const uint8_t* shifts,
                                                                uint8_t* tq, uint8_t* td) {
    const int steps = cols >> 7;
    const long total = ((rows + 15) >> 4) * steps * 64;
    for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < total; f += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(f & 63), g = lane >> 4;
        const long ts = f >> 6;
        const int s = (int)(ts % steps);
        const long r = ts / steps * 16 + (lane & 15);
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        uint32_t d4 = 0x0c0c0c0cu;
        if (r < rows) {
            const uint8_t* src = codes + r * (cols >> 1) + 64 * s + 4 * g;  // k = 128 s + 32 j + 8 g at two codes a byte
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = *reinterpret_cast<const uint32_t*>(src + 16 * j);
            d4 = *reinterpret_cast<const uint32_t*>(shifts + r * (cols >> 5) + 4 * s);
        }
        *reinterpret_cast<uint4*>(tq + f * 16) = make_uint4(q[0], q[1], q[2], q[3]);
        if (g == 0) *reinterpret_cast<uint32_t*>(td + (ts * 16 + (lane & 15)) * 4) = d4;
    }
}

// ------------------------------------------------------------------ y = x . W4^T (parity hook)
// One block per 16-row tile; its 4 waves split the K blocks (the last waves take the short pieces) and meet in LDS.
__global__ __launch_bounds__(256) void mxfp4_mm_rows_dot_kernel(F4Mat m, long rows, int cols, int T, const float* x, float* y) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xp[];  // [3][MT][KP]
    __shared__ float scl[MM_MT];
    __shared__ f32x4 red[3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int KP = mm_pitch(cols), steps = cols >> 7, per = (steps + 3) >> 2;
    const int s0 = min(wave * per, steps), s1 = min(s0 + per, steps);
    F4mmStream<1, 3> st;
    st.p[0] = m.q + (((long)blockIdx.x * steps + s0) * 64 + lane) * 16;
    st.ps[0] = m.d + (((long)blockIdx.x * steps + s0) * 16 + col) * 4;
    st.n = s1 - s0;
    st.start();
    for (int t = wave; t < T; t += 4) {
        MmRow r;
        mm_row_load<false>(r, x + (long)t * cols, cols, nullptr);
        mm_row_store<f16_t, false>(r, cols, 0.f, xp, KP, scl, t);
    }
    __syncthreads();
    f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    st.run(xp + (long)(col & 7) * KP + 8 * g + 128 * s0, KP, acc);
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
            if (r < rows) y[(long)col * rows + r] = (v[i] * sc) * pow2i(m.e[r]);
        }
    }
}

// ------------------------------------------------------------------ gate/up
constexpr int GU_REC = 18;  // the words of a router record the launch reads: expert, picks, 8 h rows, 8 weights

template <int KS>
__global__ __launch_bounds__(512, 4) void moe_gateup_f4mm_kernel(MoeF4Args a) {
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
    const int steps = a.H >> 7, per = steps / KS, s0 = piece * per;
    const uint16_t* bb = xp + (long)(col & 7) * KP + 8 * g + 128 * s0;
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
            const F4Mat& m = sh ? a.sWgu : a.Wgu;
            const long r0 = (sh ? 0L : (long)rec_s[rs * GU_REC] * 2 * a.I) + i0;  // the unit's first gate row
            if (piece == 0) {  // issued ahead of the stream: they retire first
                eg4 = *reinterpret_cast<const uint32_t*>(m.e + r0 + 4 * g);
                eu4 = *reinterpret_cast<const uint32_t*>(m.e + r0 + rows_I + 4 * g);
            }
            const long blk = (r0 >> 4) * steps + s0, up = (long)(rows_I >> 4) * steps;  // 1 KiB blocks: first gate, gate -> up
            F4mmStream<2, PF> st;
            st.p[0] = m.q + (blk * 64 + lane) * 16;
            st.p[1] = st.p[0] + up * 1024;
            st.ps[0] = m.d + (blk * 16 + col) * 4;
            st.ps[1] = st.ps[0] + up * 64;
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

__global__ __launch_bounds__(256) void moe_down_f4mm_kernel(MoeF4Args a, int G) {
    WaveSpan span_(a.span);
    constexpr int U = 2, PF = 4;  // chunks of 8 floats per lane of a token column (I <= 1024); blocks per batch (8 = I 1024)
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
        F4mmStream<1, PF> st;
        uint32_t e4;
        if (shared) {
            const long blk = (long)(j0 >> 4) * (a.Is >> 7) + (c0 >> 7);
            st.p[0] = a.sWd.q + (blk * 64 + lane) * 16;
            st.ps[0] = a.sWd.d + (blk * 16 + col) * 4;
            e4 = *reinterpret_cast<const uint32_t*>(a.sWd.e + j0 + 4 * g);
        } else {
            const long r0 = (long)rec[0] * a.H + j0, blk = (r0 >> 4) * (a.I >> 7);
            st.p[0] = a.Wd.q + (blk * 64 + lane) * 16;
            st.ps[0] = a.Wd.d + (blk * 16 + col) * 4;
            e4 = *reinterpret_cast<const uint32_t*>(a.Wd.e + r0 + 4 * g);
        }
        st.n = in_dim >> 7;
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


long tile_rows(long rows) { return (rows + 15) / 16 * 16; }

}  // namespace

// ------------------------------------------------------------------ host side
bool mxfp4_rows_ok(long cols) { return cols > 0 && cols % 32 == 0 && cols <= (1L << 30); }
bool mxfp4_tile_ok(long cols) { return cols > 0 && cols % 128 == 0 && cols <= (1L << 30); }

size_t mxfp4_tile_code_bytes(long rows, long cols) { return (size_t)tile_rows(rows) * (size_t)cols / 2; }
size_t mxfp4_tile_shift_bytes(long rows, long cols) { return (size_t)tile_rows(rows) * (size_t)cols / 32; }

void launch_mxfp4_quantize_rows(long rows, long cols, const void* w_f16, uint8_t* codes, uint8_t* shifts, int8_t* exps,
                                hipStream_t s) {
    if (rows <= 0 || !mxfp4_rows_ok(cols) || !w_f16 || !codes || !shifts || !exps)
        throw std::runtime_error("EINVAL: mxfp4_quantize_rows takes rows of a multiple of 32 fp16 values");
    hipLaunchKernelGGL(mxfp4_quantize_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rows, (int)cols,
                       reinterpret_cast<const uint16_t*>(w_f16), codes, shifts, exps);
}

void launch_mxfp4_dequant_rows(long rows, long cols, const uint8_t* codes, const uint8_t* shifts, const int8_t* exps, void* w4_f16,
                               hipStream_t s) {
    if (rows <= 0 || !mxfp4_rows_ok(cols) || !codes || !shifts || !exps || !w4_f16)
        throw std::runtime_error("EINVAL: mxfp4_dequant_rows takes rows of a multiple of 32 codes");
    hipLaunchKernelGGL(mxfp4_dequant_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rows, (int)cols, codes, shifts,
                       exps, reinterpret_cast<uint16_t*>(w4_f16));
}

void launch_mxfp4_tile_order(long rows, long cols, const uint8_t* codes, const uint8_t* shifts, uint8_t* tile_codes,
                             uint8_t* tile_shifts, hipStream_t s) {
    if (rows <= 0 || !mxfp4_tile_ok(cols) || !codes || !shifts || !tile_codes || !tile_shifts)
        throw std::runtime_error("EINVAL: mxfp4_tile_order takes rows of a multiple of 128 codes");
    const long granules = tile_rows(rows) * (cols / 32);  // 16 B each
    hipLaunchKernelGGL(mxfp4_tile_order_kernel, dim3((unsigned)std::min<long>((granules + 255) / 256, 4096)), dim3(256), 0, s, rows,
                       (int)cols, codes, shifts, tile_codes, tile_shifts);
}

void launch_mxfp4_mm_rows_dot(const F4Mat& m, long rows, long cols, int T, const float* x, float* y, hipStream_t s) {
    if (rows <= 0 || !mxfp4_tile_ok(cols) || cols > 1536 || !m.q || !m.d || !m.e || !x || !y)
        throw std::runtime_error("EINVAL: mxfp4_mm_rows_dot takes rows of a multiple of 128 codes, at most 1536");
    if (T < 1 || T > MM_MT) throw std::runtime_error("EINVAL: mxfp4_mm_rows_dot takes 1..8 token rows");
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)mxfp4_mm_rows_dot_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        attr = true;
    }
    hipLaunchKernelGGL(mxfp4_mm_rows_dot_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), mmc_plane_bytes((int)cols), s, m, rows,
                       (int)cols, T, x, y);
}

bool moe_f4mm_shape_ok(int E, int H, int I, int Is) {
    return E >= 1 && E <= 64 && H > 0 && I > 0 && Is >= 0 && H % 128 == 0 && I % 128 == 0 && Is % 128 == 0 && H <= 1536 && I <= 1024;
}

bool moe_f4mm_ok(const MoeF4Args& a) {
    if (a.T < 1 || a.T > MM_MT || a.topk < 1 || a.topk > 8 || a.T * a.topk > 64 || a.slots < 1) return false;
    if (!moe_f4mm_shape_ok(a.E, a.H, a.I, a.Is)) return false;
    if (!a.x || !a.h || !a.out || !a.grp || !a.Wgu.q || !a.Wgu.d || !a.Wgu.e || !a.Wd.q || !a.Wd.d || !a.Wd.e) return false;
    if (a.Is > 0 && (!a.hs || !a.sWgu.q || !a.sWgu.d || !a.sWgu.e || !a.sWd.q || !a.sWd.d || !a.sWd.e)) return false;
    return (long)MM_MT * a.H * 4 * std::max(a.slots, 1) < (1L << 31);
}

void launch_moe_gateup_f4mm(const MoeF4Args& a, hipStream_t s) {
    if (!moe_f4mm_ok(a)) throw std::runtime_error("EINVAL: MXFP4 decode MoE outside its range");
    const int steps = a.H / 128, ks = steps % 4 == 0 ? 4 : steps % 2 == 0 ? 2 : 1;
    const int max_units = a.Is / 16 + a.slots * (a.I / 16);
    const size_t lds = mmc_plane_bytes(a.H) + (ks > 1 ? (size_t)(8 / ks) * (ks - 1) * 2 * 64 * sizeof(f32x4) : 0);
#define DSOCR_GF(KS)                                                                                                    \
    do {                                                                                                                \
        static int resident = 0;                                                                                        \
        if (!resident) {                                                                                                \
            (void)hipFuncSetAttribute((const void*)moe_gateup_f4mm_kernel<KS>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                      96 * 1024);                                                                       \
            resident = mmc_resident_blocks((const void*)moe_gateup_f4mm_kernel<KS>, 512, lds);                               \
        }                                                                                                               \
        const int nu = 8 / KS, blocks = std::max(1, std::min(resident, (max_units + nu - 1) / nu));                      \
        DSOCR_LAUNCH(moe_gateup_f4mm_kernel<KS>, dim3(blocks), dim3(512), lds, s, a);                                    \
    } while (0)
    if (ks == 4) DSOCR_GF(4);
    else if (ks == 2) DSOCR_GF(2);
    else DSOCR_GF(1);
#undef DSOCR_GF
}

int moe_down_f4mm_groups(const MoeF4Args& a) { return mmc_down_groups(a); }

void launch_moe_down_f4mm(const MoeF4Args& a, hipStream_t s) {
    if (!moe_f4mm_ok(a)) throw std::runtime_error("EINVAL: MXFP4 decode MoE outside its range");
    const int G = moe_down_f4mm_groups(a);
    DSOCR_LAUNCH(moe_down_f4mm_kernel, dim3((unsigned)(G * (a.H / DN_RT))), dim3(256), mmc_plane_bytes(a.I), s, a, G);
}

}  // namespace dsocr
