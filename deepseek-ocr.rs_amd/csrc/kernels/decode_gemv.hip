// Decode GEMV family (dec_gemv, its LDS and stream forms) and the host dispatch over them.
#include "decode_common.hpp"

namespace dsocr {

// ------------------------------------------------------------------ dec_gemv
// y[m][n] (+)= act(sum_k xn[m][k] W[n][k] + b[n]); xn = rmsnorm(x) if norm_w else x.
// A wave owns RB rows.  Every lane issues its 16-byte weight loads for the first U*64
// chunks BEFORE the block stages x through LDS, so the HBM latency of the weight
// stream overlaps the norm prologue; K <= 64*U*8 is a single batch.
template <typename WT, int MT, int RB, int U>
__global__ __launch_bounds__(256) void dec_gemv_kernel(DecGemvArgs a) {
    WaveSpan span_(a.span);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * RB;
    const bool active = n0 < a.N;
    const WT* W = reinterpret_cast<const WT*>(a.W);
    const int chunks = a.K >> 3;
    constexpr int XR = 2;
    const bool fast = a.K <= XR * 4 * 256;
    XRegs<MT, XR> xr;
    if (fast) xload<MT, XR>(xr, a.x, a.ldx, nullptr, a.M, a.K, a.norm_w);
    // accumulate (residual) rows of one or two tokens: loaded now, with x, instead of after the wave sums
    // (one dependent round trip fewer at the end of o_proj)
    constexpr bool YPRE = MT <= 2;
    float ypre[YPRE ? RB : 1][YPRE ? MT : 1];
    if constexpr (YPRE) {
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int m = 0; m < MT; ++m)
                ypre[r][m] = a.accumulate ? a.y[(long)min(m, a.M - 1) * a.ldy + min(n0 + r, a.N - 1)] : 0.f;
    }
    uint4 wq[U][RB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = u * 64 + lane;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int n = min(n0 + r, a.N - 1);
            wq[u][r] = ldg_nt16(W + (long)n * a.ldw + (min(c, chunks - 1) << 3));
        }
    }
    if (fast) xstage<MT, XR>(xr, a.M, a.K, a.norm_w != nullptr, a.eps, smem);
    else stage_rows(a.x, a.ldx, nullptr, a.M, a.K, a.norm_w, a.eps, smem);
    const float* xs = smem + XS_RED;
    if (a.xn_out && blockIdx.x == 0)  // hand the normalised rows to the next kernel
        for (int i = threadIdx.x * 4; i < a.M * a.K; i += blockDim.x * 4)
            *reinterpret_cast<float4*>(a.xn_out + i) = *reinterpret_cast<const float4*>(xs + i);
    if (!active) return;
    float acc[RB][MT];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
    for (int base = 0;;) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = base + u * 64 + lane;
            if (c < chunks) {
                float w8[RB][8];
#pragma unroll
                for (int r = 0; r < RB; ++r) unpack8<WT>(wq[u][r], w8[r]);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (m < a.M) {
                        float xv[8];
                        ld_x8(xs + m * a.K + (c << 3), xv);
#pragma unroll
                        for (int r = 0; r < RB; ++r)
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[r][m] = fmaf(xv[j], w8[r][j], acc[r][m]);
                    }
                }
            }
        }
        base += 64 * U;
        if (base >= chunks) break;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = base + u * 64 + lane;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int n = min(n0 + r, a.N - 1);
                wq[u][r] = ldg_nt16(W + (long)n * a.ldw + (min(c, chunks - 1) << 3));
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float v = wave_sum(acc[r][m]);
            const int n = n0 + r;
            if (lane == 0 && m < a.M && n < a.N) {
                v = apply_act(v + (a.bias ? a.bias[n] : 0.f), a.act);
                float* yp = a.y + (long)m * a.ldy + n;
                if (a.accumulate) {
                    if constexpr (YPRE) v = ypre[r][m] + v;
                    else v = *yp + v;
                }
                *yp = v;
            }
        }
}

// Several tokens (M = 3..8): blocks of 4 waves, RB weight rows per wave (issued first), the M
// activation rows staged once per block in LDS — wave w stages rows w and w + 4 in the GEMV chunk
// layout (lane: chunks lane, lane+64, lane+128), RMS-normalising them when NORM (its squares summed
// u-major then j, one wave sum, x / den * w: dec_route_grp's form), so the standalone RMSNorm
// launch disappears.  Per-row arithmetic that of dec_gemv (chunk u-major, then j; wave sum; + bias,
// act, y); rows past M are clamped to row M-1 and discarded, so the MT x RB FMA chains interleave.
template <typename WT, int MT, int RB, bool NORM>
__global__ __launch_bounds__(256) void dec_gemv_lds_kernel(DecGemvArgs a) {
    constexpr int U = 3;
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [MT][K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * RB;
    const WT* W = reinterpret_cast<const WT*>(a.W);
    const int chunks = a.K >> 3;
    uint4 wq[U][RB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int cc = min(u * 64 + lane, chunks - 1);
#pragma unroll
        for (int r = 0; r < RB; ++r) wq[u][r] = ldg_nt16(W + (long)min(n0 + r, a.N - 1) * a.ldw + (cc << 3));
    }
#pragma unroll
    for (int h = 0; h < (MT + 3) / 4; ++h) {
        const int m = wave + 4 * h;
        if (m < a.M) {
            float xv[U][8], nw[U][8];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int cc = min(u * 64 + lane, chunks - 1);
                ld_x8(a.x + (long)m * a.ldx + (cc << 3), xv[u]);
                if (NORM) ld_x8(a.norm_w + (cc << 3), nw[u]);
            }
            if (NORM) {
                float q = 0.f;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (u * 64 + lane < chunks)
#pragma unroll
                        for (int j = 0; j < 8; ++j) q += xv[u][j] * xv[u][j];
                const float den = sqrtf(wave_sum(q) / (float)a.K + a.eps);
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[u][j] = (xv[u][j] / den) * nw[u][j];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = u * 64 + lane;
                if (c < chunks) {
                    float* d = xs + (long)m * a.K + (c << 3);
                    *reinterpret_cast<float4*>(d) = make_float4(xv[u][0], xv[u][1], xv[u][2], xv[u][3]);
                    *reinterpret_cast<float4*>(d + 4) = make_float4(xv[u][4], xv[u][5], xv[u][6], xv[u][7]);
                }
            }
        }
    }
    __syncthreads();
    if (n0 >= a.N) return;
    float acc[RB][MT];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = u * 64 + lane;
        if (c < chunks) {
            float w8[RB][8];
#pragma unroll
            for (int r = 0; r < RB; ++r) unpack8<WT>(wq[u][r], w8[r]);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float xv[8];
                ld_x8(xs + (long)min(m, a.M - 1) * a.K + (c << 3), xv);
#pragma unroll
                for (int r = 0; r < RB; ++r)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[r][m] = fmaf(xv[j], w8[r][j], acc[r][m]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float v = wave_sum(acc[r][m]);
            const int n = n0 + r;
            if (lane == 0 && m < a.M && n < a.N) {
                v = apply_act(v + (a.bias ? a.bias[n] : 0.f), a.act);
                float* yp = a.y + (long)m * a.ldy + n;
                if (a.accumulate) v = *yp + v;
                *yp = v;
            }
        }
}

// Large-N variant (lm_head: 129280 rows): a fixed grid of waves walks the row groups with a
// two-deep register pipeline (the loads of group i+1 are in flight while group i is
// reduced), so the per-block x staging / norm prologue is paid once per ~8 row groups.
template <typename WT, int U, int RB>
__device__ __forceinline__ void gemv_issue(uint4 (&q)[U][RB], const WT* W, int n0, int N, long ldw, int chunks,
                                           int lane, bool ok) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = u * 64 + lane;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int n = min(n0 + r, N - 1);
            q[u][r] = ldg_nt16(W + (long)n * ldw + (min(c, chunks - 1) << 3));
            (void)ok;
        }
    }
}

template <typename WT, int MT, int U, int RB>
__device__ __forceinline__ void gemv_finish(const uint4 (&q)[U][RB], const float* xs, const DecGemvArgs& a, int n0,
                                            int chunks, int lane) {
    float acc[RB][MT];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = u * 64 + lane;
        if (c < chunks) {
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                float w8[8];
                unpack8<WT>(q[u][r], w8);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (m < a.M) {
                        float xv[8];
                        ld_x8(xs + m * a.K + (c << 3), xv);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[r][m] = fmaf(xv[j], w8[j], acc[r][m]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float v = wave_sum(acc[r][m]);
            const int n = n0 + r;
            if (lane == 0 && m < a.M && n < a.N) {
                v = apply_act(v + (a.bias ? a.bias[n] : 0.f), a.act);
                float* yp = a.y + (long)m * a.ldy + n;
                if (a.accumulate) v = *yp + v;
                *yp = v;
            }
        }
}

template <typename WT, int MT, int RB>
__global__ __launch_bounds__(256) void dec_gemv_stream_kernel(DecGemvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int U = 3;  // K <= 1536: one batch per row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WT* W = reinterpret_cast<const WT*>(a.W);
    const int chunks = a.K >> 3;
    const int ngroups = (a.N + RB - 1) / RB;
    const int stride = gridDim.x * 4;
    int g = blockIdx.x * 4 + wave;
    uint4 qa[U][RB], qb[U][RB];
    XRegs<MT, 2> xr;  // K <= 1536 here
    xload<MT, 2>(xr, a.x, a.ldx, nullptr, a.M, a.K, a.norm_w);
    gemv_issue<WT, U, RB>(qa, W, g * RB, a.N, a.ldw, chunks, lane, g < ngroups);
    xstage<MT, 2>(xr, a.M, a.K, a.norm_w != nullptr, a.eps, smem);
    const float* xs = smem + XS_RED;
    for (; g < ngroups; g += 2 * stride) {
        const int g2 = g + stride, g3 = g2 + stride;
        gemv_issue<WT, U, RB>(qb, W, g2 * RB, a.N, a.ldw, chunks, lane, g2 < ngroups);
        gemv_finish<WT, MT, U, RB>(qa, xs, a, g * RB, chunks, lane);
        if (g2 >= ngroups) break;
        gemv_issue<WT, U, RB>(qa, W, g3 * RB, a.N, a.ldw, chunks, lane, g3 < ngroups);
        gemv_finish<WT, MT, U, RB>(qb, xs, a, g2 * RB, chunks, lane);
    }
}

// Which kernel one launch of a.M <= 16 rows runs: a pure host decision (no device call; the stream kernel's
// residency query stays in the launch).  dec_gemv_rb switches on it and dec_gemv_kernel_kind names it.
enum class GemvKind { MM, LDS_R1, LDS_R2, RB1, STREAM, RB4, RB2 };
static int gemv_mt(int M) { return M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : M <= 8 ? 8 : 16; }  // staged-row template
static GemvKind gemv_kind(const DecGemvArgs& a) {
    const int MT = gemv_mt(a.M);
    if (MT >= 4 && MT <= 8) {  // several tokens: no LDS staging
        // matrix-core form (decode_mm.hip): weights straight into MFMA, activations as 16-bit planes
        if (dec_mm_ok(a)) return GemvKind::MM;
        // rows per wave of dec_gemv_lds, measured on MI355X at M = 8, K = 1280 (tools/kbench gemv8): 2 for
        // N = 3840 (8.4 us, 11.1 with the norm fused vs 5 + 10.6 for a separate RMSNorm), 1 for N = 1280 (5.9)
        if (a.N <= 16384 && !a.xn_out && a.K <= 64 * 3 * 8 && a.K % 8 == 0)
            return a.N >= 2560 ? GemvKind::LDS_R2 : GemvKind::LDS_R1;
    }
    // small N: one row per wave so the whole matrix is in flight at once; large N: RB rows per wave
    if (a.N <= 16384) return GemvKind::RB1;
    if (a.K <= 64 * 3 * 8 && MT <= 2) return GemvKind::STREAM;
    return MT <= 2 ? GemvKind::RB4 : GemvKind::RB2;
}
// rows per launch: <= 16 and the staged rows must fit the 64 KB dynamic LDS window (0: K too large)
static int gemv_rows_per_launch(int K) {
    return (int)std::min<size_t>(16, (STAGE_LDS_MAX - sizeof(float) * XS_RED) / (sizeof(float) * (size_t)K));
}

const char* dec_gemv_kernel_kind(const DecGemvArgs& a, int* rows_per_launch) {
    const int per = a.K > 0 ? gemv_rows_per_launch(a.K) : 0;
    if (rows_per_launch) *rows_per_launch = per;
    if (a.M <= 0 || a.N <= 0 || per < 1) return "none";
    DecGemvArgs p = a;  // the first row chunk
    p.M = std::min(per, a.M);
    switch (gemv_kind(p)) {
        case GemvKind::MM: return dec_mm_kernel_kind(p);
        case GemvKind::LDS_R1: return "dec_gemv_lds_r1";
        case GemvKind::LDS_R2: return "dec_gemv_lds_r2";
        case GemvKind::RB1: return "dec_gemv_rb1";
        case GemvKind::STREAM: return "dec_gemv_stream";
        case GemvKind::RB4: return "dec_gemv_rb4";
        case GemvKind::RB2: return "dec_gemv_rb2";
    }
    return "none";
}

template <typename WT, int MT>
static void dec_gemv_rb(const DecGemvArgs& a, hipStream_t s) {
    const size_t lds = stage_bytes(a.M, a.K);
    const GemvKind kind = gemv_kind(a);  // gemv_mt(a.M) == MT: every branch below exists for this MT
    if constexpr (MT >= 4 && MT <= 8) {
        if (kind == GemvKind::MM) {
            launch_dec_mm(a, s);
            return;
        }
        if (kind == GemvKind::LDS_R1 || kind == GemvKind::LDS_R2) {
            const size_t xl = sizeof(float) * MT * (size_t)a.K;
            with_rows<1, 2>(kind == GemvKind::LDS_R1 ? 1 : 2, [&](auto rb) {
                constexpr int R = decltype(rb)::value;
                const dim3 g((a.N + 4 * R - 1) / (4 * R));
                if (a.norm_w) DSOCR_LAUNCH((dec_gemv_lds_kernel<WT, MT, R, true>), g, dim3(256), xl, s, a);
                else DSOCR_LAUNCH((dec_gemv_lds_kernel<WT, MT, R, false>), g, dim3(256), xl, s, a);
            });
            return;
        }
    }
    if (kind == GemvKind::RB1) {
        constexpr int RB = 1;
        DSOCR_LAUNCH((dec_gemv_kernel<WT, MT, RB, 3>), dim3((a.N + 4 * RB - 1) / (4 * RB)), dim3(256), lds, s, a);
        return;
    }
    if constexpr (MT <= 2) {
        if (kind == GemvKind::STREAM) {
            constexpr int RB = 4;
            // exactly one resident wave of blocks (no tail of late-starting blocks); asked once per instantiation
            static int resident = 0;
            if (!resident)
                resident = std::max(1, blocks_per_cu(dec_gemv_stream_kernel<WT, MT, RB>, lds)) * std::max(1, device_cus());
            const int groups = (a.N + RB - 1) / RB;
            const int blocks = std::min((groups + 3) / 4, resident);
            DSOCR_LAUNCH((dec_gemv_stream_kernel<WT, MT, RB>), dim3(blocks), dim3(256), lds, s, a);
            return;
        }
    }
    // GemvKind::RB4 (one or two rows) / GemvKind::RB2 (more)
    constexpr int RB = MT <= 2 ? 4 : 2;
    if (kind != (MT <= 2 ? GemvKind::RB4 : GemvKind::RB2)) throw std::runtime_error("EINTERNAL: dec_gemv dispatch");
    DSOCR_LAUNCH((dec_gemv_kernel<WT, MT, RB, 3>), dim3((a.N + 4 * RB - 1) / (4 * RB)), dim3(256), lds, s, a);
}
void launch_dec_gemv(const DecGemvArgs& a, hipStream_t s) {
    if (a.M == 0 || a.N == 0) return;
    const int per = gemv_rows_per_launch(a.K);
    if (per < 1) throw std::runtime_error("EINVAL: dec_gemv K too large for LDS staging");
    for (int m0 = 0; m0 < a.M; m0 += per) {
        DecGemvArgs p = a;
        p.M = std::min(per, a.M - m0);
        p.x = a.x + (long)m0 * a.ldx;
        p.y = a.y + (long)m0 * a.ldy;
        with_wt(a.wdtype, [&](auto wt) {
            with_rows<1, 2, 4, 8, 16>(gemv_mt(p.M), [&](auto mt) { dec_gemv_rb<decltype(wt), decltype(mt)::value>(p, s); });
        });
    }
}

}  // namespace dsocr
