// Row ops of the DeepSeek-OCR-2 vision encoder (vision/qwen2.rs): the [image tokens | queries] sequence,
// rotate-half RoPE on the fused q|k|v rows, and the query half of the output.  All f32.
#include <algorithm>

#include "dev_common.hpp"
#include "kernels.hpp"

namespace dsocr {

// out [n][2P][D]: rows 0..P-1 of sequence i = feat[i], rows P..2P-1 = the query table (D % 4 == 0)
__global__ __launch_bounds__(256) void ocr2_build_seq_kernel(const float4* feat, const float4* query, int n, int P, int D4,
                                                             float4* out) {
    const long total = (long)n * 2 * P * D4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % D4);
        const long row = idx / D4;
        const int r = (int)(row % (2 * P));
        const long i = row / (2 * P);
        out[idx] = r < P ? feat[(i * P + r) * D4 + c] : query[(long)(r - P) * D4 + c];
    }
}

void launch_ocr2_build_seq(const float* feat, const float* query, int n, int P, int D, float* out, hipStream_t s) {
    const long total = (long)n * 2 * P * (D / 4);
    if (total <= 0) return;
    const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(ocr2_build_seq_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(feat),
                       reinterpret_cast<const float4*>(query), n, P, D / 4, reinterpret_cast<float4*>(out));
}

// one thread per (row, head, d < hd/2): the pair (d, d + hd/2) of a head, in place.
// out = x * cos + rotate_half(x) * sin, rotate_half(x) = [-x2 | x1] (block.rs:1426-1471)
__global__ __launch_bounds__(256) void ocr2_rope_kernel(float* x, long ld, long rows, int L, int n_heads, int hd,
                                                        const float* cos_t, const float* sin_t) {
    const int half = hd / 2;
    const long total = rows * n_heads * half;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int d = (int)(idx % half);
        const int h = (int)((idx / half) % n_heads);
        const long row = idx / ((long)half * n_heads);
        const int pos = (int)(row % L);
        float* p = x + row * ld + (long)h * hd;
        const float* cs = cos_t + (long)pos * hd;
        const float* sn = sin_t + (long)pos * hd;
        const float x1 = p[d], x2 = p[d + half];
        p[d] = x1 * cs[d] + (-x2) * sn[d];
        p[d + half] = x2 * cs[d + half] + x1 * sn[d + half];
    }
}

void launch_ocr2_rope(float* x, long ld, long rows, int L, int n_heads, int hd, const float* cos_t, const float* sin_t,
                      hipStream_t s) {
    const long total = rows * n_heads * (hd / 2);
    if (total <= 0) return;
    const int blocks = (int)std::min<long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(ocr2_rope_kernel, dim3(blocks), dim3(256), 0, s, x, ld, rows, L, n_heads, hd, cos_t, sin_t);
}

__global__ __launch_bounds__(256) void ocr2_take_queries_kernel(const float4* src, int n, int P, int D4, float4* dst) {
    const long total = (long)n * P * D4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % D4);
        const long row = idx / D4;
        const int r = (int)(row % P);
        const long i = row / P;
        dst[idx] = src[((i * 2 + 1) * P + r) * D4 + c];
    }
}

void launch_ocr2_take_queries(const float* src, int n, int P, int D, float* dst, hipStream_t s) {
    const long total = (long)n * P * (D / 4);
    if (total <= 0) return;
    const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(ocr2_take_queries_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(src), n, P,
                       D / 4, reinterpret_cast<float4*>(dst));
}

}  // namespace dsocr
