// The kernels around the convolutions that the frozen networks share (syncnet.hip, wav2lip.hip, s3fd.hip, face_recon.hip, fan.hip,
// head_mask.hip): the weight pack with the BatchNorm fold, the two bias folds, the NCHW <-> NHWC layouts, a
// copy and the 3 x 3 / 2 max pool.  Each is defined here once and reached through conv_net.h's launch functions.  Every element
// decode comes from conv_frag.h and conv_net_core.h, which the tests/*_core_host.cpp programs walk on the CPU.
#include <hip/hip_runtime.h>

#include "conv_mfma.h"
#include "conv_net.h"
#include "conv_net_core.h"

// ---- packed weights ------------------------------------------------------------------------------------------------------------
// one thread per element of the packed matrix; the fold is fp32((double)W * s) with s = conv_bn_scale, one rounding
__global__ __launch_bounds__(256) void conv_net_pack_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                            const float* __restrict__ var, double eps, int wc, int cin, int cinp, int cout, int np,
                                                            int taps, int K, int stem, __bf16* __restrict__ hi, __bf16* __restrict__ lo) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)K * np) return;
    int k, n;
    cf_pack_decode(e, np / 32, &k, &n);
    float w = 0.0f;
    if (n < cout) {
        const double s = conv_bn_scale(gamma, var, eps, n);
        if (stem) {
            if (k < CN_STEM_K) {
                int ky, kx, c;
                cn_stem_tap(k, &ky, &kx, &c);
                w = (float)((double)W[((size_t)n * wc + c) * 49 + ky * 7 + kx] * s);
            }
        } else {
            const int tap = k / cinp, ci = k - tap * cinp;
            if (ci < cin) w = (float)((double)W[((size_t)n * wc + ci) * taps + tap] * s);
        }
    }
    const __bf16 h = (__bf16)w;
    hi[e] = h;
    lo[e] = conv_lo(w, h);
}

// Two kernels, not one: (0 - mean) s + beta and beta - mean s agree in every bit except the sign of a zero result (beta = -0,
// mean = +0), and the packed bytes of each network stay what its own expression gives.
__global__ __launch_bounds__(256) void conv_net_bias_bn_kernel(const float* __restrict__ bias, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ mean,
                                                               const float* __restrict__ var, double eps, int cout, float* __restrict__ dst) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < cout) dst[n] = (float)(((double)bias[n] - (double)mean[n]) * conv_bn_scale(gamma, var, eps, n) + (double)beta[n]);
}

__global__ __launch_bounds__(256) void conv_net_shift_bn_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ mean, const float* __restrict__ var, double eps, int np,
                                                                float* __restrict__ dst) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < np) dst[n] = gamma ? (float)((double)beta[n] - (double)mean[n] * conv_bn_scale(gamma, var, eps, n)) : 0.0f;
}

__global__ __launch_bounds__(256) void conv_net_copy_kernel(const float* __restrict__ src, size_t n, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- layouts -------------------------------------------------------------------------------------------------------------------
// one thread per element of the Cp channels of the padded destination.  The cell is decoded with cn_row_cell -- one 64-bit division by
// the map's cells and 32-bit arithmetic inside the image -- because on a large image batch this kernel is bound by its index
// divisions, not by memory
__global__ __launch_bounds__(256) void conv_net_to_nhwc_kernel(const float* __restrict__ src, int n, int C, int H, int W, int pad, int Cp,
                                                               float* __restrict__ dst, int dstride) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const long long cells = (long long)n * Hp * Wp;
    const size_t total = (size_t)cells * Cp;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t cell = e / Cp;
        const int c = (int)(e - cell * Cp);
        int img, yp, xp;
        cn_row_cell((long long)cell, cells, Hp, Wp, &img, &yp, &xp);
        float v = 0.0f;
        if (c < C && xp >= pad && xp < Wp - pad && yp >= pad && yp < Hp - pad)
            v = src[(((size_t)img * C + c) * H + (yp - pad)) * W + (xp - pad)];
        dst[cell * dstride + c] = v;
    }
}

// one thread per element of the destination
__global__ __launch_bounds__(256) void conv_net_to_nchw_kernel(const float* __restrict__ src, int sstride, int n, int C, int H, int W, int pad,
                                                               float* __restrict__ dst) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const size_t total = (size_t)n * C * H * W;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int x = (int)(e % W);
        size_t t = e / W;
        const int y = (int)(t % H);
        t /= H;
        const int c = (int)(t % C), img = (int)(t / C);
        dst[e] = src[(((size_t)img * Hp + (y + pad)) * Wp + (x + pad)) * sstride + c];
    }
}

// ---- pool ------------------------------------------------------------------------------------------------------------------------
// the maximum over the taps of the 3 x 3 window that lie inside the map (F.max_pool2d pads with -inf).  One thread per four
// channels of an output cell.
__global__ __launch_bounds__(256) void conv_net_max_pool_kernel(const float* __restrict__ in, int n, int Hi, int Wi, int C, float* __restrict__ out) {
    const int Ho = cn_pool_out(Hi), Wo = cn_pool_out(Wi), C4 = C / 4;
    const size_t total = (size_t)n * Ho * Wo * C4;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % C4) * 4;
        int img, yo, xo;
        cn_cell(e / C4, Ho, Wo, &img, &yo, &xo);
        int ya, yb, xa, xb;
        cn_pool_range(yo, Hi, &ya, &yb);
        cn_pool_range(xo, Wi, &xa, &xb);
        float4 v = *reinterpret_cast<const float4*>(in + (((size_t)img * Hi + ya) * Wi + xa) * C + c);
        for (int y = ya; y < yb; ++y)
            for (int x = xa; x < xb; ++x) {
                const float4 t = *reinterpret_cast<const float4*>(in + (((size_t)img * Hi + y) * Wi + x) * C + c);
                v.x = fmaxf(v.x, t.x);
                v.y = fmaxf(v.y, t.y);
                v.z = fmaxf(v.z, t.z);
                v.w = fmaxf(v.w, t.w);
            }
        *reinterpret_cast<float4*>(out + e * 4) = v;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
void conv_net_pack(const float* W, const float* gamma, const float* var, double eps, int wc, int cin, int cinp, int cout, int np, int taps, int K,
                   int stem, __bf16* hi, __bf16* lo, hipStream_t st) {
    const size_t elems = (size_t)K * np;
    conv_net_pack_kernel<<<(unsigned)((elems + 255) / 256), 256, 0, st>>>(W, gamma, var, eps, wc, cin, cinp, cout, np, taps, K, stem, hi, lo);
}

void conv_net_bias_bn(const float* bias, const float* gamma, const float* beta, const float* mean, const float* var, double eps, int cout, float* dst,
                      hipStream_t st) {
    conv_net_bias_bn_kernel<<<(cout + 255) / 256, 256, 0, st>>>(bias, gamma, beta, mean, var, eps, cout, dst);
}

void conv_net_shift_bn(const float* gamma, const float* beta, const float* mean, const float* var, double eps, int np, float* dst, hipStream_t st) {
    conv_net_shift_bn_kernel<<<(np + 255) / 256, 256, 0, st>>>(gamma, beta, mean, var, eps, np, dst);
}

void conv_net_to_nhwc(const float* src, int n, int C, int H, int W, int pad, int Cp, float* dst, int dstride, hipStream_t st) {
    const size_t total = (size_t)n * (H + 2 * pad) * (W + 2 * pad) * Cp;
    conv_net_to_nhwc_kernel<<<conv_grid(total), 256, 0, st>>>(src, n, C, H, W, pad, Cp, dst, dstride);
}

void conv_net_to_nchw(const float* src, int sstride, int n, int C, int H, int W, int pad, float* dst, hipStream_t st) {
    conv_net_to_nchw_kernel<<<conv_grid((size_t)n * C * H * W), 256, 0, st>>>(src, sstride, n, C, H, W, pad, dst);
}

void conv_net_copy(const float* src, size_t n, float* dst, hipStream_t st) {
    conv_net_copy_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src, n, dst);
}

void conv_net_max_pool(const float* in, int n, int Hi, int Wi, int C, float* out, hipStream_t st) {
    const size_t work = (size_t)n * cn_pool_out(Hi) * cn_pool_out(Wi) * (C / 4);
    conv_net_max_pool_kernel<<<conv_grid(work), 256, 0, st>>>(in, n, Hi, Wi, C, out);
}
