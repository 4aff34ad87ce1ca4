// VGG16 perceptual loss term of the reference's training objective (Utils/HeadNeRFLossUtils.py:23-64, 140-154), forward and
// input-gradient backward.
//
//   prologue     nan_to_num(merge) and the masked target, ImageNet normalisation, bilinear resize to 224^2 (align_corners=False)
//                -> one batch of 2B images (predictions first, then targets), NHWC with a 1-pixel zero halo
//   conv x10     3x3 / pad 1 convolution + bias + ReLU of torchvision vgg16().features[:23] as an implicit GEMM on
//                v_mfma_f32_32x32x16_bf16 (M = output pixels, N = C_out, K = 9 C_in, k = tap * C_in + c_in); the 2x2 max-pool at
//                the head of blocks 2..4 is taken while loading the first conv's A operand
//   L1           per block end, mean |x - y| over the B prediction / target pairs: fixed-grid partial sums + one ordered finish
//   backward     the same GEMM template on a transposed, flipped weight pack (dgrad), ReLU gate in the epilogue, the pool routed
//                through its arg-max and the next block's L1 gradient added where blocks meet; the resize and 1/std back to
//                d_merge as a gather (every source pixel collects its taps in a fixed order: bit-reproducible)
//
// Precision.  N3DT_BF16: activations and weights rounded to bf16 at the MFMA operands, fp32 accumulate.  N3DT_F32: every operand
// split x = hi + lo (two bf16s), three products hi*hi + hi*lo + lo*hi per product (~16 mantissa bits, as nerf_fwd_x16s.hip).
// Activations are stored fp32 in both modes; the conversion happens while the operand is loaded.  The K step of both modes, the
// split and the order of its products are conv_mfma.h's, which lpips.hip and syncnet.hip share; the fragment order of the weight
// pack and the accumulators' rows are conv_frag.h's.
//
// Every image of the 2B batch goes through identical code with the same K order and no split-K, so a prediction equal to its
// target gives bit-identical activations, a loss of exactly 0 and a gradient of exactly 0.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/n3dt.h"
#include "conv_mfma.h"
#include "conv_net.h"
#include "n3dt_launch.h"

#define VGG_L1_BLOCKS 256
#define VGG_S 224

// torchvision vgg16().features indices 0,2,5,7,10,12,14,17,19,21
static constexpr int kCin[N3DT_VGG_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512};
static constexpr int kCout[N3DT_VGG_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512};
static constexpr int kH[N3DT_VGG_CONVS] = {224, 224, 112, 112, 56, 56, 56, 28, 28, 28};
static constexpr bool kPoolIn[N3DT_VGG_CONVS] = {false, false, true, false, true, false, false, true, false, false};
static constexpr int kBlockEnd[4] = {1, 3, 6, 9};  // the convs whose ReLU output ends blocks [:4], [4:9], [9:16], [16:23]

// ---- weight pack --------------------------------------------------------------------------------------------------------------
// One matrix per conv and direction in conv_frag.h's fragment order, [Kp/16][Np/32] fragments of 64 lanes x 8 bf16: element e holds
// B[k][n] with (k, n) = cf_pack_decode(e), so a wave reads one fragment as one contiguous KiB.
//   forward: B[tap * C_in + ci][co]  = W[co][ci][ky][kx]                      Kp = rup(9 C_in, 16), Np = C_out
//   dgrad:   B[tap * C_out + co][ci] = W[co][ci][2 - ky][2 - kx]              Kp = 9 C_out,         Np = rup(C_in, 64)
// N3DT_F32 stores a lo matrix right behind each hi matrix.  The fp32 biases follow the matrices.
struct VggPackLayout {
    size_t w[N3DT_VGG_CONVS][2];  // [conv][0 forward, 1 dgrad] byte offset of the hi matrix (lo = hi + elems * 2)
    size_t elems[N3DT_VGG_CONVS][2];
    int kp[N3DT_VGG_CONVS][2], np[N3DT_VGG_CONVS][2];
    size_t bias[N3DT_VGG_CONVS];
    size_t total;
};

static VggPackLayout vgg_layout(int precision) {
    VggPackLayout L;
    const int parts = precision == N3DT_F32 ? 2 : 1;
    size_t off = 0;
    for (int l = 0; l < N3DT_VGG_CONVS; ++l) {
        L.kp[l][0] = (int)rup(9 * kCin[l], 16);
        L.np[l][0] = kCout[l];
        L.kp[l][1] = 9 * kCout[l];
        L.np[l][1] = (int)rup(kCin[l], 64);
        for (int d = 0; d < 2; ++d) {
            L.elems[l][d] = (size_t)L.kp[l][d] * L.np[l][d];
            L.w[l][d] = off;
            off = rup(off + L.elems[l][d] * 2 * parts, 256);
        }
    }
    for (int l = 0; l < N3DT_VGG_CONVS; ++l) {
        L.bias[l] = off;
        off = rup(off + kCout[l] * sizeof(float), 256);
    }
    L.total = off;
    return L;
}

__global__ __launch_bounds__(256) void vgg_pack_kernel(const float* __restrict__ W, int cin, int cout, int kp, int np_, int dgrad, int split,
                                                       __bf16* __restrict__ hi, __bf16* __restrict__ lo) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)kp * np_) return;
    int k, n;
    cf_pack_decode(e, np_ / 32, &k, &n);
    float w = 0.0f;
    if (!dgrad) {
        if (k < 9 * cin && n < cout) {
            const int tap = k / cin, ci = k - tap * cin;
            w = W[((size_t)(n * cin + ci) * 3 + tap / 3) * 3 + tap % 3];
        }
    } else if (n < cin) {
        const int tap = k / cout, co = k - tap * cout;
        w = W[((size_t)(co * cin + n) * 3 + (2 - tap / 3)) * 3 + (2 - tap % 3)];
    }
    const __bf16 h = (__bf16)w;
    hi[e] = h;
    if (split) lo[e] = conv_lo(w, h);
}

// ---- implicit-GEMM 3x3 convolution ---------------------------------------------------------------------------------------------
struct VggConvArgs {
    const float* in;     // MODE 0/2: [n_img, H+2, W+2, cin] (zero halo); MODE 1: the un-pooled [n_img, 2H+2, 2W+2, cin]
    const __bf16* whi;   // packed B matrix (hi), [kp/16][np/32][64][8]
    const __bf16* wlo;   // its lo half (split mode)
    const float* bias;   // forward: [cout], added before the ReLU; NULL: none
    const float* gate;   // dgrad: activation in the output's (padded) layout, output kept where it is > 0; NULL: none
    float* out;          // out_pad: [n_img, H+2, W+2, cout] interior only; else [n_img, H, W, cout]
    int n_img, H, W, cin, kp, np_, cout, out_pad, relu;
};

// MODE 0: C_in % 16 == 0, halo-padded input;  MODE 1: same with the 2x2 max-pool fused into the load;  MODE 2: any C_in (conv1_1)
// 256 threads = 4 waves; a wave computes 64 output pixels x 64 output channels (2 x 2 tiles of 32 x 32), the workgroup 256 pixels
template <bool SPLIT, int MODE>
__global__ __launch_bounds__(256) void vgg_conv_kernel(VggConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int HW = a.H * a.W, M = a.n_img * HW;
    const int m0 = (blockIdx.x * 4 + wave) * 64;
    if (m0 >= M) return;  // no barriers in this kernel: an idle wave may leave
    const int nt0 = blockIdx.y * 2;
    const int Wp = a.W + 2;
    int pn[2], py[2], px[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = min(m0 + mt * 32 + r, M - 1);  // rows past M compute a clamped pixel and are never stored
        pn[mt] = m / HW;
        const int rem = m - pn[mt] * HW;
        py[mt] = rem / a.W;
        px[mt] = rem - py[mt] * a.W;
    }
    conv_f32x16 acc[2][2];
    CONV_ZERO_ACC(acc, 2);
    float av[2][8];

    if constexpr (MODE == 0) {
        const float* base[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) base[mt] = a.in + ((size_t)(pn[mt] * (a.H + 2) + py[mt]) * Wp + px[mt]) * a.cin + 8 * h;
        int s = 0;
        for (int tap = 0; tap < 9; ++tap) {
            const int toff = ((tap / 3) * Wp + tap % 3) * a.cin;
            for (int c0 = 0; c0 < a.cin; c0 += 16, ++s) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) conv_load8(base[mt] + toff + c0, av[mt]);
                conv_mma_step<SPLIT, 2>(a.whi, a.wlo, a.np_, s, nt0, lane, av, acc);
            }
        }
    } else if constexpr (MODE == 1) {
        const int Wu = 2 * a.W + 2;  // row length of the un-pooled, padded input
        int s = 0;
        for (int tap = 0; tap < 9; ++tap) {
            const float* src[2];
            bool ok[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int qy = py[mt] + tap / 3 - 1, qx = px[mt] + tap % 3 - 1;  // pooled coordinates of the tap
                ok[mt] = qy >= 0 && qy < a.H && qx >= 0 && qx < a.W;
                src[mt] = a.in + ((size_t)(pn[mt] * (2 * a.H + 2) + 2 * qy + 1) * Wu + 2 * qx + 1) * a.cin + 8 * h;
            }
            for (int c0 = 0; c0 < a.cin; c0 += 16, ++s) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    if (ok[mt]) {
                        float q[8];
                        const float* p = src[mt] + c0;
                        conv_load8(p, av[mt]);
                        conv_load8(p + a.cin, q);
#pragma unroll
                        for (int j = 0; j < 8; ++j) av[mt][j] = fmaxf(av[mt][j], q[j]);
                        conv_load8(p + (size_t)Wu * a.cin, q);
#pragma unroll
                        for (int j = 0; j < 8; ++j) av[mt][j] = fmaxf(av[mt][j], q[j]);
                        conv_load8(p + (size_t)Wu * a.cin + a.cin, q);
#pragma unroll
                        for (int j = 0; j < 8; ++j) av[mt][j] = fmaxf(av[mt][j], q[j]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j) av[mt][j] = 0.0f;
                    }
                }
                conv_mma_step<SPLIT, 2>(a.whi, a.wlo, a.np_, s, nt0, lane, av, acc);
            }
        }
    } else {
        const int K = 9 * a.cin;
        for (int s = 0; s < (a.kp >> 4); ++s) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float* base = a.in + ((size_t)(pn[mt] * (a.H + 2) + py[mt]) * Wp + px[mt]) * a.cin;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * s + 8 * h + j;
                    float v = 0.0f;
                    if (k < K) {
                        const int tap = k / a.cin, ci = k - tap * a.cin;
                        v = base[((tap / 3) * Wp + tap % 3) * a.cin + ci];
                    }
                    av[mt][j] = v;
                }
            }
            conv_mma_step<SPLIT, 2>(a.whi, a.wlo, a.np_, s, nt0, lane, av, acc);
        }
    }

    // epilogue: accumulator register i of lane (r, h) is output row cf_acc_row(i, h), column r
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = m0 + mt * 32 + cf_acc_row(i, h);
            if (m >= M) continue;
            const int n = m / HW, rem = m - n * HW, y = rem / a.W, x = rem - y * a.W;
            const size_t pix = a.out_pad ? (size_t)(n * (a.H + 2) + y + 1) * Wp + x + 1 : (size_t)(n * a.H + y) * a.W + x;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int co = (nt0 + nt) * 32 + r;
                if (co >= a.cout) continue;
                float v = acc[mt][nt][i];
                if (a.bias) v += a.bias[co];
                if (a.relu) v = v > 0.0f ? v : 0.0f;
                const size_t o = pix * a.cout + co;
                if (a.gate) v = a.gate[o] > 0.0f ? v : 0.0f;
                a.out[o] = v;
            }
        }
}

// ---- halo, prologue, L1, junction, resize backward -----------------------------------------------------------------------------
#define VGG_HALO_MAX 12
struct VggHaloList {
    float* p[VGG_HALO_MAX];
    int n_img[VGG_HALO_MAX], H[VGG_HALO_MAX], W[VGG_HALO_MAX], C[VGG_HALO_MAX];
};

__global__ __launch_bounds__(256) void vgg_halo_kernel(VggHaloList L) {
    const int b = blockIdx.y;
    const int H = L.H[b], W = L.W[b], C = L.C[b];
    const int per_img = (2 * (W + 2) + 2 * H) * C;
    const int total = L.n_img[b] * per_img;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int n = e / per_img, idx = e - n * per_img, cell = idx / C, c = idx - cell * C;
        int y, x;
        if (cell < W + 2) {
            y = 0;
            x = cell;
        } else if (cell < 2 * (W + 2)) {
            y = H + 1;
            x = cell - (W + 2);
        } else {
            const int k = cell - 2 * (W + 2);
            y = 1 + (k >> 1);
            x = (k & 1) ? W + 1 : 0;
        }
        L.p[b][((size_t)(n * (H + 2) + y) * (W + 2) + x) * C + c] = 0.0f;
    }
}

__constant__ float c_vgg_mean[3] = {0.485f, 0.456f, 0.406f};
__constant__ float c_vgg_std[3] = {0.229f, 0.224f, 0.225f};

// PyTorch's upsample_bilinear2d source index (align_corners=False, no scale_factor): scale = in / out
__device__ __forceinline__ void vgg_src_index(int dst, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
    l0 = 1.0f - l1;
}

__device__ __forceinline__ float vgg_nan_to_num(float v) {
    if (isnan(v)) return 0.0f;
    if (isinf(v)) return v > 0.0f ? FLT_MAX : -FLT_MAX;
    return v;
}

// img < B: nan_to_num(merge[img]);  img >= B: gt[img - B] with bg_value where mask < 0.5.  Normalised, then resized to 224^2.
__global__ __launch_bounds__(256) void vgg_prologue_kernel(int B, int P, const float* __restrict__ merge, const float* __restrict__ gt,
                                                           const float* __restrict__ mask, float bg, float* __restrict__ in0) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * B * VGG_S * VGG_S) return;
    const int img = e / (VGG_S * VGG_S), rem = e - img * VGG_S * VGG_S, oy = rem / VGG_S, ox = rem - oy * VGG_S;
    const bool pred = img < B;
    const int b = pred ? img : img - B;
    const float scale = (float)P / (float)VGG_S;
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    vgg_src_index(oy, P, scale, y0, y1, hy0, hy1);
    vgg_src_index(ox, P, scale, x0, x1, wx0, wx1);
    const size_t PP = (size_t)P * P;
    const int off[4] = {y0 * P + x0, y0 * P + x1, y1 * P + x0, y1 * P + x1};
    bool keep[4] = {true, true, true, true};
    if (!pred && mask) {
#pragma unroll
        for (int t = 0; t < 4; ++t) keep[t] = mask[b * PP + off[t]] >= 0.5f;
    }
    float* o = in0 + ((size_t)(img * (VGG_S + 2) + oy + 1) * (VGG_S + 2) + ox + 1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* src = (pred ? merge : gt) + (b * 3 + c) * PP;
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float u = pred ? vgg_nan_to_num(src[off[t]]) : (keep[t] ? src[off[t]] : bg);
            v[t] = (u - c_vgg_mean[c]) / c_vgg_std[c];
        }
        o[c] = hy0 * (wx0 * v[0] + wx1 * v[1]) + hy1 * (wx0 * v[2] + wx1 * v[3]);
    }
}

// sum |x - y| over the B prediction / target pairs of one padded block-end activation, VGG_L1_BLOCKS fixed-order partials
__global__ __launch_bounds__(256) void vgg_l1_partial_kernel(const float* __restrict__ act, int B, int H, int W, int C, float* __restrict__ partial) {
    __shared__ float red[256];
    const int C4 = C >> 2;
    const int total = B * H * W * C4;
    const size_t img = (size_t)(H + 2) * (W + 2) * C;
    float s = 0.0f;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += VGG_L1_BLOCKS * 256) {
        const int c4 = e % C4, pix = e / C4, x = pix % W, t = pix / W, y = t % H, n = t / H;
        const size_t o = ((size_t)(n * (H + 2) + y + 1) * (W + 2) + x + 1) * C + 4 * c4;
        const float4 p = *reinterpret_cast<const float4*>(act + o);
        const float4 q = *reinterpret_cast<const float4*>(act + o + B * img);
        s += ((fabsf(p.x - q.x) + fabsf(p.y - q.y)) + (fabsf(p.z - q.z) + fabsf(p.w - q.w)));
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

struct VggCounts {
    float n[4];
};

// terms[b] = (sum of block b's partials) / N_b;  terms[4] = ((t0 + t1) + t2) + t3, the reference's `loss += ...` order
__global__ __launch_bounds__(256) void vgg_l1_finish_kernel(const float* __restrict__ partial, VggCounts cnt, float* __restrict__ terms) {
    __shared__ float red[256];
    __shared__ float t[4];
    for (int b = 0; b < 4; ++b) {
        red[threadIdx.x] = partial[b * VGG_L1_BLOCKS + threadIdx.x];
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) t[b] = red[0] / cnt.n[b];
        __syncthreads();
    }
    if (threadIdx.x < 4) terms[threadIdx.x] = t[threadIdx.x];
    if (threadIdx.x == 0) terms[4] = ((t[0] + t[1]) + t[2]) + t[3];
}

// where blocks meet: dZ = (act > 0) * (g sign(x - y) / N_b + pool-routed gradient of the next block) for the B prediction images,
// written over the whole padded image (halo = 0).  dpool [B, H/2, W/2, C] or NULL (the last block end).
__global__ __launch_bounds__(256) void vgg_junction_kernel(const float* __restrict__ act, const float* __restrict__ dpool,
                                                           const float* __restrict__ g_total, float inv_n, int B, int H, int W, int C,
                                                           float* __restrict__ dz) {
    const int Wp = W + 2, Hp = H + 2;
    const int total = B * Hp * Wp * C;
    const size_t img = (size_t)Hp * Wp * C;
    const float g = g_total[0] * inv_n;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int c = e % C, t = e / C, xp = t % Wp, t2 = t / Wp, yp = t2 % Hp, n = t2 / Hp;
        if (xp == 0 || yp == 0 || xp == Wp - 1 || yp == Hp - 1) {
            dz[e] = 0.0f;
            continue;
        }
        const float xv = act[e], yv = act[e + B * img];
        float d = g * (float)((xv > yv) - (xv < yv));
        if (dpool) {
            const int y = yp - 1, x = xp - 1, y0 = y & ~1, x0 = x & ~1;
            // PyTorch's max_pool2d arg-max: the first strict maximum in row-major order of the 2x2 window
            const float* w0 = act + ((size_t)(n * Hp + y0 + 1) * Wp + x0 + 1) * C + c;
            const float v[4] = {w0[0], w0[C], w0[(size_t)Wp * C], w0[(size_t)Wp * C + C]};
            int am = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k] > v[am]) am = k;
            if (am == (y - y0) * 2 + (x - x0)) d += dpool[((size_t)(n * (H / 2) + (y >> 1)) * (W / 2) + (x >> 1)) * C + c];
        }
        dz[e] = xv > 0.0f ? d : 0.0f;
    }
}

// d_merge[b, c, sy, sx] = (sum over the 224^2 outputs that sampled (sy, sx), in ascending (oy, ox), of w_y w_x d_in0) / std_c;
// 0 where merge was not finite (nan_to_num's gradient).  d_in0 [B, 224, 224, 3].
__device__ __forceinline__ float vgg_tap_weight(int o, int s, int in, float scale) {
    int i0, i1;
    float l0, l1;
    vgg_src_index(o, in, scale, i0, i1, l0, l1);
    return (i0 == s ? l0 : 0.0f) + (i1 == s ? l1 : 0.0f);
}

__global__ __launch_bounds__(256) void vgg_resize_bwd_kernel(int B, int P, const float* __restrict__ merge, const float* __restrict__ din0,
                                                             float* __restrict__ d_merge) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * P * P) return;
    const int b = e / (P * P), rem = e - b * P * P, sy = rem / P, sx = rem - sy * P;
    const float scale = (float)P / (float)VGG_S;
    // outputs whose lower tap is sy - 1 or sy: src = scale (o + 0.5) - 0.5 in [sy - 1, sy + 1), widened by one on each side
    const int ylo = max(0, (int)floorf(((float)sy - 0.5f) / scale - 0.5f) - 1), yhi = min(VGG_S - 1, (int)ceilf(((float)sy + 1.5f) / scale - 0.5f) + 1);
    const int xlo = max(0, (int)floorf(((float)sx - 0.5f) / scale - 0.5f) - 1), xhi = min(VGG_S - 1, (int)ceilf(((float)sx + 1.5f) / scale - 0.5f) + 1);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = vgg_tap_weight(oy, sy, P, scale);
        if (wy == 0.0f) continue;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const float wx = vgg_tap_weight(ox, sx, P, scale);
            if (wx == 0.0f) continue;
            const float w = wy * wx;
            const float* d = din0 + ((size_t)(b * VGG_S + oy) * VGG_S + ox) * 3;
            s0 += w * d[0];
            s1 += w * d[1];
            s2 += w * d[2];
        }
    }
    const size_t PP = (size_t)P * P;
    const float s[3] = {s0, s1, s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t o = (b * 3 + c) * PP + rem;
        d_merge[o] = isfinite(merge[o]) ? s[c] / c_vgg_std[c] : 0.0f;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static size_t act_floats(int n_img, int l) { return (size_t)n_img * (kH[l] + 2) * (kH[l] + 2) * kCout[l]; }

extern "C" size_t n3dt_vgg_packed_layout_bytes(int precision) { return vgg_layout(precision).total; }

extern "C" size_t n3dt_vgg_saved_floats(int batch) {
    size_t t = 0;
    for (int l = 0; l < N3DT_VGG_CONVS; ++l) t += rup(act_floats(2 * batch, l), 64);
    return t;
}

static size_t fwd_ws_floats(int batch) { return rup((size_t)2 * batch * (VGG_S + 2) * (VGG_S + 2) * 3, 64) + 4 * VGG_L1_BLOCKS; }
static size_t bwd_buf_floats(int batch) { return rup((size_t)batch * (VGG_S + 2) * (VGG_S + 2) * 64, 64); }

extern "C" size_t n3dt_vgg_ws_floats(int batch) {
    const size_t f = fwd_ws_floats(batch), b = 2 * bwd_buf_floats(batch);
    return f > b ? f : b;
}

extern "C" void n3dt_launch_vgg_pack(int precision, const N3dtVggParams* p, void* packed, hipStream_t st) {
    const VggPackLayout L = vgg_layout(precision);
    char* base = (char*)packed;
    const int split = precision == N3DT_F32;
    for (int l = 0; l < N3DT_VGG_CONVS; ++l) {
        for (int d = 0; d < 2; ++d) {
            __bf16* hi = (__bf16*)(base + L.w[l][d]);
            const size_t n = L.elems[l][d];
            vgg_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(p->weight[l], kCin[l], kCout[l], L.kp[l][d], L.np[l][d], d, split, hi,
                                                                        split ? hi + n : hi);
        }
        conv_net_copy(p->bias[l], (size_t)kCout[l], (float*)(base + L.bias[l]), st);
    }
}

template <bool SPLIT>
static void launch_conv(const VggConvArgs& a, int mode, hipStream_t st) {
    const dim3 grid((unsigned)((a.n_img * a.H * a.W + 255) / 256), (unsigned)(a.np_ / 64));
    if (mode == 0) vgg_conv_kernel<SPLIT, 0><<<grid, 256, 0, st>>>(a);
    else if (mode == 1) vgg_conv_kernel<SPLIT, 1><<<grid, 256, 0, st>>>(a);
    else vgg_conv_kernel<SPLIT, 2><<<grid, 256, 0, st>>>(a);
}

static void conv(int precision, const VggConvArgs& a, int mode, hipStream_t st) {
    if (precision == N3DT_F32) launch_conv<true>(a, mode, st);
    else launch_conv<false>(a, mode, st);
}

static VggConvArgs weights_of(int precision, const void* packed, int l, int d) {
    const VggPackLayout L = vgg_layout(precision);
    VggConvArgs a = {};
    a.whi = (const __bf16*)((const char*)packed + L.w[l][d]);
    a.wlo = a.whi + L.elems[l][d];
    a.kp = L.kp[l][d];
    a.np_ = L.np[l][d];
    return a;
}

static void halo_one(float* p, int n_img, int H, int C, hipStream_t st) {
    VggHaloList hl = {};
    hl.p[0] = p;
    hl.n_img[0] = n_img;
    hl.H[0] = hl.W[0] = H;
    hl.C[0] = C;
    vgg_halo_kernel<<<dim3(64, 1), 256, 0, st>>>(hl);
}

static float* act_ptr(void* saved, int batch, int l) {
    float* p = (float*)saved;
    for (int i = 0; i < l; ++i) p += rup(act_floats(2 * batch, i), 64);
    return p;
}

extern "C" void n3dt_launch_vgg_fwd(int batch, int P, int precision, const void* packed, const float* merge, const float* gt,
                                    const float* mask, float bg, float* terms, void* saved, void* ws, hipStream_t st) {
    const VggPackLayout L = vgg_layout(precision);
    float* in0 = (float*)ws;
    float* partial = in0 + rup((size_t)2 * batch * (VGG_S + 2) * (VGG_S + 2) * 3, 64);
    const int n_img = 2 * batch;
    VggHaloList hl = {};
    for (int l = 0; l < N3DT_VGG_CONVS; ++l) {
        hl.p[l] = act_ptr(saved, batch, l);
        hl.n_img[l] = n_img;
        hl.H[l] = hl.W[l] = kH[l];
        hl.C[l] = kCout[l];
    }
    hl.p[10] = in0;
    hl.n_img[10] = n_img;
    hl.H[10] = hl.W[10] = VGG_S;
    hl.C[10] = 3;
    vgg_halo_kernel<<<dim3(64, 11), 256, 0, st>>>(hl);
    vgg_prologue_kernel<<<(n_img * VGG_S * VGG_S + 255) / 256, 256, 0, st>>>(batch, P, merge, gt, mask, bg, in0);
    const float* in = in0;
    for (int l = 0; l < N3DT_VGG_CONVS; ++l) {
        VggConvArgs a = weights_of(precision, packed, l, 0);
        a.in = in;
        a.bias = (const float*)((const char*)packed + L.bias[l]);
        a.out = act_ptr(saved, batch, l);
        a.n_img = n_img;
        a.H = a.W = kH[l];
        a.cin = kCin[l];
        a.cout = kCout[l];
        a.out_pad = 1;
        a.relu = 1;
        conv(precision, a, l == 0 ? 2 : (kPoolIn[l] ? 1 : 0), st);
        in = a.out;
    }
    VggCounts cnt;
    for (int b = 0; b < 4; ++b) {
        const int l = kBlockEnd[b];
        vgg_l1_partial_kernel<<<VGG_L1_BLOCKS, 256, 0, st>>>(act_ptr(saved, batch, l), batch, kH[l], kH[l], kCout[l], partial + b * VGG_L1_BLOCKS);
        cnt.n[b] = (float)((double)batch * kH[l] * kH[l] * kCout[l]);
    }
    vgg_l1_finish_kernel<<<1, 256, 0, st>>>(partial, cnt, terms);
}

// ONE conv of the table at a geometry the caller names, on the caller's buffers (n3dt_vgg_conv_stage): the arguments the two loops
// above and below form for layer l, with n_img, H, W from the caller instead of 2 batch, kH[l], kH[l].
extern "C" void n3dt_launch_vgg_conv_stage(int precision, const void* packed, int l, int dgrad, int n_img, int H, int W, const float* in,
                                           const float* gate, float* out, int out_pad, hipStream_t st) {
    VggConvArgs a = weights_of(precision, packed, l, dgrad ? 1 : 0);
    a.in = in;
    a.out = out;
    a.n_img = n_img;
    a.H = H;
    a.W = W;
    a.out_pad = out_pad;
    if (!dgrad) {
        a.bias = (const float*)((const char*)packed + vgg_layout(precision).bias[l]);
        a.cin = kCin[l];
        a.cout = kCout[l];
        a.relu = 1;
        conv(precision, a, l == 0 ? 2 : (kPoolIn[l] ? 1 : 0), st);
    } else {
        a.gate = gate;
        a.cin = kCout[l];
        a.cout = kCin[l];
        conv(precision, a, 0, st);
    }
}

extern "C" void n3dt_launch_vgg_bwd(int batch, int P, int precision, const void* packed, const float* merge, const float* g_total,
                                    const void* saved, float* d_merge, void* ws, hipStream_t st) {
    float* buf[2] = {(float*)ws, (float*)ws + bwd_buf_floats(batch)};
    void* sv = const_cast<void*>(saved);
    int cur = 0;  // buf[cur] holds the latest gradient: the pooled gradient of the block just finished, then each dZ in turn
    for (int b = 3; b >= 0; --b) {
        const int le = kBlockEnd[b];
        // dZ of the block-end conv: its L1 gradient, plus (b < 3) the next block's pooled gradient [B, H/2, W/2, C] from buf[cur]
        const float inv_n = (float)(1.0 / ((double)batch * kH[le] * kH[le] * kCout[le]));
        const int total = batch * (kH[le] + 2) * (kH[le] + 2) * kCout[le];
        vgg_junction_kernel<<<min((total + 255) / 256, 4096), 256, 0, st>>>(act_ptr(sv, batch, le), b < 3 ? buf[cur] : nullptr, g_total, inv_n,
                                                                            batch, kH[le], kH[le], kCout[le], buf[cur ^ 1]);
        cur ^= 1;
        const int lfirst = b == 0 ? 0 : kBlockEnd[b - 1] + 1;
        for (int l = le; l >= lfirst; --l) {
            VggConvArgs a = weights_of(precision, packed, l, 1);
            a.in = buf[cur];
            a.out = buf[cur ^ 1];
            a.n_img = batch;
            a.H = a.W = kH[l];
            a.cin = kCout[l];
            a.cout = kCin[l];
            if (l > lfirst) {  // the input is the previous conv's ReLU output: gate it here
                a.out_pad = 1;
                a.gate = act_ptr(sv, batch, l - 1);
                halo_one(a.out, batch, kH[l], kCin[l], st);
            } else {
                a.out_pad = 0;  // the pooled gradient [B, H, W, C_in] (blocks 2..4) or d_in0 [B, 224, 224, 3] (conv1_1)
            }
            conv(precision, a, 0, st);
            cur ^= 1;
        }
    }
    // buf[cur] holds d_in0
    vgg_resize_bwd_kernel<<<(batch * P * P + 255) / 256, 256, 0, st>>>(batch, P, merge, buf[cur], d_merge);
}
