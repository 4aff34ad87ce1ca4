// The head-mask generator (include/n3dt.h, n3dt_head_mask_*; the reference's DataProcess/Gen_HeadMask.py: BiSeNet on ResNet-18,
// argmax, LUT, largest component, hair erosion, green-screen filter, dilated eye mask).  The table, every map's
// size -- known only at run time -- and every address that can go wrong at an edge come from head_mask_core.h, which
// tests/head_mask_core_host.cpp also compiles and walks over the same grids.  That program re-types the loop nest of the
// convolution kernel below (block / wave / lane / tap / K step): a change to that loop here must be made there too.
//
//   conv x31   Conv2d (+ folded BatchNorm) (+ shortcut) (+ ReLU) as an implicit GEMM on v_mfma_f32_32x32x16_bf16 (M = output pixels,
//              N = C_out, k = tap * C_in + c_in; the stem: k = (tap, channel) flattened, 147 padded to 160), every operand split
//              x = hi + lo into two bf16s, three products accumulated in fp32: conv_mfma.h's step in its split form.  The A fetch
//              tests each tap against the input's extent and may read through a nearest upsample, a per-(image, channel) scale
//              and an added term (head_mask_core.h), zero padding behind them
//   small x5   global average -> 1 x 1 convolution (-> BatchNorm) -> ReLU / sigmoid on M = images: float64, fixed order, one kernel
//   pool       3 x 3 / 2 max with padding 1, out-of-range taps ignored
//   labels     per output pixel the argmax over the classes of the bilinear (align_corners) interpolation of the low-resolution
//              logits, float64, first maximum wins; the full-resolution logit volume is never formed
//   post       byte maps, integers only: dilation, LUT, union-find components (atomicMin / atomicAdd), Jacobi erosion, hue filter
//
// Every image goes through identical code with the same K order, no split-K and no float atomics.  Every element of every map is
// written exactly once per forward; nothing is cleared.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/n3dt.h"
#include "conv_mfma.h"
#include "conv_net.h"
#include "head_mask_core.h"
#include "n3dt_launch.h"

// ---- packed weights ------------------------------------------------------------------------------------------------------------
// Per spatial convolution one B matrix in conv_frag.h's fragment order, hi then lo, BatchNorm scale folded in; per small
// convolution the folded fp32 matrix transposed to [C_in][C_out]; then per convolution hm_np fp32 biases (0 without a BatchNorm).
struct HmPackLayout {
    size_t w[HM_CONVS], elems[HM_CONVS], bias[HM_CONVS], total;
};

static HmPackLayout hm_layout() {
    HmPackLayout L;
    size_t off = 0;
    for (int j = 0; j < HM_CONVS; ++j) {
        L.elems[j] = (size_t)hm_K(j) * hm_np(j);
        L.w[j] = off;
        off = rup(off + L.elems[j] * (HM_TABLE[j].kind == HM_SMALL ? sizeof(float) : 2 * sizeof(__bf16)), 256);
    }
    for (int j = 0; j < HM_CONVS; ++j) {
        L.bias[j] = off;
        off = rup(off + hm_np(j) * sizeof(float), 256);
    }
    L.total = off;
    return L;
}

// The spatial pack (W [cout, cin, k, k] -> B [K][np], row k = tap * cin + ci; the stem: (ky * 7 + kx) * 3 + ci, rows 147 .. 159 zero;
// columns from cout on zero), the BatchNorm's scale (1 where the convolution has none) and shift in float64, and the layouts are
// conv_net.hip's.

// a small convolution: W [cout, cin] -> dst [cin][cout] fp32, folded
__global__ __launch_bounds__(256) void head_mask_pack_small_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                                   const float* __restrict__ var, double eps, int cin, int cout,
                                                                   float* __restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= cin * cout) return;
    const int ci = e / cout, co = e - ci * cout;
    dst[e] = (float)((double)W[(size_t)co * cin + ci] * conv_bn_scale(gamma, var, eps, co));
}

// ---- implicit-GEMM convolution ---------------------------------------------------------------------------------------------------
struct HmConvArgs {
    const float* in;      // [n, Hs, Ws, csplit]; the stem: the image [n, Hi + 6, Wi + 6, 3]
    const float* in2;     // [n, Hs, Ws, cin - csplit]: the channels from csplit on, or NULL (csplit = cin)
    const float* skip;    // [n, Ho, Wo, np] or NULL
    const float* addmap;  // [n, Hs, Ws, cin] or NULL
    const float* scale;   // [n][vstride], or NULL: no transform
    const float* addvec;  // [n][vstride] or NULL
    const __bf16* whi;    // packed B matrix (hi), [K/16][np/32][64][8]
    const __bf16* wlo;
    const float* bias;    // [np]
    float* out;           // [n, Ho, Wo, np], every cell written
    int n, Hs, Ws, Hi, Wi, Ho, Wo, cin, csplit, np, k, stride, pad, relu, addself, vstride;
};

#define HM_PLAIN 0
#define HM_STEMK 1
#define HM_XFORM 2

// 256 threads = 4 waves; wave tile t = 4 blockIdx.x + wave computes CN_TILE_M output pixels x 32 NT columns, the column tile
// fastest.  A k-step is 16 channels of one tap (C_in % 16 == 0); HM_STEMK: 16 consecutive k of the flattened (tap, channel) on the
// haloed image, those from 147 on read as 0 against zero weight rows.  HM_XFORM: the fetched value v becomes v * scale + (addvec |
// addmap | v | 0), in fp32, mul then add.  Epilogue: conv + bias (+ skip), then the ReLU -- relu(shortcut + residual).
template <int NT, int MODE>
__global__ __launch_bounds__(256) void head_mask_conv_kernel(HmConvArgs a) {
    const ConvWaveTile t = conv_wave_tile<NT>(a.np, a.n, a.Ho, a.Wo);
    if (t.idle()) return;  // no barriers in this kernel: an idle wave may leave
    const int lane = t.lane, r = t.r, h = t.h, nt0 = t.nt0(NT);
    const long long M = t.M, m0 = t.m0;
    int img[2], yo[2], xo[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) cn_row_cell(m0 + mt * 32 + r, M, a.Ho, a.Wo, &img[mt], &yo[mt], &xo[mt]);  // rows past M: the last pixel again, never stored
    conv_f32x16 acc[2][NT];
    CONV_ZERO_ACC(acc, NT);
    float av[2][8];

    if (MODE == HM_STEMK) {
        const int Wp = a.Wi + 6;
        const float* base[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) base[mt] = a.in + cn_field_base(img[mt], yo[mt], xo[mt], a.stride, a.Hi + 6, Wp, 3);
        for (int s = 0; s < CN_STEM_KP / 16; ++s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * h + j;
                const bool real = k < CN_STEM_K;
                const size_t off = cn_stem_offset(real ? k : 0, Wp);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const float v = base[mt][off];
                    av[mt][j] = real ? v : 0.0f;
                }
            }
            conv_mma_step<true, NT>(a.whi, a.wlo, a.np, s, nt0, lane, av, acc);
        }
    } else {
        const int c2 = a.cin - a.csplit;
        int s = 0;
        for (int tap = 0; tap < a.k * a.k; ++tap) {
            long long cell[2] = {0, 0};
            int ok[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                ok[mt] = hm_tap_cell(img[mt], yo[mt], xo[mt], tap, a.k, a.stride, a.pad, a.Hi, a.Wi, a.Hs, a.Ws, &cell[mt]);
            for (int c0 = 0; c0 < a.cin; c0 += 16, ++s) {
                const int c = c0 + 8 * h;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    if (ok[mt]) {
                        const float* src = c < a.csplit ? a.in + (size_t)cell[mt] * a.csplit + c : a.in2 + (size_t)cell[mt] * c2 + (c - a.csplit);
                        conv_load8(src, av[mt]);
                        if (MODE == HM_XFORM) {
                            float sc[8], ad[8];
                            conv_load8(a.scale + (size_t)img[mt] * a.vstride + c, sc);
                            if (a.addvec) conv_load8(a.addvec + (size_t)img[mt] * a.vstride + c, ad);
                            else if (a.addmap) conv_load8(a.addmap + (size_t)cell[mt] * a.cin + c, ad);
                            else {
#pragma unroll
                                for (int j = 0; j < 8; ++j) ad[j] = a.addself ? av[mt][j] : 0.0f;
                            }
#pragma unroll
                            for (int j = 0; j < 8; ++j) av[mt][j] = av[mt][j] * sc[j] + ad[j];
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j) av[mt][j] = 0.0f;
                    }
                }
                conv_mma_step<true, NT>(a.whi, a.wlo, a.np, s, nt0, lane, av, acc);
            }
        }
    }

    // epilogue: accumulator register i of lane (r, h) is output row cf_acc_row(i, h), column r
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long m = m0 + mt * 32 + cf_acc_row(i, h);
            if (m >= M) continue;
            float* o = a.out + (size_t)m * a.np;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int co = (nt0 + nt) * 32 + r;
                float v = acc[mt][nt][i] + a.bias[co];
                if (a.skip) v += a.skip[(size_t)m * a.np + co];
                if (a.relu) v = v > 0.0f ? v : 0.0f;
                o[co] = v;
            }
        }
}

// ---- the small stage (the 3 x 3 / 2 max pool is conv_net.hip's) --------------------------------------------------------------------
// One workgroup per image.  in: image i's HW cells of cin channels start at in + i * in_stride (HW = 1: a vector).  The mean of
// every channel, summed in float64 in cell order and kept in float64; then out[i][co] = act(sum_ci Wt[ci][co] * mean[ci] + bias[co])
// with ci ascending, float64, rounded once.  cin <= 512.
__global__ __launch_bounds__(256) void head_mask_small_kernel(const float* __restrict__ in, int HW, int cin, size_t in_stride,
                                                              const float* __restrict__ Wt, const float* __restrict__ bias, int cout, int act,
                                                              float* __restrict__ out, int out_stride) {
    __shared__ double mean[512];
    const float* p = in + (size_t)blockIdx.x * in_stride;
    for (int c = threadIdx.x; c < cin; c += 256) {
        double s = 0.0;
        for (int i = 0; i < HW; ++i) s += (double)p[(size_t)i * cin + c];
        mean[c] = s / (double)HW;
    }
    __syncthreads();
    for (int co = threadIdx.x; co < cout; co += 256) {
        double s = 0.0;
        for (int ci = 0; ci < cin; ++ci) s += (double)Wt[(size_t)ci * cout + co] * mean[ci];
        s += (double)bias[co];
        if (act == HM_RELU) s = s > 0.0 ? s : 0.0;
        else if (act == HM_SIGMOID) s = 1.0 / (1.0 + exp(-s));
        out[(size_t)blockIdx.x * out_stride + co] = (float)s;
    }
}

// ---- labels and the upsampled maps -----------------------------------------------------------------------------------------------
// logit (img, c, y, x) of a low-resolution map lies at p[img * si + c * sc + y * sy + x * sx]
struct HmLogits {
    const float* p;
    long long si, sc, sy, sx;
    int nc, h, w;
};

// One thread per output pixel: the four cells' nc logits interpolated in float64 (align_corners), the first maximum wins
__global__ __launch_bounds__(256) void head_mask_labels_kernel(HmLogits L, int n, int H, int W, uint8_t* __restrict__ labels) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * H * W) return;
    int img, Y, X;
    cn_cell(e, H, W, &img, &Y, &X);
    int y0, y1, x0, x1;
    double wy, wx;
    hm_lerp(Y, L.h, H, &y0, &y1, &wy);
    hm_lerp(X, L.w, W, &x0, &x1, &wx);
    const float* p = L.p + (long long)img * L.si;
    int best = 0;
    double top = 0.0;
    for (int c = 0; c < L.nc; ++c) {
        const float* q = p + c * L.sc;
        const double v00 = q[y0 * L.sy + x0 * L.sx], v01 = q[y0 * L.sy + x1 * L.sx], v10 = q[y1 * L.sy + x0 * L.sx], v11 = q[y1 * L.sy + x1 * L.sx];
        const double v = (1.0 - wy) * ((1.0 - wx) * v00 + wx * v01) + wy * ((1.0 - wx) * v10 + wx * v11);
        if (c == 0 || v > top) {
            top = v;
            best = c;
        }
    }
    labels[e] = (uint8_t)best;
}

// the same interpolation written out: out [n, nc, H, W] fp32, one thread per element
__global__ __launch_bounds__(256) void head_mask_upsample_kernel(HmLogits L, int n, int H, int W, float* __restrict__ out) {
    const size_t total = (size_t)n * L.nc * H * W;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int X = (int)(e % W);
        size_t t = e / W;
        const int Y = (int)(t % H);
        t /= H;
        const int c = (int)(t % L.nc), img = (int)(t / L.nc);
        int y0, y1, x0, x1;
        double wy, wx;
        hm_lerp(Y, L.h, H, &y0, &y1, &wy);
        hm_lerp(X, L.w, W, &x0, &x1, &wx);
        const float* q = L.p + (long long)img * L.si + c * L.sc;
        const double v00 = q[y0 * L.sy + x0 * L.sx], v01 = q[y0 * L.sy + x1 * L.sx], v10 = q[y1 * L.sy + x0 * L.sx], v11 = q[y1 * L.sy + x1 * L.sx];
        out[e] = (float)((1.0 - wy) * ((1.0 - wx) * v00 + wx * v01) + wy * ((1.0 - wx) * v10 + wx * v11));
    }
}

// ---- frames ----------------------------------------------------------------------------------------------------------------------
// frames: bytes [n, H, W, 3], or floats [n, 3, H, W] in [0, 1] rounded once to bytes (floor(255 u + 0.5), clamped, NaN -> 0) ->
// rgb [n, H, W, 3] bytes and x [n, 3, H, W] = ToTensor + Normalize: (byte / 255 - mean) / std in fp32
__global__ __launch_bounds__(256) void head_mask_frames_kernel(const void* __restrict__ frames, int is_float, int n, int H, int W,
                                                               uint8_t* __restrict__ rgb, float* __restrict__ x) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * H * W) return;
    const size_t plane = (size_t)H * W, img = e / plane, px = e - img * plane;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int b;
        if (is_float) {
            float u = ((const float*)frames)[(img * 3 + c) * plane + px];
            if (!(u > 0.0f)) u = 0.0f;
            if (u > 1.0f) u = 1.0f;
            b = (int)floorf(255.0f * u + 0.5f);
        } else {
            b = ((const uint8_t*)frames)[e * 3 + c];
        }
        rgb[e * 3 + c] = (uint8_t)b;
        x[(img * 3 + c) * plane + px] = ((float)b / 255.0f - mean[c]) / sd[c];
    }
}

// src bytes [n, Hs, Ws, C] -> dst [n, Hd, Wd, C]: bilinear with half-pixel centres (conv_net_core.h's cn_bilinear), float64, rounded to
// the nearest byte.  An equal size is a copy.  OpenCV's fixed-point INTER_LINEAR is not reproduced.
__global__ __launch_bounds__(256) void head_mask_resize_kernel(const uint8_t* __restrict__ src, int n, int Hs, int Ws, int C, int Hd, int Wd,
                                                               uint8_t* __restrict__ dst) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * Hd * Wd * C) return;
    const int c = (int)(e % C);
    int img, y, x;
    cn_cell(e / C, Hd, Wd, &img, &y, &x);
    int y0, y1, x0, x1;
    double wy, wx;
    cn_bilinear(y, Hs, Hd, &y0, &y1, &wy);
    cn_bilinear(x, Ws, Wd, &x0, &x1, &wx);
    const uint8_t* p = src + (size_t)img * Hs * Ws * C + c;
    const double v00 = p[((size_t)y0 * Ws + x0) * C], v01 = p[((size_t)y0 * Ws + x1) * C], v10 = p[((size_t)y1 * Ws + x0) * C], v11 = p[((size_t)y1 * Ws + x1) * C];
    const double v = (1.0 - wy) * ((1.0 - wx) * v00 + wx * v01) + wy * ((1.0 - wx) * v10 + wx * v11);
    dst[e] = (uint8_t)(int)floor(v + 0.5);
}

// ---- the post-process: bytes and integers ----------------------------------------------------------------------------------------
// eye = 255 where the label is 4 or 5; work = lut[label]
__global__ __launch_bounds__(256) void head_mask_lut_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ lut, size_t total,
                                                            uint8_t* __restrict__ work, uint8_t* __restrict__ eye) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const uint8_t l = labels[e];
    work[e] = lut[l];
    eye[e] = (l == 4 || l == 5) ? 255 : 0;
}

// dst = the maximum of src over the non-zero taps of elem [eh, ew] anchored at (ay, ax) that lie inside the map
__global__ __launch_bounds__(256) void head_mask_dilate_kernel(const uint8_t* __restrict__ src, int n, int H, int W, const uint8_t* __restrict__ elem,
                                                               int eh, int ew, int ay, int ax, uint8_t* __restrict__ dst) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * H * W) return;
    int img, y, x;
    cn_cell(e, H, W, &img, &y, &x);
    const uint8_t* p = src + (size_t)img * H * W;
    int v = 0;
    for (int i = 0; i < eh; ++i) {
        const int yy = y + i - ay;
        if (yy < 0 || yy >= H) continue;
        for (int j = 0; j < ew; ++j) {
            const int xx = x + j - ax;
            if (xx < 0 || xx >= W || !elem[i * ew + j]) continue;
            const int t = p[(size_t)yy * W + xx];
            v = t > v ? t : v;
        }
    }
    dst[e] = (uint8_t)v;
}

// union-find over each image's grid; parent holds raster indices within the image, -1 on a zero pixel
__device__ __forceinline__ int hm_find(volatile int* parent, int x) {
    int p = parent[x];
    while (p != x) {
        x = p;
        p = parent[x];
    }
    return x;
}

__global__ __launch_bounds__(256) void head_mask_cc_init_kernel(const uint8_t* __restrict__ work, int n, int HW, int* __restrict__ parent,
                                                                int* __restrict__ area, unsigned long long* __restrict__ best) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (size_t)n) best[e] = ~0ull;
    if (e >= (size_t)n * HW) return;
    parent[e] = work[e] ? (int)(e % (size_t)HW) : -1;
    area[e] = 0;
}

// merge every non-zero pixel with its W, NW, N and NE neighbours: the larger root is hung under the smaller with atomicMin, so a
// component's final root is its smallest raster index whatever the schedule
__global__ __launch_bounds__(256) void head_mask_cc_merge_kernel(const uint8_t* __restrict__ work, int n, int H, int W, int* __restrict__ parent) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * H * W || !work[e]) return;
    int img, y, x;
    cn_cell(e, H, W, &img, &y, &x);
    const uint8_t* wk = work + (size_t)img * H * W;
    int* par = parent + (size_t)img * H * W;
    const int dy[4] = {0, -1, -1, -1}, dx[4] = {-1, -1, 0, 1};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int yy = y + dy[t], xx = x + dx[t];
        if (yy < 0 || xx < 0 || xx >= W || !wk[yy * W + xx]) continue;
        int a = y * W + x, b = yy * W + xx;
        for (;;) {
            a = hm_find(par, a);
            b = hm_find(par, b);
            if (a == b) break;
            if (a < b) {
                const int s = a;
                a = b;
                b = s;
            }
            const int old = atomicMin(&par[a], b);  // a > b: hang root a under b
            if (old == a) break;
            a = old;  // a was no root any more: go on from what it pointed to
        }
    }
}

// parent = root; the root's area counts its pixels
__global__ __launch_bounds__(256) void head_mask_cc_count_kernel(int n, int HW, int* __restrict__ parent, int* __restrict__ area) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * HW) return;
    const size_t img = e / (size_t)HW;
    int* par = parent + img * HW;
    const int x = (int)(e - img * HW);
    if (par[x] < 0) return;
    const int root = hm_find(par, x);
    par[x] = root;  // a reader passing through sees the old link or the root: both lead to the root
    atomicAdd(&area[img * HW + root], 1);
}

// the largest area wins, a tie goes to the smaller root: the minimum of (HW - area, root)
__global__ __launch_bounds__(256) void head_mask_cc_pick_kernel(int n, int HW, const int* __restrict__ parent, const int* __restrict__ area,
                                                                unsigned long long* __restrict__ best) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * HW) return;
    const size_t img = e / (size_t)HW;
    const int x = (int)(e - img * HW);
    if (parent[e] != x) return;
    atomicMin(&best[img], ((unsigned long long)(unsigned)(HW - area[e]) << 32) | (unsigned)x);
}

// keep the picked component's pixels.  final = 0 (the first pass): work keeps its values there, orig gets a copy and t the erosion's
// working image (face 1 -> 2, hair 2 -> 1).  final = 1: head = 255 on a kept pixel that the hue filter does not clear, eye = eye_in & head.
__global__ __launch_bounds__(256) void head_mask_cc_apply_kernel(int n, int HW, const int* __restrict__ parent, const unsigned long long* __restrict__ best,
                                                                 uint8_t* __restrict__ work, uint8_t* __restrict__ orig, uint8_t* __restrict__ t, int final,
                                                                 const uint8_t* __restrict__ rgb, int hue_lo, int hue_hi, const uint8_t* __restrict__ eye_in,
                                                                 uint8_t* __restrict__ head, uint8_t* __restrict__ eye) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * HW) return;
    const size_t img = e / (size_t)HW;
    const int root = (int)(unsigned)(best[img] & 0xffffffffull);
    const uint8_t v = (parent[e] >= 0 && parent[e] == root) ? work[e] : 0;
    if (!final) {
        work[e] = v;
        orig[e] = v;
        t[e] = v == 1 ? 2 : v == 2 ? 1 : v;
        return;
    }
    const int hue = hm_hue(rgb[e * 3], rgb[e * 3 + 1], rgb[e * 3 + 2]);  // the true R where OpenCV expects B: the reference's call
    const uint8_t hd = (v && !(hue >= hue_lo && hue <= hue_hi)) ? 255 : 0;
    head[e] = hd;
    eye[e] = eye_in[e] & hd;
}

// one Jacobi pass of the hair erosion: a pixel whose ORIGINAL label is hair (2) is zeroed when N + S + E + W < 4 centre, zero border
__global__ __launch_bounds__(256) void head_mask_erode_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ orig, int n, int H, int W,
                                                              uint8_t* __restrict__ dst) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * H * W) return;
    int img, y, x;
    cn_cell(e, H, W, &img, &y, &x);
    const uint8_t* p = src + (size_t)img * H * W;
    const int c = p[y * W + x];
    const int sum = (y > 0 ? p[(y - 1) * W + x] : 0) + (y < H - 1 ? p[(y + 1) * W + x] : 0) + (x > 0 ? p[y * W + x - 1] : 0) + (x < W - 1 ? p[y * W + x + 1] : 0);
    dst[e] = (orig[e] == 2 && sum < 4 * c) ? 0 : (uint8_t)c;
}

// the erosion's working image back to labels: 1 -> 2 (hair), 2 -> 1 (face)
__global__ __launch_bounds__(256) void head_mask_unswap_kernel(const uint8_t* __restrict__ src, size_t total, uint8_t* __restrict__ dst) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const uint8_t v = src[e];
    dst[e] = v == 1 ? 2 : v == 2 ? 1 : v;
}

__global__ __launch_bounds__(256) void head_mask_green_kernel(const uint8_t* __restrict__ rgb, size_t total, int hue_lo, int hue_hi, uint8_t* __restrict__ cleared) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int hue = hm_hue(rgb[e * 3], rgb[e * 3 + 1], rgb[e * 3 + 2]);
    cleared[e] = (hue >= hue_lo && hue <= hue_hi) ? 255 : 0;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline unsigned hm_blocks(size_t work) { return (unsigned)((work + 255) / 256); }

extern "C" size_t n3dt_head_mask_packed_layout_bytes(void) { return hm_layout().total; }
extern "C" size_t n3dt_head_mask_ws_bytes(int n, int H, int W) { return hm_workspace(n, H, W).total; }
extern "C" size_t n3dt_head_mask_block_ws_bytes(int block, int n, int Hi, int Wi, int Hs, int Ws) { return hm_block_ws(block, n, Hi, Wi, Hs, Ws).total; }
extern "C" size_t n3dt_head_mask_post_ws_bytes(int n, int H, int W) { return hm_post_ws(n, H, W).total; }

extern "C" void n3dt_launch_head_mask_pack(const N3dtHeadMaskParams* p, void* packed, hipStream_t st) {
    const HmPackLayout L = hm_layout();
    char* base = (char*)packed;
    for (int j = 0; j < HM_CONVS; ++j) {
        const HmConv t = HM_TABLE[j];
        const int cout = hm_cout(j, p->n_classes), np = hm_np(j);
        const float* gamma = t.bn ? p->bn_weight[j] : nullptr;
        if (t.kind == HM_SMALL) {
            head_mask_pack_small_kernel<<<hm_blocks((size_t)t.cin * cout), 256, 0, st>>>(p->weight[j], gamma, p->bn_var[j], p->bn_eps, t.cin, cout,
                                                                                         (float*)(base + L.w[j]));
        } else {
            __bf16* hi = (__bf16*)(base + L.w[j]);
            conv_net_pack(p->weight[j], gamma, p->bn_var[j], p->bn_eps, t.cin, t.cin, t.cin, cout, np, t.k * t.k, hm_K(j), t.kind == HM_STEM, hi,
                          hi + L.elems[j], st);
        }
        conv_net_shift_bn(gamma, p->bn_bias[j], p->bn_mean[j], p->bn_var[j], p->bn_eps, np, (float*)(base + L.bias[j]), st);
    }
}

// the spatial convolution j of step t on maps given as pointers
static void hm_conv_launch(int j, int n, const HmStep& t, const void* packed, const float* in, const float* in2, const float* skip, const float* addmap,
                           const float* scale, const float* addvec, int vstride, float* out, hipStream_t st) {
    const HmPackLayout L = hm_layout();
    const HmConv c = HM_TABLE[j];
    const char* pk = (const char*)packed;
    HmConvArgs a;
    a.in = in; a.in2 = in2; a.skip = skip; a.addmap = addmap; a.scale = scale; a.addvec = addvec;
    a.whi = (const __bf16*)(pk + L.w[j]);
    a.wlo = a.whi + L.elems[j];
    a.bias = (const float*)(pk + L.bias[j]);
    a.out = out;
    a.n = n; a.Hs = t.Hs; a.Ws = t.Ws; a.Hi = t.Hi; a.Wi = t.Wi;
    a.Ho = hm_out_h(j, t.Hi); a.Wo = hm_out_h(j, t.Wi);
    a.cin = c.cin; a.csplit = in2 ? c.cin / 2 : c.cin; a.np = hm_np(j); a.k = c.k; a.stride = c.stride; a.pad = c.pad;
    a.relu = c.act == HM_RELU; a.addself = t.addself; a.vstride = vstride;
    const size_t M = (size_t)n * a.Ho * a.Wo;
    const int nt = cn_wave_ntiles((long long)M, a.np);
    const size_t tiles = (M + CN_TILE_M - 1) / CN_TILE_M * (a.np / (32 * nt));
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    if (c.kind == HM_STEM) {
        if (nt == 1) head_mask_conv_kernel<1, HM_STEMK><<<grid, 256, 0, st>>>(a);
        else head_mask_conv_kernel<2, HM_STEMK><<<grid, 256, 0, st>>>(a);
    } else if (scale) {
        if (nt == 1) head_mask_conv_kernel<1, HM_XFORM><<<grid, 256, 0, st>>>(a);
        else head_mask_conv_kernel<2, HM_XFORM><<<grid, 256, 0, st>>>(a);
    } else {
        if (nt == 1) head_mask_conv_kernel<1, HM_PLAIN><<<grid, 256, 0, st>>>(a);
        else head_mask_conv_kernel<2, HM_PLAIN><<<grid, 256, 0, st>>>(a);
    }
}

static void hm_small_launch(int j, int n, int n_classes, const void* packed, const float* in, int HW, size_t in_stride, float* out, int out_stride,
                            hipStream_t st) {
    const HmPackLayout L = hm_layout();
    const char* pk = (const char*)packed;
    head_mask_small_kernel<<<n, 256, 0, st>>>(in, HW, HM_TABLE[j].cin, in_stride, (const float*)(pk + L.w[j]), (const float*)(pk + L.bias[j]),
                                              hm_cout(j, n_classes), HM_TABLE[j].act, out, out_stride);
}

static HmLogits hm_nhwc_logits(const float* p, int nc, int h, int w) {
    HmLogits L;
    L.p = p; L.nc = nc; L.h = h; L.w = w;
    L.sc = 1; L.sx = HM_MAX_CLASSES; L.sy = (long long)w * HM_MAX_CLASSES; L.si = (long long)h * L.sy;
    return L;
}

// x [n, 3, H, W] -> for each output o in `outputs` out[o]: [n, n_classes, h_o, w_o], or [n, n_classes, H, W] where `upsample`
extern "C" void n3dt_launch_head_mask_fwd(int n, int H, int W, int n_classes, const void* packed, const float* x, int outputs, int upsample,
                                          float* const* out, void* workspace, hipStream_t st) {
    const HmWorkspace w = hm_workspace(n, H, W);
    char* ws = (char*)workspace;
    float* region[HM_REGIONS];
    for (int r = 0; r < HM_REGIONS; ++r) region[r] = (float*)(ws + w.region[r]);
    float* vec = region[HM_R_VEC];
    conv_net_to_nhwc(x, n, 3, H, W, 3, 3, region[HM_R_IMG], 3, st);
    HmStep steps[HM_MAX_STEPS];
    const int count = hm_chain(H, W, outputs, steps);
    for (int s = 0; s < count; ++s) {
        const HmStep t = steps[s];
        if (t.block == HM_POOL_BLOCK) {
            conv_net_max_pool(region[t.in], n, t.Hi, t.Wi, 64, region[t.out], st);
        } else if (HM_TABLE[t.block].kind == HM_SMALL) {
            if (t.invec >= 0) hm_small_launch(t.block, n, n_classes, packed, vec + t.invec, 1, HM_VEC, vec + t.out, HM_VEC, st);
            else hm_small_launch(t.block, n, n_classes, packed, region[t.in], t.Hi * t.Wi, (size_t)t.Hi * t.Wi * HM_TABLE[t.block].cin, vec + t.out, HM_VEC, st);
        } else {
            hm_conv_launch(t.block, n, t, packed, region[t.in], t.in2 < 0 ? nullptr : region[t.in2], t.skip < 0 ? nullptr : region[t.skip],
                           t.addmap < 0 ? nullptr : region[t.addmap], t.scale < 0 ? nullptr : vec + t.scale, t.addvec < 0 ? nullptr : vec + t.addvec, HM_VEC,
                           region[t.out], st);
        }
    }
    for (int o = 0; o < 3; ++o) {
        if (!(outputs & (1 << o))) continue;
        int h, wd;
        hm_logit_hw(H, W, o, &h, &wd);
        const float* lg = region[HM_R_LOG0 + o];
        if (upsample) head_mask_upsample_kernel<<<conv_grid((size_t)n * n_classes * H * W), 256, 0, st>>>(hm_nhwc_logits(lg, n_classes, h, wd), n, H, W, out[o]);
        else conv_net_to_nchw(lg, HM_MAX_CLASSES, n, n_classes, h, wd, 0, out[o], st);
    }
}

// One block alone.  in [n, C_in, Hs, Ws] (the stem, the pool and the small blocks: [n, C_in, Hi, Wi]) -> out [n, C_out, Ho, Wo], a
// small block [n, C_out].  aux: the shortcut [n, C_out, Ho, Wo] of a BasicBlock's second convolution; the second half of the
// channels [n, 128, Hi, Wi] of ffm.convblk; with a scale, conv_head16's added map [n, 128, Hs, Ws].  scale, addvec: [n, C_in];
// conv_out.conv with a scale adds the value itself.
extern "C" void n3dt_launch_head_mask_block(int block, int n, int Hi, int Wi, int Hs, int Ws, int n_classes, const void* packed, const float* in,
                                            const float* aux, const float* scale, const float* addvec, float* out, void* workspace, hipStream_t st) {
    const HmBlockWs w = hm_block_ws(block, n, Hi, Wi, Hs, Ws);
    float* map0 = (float*)((char*)workspace + w.in);
    float* map1 = (float*)((char*)workspace + w.aux);
    float* map2 = (float*)((char*)workspace + w.out);
    if (block == HM_POOL_BLOCK) {
        conv_net_to_nhwc(in, n, 64, Hi, Wi, 0, 64, map0, 64, st);
        conv_net_max_pool(map0, n, Hi, Wi, 64, map2, st);
        conv_net_to_nchw(map2, 64, n, 64, cn_pool_out(Hi), cn_pool_out(Wi), 0, out, st);
        return;
    }
    const HmConv c = HM_TABLE[block];
    if (c.kind == HM_SMALL) {
        conv_net_to_nhwc(in, n, c.cin, Hi, Wi, 0, c.cin, map0, c.cin, st);
        hm_small_launch(block, n, n_classes, packed, map0, Hi * Wi, (size_t)Hi * Wi * c.cin, out, c.cout, st);
        return;
    }
    HmStep t = hm_step(block, Hi, Wi, 0, 0);
    const int Ho = hm_out_h(block, Hi), Wo = hm_out_h(block, Wi), np = hm_np(block), cout = hm_cout(block, n_classes);
    const float *in2 = nullptr, *skip = nullptr, *addmap = nullptr;
    if (c.kind == HM_STEM) {
        conv_net_to_nhwc(in, n, 3, Hi, Wi, 3, 3, map0, 3, st);
    } else {
        t.Hs = Hs;
        t.Ws = Ws;
        const int cin0 = block == HM_FFM_BLK ? c.cin / 2 : c.cin;
        conv_net_to_nhwc(in, n, cin0, Hs, Ws, 0, cin0, map0, cin0, st);
        if (block == HM_FFM_BLK) {
            conv_net_to_nhwc(aux, n, cin0, Hs, Ws, 0, cin0, map1, cin0, st);
            in2 = map1;
        } else if (hm_takes_skip(block)) {
            conv_net_to_nhwc(aux, n, np, Ho, Wo, 0, np, map1, np, st);
            skip = map1;
        } else if (block == HM_HEAD16 && scale && aux) {
            conv_net_to_nhwc(aux, n, c.cin, Hs, Ws, 0, c.cin, map1, c.cin, st);
            addmap = map1;
        }
        t.addself = block == HM_OUT && scale;
    }
    hm_conv_launch(block, n, t, packed, map0, in2, skip, addmap, scale, addvec, c.cin, map2, st);
    conv_net_to_nchw(map2, np, n, cout, Ho, Wo, 0, out, st);
}

extern "C" void n3dt_launch_head_mask_frames(int n, int H, int W, const void* frames, int is_float, uint8_t* rgb, float* x, hipStream_t st) {
    head_mask_frames_kernel<<<hm_blocks((size_t)n * H * W), 256, 0, st>>>(frames, is_float, n, H, W, rgb, x);
}

extern "C" void n3dt_launch_head_mask_resize(int n, int Hs, int Ws, int C, const uint8_t* src, int Hd, int Wd, uint8_t* dst, hipStream_t st) {
    head_mask_resize_kernel<<<hm_blocks((size_t)n * Hd * Wd * C), 256, 0, st>>>(src, n, Hs, Ws, C, Hd, Wd, dst);
}

// logits [n, nc, h, w] -> labels [n, H, W]
extern "C" void n3dt_launch_head_mask_labels(int n, int nc, int h, int w, int H, int W, const float* logits, uint8_t* labels, hipStream_t st) {
    HmLogits L;
    L.p = logits; L.nc = nc; L.h = h; L.w = w;
    L.sx = 1; L.sy = w; L.sc = (long long)h * w; L.si = L.sc * nc;
    head_mask_labels_kernel<<<hm_blocks((size_t)n * H * W), 256, 0, st>>>(L, n, H, W, labels);
}

extern "C" void n3dt_launch_head_mask_green(int n, int H, int W, const uint8_t* rgb, int hue_lo, int hue_hi, uint8_t* cleared, hipStream_t st) {
    head_mask_green_kernel<<<hm_blocks((size_t)n * H * W), 256, 0, st>>>(rgb, (size_t)n * H * W, hue_lo, hue_hi, cleared);
}

// keep the largest 8-connected component of work's non-zero pixels
static void hm_components(int n, int H, int W, const HmPostWs& w, char* ws, uint8_t* work, uint8_t* orig, uint8_t* t, int final, const uint8_t* rgb,
                          int hue_lo, int hue_hi, const uint8_t* eye_in, uint8_t* head, uint8_t* eye, hipStream_t st) {
    int* parent = (int*)(ws + w.parent);
    int* area = (int*)(ws + w.area);
    unsigned long long* best = (unsigned long long*)(ws + w.best);
    const int HW = H * W;
    const unsigned grid = hm_blocks((size_t)n * HW);
    head_mask_cc_init_kernel<<<grid, 256, 0, st>>>(work, n, HW, parent, area, best);
    head_mask_cc_merge_kernel<<<grid, 256, 0, st>>>(work, n, H, W, parent);
    head_mask_cc_count_kernel<<<grid, 256, 0, st>>>(n, HW, parent, area);
    head_mask_cc_pick_kernel<<<grid, 256, 0, st>>>(n, HW, parent, area, best);
    head_mask_cc_apply_kernel<<<grid, 256, 0, st>>>(n, HW, parent, best, work, orig, t, final, rgb, hue_lo, hue_hi, eye_in, head, eye);
}

// labels [n, H, W], rgb [n, H, W, 3] -> head, eye [n, H, W] in {0, 255}.  The caller's `eye` holds the undilated eye mask until the
// last kernel; the dilations run in the erosion's two buffers once the erosion is done with them.
extern "C" void n3dt_launch_head_mask_postprocess(int n, int H, int W, const uint8_t* labels, const uint8_t* rgb, const uint8_t* lut, const uint8_t* element,
                                                  int eh, int ew, int ay, int ax, int dilations, int erosions, int hue_lo, int hue_hi, uint8_t* head,
                                                  uint8_t* eye, void* workspace, hipStream_t st) {
    const HmPostWs w = hm_post_ws(n, H, W);
    char* ws = (char*)workspace;
    uint8_t* work = (uint8_t*)(ws + w.work);
    uint8_t* orig = (uint8_t*)(ws + w.orig);
    uint8_t* a = (uint8_t*)(ws + w.a);
    uint8_t* b = (uint8_t*)(ws + w.b);
    const size_t px = (size_t)n * H * W;
    const unsigned grid = hm_blocks(px);
    head_mask_lut_kernel<<<grid, 256, 0, st>>>(labels, lut, px, work, eye);
    hm_components(n, H, W, w, ws, work, orig, a, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, st);
    uint8_t *src = a, *dst = b;
    for (int i = 0; i < erosions; ++i) {
        head_mask_erode_kernel<<<grid, 256, 0, st>>>(src, orig, n, H, W, dst);
        uint8_t* s = src;
        src = dst;
        dst = s;
    }
    head_mask_unswap_kernel<<<grid, 256, 0, st>>>(src, px, work);
    const uint8_t* e_src = eye;
    uint8_t* bufs[2] = {a, b};
    for (int i = 0; i < dilations; ++i) {
        head_mask_dilate_kernel<<<grid, 256, 0, st>>>(e_src, n, H, W, element, eh, ew, ay, ax, bufs[i & 1]);
        e_src = bufs[i & 1];
    }
    if (dilations == 0) {
        head_mask_unswap_kernel<<<grid, 256, 0, st>>>(eye, px, a);  // {0, 255} pass through unchanged: a plain copy
        e_src = a;
    }
    hm_components(n, H, W, w, ws, work, nullptr, nullptr, 1, rgb, hue_lo, hue_hi, e_src, head, eye, st);
}
