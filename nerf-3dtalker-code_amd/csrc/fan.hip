// The AWing FAN landmark detector, frozen and inference-only (include/n3dt.h, n3dt_fan_*; the reference's
// s_face3d/util/my_awing_arch.py -- FAN over HourGlass, ConvBlock and CoordConvTh, calculate_points behind it -- as
// s_face3d/extract_kp_videos_safe.py's KeypointExtractor runs it).  The table, the launch plan and every index
// rule that can go wrong at an edge come from fan_core.h, which tests/fan_core_host.cpp also compiles and walks.  That program
// re-types the loop nest of the convolution kernel below (block / wave / lane / tap / K step): a change to that loop here must be
// made there too.
//
//   crops      frames [n,3,H,W] fp32 RGB + boxes -> [n,3,256,256] BGR, bilinear with half-pixel centres, float64 per output pixel
//   conv       every convolution of the table (1 x 1, 3 x 3, the 7 x 7 / 2 stem) as one implicit GEMM on v_mfma_f32_32x32x16_bf16:
//              M = pixels of the output map, N = C_out padded to 32, k = tap * C_in + c_in (the stem: (tap, channel) flattened, 147
//              padded to 160); every operand split x = hi + lo, three products, fp32 accumulation: conv_mfma.h's step in its split
//              form.  The A fetch applies a ConvBlock's pre-activation relu(g x + b) and predicates a tap outside the map to zero
//              BEHIND it; the epilogue adds the bias, the coordinate channels' constant maps (the second one gated), stores the raw
//              value for the block's next convolution, adds the residual's channel slice, and stores into a channel slice.
//   pool       2 x 2 average;  upadd: upper branch + nearest x 2 of the lower
//   gate       min(max(v, 0), 1) > 0.05f of a stack's last heat-map channel, one byte per cell
//   points     calculate_points as get_landmarks calls it (B = 1: every rule per frame), one workgroup per frame, float64
//   tail       scale by the crop, 98 -> 68 through a table, the box's origin, the carry-forward
//
// Every image goes through identical code with the same K order, no split-K and no atomics: an image's result depends neither on
// its position in the batch nor on the batch size.  Every element of every map is written exactly once per forward; nothing is
// cleared.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/n3dt.h"
#include "conv_mfma.h"
#include "conv_net.h"
#include "fan_core.h"
#include "n3dt_launch.h"

// ---- packed weights ----------------------------------------------------------------------------------------------------------------
// Per convolution one B matrix in conv_frag.h's fragment order, hi then lo (a folded BatchNorm's scale inside), the fp32 bias
// vector [np] and the pre-activation's (g, b) [2][cinp]; then the stem's coordinate map [128,128,64] and per stack the hourglass
// CoordConv's [64,64,256] maps: xx, yy, rr (+ bias), and from the second stack on the gated xx, yy.
struct FanLayout {
    size_t w[FAN_MAX_CONVS], elems[FAN_MAX_CONVS], bias[FAN_MAX_CONVS], pre[FAN_MAX_CONVS];
    size_t stem_map, map1[FAN_MAX_MODULES], map2[FAN_MAX_MODULES], total;
};

static FanLayout fan_layout(int modules, int N) {
    FanLayout L;
    size_t off = 0;
    for (int j = 0; j < FAN_MAX_CONVS; ++j) {
        L.w[j] = L.elems[j] = L.bias[j] = L.pre[j] = 0;
        if (!fan_conv_exists(j, modules)) continue;
        const FanConv c = fan_conv(j, N);
        L.elems[j] = (size_t)fan_K(&c) * fan_np(&c);
        L.w[j] = off;
        off = rup(off + L.elems[j] * 2 * sizeof(__bf16), 256);
        L.bias[j] = off;
        off = rup(off + fan_np(&c) * sizeof(float), 256);
        L.pre[j] = off;
        off = rup(off + 2 * (size_t)fan_cinp(&c) * sizeof(float), 256);
    }
    L.stem_map = off;
    off += (size_t)FAN_STEM_HW * FAN_STEM_HW * 64 * sizeof(float);
    for (int s = 0; s < FAN_MAX_MODULES; ++s) {
        L.map1[s] = L.map2[s] = 0;
        if (s >= modules) continue;
        L.map1[s] = off;
        off += (size_t)FAN_CELLS * 256 * sizeof(float);
        if (s > 0) {
            L.map2[s] = off;
            off += (size_t)FAN_CELLS * 256 * sizeof(float);
        }
    }
    L.total = off;
    return L;
}

// The pack is conv_net.hip's: W [cout, wc, k, k] (wc >= cin channels: a CoordConv's weight also holds the coordinate channels) ->
// B [K][np], row k = tap * cinp + ci (the stem: (ky * 7 + kx) * 3 + ci, rows 147 .. 159 zero); rows of padded channels and columns
// from cout on are zero; each weight times its column's folded BatchNorm scale (post) in float64, rounded once to fp32, then split.

// the bias vector [np] -- kind LAST: s (b - mean) + beta; STEM and COORD: 0 (their bias lies in the coordinate map); else the
// convolution's own bias or 0 -- and the pre-activation's g = gamma / sqrt(var + eps), b = beta - mean g, [2][cinp], 0 past cin
__global__ __launch_bounds__(256) void fan_vec_kernel(const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ mean, const float* __restrict__ var, int kind, int pre, int cin, int cinp,
                                                      int cout, int np, float* __restrict__ dbias, float* __restrict__ dpre) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < np) {
        double v = 0.0;
        if (i < cout && bias && kind != FAN_STEM && kind != FAN_COORD) {
            v = (double)bias[i];
            if (kind == FAN_LAST) v = (v - (double)mean[i]) * conv_bn_scale(gamma, var, FAN_BN_EPS, i) + (double)beta[i];
        }
        dbias[i] = (float)v;
    }
    if (i < cinp) {
        double g = 0.0, b = 0.0;
        if (pre && i < cin) {
            g = conv_bn_scale(gamma, var, FAN_BN_EPS, i);
            b = (double)beta[i] - (double)mean[i] * g;
        }
        dpre[i] = (float)g;
        dpre[cinp + i] = (float)b;
    }
}

// the stem's coordinate channels, bias and bn1 as a constant map [128, 128, 64]: s (sum over the taps inside the image of
// W[co][3 + c] coords[c] + bias - mean) + beta, float64, rounded once.  coords [3, 256, 256]: xx, yy, rr.
__global__ __launch_bounds__(256) void fan_stem_map_kernel(const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                                                           const float* __restrict__ coords, float* __restrict__ map) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)FAN_STEM_HW * FAN_STEM_HW * 64) return;
    const int co = (int)(e % 64), x = (int)(e / 64 % FAN_STEM_HW), y = (int)(e / 64 / FAN_STEM_HW);
    double s = 0.0;
    for (int c = 0; c < 3; ++c)
        for (int ky = 0; ky < 7; ++ky)
            for (int kx = 0; kx < 7; ++kx) {
                const int iy = fan_tap_pixel(y, ky, 2, 3), ix = fan_tap_pixel(x, kx, 2, 3);
                if (fan_inside(iy, ix, FAN_IMG, FAN_IMG))
                    s += (double)W[((size_t)co * 6 + 3 + c) * 49 + ky * 7 + kx] * (double)coords[((size_t)c * FAN_IMG + iy) * FAN_IMG + ix];
            }
    map[e] = (float)((s + (double)bias[co] - (double)mean[co]) * conv_bn_scale(gamma, var, FAN_BN_EPS, co) + (double)beta[co]);
}

// the hourglass CoordConv's coordinate channels: map1 [4096, 256] = W[co][256..258] . (xx, yy, rr) + bias, and (gated) map2 =
// W[co][259..260] . (xx, yy); W [256, wc]; coords [3, 64, 64]
__global__ __launch_bounds__(256) void fan_coord_map_kernel(const float* __restrict__ W, const float* __restrict__ bias, int wc,
                                                            const float* __restrict__ coords, float* __restrict__ map1, float* __restrict__ map2) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)FAN_CELLS * 256) return;
    const int co = (int)(e % 256), cell = (int)(e / 256);
    const float* w = W + (size_t)co * wc + 256;
    const double xx = coords[cell], yy = coords[FAN_CELLS + cell], rr = coords[2 * FAN_CELLS + cell];
    map1[e] = (float)((double)w[0] * xx + (double)w[1] * yy + (double)w[2] * rr + (double)bias[co]);
    if (map2) map2[e] = (float)((double)w[3] * xx + (double)w[4] * yy);
}

// layouts: conv_net.hip's, with no halo and the channels padded to the map's cs

// ---- implicit-GEMM convolution -----------------------------------------------------------------------------------------------------
struct FanConvArgs {
    const float* in;      // [n, Hi, Wi, in_cs], already at the slice's first channel
    const __bf16* whi;    // packed B matrix (hi), [K/16][np/32][64][8]
    const __bf16* wlo;
    const float* bias;    // [np]
    const float* pre;     // [2][cin]: g, b of relu(g x + b), or NULL
    const float* map1;    // [Ho Wo, np] added to every image, or NULL
    const float* map2;    // [Ho Wo, np] added where the cell's gate is set, or NULL
    const uint8_t* gate;  // cell (img, y, x) at gate[img * gate_stride + y * Wo + x]
    const float* skip;    // [n, Ho, Wo, skip_cs] at the slice's first channel, or NULL
    float* out;           // [n, Ho, Wo, out_cs] at the slice's first channel
    float* raw;           // [n, Ho, Wo, raw_cs]: the value in front of the skip, or NULL
    long long gate_stride;
    int n, Hi, Wi, Ho, Wo, cin, in_cs, np, cstore, out_cs, skip_cs, raw_cs, k, stride, pad, relu;
};

// 256 threads = 4 waves; wave tile t = 4 blockIdx.x + wave computes CN_TILE_M pixels x 32 NT columns, the column tile fastest.
// A k-step is 16 channels of one tap (cin % 16 == 0); STEM: 16 consecutive k of the flattened (tap, channel), those from 147 on
// zero against zero weight rows.  Kernel size, stride and every map size are run-time arguments; the row index is 64-bit.  Columns
// from cstore on are not stored (a heat map keeps N + 1 padded to 16 of its 32-padded columns; the padding columns are 0).
template <int NT, bool STEM>
__global__ __launch_bounds__(256) void fan_conv_kernel(FanConvArgs a) {
    const ConvWaveTile t = conv_wave_tile<NT>(a.np, a.n, a.Ho, a.Wo);
    if (t.idle()) return;  // no barriers in this kernel: an idle wave may leave
    const int lane = t.lane, r = t.r, h = t.h, nt0 = t.nt0(NT);
    const long long M = t.M, m0 = t.m0;
    const float* base[2];
    int y0[2], x0[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int img, y, x;
        cn_row_cell(m0 + mt * 32 + r, M, a.Ho, a.Wo, &img, &y, &x);  // rows past M compute the last pixel again and are never stored
        base[mt] = a.in + (size_t)img * a.Hi * a.Wi * a.in_cs;
        y0[mt] = fan_tap_pixel(y, 0, a.stride, a.pad);
        x0[mt] = fan_tap_pixel(x, 0, a.stride, a.pad);
    }
    conv_f32x16 acc[2][NT];
    CONV_ZERO_ACC(acc, NT);
    float av[2][8];

    if (STEM) {
        for (int s = 0; s < CN_STEM_KP / 16; ++s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * h + j;
                int ky, kx, c;
                cn_stem_tap(k < CN_STEM_K ? k : 0, &ky, &kx, &c);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const int iy = y0[mt] + ky, ix = x0[mt] + kx;
                    float v = 0.0f;
                    if (k < CN_STEM_K && fan_inside(iy, ix, a.Hi, a.Wi)) v = base[mt][((size_t)iy * a.Wi + ix) * 3 + c];
                    av[mt][j] = v;
                }
            }
            conv_mma_step<true, NT>(a.whi, a.wlo, a.np, s, nt0, lane, av, acc);
        }
    } else {
        int s = 0;
        for (int tap = 0; tap < a.k * a.k; ++tap) {
            const int ky = tap / a.k, kx = tap - ky * a.k;
            const float* p[2];
            bool ok[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int iy = y0[mt] + ky, ix = x0[mt] + kx;
                ok[mt] = fan_inside(iy, ix, a.Hi, a.Wi);
                p[mt] = ok[mt] ? base[mt] + ((size_t)iy * a.Wi + ix) * a.in_cs + 8 * h : base[mt];
            }
            for (int c0 = 0; c0 < a.cin; c0 += 16, ++s) {
                float g[8], b[8];
                if (a.pre) {
                    conv_load8(a.pre + c0 + 8 * h, g);
                    conv_load8(a.pre + a.cin + c0 + 8 * h, b);
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    if (ok[mt]) {
                        conv_load8(p[mt] + c0, av[mt]);
                        if (a.pre) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                const float t = g[j] * av[mt][j] + b[j];
                                av[mt][j] = t > 0.0f ? t : 0.0f;
                            }
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j) av[mt][j] = 0.0f;  // the zero padding, behind the activation
                    }
                }
                conv_mma_step<true, NT>(a.whi, a.wlo, a.np, s, nt0, lane, av, acc);
            }
        }
    }

    // epilogue: accumulator register i of lane (r, h) is output row cf_acc_row(i, h), column r
    const long long hw = (long long)a.Ho * a.Wo;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long m = m0 + mt * 32 + cf_acc_row(i, h);
            if (m >= M) continue;
            const long long img = m / hw, cell = m - img * hw;
            const bool gated = a.map2 && a.gate[img * a.gate_stride + cell] != 0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int co = (nt0 + nt) * 32 + r;
                if (co >= a.cstore) continue;
                float v = acc[mt][nt][i] + a.bias[co];
                if (a.map1) v += a.map1[(size_t)cell * a.np + co];
                if (gated) v += a.map2[(size_t)cell * a.np + co];
                if (a.raw) a.raw[(size_t)m * a.raw_cs + co] = v;
                if (a.skip) v += a.skip[(size_t)m * a.skip_cs + co];
                if (a.relu) v = v > 0.0f ? v : 0.0f;
                a.out[(size_t)m * a.out_cs + co] = v;
            }
        }
}

// ---- pool, upsample-add, gate --------------------------------------------------------------------------------------------------------
// in [n, H, W, C] -> out [n, H / 2, W / 2, C]: the mean of the 2 x 2 window, summed in float64, rounded once.  Four channels a thread.
__global__ __launch_bounds__(256) void fan_pool_kernel(const float* __restrict__ in, int n, int H, int W, int C, float* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
    const size_t total = (size_t)n * Ho * Wo * C4;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % C4) * 4;
        size_t t = e / C4;
        const int xo = (int)(t % Wo);
        t /= Wo;
        const int yo = (int)(t % Ho);
        const size_t img = t / Ho;
        const float* p = in + ((img * H + 2 * yo) * W + 2 * xo) * C + c;
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + C);
        const float4 d = *reinterpret_cast<const float4*>(p + (size_t)W * C), f = *reinterpret_cast<const float4*>(p + (size_t)W * C + C);
        float4 v;
        v.x = (float)((((double)a.x + (double)b.x) + ((double)d.x + (double)f.x)) * 0.25);
        v.y = (float)((((double)a.y + (double)b.y) + ((double)d.y + (double)f.y)) * 0.25);
        v.z = (float)((((double)a.z + (double)b.z) + ((double)d.z + (double)f.z)) * 0.25);
        v.w = (float)((((double)a.w + (double)b.w) + ((double)d.w + (double)f.w)) * 0.25);
        *reinterpret_cast<float4*>(out + e * 4) = v;
    }
}

// out [n, H, W, C] = up [n, H, W, C] + low [n, H / 2, W / 2, C] at (y / 2, x / 2)
__global__ __launch_bounds__(256) void fan_upadd_kernel(const float* __restrict__ low, const float* __restrict__ up, int n, int H, int W, int C,
                                                        float* __restrict__ out) {
    const int C4 = C / 4;
    const size_t total = (size_t)n * H * W * C4;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % C4) * 4;
        size_t t = e / C4;
        const int x = (int)(t % W);
        t /= W;
        const int y = (int)(t % H);
        const size_t img = t / H;
        const float4 a = *reinterpret_cast<const float4*>(up + e * 4);
        const float4 b = *reinterpret_cast<const float4*>(low + ((img * (H / 2) + y / 2) * (W / 2) + x / 2) * C + c);
        float4 v;
        v.x = a.x + b.x; v.y = a.y + b.y; v.z = a.z + b.z; v.w = a.w + b.w;
        *reinterpret_cast<float4*>(out + e * 4) = v;
    }
}

// gates [n, slots, 4096] slot `slot` <- clamp(heat [n, 4096, cs] channel N, 0, 1) > 0.05f, the reference's fp32 comparison
__global__ __launch_bounds__(256) void fan_gate_kernel(const float* __restrict__ heat, int n, int cs, int N, int slots, int slot, uint8_t* __restrict__ gates) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * FAN_CELLS) return;
    const size_t img = e / FAN_CELLS, cell = e - img * FAN_CELLS;
    const float v = fminf(fmaxf(heat[e * cs + N], 0.0f), 1.0f);
    gates[(img * slots + slot) * FAN_CELLS + cell] = v > FAN_GATE_LEVEL ? 1 : 0;
}

// ---- crops -------------------------------------------------------------------------------------------------------------------------
// One thread per output pixel (frame, Y, X): the box's rows y1 .. y2 - 1 and columns x1 .. x2 - 1 resampled to 256 x 256 bilinearly
// with half-pixel centres (conv_net_core.h's cn_bilinear), float64, rounded once; RGB in, BGR out.  A bad box gives zeros.
__global__ __launch_bounds__(256) void fan_crop_kernel(int n, int H, int W, const float* __restrict__ frames, const int* __restrict__ boxes,
                                                       float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * FAN_IMG * FAN_IMG) return;
    const int X = (int)(e % FAN_IMG), Y = (int)(e / FAN_IMG % FAN_IMG);
    const size_t f = e / ((size_t)FAN_IMG * FAN_IMG), plane = (size_t)FAN_IMG * FAN_IMG;
    float* o = out + f * 3 * plane + (size_t)Y * FAN_IMG + X;
    const int* box = boxes + f * 4;
    if (!fan_box_ok(box, H, W)) {
        o[0] = o[plane] = o[2 * plane] = 0.0f;
        return;
    }
    int ya, yb, xa, xb;
    double wy, wx;
    cn_bilinear(Y, box[1] - box[0], FAN_IMG, &ya, &yb, &wy);
    cn_bilinear(X, box[3] - box[2], FAN_IMG, &xa, &xb, &wx);
    ya += box[0]; yb += box[0]; xa += box[2]; xb += box[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = frames + (f * 3 + c) * (size_t)H * W;
        const double top = (1.0 - wx) * (double)p[(size_t)ya * W + xa] + wx * (double)p[(size_t)ya * W + xb];
        const double bot = (1.0 - wx) * (double)p[(size_t)yb * W + xa] + wx * (double)p[(size_t)yb * W + xb];
        o[(2 - c) * plane] = (float)((1.0 - wy) * top + wy * bot);
    }
}

// ---- points ------------------------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per frame.  heat: landmark l of frame f, cell i at heat[f * fstride + l * lstride + i * cstride].
// Wave w finds the argmax of landmarks w, w + 4, ..; the frame-wide flags are reduced over the argmaxes in LDS by one thread; then
// thread l writes landmark l.  status bit 1 (value 2): a landmark at cell 4095, where the reference raises; all points -1.
__global__ __launch_bounds__(256) void fan_points_kernel(const float* __restrict__ heat, long long fstride, long long lstride, long long cstride, int N,
                                                         double* __restrict__ pts, int* __restrict__ status) {
    __shared__ int arg[FAN_MAX_LANDMARKS + 1];
    __shared__ int flags[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* frame = heat + (size_t)blockIdx.x * fstride;
    for (int l = wave; l < N; l += 4) {
        const float* p = frame + (size_t)l * lstride;
        float bv = p[(size_t)lane * cstride];
        int bi = lane;
        for (int i = lane + 64; i < FAN_CELLS; i += 64) {
            const float v = p[(size_t)i * cstride];
            if (fan_better(v, i, bv, bi)) { bv = v; bi = i; }
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
            const float ov = __shfl_xor(bv, w, 64);
            const int oi = __shfl_xor(bi, w, 64);
            if (fan_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) arg[l] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int up = 0, down = 0, err = 0;
        for (int l = 0; l < N; ++l) {
            up |= fan_flag_up(arg[l]);
            down |= fan_flag_down(arg[l]);
            err |= arg[l] == FAN_CELLS - 1;
        }
        flags[0] = up; flags[1] = down; flags[2] = err;
        status[blockIdx.x] = err ? 2 : 0;
    }
    __syncthreads();
    const int l = threadIdx.x;
    if (l >= N) return;
    double* o = pts + ((size_t)blockIdx.x * N + l) * 2;
    if (flags[2]) {
        o[0] = o[1] = -1.0;
        return;
    }
    const float* p = frame + (size_t)l * lstride;
    const int i = arg[l];
    const double xu = p[(size_t)fan_x_up(i) * cstride], xd = p[(size_t)fan_x_down(i) * cstride];
    const double yu = p[(size_t)fan_y_up(i, flags[0]) * cstride], yd = p[(size_t)fan_y_down(i, flags[1]) * cstride];
    o[0] = (double)(i % FAN_HEAT) + 0.25 * fan_sign(xu - xd) + 0.5;
    o[1] = (double)(i / FAN_HEAT) + 0.25 * fan_sign(yu - yd) + 0.5;
}

// ---- tail --------------------------------------------------------------------------------------------------------------------------
// One thread per output point.  pts [n, N, 2] heat-map units -> out [n, P, 2] image pixels: times (w / 64, h / 64) of the box; with a
// table [P][2] the mean of two source points rounded to fp32 and the box's origin added in fp32 (facexlib's float32 array), without
// one the origin added in float64.  A frame whose decode failed or whose box is bad gets -1; status_out = decode status | 4 (box).
__global__ __launch_bounds__(256) void fan_tail_kernel(int n, int N, int P, int H, int W, const double* __restrict__ pts, const int* __restrict__ dstatus,
                                                       const int* __restrict__ boxes, const int* __restrict__ table, double* __restrict__ out,
                                                       int* __restrict__ status) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * P) return;
    const size_t f = e / P;
    const int q = (int)(e - f * P);
    const int* box = boxes + f * 4;
    const int st = dstatus[f] | (fan_box_ok(box, H, W) ? 0 : 4);
    if (q == 0) status[f] = st;
    if (st) {
        out[e * 2] = out[e * 2 + 1] = -1.0;
        return;
    }
    const double sc[2] = {(double)(box[3] - box[2]) / 64.0, (double)(box[1] - box[0]) / 64.0};
    const int origin[2] = {box[2], box[0]};
    const double* p = pts + f * N * 2;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (table) {
            const double m = (p[table[q * 2] * 2 + a] * sc[a] + p[table[q * 2 + 1] * 2 + a] * sc[a]) / 2.0;
            out[e * 2 + a] = (double)((float)m + (float)origin[a]);
        } else {
            out[e * 2 + a] = p[q * 2 + a] * sc[a] + (double)origin[a];
        }
    }
}

// the carry-forward: a failed frame takes the points of the last frame before it that did not fail; none: it stays -1
__global__ __launch_bounds__(256) void fan_carry_kernel(int n, int P, const int* __restrict__ status, double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * P * 2) return;
    const long long f = (long long)(e / ((size_t)P * 2));
    if (status[f] == 0) return;
    long long g = f - 1;
    while (g >= 0 && status[g] != 0) --g;
    if (g >= 0) out[e] = out[e - (size_t)(f - g) * P * 2];  // frame g did not fail: this kernel never writes it
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static FanPlan* fan_scratch_plan() {
    static thread_local FanPlan plan;
    return &plan;
}

extern "C" size_t n3dt_fan_packed_layout_bytes(int modules, int N) { return fan_layout(modules, N).total; }

extern "C" size_t n3dt_fan_ws_bytes(int modules, int N, int n) {
    FanPlan* p = fan_scratch_plan();
    fan_plan_forward(p, modules, N);
    return fan_ws_bytes_of(p, n);
}

extern "C" size_t n3dt_fan_block_ws_bytes(int block, int N, int n, int H, int W) {
    FanPlan* p = fan_scratch_plan();
    fan_plan_block(p, block, N, H, W);
    return fan_ws_bytes_of(p, n);
}

extern "C" void n3dt_launch_fan_pack(const N3dtFanParams* q, void* packed, hipStream_t st) {
    const int modules = q->num_modules, N = q->num_landmarks;
    const FanLayout L = fan_layout(modules, N);
    char* base = (char*)packed;
    for (int j = 0; j < fan_convs(modules); ++j) {
        if (!fan_conv_exists(j, modules)) continue;
        const FanConv c = fan_conv(j, N);
        const int np = fan_np(&c), cinp = fan_cinp(&c), K = fan_K(&c);
        const int wc = c.kind == FAN_STEM ? 6 : c.kind == FAN_COORD ? (j < FAN_FRONT_CONVS + FAN_STACK_CONVS ? 259 : 261) : c.cin;
        __bf16* hi = (__bf16*)(base + L.w[j]);
        const size_t n = L.elems[j];
        conv_net_pack(q->weight[j], c.post ? q->bn_weight[j] : nullptr, q->bn_var[j], FAN_BN_EPS, wc, c.cin, cinp, c.cout, np, c.k * c.k, K,
                      c.kind == FAN_STEM, hi, hi + n, st);
        const int most = np > cinp ? np : cinp;
        fan_vec_kernel<<<(most + 255) / 256, 256, 0, st>>>(q->bias[j], q->bn_weight[j], q->bn_bias[j], q->bn_mean[j], q->bn_var[j], c.kind, c.pre, c.cin,
                                                         cinp, c.cout, np, (float*)(base + L.bias[j]), (float*)(base + L.pre[j]));
    }
    fan_stem_map_kernel<<<FAN_STEM_HW * FAN_STEM_HW * 64 / 256, 256, 0, st>>>(q->weight[0], q->bias[0], q->bn_weight[0], q->bn_bias[0], q->bn_mean[0],
                                                                            q->bn_var[0], q->coords256, (float*)(base + L.stem_map));
    for (int s = 0; s < modules; ++s) {
        const int j = fan_stack_conv(s, 0);
        fan_coord_map_kernel<<<FAN_CELLS * 256 / 256, 256, 0, st>>>(q->weight[j], q->bias[j], s ? 261 : 259, q->coords64, (float*)(base + L.map1[s]),
                                                                  s ? (float*)(base + L.map2[s]) : nullptr);
    }
}

struct FanRun {
    int modules, N, end_relu, n;
    const char* packed;
    float* ws;
    const uint8_t* gates;  // [n, slots, 4096]: slot 0 holds the gates stack slot0 + 1 takes
    int slots, slot0;
};

static float* fan_at(const FanRun* r, size_t off) { return r->ws + off * (size_t)r->n; }

static void fan_conv_launch(const FanRun* r, const FanLayout* L, const FanStep* t, hipStream_t st) {
    const FanConv c = fan_conv(t->conv, r->N);
    const int j = t->conv;
    FanConvArgs a;
    a.in = fan_at(r, t->in) + t->in_c0;
    a.whi = (const __bf16*)(r->packed + L->w[j]);
    a.wlo = a.whi + L->elems[j];
    a.bias = (const float*)(r->packed + L->bias[j]);
    a.pre = c.pre ? (const float*)(r->packed + L->pre[j]) : nullptr;
    a.map1 = a.map2 = nullptr;
    a.gate = nullptr;
    a.gate_stride = 0;
    if (c.kind == FAN_STEM) a.map1 = (const float*)(r->packed + L->stem_map);
    if (c.kind == FAN_COORD) {
        a.map1 = (const float*)(r->packed + L->map1[t->stack]);
        if (t->stack > 0) {
            a.map2 = (const float*)(r->packed + L->map2[t->stack]);
            a.gate = r->gates + (size_t)(t->stack - 1 - r->slot0) * FAN_CELLS;
            a.gate_stride = (long long)r->slots * FAN_CELLS;
        }
    }
    a.skip = t->skip == FAN_NONE ? nullptr : fan_at(r, t->skip) + t->skip_c0;
    a.out = fan_at(r, t->out) + t->out_c0;
    a.raw = t->raw == FAN_NONE ? nullptr : fan_at(r, t->raw);
    a.n = r->n;
    a.Hi = t->H; a.Wi = t->W;
    a.pad = c.k / 2;
    a.Ho = cn_conv_out(t->H, c.k, c.stride, a.pad);
    a.Wo = cn_conv_out(t->W, c.k, c.stride, a.pad);
    a.cin = fan_cinp(&c); a.in_cs = t->in_cs; a.np = fan_np(&c);
    a.cstore = c.kind == FAN_L ? cn_round16(c.cout) : c.cout;
    a.out_cs = t->out_cs; a.skip_cs = t->skip_cs; a.raw_cs = t->raw_cs;
    a.k = c.k; a.stride = c.stride;
    a.relu = c.kind == FAN_STEM || c.kind == FAN_LAST || (c.kind == FAN_L && r->end_relu);
    const long long M = (long long)r->n * a.Ho * a.Wo;
    const int nt = cn_wave_ntiles(M, a.np);
    const long long tiles = (M + CN_TILE_M - 1) / CN_TILE_M * (a.np / (32 * nt));
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    if (c.kind == FAN_STEM) {
        if (nt == 1) fan_conv_kernel<1, true><<<grid, 256, 0, st>>>(a);
        else fan_conv_kernel<2, true><<<grid, 256, 0, st>>>(a);
    } else {
        if (nt == 1) fan_conv_kernel<1, false><<<grid, 256, 0, st>>>(a);
        else fan_conv_kernel<2, false><<<grid, 256, 0, st>>>(a);
    }
}

static void fan_step_launch(const FanRun* r, const FanLayout* L, const FanStep* t, hipStream_t st) {
    const int n = r->n;
    if (t->op == FAN_OP_CONV) fan_conv_launch(r, L, t, st);
    else if (t->op == FAN_OP_POOL)
        fan_pool_kernel<<<conv_grid((size_t)n * (t->H / 2) * (t->W / 2) * (t->C / 4)), 256, 0, st>>>(fan_at(r, t->in), n, t->H, t->W, t->C, fan_at(r, t->out));
    else
        fan_upadd_kernel<<<conv_grid((size_t)n * t->H * t->W * (t->C / 4)), 256, 0, st>>>(fan_at(r, t->in), fan_at(r, t->skip), n, t->H, t->W, t->C,
                                                                                      fan_at(r, t->out));
}

// x [n, 3, 256, 256] BGR -> heat [modules][n, N + 1, 64, 64]; gates [n, max(modules - 1, 1), 4096]: written here where
// compute_gates, else read as the caller left them
extern "C" void n3dt_launch_fan_fwd(int modules, int N, int end_relu, int n, const void* packed, const float* x, int compute_gates, uint8_t* gates,
                                    float* heat, void* workspace, hipStream_t st) {
    FanPlan* p = fan_scratch_plan();
    fan_plan_forward(p, modules, N);
    const FanLayout L = fan_layout(modules, N);
    const int slots = modules > 1 ? modules - 1 : 1, hcs = fan_heat_cs(N);
    FanRun r = {modules, N, end_relu, n, (const char*)packed, (float*)workspace, gates, slots, 0};
    conv_net_to_nhwc(x, n, 3, FAN_IMG, FAN_IMG, 0, 3, fan_at(&r, p->image), 3, st);
    for (int s = 0; s < p->steps; ++s) {
        const FanStep* t = &p->step[s];
        fan_step_launch(&r, &L, t, st);
        if (t->op == FAN_OP_CONV && fan_conv(t->conv, N).kind == FAN_L) {  // a stack's heat map exists: its gates, its copy out
            const int stack = (t->conv - FAN_FRONT_CONVS) / FAN_STACK_CONVS;
            const float* hm = fan_at(&r, p->heat[stack]);
            if (compute_gates && stack < modules - 1)
                fan_gate_kernel<<<(unsigned)(((size_t)n * FAN_CELLS + 255) / 256), 256, 0, st>>>(hm, n, hcs, N, slots, stack, gates);
            conv_net_to_nchw(hm, hcs, n, N + 1, FAN_HEAT, FAN_HEAT, 0, heat + (size_t)stack * n * (N + 1) * FAN_CELLS, st);
        }
    }
}

// one block alone: in [n, C_in, H, W] -> out [n, C_out, Ho, Wo] through maps laid out as the chain holds them
extern "C" void n3dt_launch_fan_block(int block, int modules, int N, int end_relu, int n, int H, int W, const void* packed, const float* in,
                                      const float* skip, const uint8_t* gates, float* out, void* workspace, hipStream_t st) {
    FanPlan* p = fan_scratch_plan();
    const FanBlockMaps m = fan_plan_block(p, block, N, H, W);
    const FanBlock k = fan_block(block, N);
    const FanLayout L = fan_layout(modules, N);
    const int stack = block < FAN_FRONT_BLOCKS ? 0 : (block - FAN_FRONT_BLOCKS) / FAN_STACK_BLOCKS;
    // the block's gates are handed over as [n, 4096]: one slot, the one its stack takes
    FanRun r = {modules, N, end_relu, n, (const char*)packed, (float*)workspace, gates, 1, stack > 0 ? stack - 1 : 0};
    conv_net_to_nhwc(in, n, k.cin, H, W, 0, m.in_cs, fan_at(&r, m.in), m.in_cs, st);
    if (skip) conv_net_to_nhwc(skip, n, k.cout, m.Ho, m.Wo, 0, m.out_cs, fan_at(&r, m.skip), m.out_cs, st);
    for (int s = 0; s < p->steps; ++s) {
        const FanStep* t = &p->step[s];
        fan_step_launch(&r, &L, t, st);
    }
    conv_net_to_nchw(fan_at(&r, m.out), m.out_cs, n, k.cout, m.Ho, m.Wo, 0, out, st);
}

extern "C" void n3dt_launch_fan_crops(int n, int H, int W, const float* frames, const int* boxes, float* out, hipStream_t st) {
    fan_crop_kernel<<<(unsigned)(((size_t)n * FAN_IMG * FAN_IMG + 255) / 256), 256, 0, st>>>(n, H, W, frames, boxes, out);
}

extern "C" void n3dt_launch_fan_points(int n, int N, const float* heat, long long frame_stride, double* pts, int* status, hipStream_t st) {
    fan_points_kernel<<<n, 256, 0, st>>>(heat, frame_stride, FAN_CELLS, 1, N, pts, status);
}

extern "C" void n3dt_launch_fan_tail(int n, int N, int P, int H, int W, const double* pts, const int* dstatus, const int* boxes, const int* table,
                                     int carry, double* out, int* status, hipStream_t st) {
    fan_tail_kernel<<<(unsigned)(((size_t)n * P + 255) / 256), 256, 0, st>>>(n, N, P, H, W, pts, dstatus, boxes, table, out, status);
    if (carry) fan_carry_kernel<<<(unsigned)(((size_t)n * P * 2 + 255) / 256), 256, 0, st>>>(n, P, status, out);
}
