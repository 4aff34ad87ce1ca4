// The 3-D face reconstruction net, frozen and inference-only (include/n3dt.h, n3dt_face_recon_*; the reference's
// s_face3d/models/networks.py -- ReconNetWrapper over resnet50, use_last_fc=False -- behind s_face3d/util/preprocess.py's align_img
// as XGaze_utils/data_loader_xgaze_new.py's CropAndExtract.generate calls it).  The table, every map's size --
// known only at run time, a function of the image's (H, W) -- and every address that can go wrong at an edge come from
// face_recon_core.h, which tests/face_recon_core_host.cpp also compiles and walks over the same grids.  That program re-types the
// loop nest of the convolution kernel below (block / wave / lane / K step): a change to that loop here must be made there too.
//
//   align      frames [n,3,H,W] fp32 RGB in [0,1] + landmarks -> the 224 x 224 crop align_img cuts from PIL's BICUBIC resize, per
//              output pixel, float64; the resized image is never formed
//   conv x53   Conv2d + folded BatchNorm (+ residual) (+ ReLU) as an implicit GEMM on v_mfma_f32_32x32x16_bf16 (M = cells of the
//              padded output map, N = C_out, k = tap * C_in + c_in; the stem: k = (tap, channel) flattened, 147 padded to 160),
//              every operand split x = hi + lo into two bf16s, three products accumulated in fp32: conv_mfma.h's step in its
//              split form
//   pool       3 x 3 / 2 max with padding 1, out-of-range taps ignored
//   average    over the last map, float64 in row-major cell order, rounded once
//   head       [n,2048] x [2048,257] + bias, float64 accumulation in a fixed order
//
// Every image goes through identical code with the same K order, no split-K and no atomics: an image's result depends neither on
// its position in the batch nor on the batch size.  Every element of every map, halo included, is written exactly once per
// forward; nothing is cleared.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/n3dt.h"
#include "conv_mfma.h"
#include "conv_net.h"
#include "face_recon_core.h"
#include "n3dt_launch.h"

// ---- packed weights ------------------------------------------------------------------------------------------------------------
// Per convolution one B matrix in conv_frag.h's fragment order, hi then lo, with the BatchNorm's scale folded in, then the fp32
// folded biases; then the head's [257, 2048] fp32 matrix and its 257 biases.
struct FrPackLayout {
    size_t w[FR_CONVS], elems[FR_CONVS], bias[FR_CONVS], head_w, head_b, total;
};

static FrPackLayout fr_layout() {
    FrPackLayout L;
    size_t off = 0;
    for (int j = 0; j < FR_CONVS; ++j) {
        const FrGeom g = fr_geom(j, FR_MIN_HW, FR_MIN_HW);  // K and C_out do not depend on the size
        L.elems[j] = (size_t)g.K * g.cout;
        L.w[j] = off;
        off = rup(off + L.elems[j] * 2 * sizeof(__bf16), 256);
    }
    for (int j = 0; j < FR_CONVS; ++j) {
        L.bias[j] = off;
        off = rup(off + fr_conv(j).cout * sizeof(float), 256);
    }
    L.head_w = off;
    off = rup(off + (size_t)FR_COEFFS * FR_FEAT * sizeof(float), 256);
    L.head_b = off;
    off = rup(off + FR_COEFFS * sizeof(float), 256);
    L.total = off;
    return L;
}

// The pack (W [cout, cin, k, k] -> B [K][cout], row k = tap * cin + ci; the stem: (ky * 7 + kx) * 3 + ci, rows 147 .. 159 zero), the
// eval-mode BatchNorm2d folded in as a scale and a shift in float64 -- y = (x - mean) / sqrt(var + eps) * gamma + beta -- and the
// layouts [n,C,H,W] <-> haloed NHWC are conv_net.hip's.

// ---- implicit-GEMM convolution ---------------------------------------------------------------------------------------------------
struct FrConvArgs {
    const float* in;     // [n, Hp, Wp, cinp], halo included in Hp, Wp
    const __bf16* whi;   // packed B matrix (hi), [K/16][cout/32][64][8]
    const __bf16* wlo;
    const float* bias;   // [cout], the folded BatchNorm shift
    const float* skip;   // [n, Hq, Wq, cout] (a residual block's identity; its output has no halo) or NULL
    float* out;          // [n, Hq, Wq, cout], every cell written
    int n, Ho, Wo, Hp, Wp, Hq, Wq, cinp, np, k, stride, opad, relu;
};

// 256 threads = 4 waves; wave tile t = 4 blockIdx.x + wave computes CN_TILE_M cells x 32 NT columns, the column tile fastest.
// A k-step is 16 channels of one tap (C_in % 16 == 0); STEM: 16 consecutive k of the flattened (tap, channel), those from 147 on
// read as 0 against zero weight rows.  Kernel size, stride, every map size and every halo are run-time arguments; the row index is
// 64-bit.  Epilogue: conv + bias (+ skip), then the ReLU -- relu(bn3(conv3) + identity), the reference's order.
template <int NT, bool STEM>
__global__ __launch_bounds__(256) void face_recon_conv_kernel(FrConvArgs a) {
    const ConvWaveTile t = conv_wave_tile<NT>(a.np, a.n, a.Hq, a.Wq);
    if (t.idle()) return;  // no barriers in this kernel: an idle wave may leave
    const int lane = t.lane, r = t.r, h = t.h, nt0 = t.nt0(NT);
    const long long Mq = t.M, m0 = t.m0;
    const float* base[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int img, yq, xq;
        cn_row_cell(m0 + mt * 32 + r, Mq, a.Hq, a.Wq, &img, &yq, &xq);  // rows past Mq compute the last cell again and are never stored
        const int y = cn_clampi(yq - a.opad, 0, a.Ho - 1), x = cn_clampi(xq - a.opad, 0, a.Wo - 1);
        base[mt] = a.in + cn_field_base(img, y, x, a.stride, a.Hp, a.Wp, a.cinp);
    }
    conv_f32x16 acc[2][NT];
    CONV_ZERO_ACC(acc, NT);
    float av[2][8];

    if (STEM) {
        for (int s = 0; s < CN_STEM_KP / 16; ++s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * h + j;
                const bool real = k < CN_STEM_K;
                const size_t off = cn_stem_offset(real ? k : 0, a.Wp);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const float v = base[mt][off];
                    av[mt][j] = real ? v : 0.0f;
                }
            }
            conv_mma_step<true, NT>(a.whi, a.wlo, a.np, s, nt0, lane, av, acc);
        }
    } else {
        int s = 0;
        for (int tap = 0; tap < a.k * a.k; ++tap) {
            const size_t toff = cn_tap_offset(tap, a.k, a.Wp, a.cinp) + 8 * h;
            for (int c0 = 0; c0 < a.cinp; c0 += 16, ++s) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) conv_load8(base[mt] + toff + c0, av[mt]);
                conv_mma_step<true, NT>(a.whi, a.wlo, a.np, s, nt0, lane, av, acc);
            }
        }
    }

    // epilogue: accumulator register i of lane (r, h) is output row cf_acc_row(i, h), column r; 0 in the halo
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long m = m0 + mt * 32 + cf_acc_row(i, h);
            if (m >= Mq) continue;
            int img, yq, xq;
            cn_row_cell(m, Mq, a.Hq, a.Wq, &img, &yq, &xq);
            const bool inside = cn_interior(yq, xq, a.Ho, a.Wo, a.opad);
            float* o = a.out + (size_t)m * a.np;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int co = (nt0 + nt) * 32 + r;
                float v = 0.0f;
                if (inside) {
                    v = acc[mt][nt][i] + a.bias[co];
                    if (a.skip) v += a.skip[(size_t)m * a.np + co];
                    if (a.relu) v = v > 0.0f ? v : 0.0f;
                }
                o[co] = v;
            }
        }
}

// ---- average, head (the 3 x 3 / 2 max pool is conv_net.hip's) --------------------------------------------------------------------
// in [n, H, W, C] -> out [n, C]: the mean over the H W cells, summed in float64 in row-major order, rounded once
__global__ __launch_bounds__(256) void face_recon_avg_kernel(const float* __restrict__ in, int n, int HW, int C, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * C) return;
    const int c = (int)(e % C);
    const float* p = in + (e / C) * (size_t)HW * C + c;
    double s = 0.0;
    for (int i = 0; i < HW; ++i) s += (double)p[(size_t)i * C];
    out[e] = (float)(s / (double)HW);
}

// feat [n, 2048] -> out [n, 257] = feat W^T + b: one wave per output; lane l sums k = l, l + 64, .. in float64, a butterfly adds
// the 64 partial sums, the bias is added last, the result rounded once
__global__ __launch_bounds__(256) void face_recon_head_kernel(const float* __restrict__ feat, const float* __restrict__ W, const float* __restrict__ b,
                                                              int n, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const size_t o = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= (size_t)n * FR_COEFFS) return;  // wave-uniform
    const int col = (int)(o % FR_COEFFS);
    const float* f = feat + (o / FR_COEFFS) * FR_FEAT;
    const float* w = W + (size_t)col * FR_FEAT;
    double s = 0.0;
    for (int k = lane; k < FR_FEAT; k += 64) s += (double)f[k] * (double)w[k];
    s = conv_wave_sum(s);
    if (lane == 0) out[o] = (float)(s + (double)b[col]);
}

// ---- alignment -------------------------------------------------------------------------------------------------------------------
// One thread per frame: the five landmarks (68: extract_5p; the y flip H - 1 - y; a frame whose landmarks average exactly -1, and
// every frame where lm is NULL, gets (lm3d_std[:, :2] + 1) / 2 * (W, H) unflipped), then the similarity.  lm [n, points, 2] float64.
// The mean is summed in index order where numpy's sums pairwise: for landmarks that are all -1, the case the reference's extractor
// produces, both are exact; values whose mean only ROUNDS to -1 may be judged differently by the two.
__global__ __launch_bounds__(64) void face_recon_similarity_kernel(int n, int H, int W, const double* __restrict__ lm, int points,
                                                                   const double* __restrict__ lm3d, const double* __restrict__ pinv,
                                                                   double* __restrict__ trans, int* __restrict__ geom, int* __restrict__ status) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    double lm5[5][2];
    bool fallback = lm == nullptr;
    if (!fallback) {
        const double* p = lm + (size_t)f * points * 2;
        double sum = 0.0;
        for (int i = 0; i < points * 2; ++i) sum += p[i];
        fallback = sum / (double)(points * 2) == -1.0;
        if (!fallback) {
            if (points == 5) {
                for (int i = 0; i < 5; ++i) {
                    lm5[i][0] = p[2 * i];
                    lm5[i][1] = p[2 * i + 1];
                }
            } else {
                // extract_5p: [mean(36, 39), mean(42, 45), 30, 48, 54] (0-based)
                for (int a = 0; a < 2; ++a) {
                    lm5[0][a] = (p[2 * 36 + a] + p[2 * 39 + a]) / 2.0;
                    lm5[1][a] = (p[2 * 42 + a] + p[2 * 45 + a]) / 2.0;
                    lm5[2][a] = p[2 * 30 + a];
                    lm5[3][a] = p[2 * 48 + a];
                    lm5[4][a] = p[2 * 54 + a];
                }
            }
            for (int i = 0; i < 5; ++i) lm5[i][1] = (double)(H - 1) - lm5[i][1];
        }
    }
    if (fallback)
        for (int i = 0; i < 5; ++i) {
            lm5[i][0] = (lm3d[3 * i] + 1.0) / 2.0 * (double)W;
            lm5[i][1] = (lm3d[3 * i + 1] + 1.0) / 2.0 * (double)H;
        }
    double t[5];
    int g[4];
    status[f] = fr_similarity(lm5, pinv, W, H, t, g);
    for (int i = 0; i < 5; ++i) trans[(size_t)f * 5 + i] = t[i];
    for (int i = 0; i < 4; ++i) geom[(size_t)f * 4 + i] = g[i];
}

// the frame's sample (c, y, x) as PIL holds it: 255 u, as a byte floor(255 u + 0.5) where `quantize`; u clamped to [0, 1], NaN -> 0
__device__ __forceinline__ double fr_sample(const float* plane, int W, int y, int x, int quantize) {
    float u = plane[(size_t)y * W + x];
    if (!(u > 0.0f)) u = 0.0f;
    if (u > 1.0f) u = 1.0f;
    const double v = 255.0 * (double)u;
    return quantize ? floor(v + 0.5) : v;
}

__device__ __forceinline__ double fr_clamp_byte(double v, int quantize) {
    if (quantize) v = floor(v + 0.5);
    return v < 0.0 ? 0.0 : v > 255.0 ? 255.0 : v;
}

// One thread per output pixel (frame, Y, X) of the 224 x 224 crop, all three channels: pixel (left + X, up + Y) of the frame
// resized to (w, h) by PIL's BICUBIC -- the horizontal pass over the rows the vertical taps need, clamped to [0, 255] (and rounded
// where `quantize`), then the vertical pass, clamped -- or 0 outside the resized image and in a frame whose status is not 0.
// out [n, 3, 224, 224] = value / 255.
__global__ __launch_bounds__(256) void face_recon_crop_kernel(int n, int H, int W, const float* __restrict__ frames, const int* __restrict__ geom,
                                                              const int* __restrict__ status, int quantize, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * FR_CROP * FR_CROP) return;
    const int X = (int)(e % FR_CROP), Y = (int)(e / FR_CROP % FR_CROP), f = (int)(e / ((size_t)FR_CROP * FR_CROP));
    const size_t plane = (size_t)FR_CROP * FR_CROP;
    float* o = out + (size_t)f * 3 * plane + (size_t)Y * FR_CROP + X;
    const int w = geom[f * 4], h = geom[f * 4 + 1];
    const long long xr = (long long)geom[f * 4 + 2] + X, yr = (long long)geom[f * 4 + 3] + Y;
    if (status[f] != 0 || xr < 0 || xr >= w || yr < 0 || yr >= h) {
        o[0] = o[plane] = o[2 * plane] = 0.0f;
        return;
    }
    int xa, xb, ya, yb;
    double xc, xf, yc, yf;
    fr_taps((int)xr, W, w, &xa, &xb, &xc, &xf);
    fr_taps((int)yr, H, h, &ya, &yb, &yc, &yf);
    double xsum = 0.0, ysum = 0.0;
    for (int x = xa; x < xb; ++x) xsum += fr_cubic(((double)x - xc + 0.5) / xf);
    for (int y = ya; y < yb; ++y) ysum += fr_cubic(((double)y - yc + 0.5) / yf);
    const float* fr = frames + (size_t)f * 3 * H * W;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int y = ya; y < yb; ++y) {
        double row[3] = {0.0, 0.0, 0.0};
        for (int x = xa; x < xb; ++x) {
            const double wx = fr_cubic(((double)x - xc + 0.5) / xf) / xsum;
#pragma unroll
            for (int c = 0; c < 3; ++c) row[c] += wx * fr_sample(fr + (size_t)c * H * W, W, y, x, quantize);
        }
        const double wy = fr_cubic(((double)y - yc + 0.5) / yf) / ysum;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += wy * fr_clamp_byte(row[c], quantize);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = (float)(fr_clamp_byte(acc[c], quantize) / 255.0);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
extern "C" size_t n3dt_face_recon_packed_layout_bytes(void) { return fr_layout().total; }
extern "C" size_t n3dt_face_recon_ws_bytes(int n, int H, int W) { return fr_workspace(n, H, W).total; }

extern "C" void n3dt_launch_face_recon_pack(const N3dtFaceReconParams* p, void* packed, hipStream_t st) {
    const FrPackLayout L = fr_layout();
    char* base = (char*)packed;
    for (int j = 0; j < FR_CONVS; ++j) {
        const FrGeom g = fr_geom(j, FR_MIN_HW, FR_MIN_HW);
        __bf16* hi = (__bf16*)(base + L.w[j]);
        const size_t n = L.elems[j];
        conv_net_pack(p->weight[j], p->bn_weight[j], p->bn_var[j], p->bn_eps[j], g.cin, g.cin, g.cin, g.cout, g.cout, g.k * g.k, g.K, g.role == FR_STEM,
                      hi, hi + n, st);
        conv_net_shift_bn(p->bn_weight[j], p->bn_bias[j], p->bn_mean[j], p->bn_var[j], p->bn_eps[j], g.cout, (float*)(base + L.bias[j]), st);
    }
    int col = 0;
    for (int i = 0; i < FR_HEADS; ++i) {
        const size_t n = (size_t)FR_HEAD_COLS[i] * FR_FEAT;
        conv_net_copy(p->head_weight[i], n, (float*)(base + L.head_w) + (size_t)col * FR_FEAT, st);
        conv_net_copy(p->head_bias[i], (size_t)FR_HEAD_COLS[i], (float*)(base + L.head_b) + col, st);
        col += FR_HEAD_COLS[i];
    }
}

static void fr_conv_launch(int j, int n, int Hi, int Wi, const void* packed, const float* in, const float* skip, float* out, hipStream_t st) {
    const FrPackLayout L = fr_layout();
    const FrGeom g = fr_geom(j, Hi, Wi);
    const char* pk = (const char*)packed;
    FrConvArgs a;
    a.in = in;
    a.whi = (const __bf16*)(pk + L.w[j]);
    a.wlo = a.whi + L.elems[j];
    a.bias = (const float*)(pk + L.bias[j]);
    a.skip = skip;
    a.out = out;
    a.n = n;
    a.Ho = g.Ho; a.Wo = g.Wo; a.Hp = g.Hp; a.Wp = g.Wp; a.Hq = g.Hq; a.Wq = g.Wq;
    a.cinp = g.cinp; a.np = g.cout; a.k = g.k; a.stride = g.stride; a.opad = g.opad; a.relu = g.relu;
    const size_t Mq = (size_t)n * g.Hq * g.Wq;
    const size_t mtiles = (Mq + CN_TILE_M - 1) / CN_TILE_M;
    const int nt = cn_wave_ntiles((long long)Mq, g.cout);
    const size_t tiles = mtiles * (g.cout / (32 * nt));
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    if (g.role == FR_STEM) {
        if (nt == 1) face_recon_conv_kernel<1, true><<<grid, 256, 0, st>>>(a);
        else face_recon_conv_kernel<2, true><<<grid, 256, 0, st>>>(a);
    } else {
        if (nt == 1) face_recon_conv_kernel<1, false><<<grid, 256, 0, st>>>(a);
        else face_recon_conv_kernel<2, false><<<grid, 256, 0, st>>>(a);
    }
}

static void fr_avg_launch(int n, int Hi, int Wi, const float* in, float* out, hipStream_t st) {
    face_recon_avg_kernel<<<(unsigned)(((size_t)n * FR_FEAT + 255) / 256), 256, 0, st>>>(in, n, Hi * Wi, FR_FEAT, out);
}

static void fr_head_launch(int n, const void* packed, const float* feat, float* out, hipStream_t st) {
    const FrPackLayout L = fr_layout();
    const char* pk = (const char*)packed;
    face_recon_head_kernel<<<(unsigned)(((size_t)n * FR_COEFFS + 3) / 4), 256, 0, st>>>(feat, (const float*)(pk + L.head_w), (const float*)(pk + L.head_b), n,
                                                                                      out);
}

// x [n, 3, H, W] -> out [n, 257]
extern "C" void n3dt_launch_face_recon_fwd(int n, int H, int W, const void* packed, const float* x, float* out, void* workspace, hipStream_t st) {
    const FrWorkspace w = fr_workspace(n, H, W);
    char* ws = (char*)workspace;
    float* region[FR_REGIONS];
    for (int r = 0; r < FR_REGIONS; ++r) region[r] = (float*)(ws + w.region[r]);
    conv_net_to_nhwc(x, n, 3, H, W, 3, 3, region[1], 3, st);
    FrStep steps[FR_STEPS];
    fr_chain(H, W, steps);
    for (int s = 0; s < FR_STEPS; ++s) {
        const FrStep t = steps[s];
        if (t.block == FR_POOL_BLOCK) conv_net_max_pool(region[t.in], n, t.Hi, t.Wi, 64, region[t.out], st);
        else if (t.block == FR_AVG_BLOCK) fr_avg_launch(n, t.Hi, t.Wi, region[t.in], region[t.out], st);
        else fr_conv_launch(t.block, n, t.Hi, t.Wi, packed, region[t.in], t.skip < 0 ? nullptr : region[t.skip], region[t.out], st);
    }
    fr_head_launch(n, packed, region[5], out, st);
}

extern "C" void n3dt_launch_face_recon_align(int n, int H, int W, const float* frames, const double* landmarks, int points, const double* lm3d_std,
                                             const double* pinv, int quantize, float* crops, double* trans_params, int* geom, int* status,
                                             hipStream_t st) {
    face_recon_similarity_kernel<<<(n + 63) / 64, 64, 0, st>>>(n, H, W, landmarks, points, lm3d_std, pinv, trans_params, geom, status);
    face_recon_crop_kernel<<<(unsigned)(((size_t)n * FR_CROP * FR_CROP + 255) / 256), 256, 0, st>>>(n, H, W, frames, geom, status, quantize, crops);
}

// ---- one block alone ---------------------------------------------------------------------------------------------------------------
// in [n, C_in, Hi, Wi] -> out [n, C_out, Ho, Wo] through maps laid out as the chain holds them; a bottleneck's third convolution
// takes the identity as skip [n, C_out, Ho, Wo]; the average gives [n, 2048, 1, 1], the head takes [n, 2048, 1, 1] and gives [n, 257]
struct FrBlockShape {
    int cin, cout, Ho, Wo, ipad, opad;
    size_t in_elems, out_elems;  // of the NHWC maps, per image
};

static FrBlockShape fr_block_shape(int block, int Hi, int Wi) {
    FrBlockShape b;
    b.ipad = b.opad = 0;
    if (block < FR_CONVS) {
        const FrGeom g = fr_geom(block, Hi, Wi);
        b.cin = g.cin; b.cout = g.cout; b.Ho = g.Ho; b.Wo = g.Wo; b.ipad = g.pad; b.opad = g.opad;
        b.in_elems = fr_in_elems(&g, 1);
        b.out_elems = fr_out_elems(&g, 1);
    } else if (block == FR_POOL_BLOCK) {
        b.cin = b.cout = 64; b.Ho = cn_pool_out(Hi); b.Wo = cn_pool_out(Wi);
        b.in_elems = (size_t)Hi * Wi * 64;
        b.out_elems = (size_t)b.Ho * b.Wo * 64;
    } else if (block == FR_AVG_BLOCK) {
        b.cin = b.cout = FR_FEAT; b.Ho = b.Wo = 1;
        b.in_elems = (size_t)Hi * Wi * FR_FEAT;
        b.out_elems = FR_FEAT;
    } else {
        b.cin = FR_FEAT; b.cout = FR_COEFFS; b.Ho = b.Wo = 1;
        b.in_elems = FR_FEAT;
        b.out_elems = FR_COEFFS;
    }
    return b;
}

// three regions: the input map, the output map, the skip map (as large as the output)
extern "C" size_t n3dt_face_recon_block_ws_bytes(int block, int n, int Hi, int Wi) {
    const FrBlockShape b = fr_block_shape(block, Hi, Wi);
    return cn_rup256((size_t)n * b.in_elems * sizeof(float)) + 2 * cn_rup256((size_t)n * b.out_elems * sizeof(float));
}

extern "C" void n3dt_launch_face_recon_block(int block, int n, int Hi, int Wi, const void* packed, const float* in, const float* skip, float* out,
                                             void* workspace, hipStream_t st) {
    const FrBlockShape b = fr_block_shape(block, Hi, Wi);
    const size_t out_bytes = cn_rup256((size_t)n * b.out_elems * sizeof(float));
    float* map0 = (float*)workspace;
    float* map1 = (float*)((char*)workspace + cn_rup256((size_t)n * b.in_elems * sizeof(float)));
    float* map2 = (float*)((char*)map1 + out_bytes);
    if (block == FR_HEAD_BLOCK) {
        fr_head_launch(n, packed, in, out, st);  // [n, 2048, 1, 1] is [n, 2048]
        return;
    }
    conv_net_to_nhwc(in, n, b.cin, Hi, Wi, b.ipad, b.cin, map0, b.cin, st);
    if (block == FR_AVG_BLOCK) {
        fr_avg_launch(n, Hi, Wi, map0, out, st);
        return;
    }
    if (block == FR_POOL_BLOCK) {
        conv_net_max_pool(map0, n, Hi, Wi, 64, map1, st);
    } else {
        if (skip) conv_net_to_nhwc(skip, n, b.cout, b.Ho, b.Wo, 0, b.cout, map2, b.cout, st);
        fr_conv_launch(block, n, Hi, Wi, packed, map0, skip ? map2 : nullptr, map1, st);
    }
    conv_net_to_nchw(map1, b.cout, n, b.cout, b.Ho, b.Wo, b.opad, out, st);
}
