// Wav2Lip's generator, frozen and inference-only (include/n3dt.h, n3dt_wav2lip_*; the reference's wav_models/wav2lip.py over
// wav_models/conv.py).  The geometry table, the classes of a block's rows and every address that can go
// wrong at an edge come from wav2lip_core.h, which tests/wav2lip_core_host.cpp also compiles and walks over the same grid for all
// 51 blocks.  That program re-types the loop nest of the convolution kernel below (block / wave / class / lane / K step) and the
// pack kernel's weight lookup: a change to either here must be made there too.  The MFMA step, the fragment order of the packed
// weights and the epilogue's register -> row map are conv_mfma.h's and conv_frag.h's, shared with syncnet.hip, unchanged.
//
//   face inputs  frames [F,3,H,W] fp32 RGB + crop boxes -> [n,6,96,96]: the target frame's crop, BGR, rows 48..95 zero, then the
//                reference frame's crop, BGR; bilinear with half-pixel centres in float64 (conv_net_core.h's cn_bilinear)
//   layout       [n,C,H,W] -> NHWC with C padded to 16 and the consumer's zero halo, into a map or a slice of a CAT buffer
//   conv x50     Conv2d / ConvTranspose2d + folded BatchNorm2d (+ the block's own input) + ReLU as an implicit GEMM on
//                v_mfma_f32_32x32x16_bf16, both operands split into two bf16s, three products in fp32 (conv_mma_step<true, NT>):
//                the only mode.  One launch per block covers all its classes (four parity classes of a stride-2 transposed
//                block, nine pixels of the first one).  Output row stride and channel offset are arguments: a block that ends in
//                a concatenation writes its slice of the CAT buffer, and so does the encoder block whose feature is the rest.
//   head         nn.Conv2d(32, 3, 1) in float64 from fp32 operands, sigmoid, stored NCHW [n,3,96,96] fp32 (C_out 3 gets a kernel
//                of its own; C_out 16 of the first face block is a packed matrix of 32 columns whose last 16 are never stored)
//   paste        each generated face resampled to its box and written over a copy of its frame, BGR -> RGB
//
// K order fixed, no split-K, no atomics: a window's output depends neither on its position in the batch nor on the batch size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/n3dt.h"
#include "conv_mfma.h"
#include "conv_net.h"
#include "wav2lip_core.h"
#include "n3dt_launch.h"

// ---- packed weights ------------------------------------------------------------------------------------------------------------
// Per block and class one B matrix in conv_frag.h's fragment order, [Kc/16][np/32] fragments, hi then lo; then the folded fp32
// biases.  The head's 3 x 32 fp32 weights lie where a block's matrices would.
struct W2lPackLayout {
    size_t w[W2L_BLOCKS], bias[W2L_BLOCKS], total;
};

static W2lPackLayout w2l_layout() {
    W2lPackLayout L;
    size_t off = 0;
    for (int b = 0; b < W2L_BLOCKS; ++b) {
        L.w[b] = off;
        off = rup(off + (b == W2L_HEAD ? W2L_OUT_C * W2L_HEAD_C * sizeof(float) : w2l_packed_elems(b) * sizeof(__bf16)), 256);
    }
    for (int b = 0; b < W2L_BLOCKS; ++b) {
        L.bias[b] = off;
        off = rup(off + W2L_TABLE[b].cout * sizeof(float), 256);
    }
    L.total = off;
    return L;
}

// one class of one block.  Conv2d weights are [C_out, C_in, kh, kw], ConvTranspose2d weights [C_in, C_out, kh, kw]; tap `tap` of
// the class is kernel element kidx[tap] (the tap itself where identity).  Columns cout .. np - 1 and channels cin .. cinp - 1: 0.
__global__ __launch_bounds__(256) void wav2lip_pack_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                           const float* __restrict__ var, int tr, int cin, int cinp, int cout, int np,
                                                           int taps_full, int Kc, int identity, int4 kidx, __bf16* __restrict__ hi,
                                                           __bf16* __restrict__ lo) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)Kc * np) return;
    int k, n;
    cf_pack_decode(e, np / 32, &k, &n);
    const int tap = k / cinp, ci = k - tap * cinp;
    const int kid = identity ? tap : tap == 0 ? kidx.x : tap == 1 ? kidx.y : tap == 2 ? kidx.z : kidx.w;
    float w = 0.0f;
    if (ci < cin && n < cout) {
        const size_t at = tr ? ((size_t)ci * cout + n) * taps_full + kid : ((size_t)n * cin + ci) * taps_full + kid;
        w = (float)((double)W[at] * conv_bn_scale(gamma, var, SN_BN_EPS, n));
    }
    const __bf16 h = (__bf16)w;
    hi[e] = h;
    lo[e] = conv_lo(w, h);
}

// the head has no batch norm: weights [3,32,1,1] and bias [3] as they are
__global__ __launch_bounds__(128) void wav2lip_head_pack_kernel(const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ w,
                                                                float* __restrict__ b) {
    const int t = threadIdx.x;
    if (t < W2L_OUT_C * W2L_HEAD_C) w[t] = W[t];
    if (t < W2L_OUT_C) b[t] = bias[t];
}

// ---- prologue and paste ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double w2l_sample(const float* __restrict__ plane, int width, int y1, int x1, int ya, int yb, int xa, int xb, double wy,
                                             double wx, bool clamp01) {
    double v[4];
    const size_t at[4] = {(size_t)(y1 + ya) * width + (x1 + xa), (size_t)(y1 + ya) * width + (x1 + xb), (size_t)(y1 + yb) * width + (x1 + xa),
                          (size_t)(y1 + yb) * width + (x1 + xb)};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float u = plane[at[i]];
        if (clamp01) {
            if (!(u > 0.0f)) u = 0.0f;  // negative, -0 and NaN
            if (u > 1.0f) u = 1.0f;
        }
        v[i] = (double)u;
    }
    const double uy = 1.0 - wy, ux = 1.0 - wx;
    return uy * (ux * v[0] + wx * v[1]) + wy * (ux * v[2] + wx * v[3]);
}

// one thread per element of out [n, 6, 96, 96].  boxes: [n, 4] or, with box_stride 0, one box for every frame.
__global__ __launch_bounds__(256) void wav2lip_face_inputs_kernel(int n, int height, int width, const float* __restrict__ frames,
                                                                  const float* __restrict__ ref_frames, const int* __restrict__ boxes,
                                                                  int box_stride, float* __restrict__ out) {
    const size_t total = (size_t)n * W2L_FACE_C * W2L_IMG * W2L_IMG;
    const size_t plane = (size_t)height * width;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int x = (int)(e % W2L_IMG);
        size_t t = e / W2L_IMG;
        const int y = (int)(t % W2L_IMG);
        t /= W2L_IMG;
        const int ch = (int)(t % W2L_FACE_C), frame = (int)(t / W2L_FACE_C);
        if (ch < 3 && y >= W2L_IMG / 2) {  // the masked lower half of the target
            out[e] = 0.0f;
            continue;
        }
        const int c = 2 - ch % 3;  // BGR: output channel 0 is the frame's blue
        int y1, h, x1, w;
        cn_clamp_box(boxes + (size_t)frame * box_stride, height, width, &y1, &h, &x1, &w);
        int ya, yb, xa, xb;
        double wy, wx;
        cn_bilinear(y, h, W2L_IMG, &ya, &yb, &wy);
        cn_bilinear(x, w, W2L_IMG, &xa, &xb, &wx);
        const float* src = (ch < 3 ? frames : ref_frames) + ((size_t)frame * 3 + c) * plane;
        out[e] = (float)w2l_sample(src, width, y1, x1, ya, yb, xa, xb, wy, wx, true);
    }
}

// one thread per element of out [n, 3, H, W]: inside the frame's box the face [n, 3, 96, 96] (BGR) resampled to the box, else the frame
__global__ __launch_bounds__(256) void wav2lip_paste_kernel(int n, int height, int width, const float* __restrict__ faces,
                                                            const float* __restrict__ frames, const int* __restrict__ boxes, int box_stride,
                                                            float* __restrict__ out) {
    const size_t total = (size_t)n * 3 * height * width;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int x = (int)(e % width);
        size_t t = e / width;
        const int y = (int)(t % height);
        t /= height;
        const int c = (int)(t % 3), frame = (int)(t / 3);
        int y1, h, x1, w;
        cn_clamp_box(boxes + (size_t)frame * box_stride, height, width, &y1, &h, &x1, &w);
        float v = frames[e];
        if (y >= y1 && y < y1 + h && x >= x1 && x < x1 + w) {
            int ya, yb, xa, xb;
            double wy, wx;
            cn_bilinear(y - y1, W2L_IMG, h, &ya, &yb, &wy);
            cn_bilinear(x - x1, W2L_IMG, w, &xa, &xb, &wx);
            const float* src = faces + ((size_t)frame * 3 + (2 - c)) * W2L_IMG * W2L_IMG;
            v = (float)w2l_sample(src, W2L_IMG, 0, 0, ya, yb, xa, xb, wy, wx, false);
        }
        out[e] = v;
    }
}

// layouts: conv_net.hip's -- [n,C,H,W] -> NHWC with C padded to 16 and the consumer's zero halo, into a map or a slice of a CAT
// buffer (the destination's cell stride is an argument), and back

// ---- implicit-GEMM convolution ---------------------------------------------------------------------------------------------------
struct W2lConvArgs {
    const float* in;     // channel 0 of the block's input in [n, Hp, Wp, .] cells of istride floats, zero halo included
    const __bf16* w;     // the block's packed matrices, class after class, hi then lo
    const float* bias;   // [cout], batch norm folded in
    float* out;          // channel 0 of the block's output in [n, Hq, Wq, .] cells of ostride floats, every cell written
    int n, Ho, Wo, Hp, Wp, Hq, Wq, cinp, istride, cout, np, ostride, tr, sh, sw, ihalo, pad, opad, residual, ncls;
    W2lClass cls[W2L_MAX_CLASSES];
};

// 256 threads = 4 waves; wave tile t = 4 blockIdx.x + wave belongs to the class c with cls[c].tile0 <= t < cls[c + 1].tile0 and
// computes CN_TILE_M of its rows x 32 NT channels, the channel tile fastest.  A k-step is 16 channels of one tap.
template <int NT>
__global__ __launch_bounds__(256) void wav2lip_conv_kernel(W2lConvArgs a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const long long tile = (long long)blockIdx.x * 4 + wave;
    W2lClass k = a.cls[0];
#pragma unroll
    for (int c = 1; c < W2L_MAX_CLASSES; ++c)
        if (c < a.ncls && tile >= a.cls[c].tile0) k = a.cls[c];
    const long long Mc = w2l_class_rows(&k, a.n);
    const int ntn = a.np / (32 * NT);
    const long long lt = tile - k.tile0;
    const long long m0 = lt / ntn * CN_TILE_M;
    if (m0 >= Mc) return;  // no barriers in this kernel: an idle wave may leave
    const int nt0 = (int)(lt % ntn) * NT;
    const int taps = k.tkh * k.tkw;
    const __bf16* whi = a.w + k.woff;
    const __bf16* wlo = whi + (size_t)taps * a.cinp * a.np;
    const float* base[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int img, yq, xq;
        w2l_row_cell(m0 + mt * 32 + r, Mc, k.oy, k.ox, k.Hc, k.Wc, k.step, &img, &yq, &xq);  // rows past Mc: the last cell again, never stored
        const int y = cn_clampi(yq - a.opad, 0, a.Ho - 1), x = cn_clampi(xq - a.opad, 0, a.Wo - 1);
        base[mt] = a.in + w2l_cell(img, w2l_in_cell(y, a.tr, a.sh, a.ihalo, a.pad), w2l_in_cell(x, a.tr, a.sw, a.ihalo, a.pad), a.Hp, a.Wp, a.istride);
    }
    conv_f32x16 acc[2][NT];
    CONV_ZERO_ACC(acc, NT);
    float av[2][8];

    int s = 0;
    for (int tap = 0; tap < taps; ++tap) {
        const size_t toff = w2l_tap_offset(tap, k.tkw, a.Wp, a.istride) + 8 * h;
        for (int c0 = 0; c0 < a.cinp; c0 += 16, ++s) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) conv_load8(base[mt] + toff + c0, av[mt]);
            conv_mma_step<true, NT>(whi, wlo, a.np, s, nt0, lane, av, acc);
        }
    }

    // epilogue: accumulator register i of lane (r, h) is row cf_acc_row(i, h) of the tile, column r.
    // conv + folded bias, then the block's own input, then ReLU (wav_models/conv.py:15-19, 42-44); 0 in the halo.
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long m = m0 + mt * 32 + cf_acc_row(i, h);
            if (m >= Mc) continue;
            int img, yq, xq;
            w2l_row_cell(m, Mc, k.oy, k.ox, k.Hc, k.Wc, k.step, &img, &yq, &xq);
            const bool inside = cn_interior(yq, xq, a.Ho, a.Wo, a.opad);
            float* o = a.out + w2l_cell(img, yq, xq, a.Hq, a.Wq, a.ostride);
            const float* res = nullptr;
            if (inside && a.residual) res = a.in + w2l_cell(img, yq - a.opad + a.ihalo, xq - a.opad + a.ihalo, a.Hp, a.Wp, a.istride);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int co = (nt0 + nt) * 32 + r;
                if (co >= a.cout) continue;  // the zero columns of a matrix padded to 32 are never stored
                float v = 0.0f;
                if (inside) {
                    v = acc[mt][nt][i] + a.bias[co];
                    if (res) v += res[co];
                    v = v > 0.0f ? v : 0.0f;
                }
                o[co] = v;
            }
        }
}

// ---- head ------------------------------------------------------------------------------------------------------------------------
// one thread per pixel of in [n, 96, 96, 32] (no halo): three dot products of 32 in float64, channel order, then 1 / (1 + exp(-v))
// where `sigmoid`; out [n, 3, 96, 96]
__global__ __launch_bounds__(256) void wav2lip_head_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                           int n, int sigmoid, float* __restrict__ out) {
    const size_t hw = (size_t)W2L_IMG * W2L_IMG, total = (size_t)n * hw;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t img = e / hw, p = e - img * hw;
        double acc[W2L_OUT_C];
#pragma unroll
        for (int o = 0; o < W2L_OUT_C; ++o) acc[o] = (double)bias[o];
#pragma unroll
        for (int c0 = 0; c0 < W2L_HEAD_C; c0 += 8) {
            float x[8];
            conv_load8(in + e * W2L_HEAD_C + c0, x);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int o = 0; o < W2L_OUT_C; ++o) acc[o] = fma((double)x[j], (double)w[o * W2L_HEAD_C + c0 + j], acc[o]);
        }
#pragma unroll
        for (int o = 0; o < W2L_OUT_C; ++o) {
            const double v = sigmoid ? 1.0 / (1.0 + exp(-acc[o])) : acc[o];
            out[(img * W2L_OUT_C + o) * hw + p] = (float)v;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// workspace: the seven CAT buffers (the retained skip features with the decoder's part beside them) and two maps that the other
// blocks alternate between
struct W2lWorkspace {
    size_t cat[W2L_CATS], map[2], total;  // byte offsets
};

static W2lWorkspace w2l_workspace(int n) {
    W2lWorkspace w;
    size_t off = 0;
    auto take = [&off](size_t floats) {
        const size_t at = off;
        off += rup(floats * sizeof(float), 256);
        return at;
    };
    for (int j = 0; j < W2L_CATS; ++j) w.cat[j] = take((size_t)n * w2l_cat_elems(j));
    w.map[0] = take((size_t)n * w2l_max_map_elems());
    w.map[1] = take((size_t)n * w2l_max_map_elems());
    w.total = off;
    return w;
}

extern "C" size_t n3dt_wav2lip_packed_layout_bytes(void) { return w2l_layout().total; }
extern "C" size_t n3dt_wav2lip_ws_bytes(int n) { return w2l_workspace(n).total; }

extern "C" void n3dt_launch_wav2lip_pack(const N3dtWav2lipParams* p, void* packed, hipStream_t st) {
    const W2lPackLayout L = w2l_layout();
    char* base = (char*)packed;
    for (int b = 0; b < W2L_HEAD; ++b) {
        const W2lGeom g = w2l_geom(b);
        W2lClass cls[W2L_MAX_CLASSES];
        long long tiles;
        const int ncls = w2l_classes(&g, 1, 1, cls, &tiles);
        for (int c = 0; c < ncls; ++c) {
            const int Kc = cls[c].tkh * cls[c].tkw * g.cinp;
            const size_t elems = (size_t)Kc * g.np;
            __bf16* hi = (__bf16*)(base + L.w[b]) + cls[c].woff;
            const int4 kidx = make_int4(cls[c].kidx[0], cls[c].kidx[1], cls[c].kidx[2], cls[c].kidx[3]);
            wav2lip_pack_kernel<<<(unsigned)((elems + 255) / 256), 256, 0, st>>>(p->weight[b], p->bn_weight[b], p->bn_var[b], g.tr, g.cin, g.cinp,
                                                                                 g.cout, g.np, g.kh * g.kw, Kc, !g.tr, kidx, hi, hi + elems);
        }
        conv_net_bias_bn(p->bias[b], p->bn_weight[b], p->bn_bias[b], p->bn_mean[b], p->bn_var[b], SN_BN_EPS, g.cout, (float*)(base + L.bias[b]), st);
    }
    wav2lip_head_pack_kernel<<<1, 128, 0, st>>>(p->weight[W2L_HEAD], p->bias[W2L_HEAD], (float*)(base + L.w[W2L_HEAD]), (float*)(base + L.bias[W2L_HEAD]));
}

extern "C" void n3dt_launch_wav2lip_face_inputs(int n, int height, int width, const float* frames, const float* ref_frames, const int* boxes,
                                                int box_stride, float* out, hipStream_t st) {
    wav2lip_face_inputs_kernel<<<conv_grid((size_t)n * W2L_FACE_C * W2L_IMG * W2L_IMG), 256, 0, st>>>(n, height, width, frames,
                                                                                                     ref_frames ? ref_frames : frames, boxes, box_stride, out);
}

extern "C" void n3dt_launch_wav2lip_paste(int n, int height, int width, const float* faces, const float* frames, const int* boxes, int box_stride,
                                          float* out, hipStream_t st) {
    wav2lip_paste_kernel<<<conv_grid((size_t)n * 3 * height * width), 256, 0, st>>>(n, height, width, faces, frames, boxes, box_stride, out);
}

// block `block` (not the head) on `in` (channel 0 of its input, cells of istride floats) -> `out` (cells of ostride floats)
static void w2l_conv(int block, int n, const void* packed, const float* in, int istride, float* out, int ostride, hipStream_t st) {
    const W2lPackLayout L = w2l_layout();
    const W2lGeom g = w2l_geom(block);
    const char* pk = (const char*)packed;
    W2lConvArgs a;
    a.in = in;
    a.w = (const __bf16*)(pk + L.w[block]);
    a.bias = (const float*)(pk + L.bias[block]);
    a.out = out;
    a.n = n;
    a.Ho = g.Ho; a.Wo = g.Wo; a.Hp = g.Hp; a.Wp = g.Wp; a.Hq = g.Hq; a.Wq = g.Wq;
    a.cinp = g.cinp; a.istride = istride; a.cout = g.cout; a.np = g.np; a.ostride = ostride;
    a.tr = g.tr; a.sh = g.sh; a.sw = g.sw; a.ihalo = g.ihalo; a.pad = g.pad; a.opad = g.opad; a.residual = g.residual;
    const int nt = w2l_wave_ntiles(&g, n);
    long long tiles;
    a.ncls = w2l_classes(&g, n, nt, a.cls, &tiles);
    for (int c = a.ncls; c < W2L_MAX_CLASSES; ++c) a.cls[c] = a.cls[0];
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    if (nt == 1) wav2lip_conv_kernel<1><<<grid, 256, 0, st>>>(a);
    else wav2lip_conv_kernel<2><<<grid, 256, 0, st>>>(a);
}

static void w2l_head(int n, const void* packed, const float* in, int sigmoid, float* out, hipStream_t st) {
    const W2lPackLayout L = w2l_layout();
    const char* pk = (const char*)packed;
    wav2lip_head_kernel<<<conv_grid((size_t)n * W2L_IMG * W2L_IMG), 256, 0, st>>>(in, (const float*)(pk + L.w[W2L_HEAD]),
                                                                                   (const float*)(pk + L.bias[W2L_HEAD]), n, sigmoid, out);
}

extern "C" void n3dt_launch_wav2lip_fwd(int n, const void* packed, const float* mel, const float* faces, float* out, void* workspace, hipStream_t st) {
    const W2lWorkspace w = w2l_workspace(n);
    char* ws = (char*)workspace;
    float* map[2] = {(float*)(ws + w.map[0]), (float*)(ws + w.map[1])};
    float* cur = map[0];  // the map the last block outside the CAT buffers wrote
    for (int b = 0; b < W2L_HEAD; ++b) {
        const W2lGeom g = w2l_geom(b);
        if (b == 0 || b == W2L_FIRST_AUDIO) {
            cur = map[0];
            conv_net_to_nhwc(b == 0 ? faces : mel, n, g.cin, g.Hi, g.Wi, g.ihalo, g.cinp, cur, g.cinp, st);
        }
        const float* in = g.in_cat >= 0 ? (const float*)(ws + w.cat[g.in_cat]) + g.in_off : cur;
        float* dst = g.out_cat >= 0 ? (float*)(ws + w.cat[g.out_cat]) + g.out_off : (g.in_cat < 0 && cur == map[0]) ? map[1] : map[0];
        w2l_conv(b, n, packed, in, g.istride, dst, g.out_stride, st);
        if (g.out_cat < 0) cur = dst;
    }
    w2l_head(n, packed, cur, 1, out, st);
}

// one block alone: in [n, C_in, Hi, Wi] (and, for a block that ends in a concatenation, skip [n, C - C_out, Ho, Wo]) ->
// out [n, C_out, Ho, Wo] (or [n, C, Ho, Wo]); the head gives its logits.  The input is laid out where the chain holds it: a
// block that reads a CAT buffer gets its input in that buffer's slice, with the buffer's row stride (the two maps are sized for
// the inputs outside the CAT buffers only); every other block in map 0.  Outputs go to map 1, or to the CAT buffer with `skip`.
extern "C" void n3dt_launch_wav2lip_block(int block, int n, const void* packed, const float* in, const float* skip, float* out, void* workspace,
                                          hipStream_t st) {
    const W2lWorkspace w = w2l_workspace(n);
    const W2lGeom g = w2l_geom(block);
    char* ws = (char*)workspace;
    float* src = g.in_cat >= 0 ? (float*)(ws + w.cat[g.in_cat]) + g.in_off : (float*)(ws + w.map[0]);
    float* map1 = (float*)(ws + w.map[1]);
    conv_net_to_nhwc(in, n, g.cin, g.Hi, g.Wi, g.ihalo, g.cinp, src, g.istride, st);
    if (block == W2L_HEAD) {
        w2l_head(n, packed, src, 0, out, st);
        return;
    }
    if (skip && block >= W2L_FIRST_DEC && g.out_cat >= 0) {  // these blocks read a map of their own: the CAT buffer is free
        const int j = g.out_cat, C = W2L_CAT_C[j], A = W2L_CAT_A[j];
        float* cat = (float*)(ws + w.cat[j]);
        conv_net_to_nhwc(skip, n, C - A, g.Ho, g.Wo, g.opad, C - A, cat + A, C, st);
        w2l_conv(block, n, packed, src, g.istride, cat, C, st);
        conv_net_to_nchw(cat, C, n, C, g.Ho, g.Wo, g.opad, out, st);
        return;
    }
    w2l_conv(block, n, packed, src, g.istride, map1, g.cout, st);
    conv_net_to_nchw(map1, g.cout, n, g.cout, g.Ho, g.Wo, g.opad, out, st);
}
