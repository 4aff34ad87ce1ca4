/*
 * head_mask_core.h -- the table, the run-time geometry and the index arithmetic of n3dt_head_mask (include/n3dt.h): the reference's
 * DataProcess/BiSeNet.py face parser on DataProcess/resnet.py's ResNet-18, frozen, inference only, and the integer post-process of
 * DataProcess/Gen_HeadMask.py and correct_head_mask.py behind it.
 *
 * Included by csrc/head_mask.hip, whose kernels take their sizes and addresses from the functions below, and by
 * tests/head_mask_core_host.cpp, which walks the same functions over the kernels' grids on the CPU.  The rows of the implicit GEMM,
 * the stem's gather, the pool's window and the wave-tile rule are conv_net_core.h's, the fragment arithmetic conv_frag.h's.
 * Compiles as host C++ on its own.
 *
 * Blocks.  37 of them: 0..35 the convolutions in state-dict order (cp.resnet: conv1, then per BasicBlock conv1, conv2 and, where
 * the channels or the stride change, downsample.0; cp.arm16: conv, conv_atten; cp.arm32: conv, conv_atten; cp.conv_head32;
 * cp.conv_head16; cp.conv_avg; ffm: convblk, conv1, conv2; then per head conv, conv_out), 36 the 3 x 3 / 2 max pool.
 *
 * Maps.  NHWC fp32 WITHOUT halos, except the image in front of the stem (3 pixels, as face_recon's): the convolution kernel tests
 * every tap against the extent of its input and reads 0 outside it.  A consumer may read its input through a nearest upsample
 * (Hs x Ws -> Hi x Wi), a per-(image, channel) scale and an added term -- a per-(image, channel) vector, a second map at the
 * source's own resolution, or the value itself -- so that the attention-refined sums of the context path and the feature-fusion
 * module's output are never written: the padding's zeros lie behind that transform.  A head's n_classes columns are padded to 32.
 */
#ifndef N3DT_HEAD_MASK_CORE_H
#define N3DT_HEAD_MASK_CORE_H

#include <math.h>
#include <stdint.h>

#include "conv_net_core.h"

#define HM_CONVS 36
#define HM_BLOCKS 37
#define HM_POOL_BLOCK 36
#define HM_MAX_CLASSES 32
#define HM_MIN_HW 32
#define HM_MAX_IMAGES 1024
#define HM_WS_BUDGET ((size_t)4 << 30)
#define HM_MAX_STEPS 40
#define HM_MAX_ELEMENT 64 /* the eye mask's structuring element: at most 64 x 64 */

enum { HM_STEM = 0, HM_SPATIAL = 1, HM_SMALL = 2 };    /* kind */
enum { HM_NONE = 0, HM_RELU = 1, HM_SIGMOID = 2 };     /* activation */

/* C_in, C_out (0: n_classes, packed as 32 columns), kernel, stride, padding, kind, activation, BatchNorm behind it */
typedef struct HmConv {
    int cin, cout, k, stride, pad, kind, act, bn;
} HmConv;

static const HmConv HM_TABLE[HM_CONVS] = {
    {3, 64, 7, 2, 3, HM_STEM, HM_RELU, 1},
    {64, 64, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},     {64, 64, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},   /* layer1.0 */
    {64, 64, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},     {64, 64, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},   /* layer1.1 */
    {64, 128, 3, 2, 1, HM_SPATIAL, HM_RELU, 1},    {128, 128, 3, 1, 1, HM_SPATIAL, HM_RELU, 1}, {64, 128, 1, 2, 0, HM_SPATIAL, HM_NONE, 1},
    {128, 128, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},   {128, 128, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},
    {128, 256, 3, 2, 1, HM_SPATIAL, HM_RELU, 1},   {256, 256, 3, 1, 1, HM_SPATIAL, HM_RELU, 1}, {128, 256, 1, 2, 0, HM_SPATIAL, HM_NONE, 1},
    {256, 256, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},   {256, 256, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},
    {256, 512, 3, 2, 1, HM_SPATIAL, HM_RELU, 1},   {512, 512, 3, 1, 1, HM_SPATIAL, HM_RELU, 1}, {256, 512, 1, 2, 0, HM_SPATIAL, HM_NONE, 1},
    {512, 512, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},   {512, 512, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},
    {256, 128, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},   {128, 128, 1, 1, 0, HM_SMALL, HM_SIGMOID, 1}, /* arm16 */
    {512, 128, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},   {128, 128, 1, 1, 0, HM_SMALL, HM_SIGMOID, 1}, /* arm32 */
    {128, 128, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},                                                  /* conv_head32 */
    {128, 128, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},                                                  /* conv_head16 */
    {512, 128, 1, 1, 0, HM_SMALL, HM_RELU, 1},                                                    /* conv_avg */
    {256, 256, 1, 1, 0, HM_SPATIAL, HM_RELU, 1},   {256, 64, 1, 1, 0, HM_SMALL, HM_RELU, 0},     {64, 256, 1, 1, 0, HM_SMALL, HM_SIGMOID, 0}, /* ffm */
    {256, 256, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},   {256, 0, 1, 1, 0, HM_SPATIAL, HM_NONE, 0},    /* conv_out */
    {128, 64, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},    {64, 0, 1, 1, 0, HM_SPATIAL, HM_NONE, 0},     /* conv_out16 */
    {128, 64, 3, 1, 1, HM_SPATIAL, HM_RELU, 1},    {64, 0, 1, 1, 0, HM_SPATIAL, HM_NONE, 0},     /* conv_out32 */
};

enum {
    HM_ARM16 = 20, HM_ARM16_ATT = 21, HM_ARM32 = 22, HM_ARM32_ATT = 23, HM_HEAD32 = 24, HM_HEAD16 = 25, HM_AVG = 26,
    HM_FFM_BLK = 27, HM_FFM_1 = 28, HM_FFM_2 = 29, HM_OUT = 30, HM_OUT16 = 32, HM_OUT32 = 34
};

/* the packed matrix's columns: a head's n_classes padded to one 32-column tile */
static inline int hm_np(int j) { return HM_TABLE[j].cout ? HM_TABLE[j].cout : HM_MAX_CLASSES; }
static inline int hm_cout(int j, int n_classes) { return HM_TABLE[j].cout ? HM_TABLE[j].cout : n_classes; }
static inline int hm_K(int j) { return HM_TABLE[j].kind == HM_STEM ? CN_STEM_KP : HM_TABLE[j].k * HM_TABLE[j].k * HM_TABLE[j].cin; }
/* a BasicBlock's second convolution adds the shortcut in front of its ReLU */
static inline int hm_takes_skip(int j) { return j == 2 || j == 4 || j == 6 || j == 9 || j == 11 || j == 14 || j == 16 || j == 19; }

CN_HD int hm_hw_ok(int H, int W) { return H >= HM_MIN_HW && W >= HM_MIN_HW && H <= CN_MAX_FRAME_HW && W <= CN_MAX_FRAME_HW; }

/* ---- addresses -------------------------------------------------------------------------------------------------------------------
 * F.interpolate(mode='nearest'): destination index dst of `out` reads source index min(int(floorf(dst * float(in) / out)), in - 1),
 * in float32 as torch computes it; an equal size is the identity */
CN_HD int hm_nearest(int dst, int in, int out) {
    if (in == out) return dst;
    const float scale = (float)in / (float)out;
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}

/* tap (ky, kx) = (tap / k, tap % k) of output pixel (yo, xo): the pixel (iy, ix) = (yo stride + ky - pad, ..) of the Hi x Wi input,
 * which is cell (hm_nearest(iy), hm_nearest(ix)) of the Hs x Ws source map [n, Hs, Ws]; returns 0 (and no cell) in the padding */
CN_HD int hm_tap_cell(int img, int yo, int xo, int tap, int k, int stride, int pad, int Hi, int Wi, int Hs, int Ws, long long* cell) {
    const int ky = tap / k, kx = tap - ky * k;
    const int iy = yo * stride + ky - pad, ix = xo * stride + kx - pad;
    if (iy < 0 || iy >= Hi || ix < 0 || ix >= Wi) return 0;
    *cell = ((long long)img * Hs + hm_nearest(iy, Hs, Hi)) * Ws + hm_nearest(ix, Ws, Wi);
    return 1;
}

/* F.interpolate(mode='bilinear', align_corners=True) along one axis, float64: src = d (in - 1) / (out - 1) */
CN_HD void hm_lerp(int d, int in, int out, int* i0, int* i1, double* w1) {
    const double scale = out > 1 ? (double)(in - 1) / (double)(out - 1) : 0.0;
    const double src = scale * (double)d;
    int a = (int)src;
    if (a > in - 1) a = in - 1;
    *i0 = a;
    *i1 = a < in - 1 ? a + 1 : a;
    *w1 = src - (double)a;
}

/* OpenCV's 8-bit hue of cvtColor(.., COLOR_BGR2HSV) for the bytes it is handed as (b, g, r): range 180, 12 fractional bits, the
 * divisor table rounded to nearest-even as its saturate_cast does */
CN_HD int hm_hue(int b, int g, int r) {
    int v = b > g ? b : g, vmin = b < g ? b : g;
    if (r > v) v = r;
    if (r < vmin) vmin = r;
    const int diff = v - vmin;
    if (diff == 0) return 0;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    const int hdiv = (int)rint((double)(180 << 12) / (6.0 * (double)diff));
    int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    h = (h * hdiv + (1 << 11)) >> 12;
    if (h < 0) h += 180;
    return h;
}

/* ---- the chain -------------------------------------------------------------------------------------------------------------------
 * regions of the workspace */
enum {
    HM_R_IMG = 0, HM_R_STEM, HM_R_P0, HM_R_P1, HM_R_T, HM_R_D, HM_R_F8, HM_R_F16, HM_R_F32, HM_R_ARM32, HM_R_ARM16, HM_R_CP16, HM_R_CP8,
    HM_R_FFM, HM_R_MID, HM_R_LOG0, HM_R_LOG1, HM_R_LOG2, HM_R_VEC, HM_REGIONS
};
/* the per-image vectors of the small stage, floats from the start of an image's row of HM_R_VEC */
enum { HM_V_AVG = 0, HM_V_ATT32 = 128, HM_V_ATT16 = 256, HM_V_FFM1 = 384, HM_V_FFM2 = 448, HM_VEC = 704 };

/* one launch.  A spatial convolution reads region `in` [n, Hs, Ws, C] (channels from `csplit` on: region `in2`) as an Hi x Wi map,
 * times vector `scale`, plus vector `addvec` / region `addmap` [n, Hs, Ws, C] / itself; adds region `skip`; writes region `out`.
 * A small convolution averages region `in` over Hi x Wi (or takes vector `invec`) and writes vector `out`. */
typedef struct HmStep {
    int block, Hi, Wi, Hs, Ws, in, in2, skip, addmap, scale, addvec, addself, invec, out;
} HmStep;

static inline HmStep hm_step(int block, int Hi, int Wi, int in, int out) {
    const HmStep s = {block, Hi, Wi, Hi, Wi, in, -1, -1, -1, -1, -1, 0, -1, out};
    return s;
}

static inline int hm_out_h(int j, int Hi) { return cn_conv_out(Hi, HM_TABLE[j].k, HM_TABLE[j].stride, HM_TABLE[j].pad); }

/* the sizes of the three feature maps and the stem's and pool's outputs for an H x W image */
typedef struct HmSizes {
    int H2, W2, H4, W4, H8, W8, H16, W16, H32, W32;
} HmSizes;

static inline HmSizes hm_sizes(int H, int W) {
    HmSizes z;
    z.H2 = hm_out_h(0, H); z.W2 = hm_out_h(0, W);
    z.H4 = cn_pool_out(z.H2); z.W4 = cn_pool_out(z.W2);
    z.H8 = hm_out_h(5, z.H4); z.W8 = hm_out_h(5, z.W4);
    z.H16 = hm_out_h(10, z.H8); z.W16 = hm_out_h(10, z.W8);
    z.H32 = hm_out_h(15, z.H16); z.W32 = hm_out_h(15, z.W16);
    return z;
}

/* the low-resolution size of output o (0: out, 1: out16 -- both at 1/8 -- 2: out32 at 1/16) */
static inline void hm_logit_hw(int H, int W, int o, int* h, int* w) {
    const HmSizes z = hm_sizes(H, W);
    *h = o == 2 ? z.H16 : z.H8;
    *w = o == 2 ? z.W16 : z.W8;
}

/* what the forward launches for the outputs in `outputs` (bit 0: out, 1: out16, 2: out32), in its order; returns the count */
static inline int hm_chain(int H, int W, int outputs, HmStep steps[HM_MAX_STEPS]) {
    const HmSizes z = hm_sizes(H, W);
    int s = 0;
    steps[s++] = hm_step(0, H, W, HM_R_IMG, HM_R_STEM);
    steps[s++] = hm_step(HM_POOL_BLOCK, z.H2, z.W2, HM_R_STEM, HM_R_P0);
    int h = z.H4, w = z.W4, cur = HM_R_P0, j = 1;
    const int keep[4] = {-1, HM_R_F8, HM_R_F16, HM_R_F32};
    for (int layer = 0; layer < 4; ++layer)
        for (int b = 0; b < 2; ++b) {
            const int down = layer > 0 && b == 0;
            const int ho = hm_out_h(j, h), wo = hm_out_h(j, w);
            const int nxt = (b == 1 && layer > 0) ? keep[layer] : (cur == HM_R_P0 ? HM_R_P1 : HM_R_P0);
            steps[s++] = hm_step(j, h, w, cur, HM_R_T);
            if (down) steps[s++] = hm_step(j + 2, h, w, cur, HM_R_D);
            HmStep c2 = hm_step(j + 1, ho, wo, HM_R_T, nxt);
            c2.skip = down ? HM_R_D : cur;
            steps[s++] = c2;
            cur = nxt;
            h = ho;
            w = wo;
            j += down ? 3 : 2;
        }
    HmStep t = hm_step(HM_AVG, z.H32, z.W32, HM_R_F32, HM_V_AVG);
    steps[s++] = t;
    steps[s++] = hm_step(HM_ARM32, z.H32, z.W32, HM_R_F32, HM_R_ARM32);
    steps[s++] = hm_step(HM_ARM32_ATT, z.H32, z.W32, HM_R_ARM32, HM_V_ATT32);
    t = hm_step(HM_HEAD32, z.H16, z.W16, HM_R_ARM32, HM_R_CP16);  /* up(arm32 * atten + avg) */
    t.Hs = z.H32; t.Ws = z.W32; t.scale = HM_V_ATT32; t.addvec = HM_V_AVG;
    steps[s++] = t;
    if (outputs & 3) {
        steps[s++] = hm_step(HM_ARM16, z.H16, z.W16, HM_R_F16, HM_R_ARM16);
        steps[s++] = hm_step(HM_ARM16_ATT, z.H16, z.W16, HM_R_ARM16, HM_V_ATT16);
        t = hm_step(HM_HEAD16, z.H8, z.W8, HM_R_ARM16, HM_R_CP8);  /* up(arm16 * atten + feat32_up) */
        t.Hs = z.H16; t.Ws = z.W16; t.scale = HM_V_ATT16; t.addmap = HM_R_CP16;
        steps[s++] = t;
    }
    if (outputs & 1) {
        t = hm_step(HM_FFM_BLK, z.H8, z.W8, HM_R_F8, HM_R_FFM);  /* cat(feat8, feat_cp8) as two channel slices */
        t.in2 = HM_R_CP8;
        steps[s++] = t;
        steps[s++] = hm_step(HM_FFM_1, z.H8, z.W8, HM_R_FFM, HM_V_FFM1);
        t = hm_step(HM_FFM_2, 1, 1, -1, HM_V_FFM2);
        t.invec = HM_V_FFM1;
        steps[s++] = t;
        t = hm_step(HM_OUT, z.H8, z.W8, HM_R_FFM, HM_R_MID);  /* feat * atten + feat */
        t.scale = HM_V_FFM2; t.addself = 1;
        steps[s++] = t;
        steps[s++] = hm_step(HM_OUT + 1, z.H8, z.W8, HM_R_MID, HM_R_LOG0);
    }
    if (outputs & 2) {
        steps[s++] = hm_step(HM_OUT16, z.H8, z.W8, HM_R_CP8, HM_R_MID);
        steps[s++] = hm_step(HM_OUT16 + 1, z.H8, z.W8, HM_R_MID, HM_R_LOG1);
    }
    if (outputs & 4) {
        steps[s++] = hm_step(HM_OUT32, z.H16, z.W16, HM_R_CP16, HM_R_MID);
        steps[s++] = hm_step(HM_OUT32 + 1, z.H16, z.W16, HM_R_MID, HM_R_LOG2);
    }
    return s;
}

/* a step's output map, elements per image (0 for a small step: it writes a vector) */
static inline size_t hm_step_out_elems(const HmStep* st) {
    if (st->block == HM_POOL_BLOCK) return (size_t)cn_pool_out(st->Hi) * cn_pool_out(st->Wi) * 64;
    if (HM_TABLE[st->block].kind == HM_SMALL) return 0;
    return (size_t)hm_out_h(st->block, st->Hi) * hm_out_h(st->block, st->Wi) * hm_np(st->block);
}

typedef struct HmWorkspace {
    size_t region[HM_REGIONS], bytes[HM_REGIONS], total;
} HmWorkspace;

/* sized for every output, whichever the call asks for */
static inline HmWorkspace hm_workspace(int n, int H, int W) {
    HmStep steps[HM_MAX_STEPS];
    const int count = hm_chain(H, W, 7, steps);
    size_t elems[HM_REGIONS];
    for (int r = 0; r < HM_REGIONS; ++r) elems[r] = 0;
    elems[HM_R_IMG] = (size_t)(H + 6) * (W + 6) * 3;
    elems[HM_R_VEC] = HM_VEC;
    for (int s = 0; s < count; ++s) {
        const size_t e = hm_step_out_elems(&steps[s]);
        if (e && e > elems[steps[s].out]) elems[steps[s].out] = e;
    }
    HmWorkspace w;
    size_t off = 0;
    for (int r = 0; r < HM_REGIONS; ++r) {
        w.region[r] = off;
        w.bytes[r] = cn_rup256((size_t)n * elems[r] * sizeof(float));
        off += w.bytes[r];
    }
    w.total = off;
    return w;
}

static inline int hm_max_images(int H, int W) {
    const size_t one = hm_workspace(1, H, W).total;
    size_t n = HM_WS_BUDGET / one;
    if (n > HM_MAX_IMAGES) n = HM_MAX_IMAGES;
    while (n > 1 && hm_workspace((int)n, H, W).total > HM_WS_BUDGET) --n;
    return n < 1 ? 1 : (int)n;
}

/* ---- one block alone: the input map (the stem's with its halo), the auxiliary map, the output map ------------------------------- */
typedef struct HmBlockWs {
    size_t in, aux, out, total;
} HmBlockWs;

static inline HmBlockWs hm_block_ws(int block, int n, int Hi, int Wi, int Hs, int Ws) {
    size_t in_e, out_e;
    if (block == HM_POOL_BLOCK) {
        in_e = (size_t)Hi * Wi * 64;
        out_e = (size_t)cn_pool_out(Hi) * cn_pool_out(Wi) * 64;
    } else if (HM_TABLE[block].kind == HM_STEM) {
        in_e = (size_t)(Hi + 6) * (Wi + 6) * 3;
        out_e = (size_t)hm_out_h(0, Hi) * hm_out_h(0, Wi) * 64;
    } else if (HM_TABLE[block].kind == HM_SMALL) {
        in_e = (size_t)Hi * Wi * HM_TABLE[block].cin;
        out_e = HM_TABLE[block].cout;
    } else {
        in_e = (size_t)Hs * Ws * HM_TABLE[block].cin;
        out_e = (size_t)hm_out_h(block, Hi) * hm_out_h(block, Wi) * hm_np(block);
    }
    HmBlockWs w;
    w.in = 0;
    w.aux = cn_rup256((size_t)n * in_e * sizeof(float));
    w.out = w.aux + cn_rup256((size_t)n * (in_e > out_e ? in_e : out_e) * sizeof(float));
    w.total = w.out + cn_rup256((size_t)n * out_e * sizeof(float));
    return w;
}

/* ---- the post-process's workspace: per pixel two int32 (parent, area), four bytes (the working image, two erosion / dilation
 * buffers, the original labels); per image one 64-bit key */
typedef struct HmPostWs {
    size_t parent, area, best, work, orig, a, b, total;
} HmPostWs;

static inline HmPostWs hm_post_ws(int n, int H, int W) {
    const size_t px = (size_t)n * H * W;
    HmPostWs w;
    size_t off = 0;
    w.parent = off; off += cn_rup256(px * 4);
    w.area = off;   off += cn_rup256(px * 4);
    w.best = off;   off += cn_rup256((size_t)n * 8);
    w.work = off;   off += cn_rup256(px);
    w.orig = off;   off += cn_rup256(px);
    w.a = off;      off += cn_rup256(px);
    w.b = off;      off += cn_rup256(px);
    w.total = off;
    return w;
}

#endif
