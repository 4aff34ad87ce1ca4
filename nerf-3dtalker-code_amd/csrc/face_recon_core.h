/*
 * face_recon_core.h -- the geometry table and the index arithmetic of n3dt_face_recon (include/n3dt.h): Deep3DFaceRecon's
 * ResNet-50 coefficient regressor (the reference's s_face3d/models/networks.py, ReconNetWrapper over resnet50 with
 * use_last_fc=False) behind the crop of s_face3d/util/preprocess.py's align_img, frozen, inference only.
 *
 * Included by csrc/face_recon.hip, whose kernels take their sizes and addresses from the functions below, and by
 * tests/face_recon_core_host.cpp, which walks the same functions over the kernels' grids on the CPU under the address and
 * undefined-behaviour sanitizers.  The rows of the implicit GEMM, the halo test, the receptive field's base, the stem's gather, the pool's window and the
 * wave-tile rule are conv_net_core.h's; the fragment arithmetic is conv_frag.h's.  Compiles as host C++ on its own.
 *
 * Blocks.  56 of them: 0..52 the convolutions in state-dict order (conv1; then per bottleneck conv1, conv2, conv3 and, in the
 * first bottleneck of a layer, downsample.0), 53 the 3 x 3 / 2 max pool, 54 the global average, 55 the 257-column head.
 *
 * Maps.  NHWC fp32.  A map carries the zero halo its only consumer's padding needs: 3 on the image in front of the stem, 1 on a
 * bottleneck's conv1 output in front of its 3 x 3, 0 everywhere else (the max pool tests its taps instead).  The image keeps its 3
 * channels: the stem's K is (tap, channel) flattened, 7 x 7 x 3 = 147 padded to 160, and since (kx, c) is contiguous in NHWC a
 * k below 147 lies at ky * Wp * 3 + (k - 21 ky) floats from the field's base.  The map sizes are known only at run time:
 * everything here is a function of the image's (H, W).
 */
#ifndef N3DT_FACE_RECON_CORE_H
#define N3DT_FACE_RECON_CORE_H

#include <math.h>

#include "conv_net_core.h"

#define FR_CONVS 53
#define FR_BOTTLENECKS 16
#define FR_BLOCKS 56
#define FR_POOL_BLOCK 53
#define FR_AVG_BLOCK 54
#define FR_HEAD_BLOCK 55
#define FR_FEAT 2048
#define FR_COEFFS 257
#define FR_HEADS 7
#define FR_MIN_HW 32
#define FR_MAX_IMAGES 1024
#define FR_WS_BUDGET ((size_t)4 << 30) /* bytes of workspace one call may ask for: caps n */
#define FR_REGIONS 6                   /* two block maps, downsample / stem, conv1, conv2, the averages */
#define FR_CROP 224
#define FR_RESCALE 102.0
#define FR_MIN_SCALE (1.0 / 16.0)
#define FR_MAX_SCALE 16.0

static const int FR_HEAD_COLS[FR_HEADS] = {80, 64, 80, 3, 27, 2, 1}; /* id, exp, tex, angle, gamma, (tx, ty), tz */
static const int FR_LAYER_BLOCKS[4] = {3, 4, 6, 3};

/* role of a convolution inside its bottleneck */
enum { FR_STEM = 0, FR_CONV1 = 1, FR_CONV2 = 2, FR_CONV3 = 3, FR_DOWN = 4 };

/* C_in, C_out, kernel, stride, padding, role, ReLU, the halo of its output */
typedef struct FrConv {
    int cin, cout, k, stride, pad, role, relu, opad;
} FrConv;

/* convolution j of the 53 in state-dict order */
static inline FrConv fr_conv(int j) {
    FrConv c = {3, 64, 7, 2, 3, FR_STEM, 1, 0};
    if (j == 0) return c;
    int at = 1, inplanes = 64;
    for (int layer = 0; layer < 4; ++layer) {
        const int planes = 64 << layer;
        for (int b = 0; b < FR_LAYER_BLOCKS[layer]; ++b) {
            const int stride = (b == 0 && layer > 0) ? 2 : 1, count = b == 0 ? 4 : 3;
            if (j < at + count) {
                const int role = FR_CONV1 + (j - at);
                const FrConv c1 = {inplanes, planes, 1, 1, 0, FR_CONV1, 1, 1};
                const FrConv c2 = {planes, planes, 3, stride, 1, FR_CONV2, 1, 0};
                const FrConv c3 = {planes, planes * 4, 1, 1, 0, FR_CONV3, 1, 0};
                const FrConv cd = {inplanes, planes * 4, 1, stride, 0, FR_DOWN, 0, 0};
                return role == FR_CONV1 ? c1 : role == FR_CONV2 ? c2 : role == FR_CONV3 ? c3 : cd;
            }
            at += count;
            inplanes = planes * 4;
        }
    }
    return c; /* not reached for j < FR_CONVS */
}

/* the first convolution of bottleneck b (0..15), and whether it has a downsample branch */
static inline int fr_bottleneck_first(int b) {
    int at = 1, k = 0;
    for (int layer = 0; layer < 4; ++layer)
        for (int i = 0; i < FR_LAYER_BLOCKS[layer]; ++i, ++k) {
            if (k == b) return at;
            at += i == 0 ? 4 : 3;
        }
    return at;
}
static inline int fr_bottleneck_down(int b) { return b == 0 || b == 3 || b == 7 || b == 13; }

/* one GEMM: input [n, Hp, Wp, cinp] with halo pad (its own padding), output [n, Hq, Wq, cout] with halo opad; K = the packed
 * matrix's rows: k k cin, for the stem 160 */
typedef struct FrGeom {
    int Hi, Wi, Ho, Wo, Hp, Wp, Hq, Wq, cin, cinp, cout, pad, opad, k, stride, K, relu, role;
} FrGeom;

static inline FrGeom fr_geom(int j, int Hi, int Wi) {
    const FrConv t = fr_conv(j);
    FrGeom g;
    g.Hi = Hi;
    g.Wi = Wi;
    g.Ho = cn_conv_out(Hi, t.k, t.stride, t.pad);
    g.Wo = cn_conv_out(Wi, t.k, t.stride, t.pad);
    g.pad = t.pad;
    g.opad = t.opad;
    g.Hp = Hi + 2 * t.pad;
    g.Wp = Wi + 2 * t.pad;
    g.Hq = g.Ho + 2 * t.opad;
    g.Wq = g.Wo + 2 * t.opad;
    g.cin = t.cin;
    g.cinp = t.role == FR_STEM ? 3 : t.cin; /* every other C_in is a multiple of 64 */
    g.cout = t.cout;
    g.k = t.k;
    g.stride = t.stride;
    g.K = t.role == FR_STEM ? CN_STEM_KP : t.k * t.k * t.cin;
    g.relu = t.relu;
    g.role = t.role;
    return g;
}

static inline size_t fr_in_elems(const FrGeom* g, int n) { return (size_t)n * g->Hp * g->Wp * g->cinp; }
static inline size_t fr_out_elems(const FrGeom* g, int n) { return (size_t)n * g->Hq * g->Wq * g->cout; }

CN_HD int fr_hw_ok(int H, int W) { return H >= FR_MIN_HW && W >= FR_MIN_HW && H <= CN_MAX_FRAME_HW && W <= CN_MAX_FRAME_HW; }

/* ---- the chain -------------------------------------------------------------------------------------------------------------------
 * what the forward launches, in its order: 53 convolutions, the pool and the average (the head reads the averages and writes the
 * caller's buffer).  Regions of the workspace: 0 and 1 the bottlenecks' input and output in turn (1 first holds the image),
 * 2 the stem's output, then a downsample branch, 3 conv1's output, 4 conv2's, 5 the averages. */
typedef struct FrStep {
    int block, Hi, Wi, in, skip, out; /* regions; skip -1: none */
} FrStep;

#define FR_STEPS (FR_CONVS + 2)

static inline void fr_chain(int H, int W, FrStep steps[FR_STEPS]) {
    int s = 0;
    const FrGeom stem = fr_geom(0, H, W);
    const FrStep s0 = {0, H, W, 1, -1, 2};
    steps[s++] = s0;
    const FrStep sp = {FR_POOL_BLOCK, stem.Ho, stem.Wo, 2, -1, 0};
    steps[s++] = sp;
    int h = cn_pool_out(stem.Ho), w = cn_pool_out(stem.Wo), cur = 0;
    for (int b = 0; b < FR_BOTTLENECKS; ++b) {
        const int j = fr_bottleneck_first(b), down = fr_bottleneck_down(b);
        const FrGeom g2 = fr_geom(j + 1, h, w);
        const FrStep c1 = {j, h, w, cur, -1, 3}, c2 = {j + 1, h, w, 3, -1, 4};
        steps[s++] = c1;
        steps[s++] = c2;
        if (down) {
            const FrStep cd = {j + 3, h, w, cur, -1, 2};
            steps[s++] = cd;
        }
        const FrStep c3 = {j + 2, g2.Ho, g2.Wo, 4, down ? 2 : cur, 1 - cur};
        steps[s++] = c3;
        cur = 1 - cur;
        h = g2.Ho;
        w = g2.Wo;
    }
    const FrStep sa = {FR_AVG_BLOCK, h, w, cur, -1, 5};
    steps[s++] = sa;
}

/* the pool's output map [n, Ho, Wo, 64], no halo */
static inline size_t fr_step_out_elems(const FrStep* st) {
    if (st->block == FR_POOL_BLOCK) return (size_t)cn_pool_out(st->Hi) * cn_pool_out(st->Wi) * 64;
    if (st->block == FR_AVG_BLOCK) return FR_FEAT;
    const FrGeom g = fr_geom(st->block, st->Hi, st->Wi);
    return fr_out_elems(&g, 1);
}

typedef struct FrWorkspace {
    size_t region[FR_REGIONS], bytes[FR_REGIONS], total;
} FrWorkspace;

static inline FrWorkspace fr_workspace(int n, int H, int W) {
    FrStep steps[FR_STEPS];
    fr_chain(H, W, steps);
    size_t elems[FR_REGIONS] = {0, 0, 0, 0, 0, 0};
    elems[1] = (size_t)(H + 6) * (W + 6) * 3; /* the image with the stem's halo */
    for (int s = 0; s < FR_STEPS; ++s) {
        const size_t e = fr_step_out_elems(&steps[s]);
        if (e > elems[steps[s].out]) elems[steps[s].out] = e;
    }
    FrWorkspace w;
    size_t off = 0;
    for (int r = 0; r < FR_REGIONS; ++r) {
        w.region[r] = off;
        w.bytes[r] = cn_rup256((size_t)n * elems[r] * sizeof(float));
        off += w.bytes[r];
    }
    w.total = off;
    return w;
}

/* the most images one call takes at H x W: the workspace budget, and FR_MAX_IMAGES */
static inline int fr_max_images(int H, int W) {
    const size_t one = fr_workspace(1, H, W).total;
    size_t n = FR_WS_BUDGET / one;
    if (n > FR_MAX_IMAGES) n = FR_MAX_IMAGES;
    while (n > 1 && fr_workspace((int)n, H, W).total > FR_WS_BUDGET) --n;
    return (int)n;
}

/* ---- the alignment prologue, float64 ---------------------------------------------------------------------------------------------
 * PIL's bicubic filter, a = -0.5 */
CN_HD double fr_cubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

/* PIL's resample along one axis of `in` source samples to `out`: output index o takes source samples [*lo, *hi) with weights
 * fr_cubic((x - *center + 0.5) / *fs), normalised by their sum */
CN_HD void fr_taps(int o, int in, int out, int* lo, int* hi, double* center, double* fs) {
    const double scale = (double)in / (double)out;
    const double f = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * f, c = ((double)o + 0.5) * scale;
    int a = (int)(c - support + 0.5), b = (int)(c + support + 0.5);
    if (a < 0) a = 0;
    if (b > in) b = in;
    *lo = a;
    *hi = b;
    *center = c;
    *fs = f;
}

/* truncation toward zero as astype(int32) does it, for a finite value inside the int range (the status test comes first) */
CN_HD int fr_trunc(double v) {
    if (!(v > -2.0e9)) v = -2.0e9;
    if (v > 2.0e9) v = 2.0e9;
    return (int)v;
}

/* the similarity of one frame: lm5 [5][2] image landmarks with y already flipped, pinv [4][5] the pseudo-inverse of
 * [lm3d_std, 1] -> trans (w0, h0, s, t0, t1), geom (w, h, left, up); returns the status (0: fine) */
CN_HD int fr_similarity(const double lm5[5][2], const double* pinv, int W0, int H0, double trans[5], int geom[4]) {
    double k[2][4];
    int finite = 1;
    for (int a = 0; a < 2; ++a)
        for (int r = 0; r < 4; ++r) {
            double s = 0.0;
            for (int p = 0; p < 5; ++p) s += pinv[r * 5 + p] * lm5[p][a];
            k[a][r] = s;
            if (!(s - s == 0.0)) finite = 0;
        }
    const double n1 = sqrt(k[0][0] * k[0][0] + k[0][1] * k[0][1] + k[0][2] * k[0][2]);
    const double n2 = sqrt(k[1][0] * k[1][0] + k[1][1] * k[1][1] + k[1][2] * k[1][2]);
    const double s = FR_RESCALE / ((n1 + n2) / 2.0);
    const double t0 = k[0][3], t1 = k[1][3], w0 = (double)W0, h0 = (double)H0;
    trans[0] = w0;
    trans[1] = h0;
    trans[2] = s;
    trans[3] = t0;
    trans[4] = t1;
    geom[0] = geom[1] = geom[2] = geom[3] = 0;
    if (!finite || !(s >= FR_MIN_SCALE && s <= FR_MAX_SCALE)) return 1;
    const int w = fr_trunc(w0 * s), h = fr_trunc(h0 * s);
    if (w < 1 || h < 1) return 1;
    geom[0] = w;
    geom[1] = h;
    geom[2] = fr_trunc((double)w / 2.0 - FR_CROP / 2.0 + (t0 - w0 / 2.0) * s);
    geom[3] = fr_trunc((double)h / 2.0 - FR_CROP / 2.0 + (h0 / 2.0 - t1) * s);
    return 0;
}

#endif
