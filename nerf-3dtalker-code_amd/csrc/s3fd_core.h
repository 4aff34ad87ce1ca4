/*
 * s3fd_core.h -- the geometry table and the index arithmetic of n3dt_s3fd (include/n3dt.h): the S3FD face detector (the
 * reference's face_detection/detection/sfd/net_s3fd.py), frozen, inference only.
 *
 * Included by csrc/s3fd.hip, whose kernels take their sizes and addresses from the functions below, and by
 * tests/s3fd_core_host.cpp, which walks the same functions over the kernels' grids on the CPU under the address and
 * undefined-behaviour sanitizers.  The rows of the implicit GEMM, the halo test, the tap offsets and the wave-tile rule are conv_net_core.h's; the
 * fragment arithmetic is conv_frag.h's.  Compiles as host C++ on its own.
 *
 * Blocks.  33 of them: 0..18 the backbone convolutions in state-dict order (conv1_1 .. conv7_2), 19..23 the five 2 x 2 / 2 max
 * pools (floor), 24..26 the three L2Norms, 27..32 the six detection levels' head pairs (conf + loc as ONE matrix).
 *
 * Maps.  NHWC fp32 with C a multiple of 16 (the image's 3 channels are padded with zero channels) and the zero halo the widest
 * consumer needs: 1 in front of a 3 x 3 convolution, 3 in front of fc6, 0 in front of a pool.  A 1 x 1 convolution that shares
 * its input with a head (fc7 -> conv6_1, conv6_2 -> conv7_1) reads past that halo: `ioff` = halo - padding.  The map sizes are
 * known only at run time: everything here is a function of the frame's (H, W).
 */
#ifndef N3DT_S3FD_CORE_H
#define N3DT_S3FD_CORE_H

#include <math.h>

#include "conv_net_core.h"

#define S3_CONVS 19
#define S3_POOLS 5
#define S3_NORMS 3
#define S3_LEVELS 6
#define S3_GEMMS (S3_CONVS + S3_LEVELS)
#define S3_BLOCKS (S3_CONVS + S3_POOLS + S3_NORMS + S3_LEVELS)
#define S3_FIRST_POOL S3_CONVS
#define S3_FIRST_NORM (S3_CONVS + S3_POOLS)
#define S3_FIRST_HEAD (S3_CONVS + S3_POOLS + S3_NORMS)
#define S3_PARAMS (S3_CONVS + 2 * S3_LEVELS) /* weight / bias pairs: the convolutions, then conf and loc of each level */
#define S3_MIN_HW 32                         /* below that pool5 is empty */
#define S3_MAX_IMAGES 1024
#define S3_MAX_FACES 64
#define S3_MAX_SMOOTH 64
#define S3_MAX_CLIP (1 << 20)
#define S3_WS_BUDGET ((size_t)4 << 30) /* bytes of workspace one call may ask for: caps n */
#define S3_NORM_EPS 1e-10
#define S3_SCORE_THRESH 0.5
#define S3_NMS_THRESH 0.3

/* C_in, C_out, kernel, stride, padding; pool: a 2 x 2 / 2 max pool follows; level: its output (through an L2Norm for 1..3) feeds
 * detection level `level` (1..6; 0: none) */
typedef struct S3Conv {
    int cin, cout, k, stride, pad, pool, level;
} S3Conv;

static const S3Conv S3_TABLE[S3_CONVS] = {
    {3, 64, 3, 1, 1, 0, 0},      /* conv1_1 */
    {64, 64, 3, 1, 1, 1, 0},     /* conv1_2 */
    {64, 128, 3, 1, 1, 0, 0},    /* conv2_1 */
    {128, 128, 3, 1, 1, 1, 0},   /* conv2_2 */
    {128, 256, 3, 1, 1, 0, 0},   /* conv3_1 */
    {256, 256, 3, 1, 1, 0, 0},   /* conv3_2 */
    {256, 256, 3, 1, 1, 1, 1},   /* conv3_3 */
    {256, 512, 3, 1, 1, 0, 0},   /* conv4_1 */
    {512, 512, 3, 1, 1, 0, 0},   /* conv4_2 */
    {512, 512, 3, 1, 1, 1, 2},   /* conv4_3 */
    {512, 512, 3, 1, 1, 0, 0},   /* conv5_1 */
    {512, 512, 3, 1, 1, 0, 0},   /* conv5_2 */
    {512, 512, 3, 1, 1, 1, 3},   /* conv5_3 */
    {512, 1024, 3, 1, 3, 0, 0},  /* fc6: padding 3, no dilation: the output is 4 larger than the input */
    {1024, 1024, 1, 1, 0, 0, 4}, /* fc7 */
    {1024, 256, 1, 1, 0, 0, 0},  /* conv6_1 */
    {256, 512, 3, 2, 1, 0, 5},   /* conv6_2 */
    {512, 128, 1, 1, 0, 0, 0},   /* conv7_1 */
    {128, 256, 3, 2, 1, 0, 6},   /* conv7_2 */
};

/* the convolution whose output is level l's (0..5) source, that source's channels, and the conf head's channels */
static const int S3_LEVEL_CONV[S3_LEVELS] = {6, 9, 12, 14, 16, 18};
CN_HD int s3_level_c(int l) { return l == 0 ? 256 : l == 3 ? 1024 : l == 5 ? 256 : 512; }
CN_HD int s3_level_conf(int l) { return l == 0 ? 4 : 2; }
CN_HD int s3_level_cols(int l) { return s3_level_conf(l) + 4; } /* stored columns of the head pair's 32 */
CN_HD int s3_level_stride(int l) { return 4 << l; }

/* halo of convolution c's input and output maps in the chain */
static inline int s3_conv_ohalo(int c) {
    if (S3_TABLE[c].pool) return 0;
    int h = S3_TABLE[c].level ? 1 : 0; /* a head reads it with padding 1 */
    if (c + 1 < S3_CONVS && S3_TABLE[c + 1].pad > h) h = S3_TABLE[c + 1].pad;
    return h;
}
static inline int s3_conv_ihalo(int c) {
    if (c == 0 || S3_TABLE[c - 1].pool) return S3_TABLE[c].pad; /* the prologue's and a pool's output carry this halo */
    return s3_conv_ohalo(c - 1);
}

/* one GEMM: input [n, Hp, Wp, cinp] with halo ihalo, read at offset ioff = ihalo - padding; output [n, Hq, Wq, cstore] with halo
 * opad; np = the packed matrix's columns (a multiple of 32), of which the first cstore are stored; K = k k cinp */
typedef struct S3Geom {
    int Hi, Wi, Ho, Wo, Hp, Wp, Hq, Wq, cin, cinp, np, cstore, ihalo, ioff, opad, k, stride, K, relu;
} S3Geom;

static inline S3Geom s3_geom_make(int Hi, int Wi, int cin, int np, int cstore, int k, int stride, int pad, int ihalo, int opad, int relu) {
    S3Geom g;
    g.Hi = Hi;
    g.Wi = Wi;
    g.Ho = cn_conv_out(Hi, k, stride, pad);
    g.Wo = cn_conv_out(Wi, k, stride, pad);
    g.ihalo = ihalo;
    g.ioff = ihalo - pad;
    g.opad = opad;
    g.Hp = Hi + 2 * ihalo;
    g.Wp = Wi + 2 * ihalo;
    g.Hq = g.Ho + 2 * opad;
    g.Wq = g.Wo + 2 * opad;
    g.cin = cin;
    g.cinp = cn_round16(cin);
    g.np = np;
    g.cstore = cstore;
    g.k = k;
    g.stride = stride;
    g.K = k * k * g.cinp;
    g.relu = relu;
    return g;
}

/* GEMM j (0..18 a backbone convolution, 19..24 the head pair of level j - 19) on an input of Hi x Wi pixels */
static inline S3Geom s3_gemm_geom(int j, int Hi, int Wi) {
    if (j < S3_CONVS) {
        const S3Conv t = S3_TABLE[j];
        return s3_geom_make(Hi, Wi, t.cin, t.cout, t.cout, t.k, t.stride, t.pad, s3_conv_ihalo(j), s3_conv_ohalo(j), 1);
    }
    const int l = j - S3_CONVS;
    return s3_geom_make(Hi, Wi, s3_level_c(l), 32, s3_level_cols(l), 3, 1, 1, 1, 0, 0);
}

static inline size_t s3_in_elems(const S3Geom* g, int n) { return (size_t)n * g->Hp * g->Wp * g->cinp; }
static inline size_t s3_out_elems(const S3Geom* g, int n) { return (size_t)n * g->Hq * g->Wq * g->cstore; }

/* every map's size from the frame's (H, W): h[c] x w[c] the input of convolution c, lh[l] x lw[l] detection level l */
typedef struct S3Sizes {
    int h[S3_CONVS], w[S3_CONVS], lh[S3_LEVELS], lw[S3_LEVELS];
} S3Sizes;

static inline S3Sizes s3_sizes(int H, int W) {
    S3Sizes s;
    for (int c = 0; c < S3_CONVS; ++c) {
        const S3Conv t = S3_TABLE[c];
        s.h[c] = H;
        s.w[c] = W;
        H = cn_conv_out(H, t.k, t.stride, t.pad);
        W = cn_conv_out(W, t.k, t.stride, t.pad);
        if (t.level) {
            s.lh[t.level - 1] = H;
            s.lw[t.level - 1] = W;
        }
        if (t.pool) {
            H /= 2;
            W /= 2;
        }
    }
    return s;
}

CN_HD int s3_hw_ok(int H, int W) { return H >= S3_MIN_HW && W >= S3_MIN_HW && H <= CN_MAX_FRAME_HW && W <= CN_MAX_FRAME_HW; }

/* head positions over the six levels, level-major, then y, then x; first[l] = the first position of level l, first[6] = P */
static inline int s3_positions(const S3Sizes* s, int first[S3_LEVELS + 1]) {
    int p = 0;
    for (int l = 0; l < S3_LEVELS; ++l) {
        if (first) first[l] = p;
        p += s->lh[l] * s->lw[l];
    }
    if (first) first[S3_LEVELS] = p;
    return p;
}

/* ---- the workspace carve for n images of H x W -----------------------------------------------------------------------------------
 * two maps that the blocks alternate between (each as large as the largest map of the chain), the L2Norm's output, the six head
 * maps, and the tail's float64 scores and boxes and its suppression flags.  Byte offsets, each a multiple of 256. */
typedef struct S3Workspace {
    size_t map[2], norm, head[S3_LEVELS], score, box, sup, total;
} S3Workspace;

static inline size_t s3_max_map_elems(const S3Sizes* s) {
    size_t m = 0;
    for (int c = 0; c < S3_CONVS; ++c) {
        const S3Geom g = s3_gemm_geom(c, s->h[c], s->w[c]);
        const size_t i = s3_in_elems(&g, 1), o = s3_out_elems(&g, 1);
        if (i > m) m = i;
        if (o > m) m = o;
    }
    return m;
}

static inline size_t s3_norm_elems(int Hl, int Wl, int C) { return (size_t)(Hl + 2) * (Wl + 2) * C; }

static inline S3Workspace s3_workspace(int n, int H, int W) {
    const S3Sizes s = s3_sizes(H, W);
    S3Workspace w;
    size_t off = 0;
    const size_t mm = s3_max_map_elems(&s);
    for (int i = 0; i < 2; ++i) {
        w.map[i] = off;
        off += cn_rup256((size_t)n * mm * sizeof(float));
    }
    size_t nm = 0;
    for (int l = 0; l < S3_NORMS; ++l) {
        const size_t e = s3_norm_elems(s.lh[l], s.lw[l], s3_level_c(l));
        if (e > nm) nm = e;
    }
    w.norm = off;
    off += cn_rup256((size_t)n * nm * sizeof(float));
    for (int l = 0; l < S3_LEVELS; ++l) {
        w.head[l] = off;
        off += cn_rup256((size_t)n * s.lh[l] * s.lw[l] * s3_level_cols(l) * sizeof(float));
    }
    const size_t P = (size_t)s3_positions(&s, 0);
    w.score = off;
    off += cn_rup256((size_t)n * P * sizeof(double));
    w.box = off;
    off += cn_rup256((size_t)n * P * 4 * sizeof(double));
    w.sup = off;
    off += cn_rup256((size_t)n * P);
    w.total = off;
    return w;
}

/* the most images one call takes at H x W: the workspace budget, and S3_MAX_IMAGES */
static inline int s3_max_images(int H, int W) {
    const size_t one = s3_workspace(1, H, W).total;
    size_t n = S3_WS_BUDGET / one;
    if (n > S3_MAX_IMAGES) n = S3_MAX_IMAGES;
    while (n > 1 && s3_workspace((int)n, H, W).total > S3_WS_BUDGET) --n;
    return (int)n;
}

/* ---- addresses -------------------------------------------------------------------------------------------------------------------
 * first element of the receptive field of output pixel (img, y, x) in the padded NHWC input [n, Hp, Wp, cinp] read at offset ioff */
CN_HD size_t s3_field_base(int img, int y, int x, int stride, int ioff, int Hp, int Wp, int cinp) {
    return (((size_t)img * Hp + (size_t)y * stride + ioff) * Wp + (size_t)x * stride + ioff) * cinp;
}

/* the pool: output pixel (y, x) of [n, Ho, Wo] = floor(Hi / 2) x floor(Wi / 2) takes input pixels (2 y + dy, 2 x + dx) of a map
 * [n, Hi + 2 ihalo, Wi + 2 ihalo, C]; where pixel (2 y, 2 x) begins */
CN_HD size_t s3_pool_base(int img, int y, int x, int Hi, int Wi, int ihalo, int C) {
    return (((size_t)img * (Hi + 2 * ihalo) + (size_t)(2 * y + ihalo)) * (Wi + 2 * ihalo) + (size_t)(2 * x + ihalo)) * C;
}

/* position p (0 .. P - 1) -> level, y, x */
CN_HD void s3_position(int p, const int* first, const int* lw, int* l, int* y, int* x) {
    int lv = 0;
    while (lv + 1 < S3_LEVELS && p >= first[lv + 1]) ++lv;
    const int r = p - first[lv];
    *l = lv;
    *y = r / lw[lv];
    *x = r - *y * lw[lv];
}

/* ---- the tail's arithmetic, float64 --------------------------------------------------------------------------------------------
 * bbox.py:104-108 literally: prior (stride / 2 + x stride, stride / 2 + y stride, 4 stride, 4 stride), variances 0.1 / 0.2 */
CN_HD void s3_decode(int stride, int y, int x, const double loc[4], double box[4]) {
    const double pcx = (double)stride / 2 + (double)x * stride, pcy = (double)stride / 2 + (double)y * stride, ps = (double)stride * 4;
    double cx = pcx + loc[0] * 0.1 * ps, cy = pcy + loc[1] * 0.1 * ps;
    const double w = ps * exp(loc[2] * 0.2), h = ps * exp(loc[3] * 0.2);
    cx -= w / 2;
    cy -= h / 2;
    box[0] = cx;
    box[1] = cy;
    box[2] = w + cx;
    box[3] = h + cy;
}

/* F.softmax over (c0, c1), channel 1 */
CN_HD double s3_score(double c0, double c1) {
    const double m = c0 > c1 ? c0 : c1;
    const double e0 = exp(c0 - m), e1 = exp(c1 - m);
    return e1 / (e0 + e1);
}

/* bbox.py:44-64: the overlap of boxes a and b with the +1 areas */
CN_HD double s3_overlap(const double* a, const double* b) {
    const double aa = (a[2] - a[0] + 1) * (a[3] - a[1] + 1), ab = (b[2] - b[0] + 1) * (b[3] - b[1] + 1);
    const double xx1 = a[0] > b[0] ? a[0] : b[0], yy1 = a[1] > b[1] ? a[1] : b[1];
    const double xx2 = a[2] < b[2] ? a[2] : b[2], yy2 = a[3] < b[3] ? a[3] : b[3];
    double w = xx2 - xx1 + 1, h = yy2 - yy1 + 1;
    if (!(w > 0.0)) w = 0.0;
    if (!(h > 0.0)) h = 0.0;
    return w * h / (aa + ab - w * h);
}

/* ---- crop boxes ------------------------------------------------------------------------------------------------------------------
 * api.py:74-76 and data_loader_xgaze_new.py:156-159: clip at 0, truncate, pad, clamp to the frame -> (x1, y1, x2, y2) */
CN_HD void s3_pad_box(const double* det, int H, int W, const int* pads, int* out) {
    int r[4];
    for (int i = 0; i < 4; ++i) {
        double v = det[i];
        if (!(v > 0.0)) v = 0.0;
        if (v > 1e9) v = 1e9;
        r[i] = (int)v;
    }
    const int y1 = r[1] - pads[0], y2 = r[3] + pads[1], x1 = r[0] - pads[2], x2 = r[2] + pads[3];
    out[0] = x1 > 0 ? x1 : 0;
    out[1] = y1 > 0 ? y1 : 0;
    out[2] = x2 < W ? x2 : W;
    out[3] = y2 < H ? y2 : H;
}

/* get_smoothened_boxes: entry i's window [*a, *b) of F boxes.  i + T <= F: [i, i + T).  Else boxes[F - T:], whose negative
 * start numpy counts from the end: [max(0, 2 F - T), F) where F < T. */
CN_HD void s3_smooth_window(int i, int F, int T, int* a, int* b) {
    if (i + T > F) {
        int s = F - T;
        if (s < 0) s = F + s < 0 ? 0 : F + s;
        *a = s;
        *b = F;
    } else {
        *a = i;
        *b = i + T;
    }
}

/* the mean of integers assigned into an integer array: the sum over the length, truncated toward zero */
CN_HD int s3_trunc_mean(long long sum, int len) { return (int)(sum / len); }

#endif
