/*
 * lpips_core.h -- the geometry and index arithmetic of n3dt_lpips (include/n3dt.h): LPIPS with AlexNet features as the
 * reference's validation scores it (Utils/Eval_utils.py:108-115).
 *
 * Included by csrc/lpips.hip, whose convolution, pool and halo kernels and whose prologue's gather take their addresses from the
 * functions below, and by tests/lpips_core_host.cpp, which walks the very same functions over those kernels' grids on the CPU
 * (under the address and undefined-behaviour sanitizers), so the reinterpretation, the tap and halo addressing, the pool
 * windows and the rows past M are checked without a GPU.  The weight pack's fragment arithmetic and the epilogue's register ->
 * row map are conv_frag.h's, shared with the other convolutions and walked by the same program; the flat element decodes of the
 * prologue's output and the distance kernel stay in lpips.hip.  Compiles as host C++ on its own; the __host__ __device__
 * qualifiers exist only under hipcc.
 *
 * Maps.  Every activation is NHWC fp32; `pad` is the zero halo the NEXT convolution needs.
 *   in0    [n, H + 4, W + 4, 3]       the scaled input, pad 2
 *   relu1  [n, H1, W1, 64]            conv 11x11 / 4 / pad 2          H1 = (H + 4 - 11) / 4 + 1
 *   pool1  [n, P1 + 4, P1w + 4, 64]   max-pool 3 / 2 of relu1, pad 2  P1 = (H1 - 3) / 2 + 1
 *   relu2  [n, P1, P1w, 192]          conv 5x5 / pad 2
 *   pool2  [n, P2 + 2, P2w + 2, 192]  max-pool 3 / 2 of relu2, pad 1  P2 = (P1 - 3) / 2 + 1
 *   relu3  [n, P2 + 2, P2w + 2, 384]  conv 3x3 / pad 1, pad 1
 *   relu4  [n, P2 + 2, P2w + 2, 256]  conv 3x3 / pad 1, pad 1
 *   relu5  [n, P2, P2w, 256]          conv 3x3 / pad 1
 */
#ifndef N3DT_LPIPS_CORE_H
#define N3DT_LPIPS_CORE_H

#include <stddef.h>

#ifdef __HIPCC__
#define LP_HD __host__ __device__ static inline
#else
#define LP_HD static inline
#endif

#define LP_LAYERS 5
#define LP_MIN_HW 31     /* the smallest input every layer still has one pixel of */
#define LP_MAX_HW 2048
#define LP_MAX_BATCH 64
#define LP_TILE_M 64     /* output pixels per wave */
#define LP_WG_M 256      /* output pixels per workgroup (4 waves) */
#define LP_TILE_N 64     /* output channels per wave */
#define LP_PARTS 128     /* fixed number of partial sums per image pair and layer */

/* torchvision alexnet().features indices 0, 3, 6, 8, 10 */
LP_HD int lp_cin(int l) { return l == 0 ? 3 : l == 1 ? 64 : l == 2 ? 192 : l == 3 ? 384 : 256; }
LP_HD int lp_cout(int l) { return l == 0 ? 64 : l == 1 ? 192 : l == 2 ? 384 : 256; }
LP_HD int lp_ksize(int l) { return l == 0 ? 11 : l == 1 ? 5 : 3; }
LP_HD int lp_stride(int l) { return l == 0 ? 4 : 1; }
LP_HD int lp_pad(int l) { return l <= 1 ? 2 : 1; }
LP_HD int lp_k(int l) { return lp_ksize(l) * lp_ksize(l) * lp_cin(l); }  /* 363, 1600, 1728, 3456, 2304 */
LP_HD int lp_kp(int l) { return (lp_k(l) + 15) / 16 * 16; }              /* 368 for conv1: the five padded rows are zero */
/* the halo relu{l+1} is stored with: relu3 and relu4 feed a 3x3 / pad 1 convolution directly */
LP_HD int lp_feat_pad(int l) { return (l == 2 || l == 3) ? 1 : 0; }

LP_HD int lp_conv_out(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }
LP_HD int lp_pool_out(int n) { return (n - 3) / 2 + 1; }  /* 3 / 2, no padding, floor */

/* extent of relu{l+1} along an axis of input extent n */
LP_HD int lp_feat_extent(int l, int n) {
    const int r1 = lp_conv_out(n, 11, 4, 2);
    if (l == 0) return r1;
    const int r2 = lp_pool_out(r1);
    if (l == 1) return r2;
    return lp_pool_out(r2);
}

/* ---- the reference's reshape(-1, 3, h, w) of an [H, W, 3] byte image ----------------------------------------------------------
 * Element [c', y', x'] of the reinterpreted image is flat byte f = c' H W + y' W + x' of the HWC buffer, which is channel f % 3 of
 * pixel f / 3.  Returns that byte's offset in the PLANAR [3, H, W] image the caller holds. */
LP_HD long long lp_reinterpret_src(int cp, int yp, int xp, int height, int width) {
    const long long hw = (long long)height * width;
    const long long f = (long long)cp * hw + (long long)yp * width + xp;
    return (f % 3) * hw + f / 3;
}

/* ---- rows of the implicit GEMM -------------------------------------------------------------------------------------------------
 * Row m of M = n_img * Ho * Wo is output pixel (img, y, x).  Rows past M compute row M - 1 again and are never stored. */
LP_HD void lp_row_pixel(long long m, long long M, int Ho, int Wo, int* img, int* y, int* x) {
    if (m > M - 1) m = M - 1;
    const long long hw = (long long)Ho * Wo;
    *img = (int)(m / hw);
    const int rem = (int)(m - (long long)*img * hw);
    *y = rem / Wo;
    *x = rem - *y * Wo;
}

/* first element of the receptive field of output pixel (img, y, x) in a padded NHWC input [n, Hp, Wp, cin] */
LP_HD size_t lp_field_base(int img, int y, int x, int stride, int Hp, int Wp, int cin) {
    return (((size_t)img * Hp + (size_t)y * stride) * Wp + (size_t)x * stride) * cin;
}

/* offset of tap (ky, kx) = (tap / ksize, tap % ksize), channel 0, from the field's base */
LP_HD size_t lp_tap_offset(int tap, int ksize, int Wp, int cin) {
    return ((size_t)(tap / ksize) * Wp + (size_t)(tap % ksize)) * cin;
}

/* conv1's gather form: k = tap * 3 + ci for k < 363.  Offset from the field's base in in0. */
LP_HD size_t lp_gather_offset(int k, int ksize, int Wp, int cin) {
    const int tap = k / cin, ci = k - tap * cin;
    return lp_tap_offset(tap, ksize, Wp, cin) + (size_t)ci;
}

/* where output pixel (img, y, x) of an [n, Ho, Wo, C] map stored with halo `pad` begins */
LP_HD size_t lp_out_pixel(int img, int y, int x, int Ho, int Wo, int pad, int C) {
    return (((size_t)img * (Ho + 2 * pad) + (size_t)(y + pad)) * (Wo + 2 * pad) + (size_t)(x + pad)) * C;
}

/* ---- pool ------------------------------------------------------------------------------------------------------------------------
 * Output (oy, ox) is the maximum over input rows 2 oy .. 2 oy + 2 and columns 2 ox .. 2 ox + 2 of an un-padded [n, Hi, Wi, C] map;
 * floor: 2 (Ho - 1) + 2 <= Hi - 1, so a window never leaves the map and trailing rows that fill no window are dropped. */
LP_HD size_t lp_pool_src(int img, int oy, int ox, int dy, int dx, int Hi, int Wi, int C) {
    return (((size_t)img * Hi + (size_t)(2 * oy + dy)) * Wi + (size_t)(2 * ox + dx)) * C;
}

/* ---- halo ------------------------------------------------------------------------------------------------------------------------
 * The 1-pixel border of a [n, H + 2, W + 2, C] map has 2 (W + 2) + 2 H cells per image: the top row, the bottom row, then the
 * left and right cell of every interior row.  Cell -> padded (y, x). */
LP_HD int lp_halo_cells(int H, int W) { return 2 * (W + 2) + 2 * H; }
LP_HD void lp_halo_cell(int cell, int H, int W, int* y, int* x) {
    if (cell < W + 2) {
        *y = 0;
        *x = cell;
    } else if (cell < 2 * (W + 2)) {
        *y = H + 1;
        *x = cell - (W + 2);
    } else {
        const int k = cell - 2 * (W + 2);
        *y = 1 + (k >> 1);
        *x = (k & 1) ? W + 1 : 0;
    }
}

/* ---- sizes -----------------------------------------------------------------------------------------------------------------------*/
typedef struct LpMaps {
    int fh[LP_LAYERS], fw[LP_LAYERS];  /* relu1..relu5 */
    size_t in0, relu[LP_LAYERS], pool[2];  /* element counts of each buffer for n_img images */
} LpMaps;

LP_HD LpMaps lp_maps(int n_img, int height, int width) {
    LpMaps g;
    for (int l = 0; l < LP_LAYERS; ++l) {
        g.fh[l] = lp_feat_extent(l, height);
        g.fw[l] = lp_feat_extent(l, width);
        const int p = lp_feat_pad(l);
        g.relu[l] = (size_t)n_img * (g.fh[l] + 2 * p) * (g.fw[l] + 2 * p) * lp_cout(l);
    }
    g.in0 = (size_t)n_img * (height + 4) * (width + 4) * 3;
    g.pool[0] = (size_t)n_img * (g.fh[1] + 4) * (g.fw[1] + 4) * 64;
    g.pool[1] = (size_t)n_img * (g.fh[2] + 2) * (g.fw[2] + 2) * 192;
    return g;
}

#endif
