/*
 * conv_net_core.h -- the index arithmetic the six frozen convolutional networks share (syncnet, wav2lip, s3fd, face_recon, fan,
 * head_mask): the rows of the implicit GEMM, the halo test, tap offsets, channel rounding, the flattened
 * 7 x 7 x 3 stem, the 3 x 3 / 2 max pool's window, the bilinear resample of the crop prologues and the rule for the column tiles
 * a wave takes.
 *
 * Included by each network's core header, by csrc/conv_net.hip, whose pack, layout and pool kernels decode their elements with the
 * functions below, and through the core headers by the six host walks under tests/ (syncnet_core_host.cpp and its siblings), which
 * call the very same functions on the CPU under the address and undefined-behaviour sanitizers.  Compiles as host C++ on its own;
 * the __host__ __device__ qualifiers exist only under hipcc.
 */
#ifndef N3DT_CONV_NET_CORE_H
#define N3DT_CONV_NET_CORE_H

#include <stddef.h>

#ifdef __HIPCC__
#define CN_HD __host__ __device__ static inline
#else
#define CN_HD static inline
#endif

#define CN_TILE_M 64           /* output cells per wave */
#define CN_MAX_FRAME_HW 4096
#define CN_STEM_K 147          /* 7 x 7 x 3 */
#define CN_STEM_KP 160
#define CN_STEM_ROW 21         /* 7 x 3: the (kx, c) of one ky, contiguous in NHWC */

CN_HD int cn_round16(int c) { return (c + 15) / 16 * 16; }
CN_HD int cn_round32(int c) { return (c + 31) / 32 * 32; }
CN_HD size_t cn_rup256(size_t x) { return (x + 255) / 256 * 256; }
CN_HD int cn_conv_out(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }

/* 32-column tiles per wave for a GEMM of M rows and np columns (np a multiple of 32): one where the number of column tiles is odd,
 * and where two would leave fewer than 1024 waves; else two.  Wav2Lip sums its tiles over classes and keeps a rule of its own. */
CN_HD int cn_wave_ntiles(long long M, int np) {
    const long long mtiles = (M + CN_TILE_M - 1) / CN_TILE_M;
    return (np % 64 != 0 || mtiles * (np / 64) < 1024) ? 1 : 2;
}

/* ---- rows of the implicit GEMM -------------------------------------------------------------------------------------------------
 * Row m of Mq = n * Hq * Wq is cell (img, yq, xq) of the (padded) output map, stored at out + m * cout.  Rows past Mq compute row
 * Mq - 1 again and are never stored. */
CN_HD void cn_row_cell(long long m, long long Mq, int Hq, int Wq, int* img, int* yq, int* xq) {
    if (m > Mq - 1) m = Mq - 1;
    const long long hw = (long long)Hq * Wq;
    *img = (int)(m / hw);
    const int rem = (int)(m - (long long)*img * hw);
    *yq = rem / Wq;
    *xq = rem - *yq * Wq;
}

/* cell e of a map [n, Hq, Wq] -> (img, yq, xq) */
CN_HD void cn_cell(size_t e, int Hq, int Wq, int* img, int* yq, int* xq) {
    *xq = (int)(e % (size_t)Wq);
    const size_t t = e / (size_t)Wq;
    *yq = (int)(t % (size_t)Hq);
    *img = (int)(t / (size_t)Hq);
}

/* first element of the receptive field of output pixel (img, y, x) in the padded NHWC input [n, Hp, Wp, cinp] of a convolution with
 * one stride for both axes */
CN_HD size_t cn_field_base(int img, int y, int x, int stride, int Hp, int Wp, int cinp) {
    return (((size_t)img * Hp + (size_t)y * stride) * Wp + (size_t)x * stride) * cinp;
}

CN_HD int cn_interior(int yq, int xq, int Ho, int Wo, int opad) { return yq >= opad && yq < Ho + opad && xq >= opad && xq < Wo + opad; }

/* a halo cell computes the nearest output pixel (and stores 0) */
CN_HD int cn_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* offset of tap (ky, kx) = (tap / kw, tap % kw), channel 0, from the field's base in a map of Wp cells a row, cinp floats a cell */
CN_HD size_t cn_tap_offset(int tap, int kw, int Wp, int cinp) { return ((size_t)(tap / kw) * Wp + (size_t)(tap % kw)) * cinp; }

/* ---- the flattened stem: K = (tap, channel) of a 7 x 7 convolution over 3 channels, 147 padded to 160 ---------------------------
 * the packed row k (< 147) -> (ky, kx, c) */
CN_HD void cn_stem_tap(int k, int* ky, int* kx, int* c) {
    *ky = k / CN_STEM_ROW;
    const int r = k - *ky * CN_STEM_ROW;
    *kx = r / 3;
    *c = r - *kx * 3;
}

/* offset of flattened k (< 147) from the field's base in a haloed image [n, Hp, Wp, 3]: (kx, c) is contiguous in NHWC */
CN_HD size_t cn_stem_offset(int k, int Wp) {
    const int ky = k / CN_STEM_ROW;
    return (size_t)ky * Wp * 3 + (size_t)(k - ky * CN_STEM_ROW);
}

/* ---- the 3 x 3 / 2 max pool with padding 1 --------------------------------------------------------------------------------------
 * output pixel o takes input pixels [*a, *b) of `in` along one axis; never empty */
CN_HD int cn_pool_out(int n) { return (n + 2 - 3) / 2 + 1; }
CN_HD void cn_pool_range(int o, int in, int* a, int* b) {
    const int lo = 2 * o - 1, hi = 2 * o + 2;
    *a = lo < 0 ? 0 : lo;
    *b = hi > in ? in : hi;
}

/* ---- the crop prologues ---------------------------------------------------------------------------------------------------------
 * F.interpolate(mode="bilinear", align_corners=False, antialias=False) along one axis: output index d of `out` from `in` source
 * samples.  src = (d + 0.5) in / out - 0.5, clamped at 0; i0 = floor(src), i1 = min(i0 + 1, in - 1), weight of i1 = src - i0. */
CN_HD void cn_bilinear(int d, int in, int out, int* i0, int* i1, double* w1) {
    double src = ((double)in / (double)out) * ((double)d + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    int a = (int)src;
    if (a > in - 1) a = in - 1;
    *i0 = a;
    *i1 = a + 1 < in ? a + 1 : in - 1;
    *w1 = src - (double)a;
}

/* a crop box (y1, y2, x1, x2), rows y1 .. y2 - 1 and columns x1 .. x2 - 1, forced inside an H x W frame: the entry point's
 * callers check their boxes on the host; the kernel clamps so that a bad box on the device cannot read outside the frame */
CN_HD void cn_clamp_box(const int* box, int H, int W, int* y1, int* h, int* x1, int* w) {
    const int ya = cn_clampi(box[0], 0, H - 1), yb = cn_clampi(box[1], ya + 1, H);
    const int xa = cn_clampi(box[2], 0, W - 1), xb = cn_clampi(box[3], xa + 1, W);
    *y1 = ya;
    *h = yb - ya;
    *x1 = xa;
    *w = xb - xa;
}

#endif
