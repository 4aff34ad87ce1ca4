/*
 * eval_metrics_core.h -- the per-tile arithmetic of n3dt_eval_metrics (include/n3dt.h): SSIM and PSNR of rendered frames as
 * the reference's validation scores them (Utils/Eval_utils.py:11-48,54-66,101-106).
 *
 * Included by csrc/eval_metrics.hip, whose kernels run the phases below with one thread per `tid` and a workgroup barrier
 * between two phases, and by tests/eval_core_host.cpp, which runs the very same functions in plain loops over `tid` on the
 * CPU (under the address and undefined-behaviour sanitizers), so the tiling, halo and bounds logic is checked without a GPU.
 * Compiles as host C++ on its own; the __host__ __device__ qualifiers exist only under hipcc.
 *
 * One workgroup (EVM_THREADS threads) owns one EVM_TILE x EVM_TILE tile of output pixels of one image pair:
 *   evm_stage   quantises and grey-converts the tile plus its EVM_HALO-pixel halo into EvmTileMem as bytes (0 outside the
 *               image: no valid window reaches there) and returns the thread's share of the squared colour-byte differences
 *               of the tile's OWN pixels (never the halo's);
 *   evm_rows    the five 7-wide horizontal sums (x, y, x^2, y^2, xy) of every row of the region, int32;
 *   evm_cols    adds seven of them vertically -- the 7x7 window sums, exact integers, the largest 49 * 255^2 = 3 186 225 --
 *               and evaluates S in float64 for every VALID window centre (3 <= y < H - 3, 3 <= x < W - 3) among the thread's
 *               pixels; returns their sum, added in pixel order;
 *   evm_reduce_step  one level of the fixed-order pairwise sum of the workgroup's values.
 * The whole image is then evm_ssim_mean / evm_psnr of the tiles' partials added in index order.
 */
#ifndef N3DT_EVAL_METRICS_CORE_H
#define N3DT_EVAL_METRICS_CORE_H

#include <math.h>

#ifdef __HIPCC__
#define EVM_HD __host__ __device__ static inline
#else
#define EVM_HD static inline
#endif

#define EVM_TILE 32                           /* output pixels per tile side */
#define EVM_HALO 3                            /* 7x7 window */
#define EVM_WIN 7
#define EVM_REG (EVM_TILE + 2 * EVM_HALO)     /* 38: the region a tile reads */
#define EVM_THREADS 256
#define EVM_MAX_HW 2147483648LL               /* height * width must stay below 2^31 */

/* cv2.cvtColor(COLOR_BGR2GRAY) on uint8: 15-bit fixed point, channel 0 weighted as B (OpenCV's BY15, GY15, RY15) */
#define EVM_BY15 3735
#define EVM_GY15 19235
#define EVM_RY15 9798

/* skimage.metrics.structural_similarity defaults on uint8: data_range 255, K1 0.01, K2 0.03, sample covariance */
#define EVM_C1 ((0.01 * 255.0) * (0.01 * 255.0))
#define EVM_C2 ((0.03 * 255.0) * (0.03 * 255.0))
#define EVM_NP 49.0
#define EVM_COV_NORM (49.0 / 48.0)
#define EVM_DBL_EPSILON 2.220446049250313e-16

typedef struct EvmPartial {
    double s;                /* sum of S over the tile's valid window centres */
    unsigned long long sse;  /* sum of squared colour-byte differences over the tile's own pixels */
} EvmPartial;

typedef struct EvmTileMem {
    unsigned char gx[EVM_REG * EVM_REG];
    unsigned char gy[EVM_REG * EVM_REG];
    int hs[5][EVM_REG * EVM_TILE];  /* horizontal sums: [x, y, xx, yy, xy][region row * EVM_TILE + tile column] */
    double red[EVM_THREADS];
    unsigned int sse[EVM_THREADS];
} EvmTileMem;

EVM_HD long long evm_tiles_x(int width) { return ((long long)width + EVM_TILE - 1) / EVM_TILE; }
EVM_HD long long evm_tiles_y(int height) { return ((long long)height + EVM_TILE - 1) / EVM_TILE; }

/* q = (unsigned char) min(max(x * 255.0f, 0.0f), 255.0f), NaN -> 0; the product is one fp32 multiply, as numpy forms it */
EVM_HD unsigned int evm_quantise(float x) {
    float v = x * 255.0f;
    if (!(v > 0.0f)) v = 0.0f;  /* negative, -0 and NaN */
    if (v > 255.0f) v = 255.0f;
    return (unsigned int)(int)v;
}

EVM_HD unsigned int evm_grey(unsigned int c0, unsigned int c1, unsigned int c2) {
    return (c0 * EVM_BY15 + c1 * EVM_GY15 + c2 * EVM_RY15 + 16384u) >> 15;
}

/* S of one window from its five exact integer sums */
EVM_HD double evm_ssim_point(int sx, int sy, int sxx, int syy, int sxy) {
    const double ux = (double)sx / EVM_NP, uy = (double)sy / EVM_NP;
    const double uxx = (double)sxx / EVM_NP, uyy = (double)syy / EVM_NP, uxy = (double)sxy / EVM_NP;
    const double vx = EVM_COV_NORM * (uxx - ux * ux);
    const double vy = EVM_COV_NORM * (uyy - uy * uy);
    const double vxy = EVM_COV_NORM * (uxy - ux * uy);
    const double a1 = 2.0 * ux * uy + EVM_C1, a2 = 2.0 * vxy + EVM_C2;
    const double b1 = ux * ux + uy * uy + EVM_C1, b2 = vx + vy + EVM_C2;
    return (a1 * a2) / (b1 * b2);
}

/* pred, gt: ONE image each, planar [3][height][width]; (y0, x0): the tile's first output pixel */
EVM_HD unsigned int evm_stage(EvmTileMem* m, int tid, const float* pred, const float* gt, int height, int width, int y0, int x0) {
    const long long plane = (long long)height * width;
    unsigned int sse = 0;
    for (int i = tid; i < EVM_REG * EVM_REG; i += EVM_THREADS) {
        const int r = i / EVM_REG, c = i - r * EVM_REG;
        const long long y = (long long)y0 - EVM_HALO + r, x = (long long)x0 - EVM_HALO + c;
        unsigned int ga = 0, gb = 0;
        if (y >= 0 && y < height && x >= 0 && x < width) {
            const long long o = y * width + x;
            const unsigned int a0 = evm_quantise(pred[o]), a1 = evm_quantise(pred[plane + o]), a2 = evm_quantise(pred[2 * plane + o]);
            const unsigned int b0 = evm_quantise(gt[o]), b1 = evm_quantise(gt[plane + o]), b2 = evm_quantise(gt[2 * plane + o]);
            ga = evm_grey(a0, a1, a2);
            gb = evm_grey(b0, b1, b2);
            if (r >= EVM_HALO && r < EVM_HALO + EVM_TILE && c >= EVM_HALO && c < EVM_HALO + EVM_TILE) {
                const int d0 = (int)a0 - (int)b0, d1 = (int)a1 - (int)b1, d2 = (int)a2 - (int)b2;
                sse += (unsigned int)(d0 * d0 + d1 * d1 + d2 * d2);  /* <= 6 pixels * 3 * 255^2 per thread */
            }
        }
        m->gx[i] = (unsigned char)ga;
        m->gy[i] = (unsigned char)gb;
    }
    return sse;
}

EVM_HD void evm_rows(EvmTileMem* m, int tid) {
    for (int i = tid; i < EVM_REG * EVM_TILE; i += EVM_THREADS) {
        const int r = i / EVM_TILE, c = i - r * EVM_TILE;
        const unsigned char* px = m->gx + r * EVM_REG + c;
        const unsigned char* py = m->gy + r * EVM_REG + c;
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int k = 0; k < EVM_WIN; ++k) {
            const int a = px[k], b = py[k];
            sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
        }
        m->hs[0][i] = sx; m->hs[1][i] = sy; m->hs[2][i] = sxx; m->hs[3][i] = syy; m->hs[4][i] = sxy;
    }
}

EVM_HD double evm_cols(const EvmTileMem* m, int tid, int height, int width, int y0, int x0) {
    double acc = 0.0;
    for (int i = tid; i < EVM_TILE * EVM_TILE; i += EVM_THREADS) {
        const int r = i / EVM_TILE, c = i - r * EVM_TILE;
        const long long y = (long long)y0 + r, x = (long long)x0 + c;
        if (y < EVM_HALO || y >= (long long)height - EVM_HALO || x < EVM_HALO || x >= (long long)width - EVM_HALO) continue;
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int k = 0; k < EVM_WIN; ++k) {  /* region rows r .. r + 6 are image rows y - 3 .. y + 3 */
            const int j = (r + k) * EVM_TILE + c;
            sx += m->hs[0][j]; sy += m->hs[1][j]; sxx += m->hs[2][j]; syy += m->hs[3][j]; sxy += m->hs[4][j];
        }
        acc += evm_ssim_point(sx, sy, sxx, syy, sxy);
    }
    return acc;
}

/* for (step = EVM_THREADS / 2; step >= 1; step /= 2) { every tid: evm_reduce_step; barrier }: the sums end in element 0 */
EVM_HD void evm_reduce_step(EvmTileMem* m, int tid, int step) {
    if (tid < step) {
        m->red[tid] += m->red[tid + step];
        m->sse[tid] += m->sse[tid + step];  /* a tile's total is at most 1024 * 3 * 255^2 < 2^32 */
    }
}

/* the image's figures from its partials added in index order */
EVM_HD double evm_ssim_mean(double s_sum, int height, int width) {
    return s_sum / ((double)(height - 2 * EVM_HALO) * (double)(width - 2 * EVM_HALO));
}

EVM_HD double evm_psnr(unsigned long long sse, int height, int width) {
    const double mse = (double)sse / ((double)height * (double)width * 3.0);
    return 20.0 * log10(255.0 / (sqrt(mse) + EVM_DBL_EPSILON));
}

#endif
