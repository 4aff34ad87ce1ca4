/*
 * wav2lip_core.h -- the geometry table and the index arithmetic of n3dt_wav2lip (include/n3dt.h): Wav2Lip's generator (the
 * reference's wav_models/wav2lip.py over wav_models/conv.py), frozen, inference only.
 *
 * Included by csrc/wav2lip.hip, whose convolution, layout, prologue and paste kernels take their addresses from the functions
 * below, and by tests/wav2lip_core_host.cpp, which walks the very same functions over the convolution kernel's grid on the CPU
 * (under the address and undefined-behaviour sanitizers) for all 51 blocks.  The fragment arithmetic of the packed weights and
 * the epilogue's register -> row map are conv_frag.h's; the rows' cell map, the resample and the box clamp are conv_net_core.h's.  Compiles as host
 * C++ on its own.
 *
 * Maps.  Every activation is NHWC fp32 with C a multiple of 16 and carries the zero halo its consumer needs.  A block's GEMM has
 * one row per CELL of its padded output map, halo cells included: a halo row computes a clamped pixel and stores 0, so every
 * cell is written by exactly one row and no buffer is ever cleared.
 *
 * Concatenations.  torch.cat((x, feats[-1]), 1) is one NHWC buffer CAT j (j = 0..6, in decoder order): channels [0, A_j) are
 * written by the last block of decoder group j, channels [A_j, C_j) by the last block of face-encoder group 6 - j, each with row
 * stride C_j; the next face-encoder block reads its slice of that buffer, the next decoder block all of it.
 *
 * Classes.  A block's rows are grouped into classes that share one weight matrix.  A Conv2d block is one class over all cells.
 * ConvTranspose2d(k 3, s 2, p 1, output_padding 1) has four, by the parity of the output pixel: an even row takes ky = 1 from
 * input row y / 2, an odd one ky = 2 from (y - 1) / 2 and ky = 0 from (y + 1) / 2, columns alike -- 1, 2, 2 and 4 taps.
 * ConvTranspose2d(k 3, s 1, p 0) on the 1 x 1 map has nine, one per output pixel, of one tap each; a class takes the halo cells
 * next to its pixel along.
 */
#ifndef N3DT_WAV2LIP_CORE_H
#define N3DT_WAV2LIP_CORE_H

#include <stddef.h>

#include "conv_net_core.h"
#include "syncnet_core.h" /* the mel window SN_MEL_H x SN_MEL_W and SN_BN_EPS, which the two Wav2Lip networks share */

#define W2L_BLOCKS 51
#define W2L_FIRST_AUDIO 18     /* 0..17 the face encoder, 18..30 the audio encoder, 31..48 the decoder, 49..50 the output block */
#define W2L_FIRST_DEC 31
#define W2L_OUT_BLOCK 49
#define W2L_HEAD 50            /* nn.Conv2d(32, 3, 1) + sigmoid: its own fp32 kernel, no batch norm, no ReLU */
#define W2L_CATS 7
#define W2L_IMG 96
#define W2L_FACE_C 6
#define W2L_OUT_C 3
#define W2L_HEAD_C 32
#define W2L_MAX_WINDOWS 128    /* bounds the workspace: about 11.2 MB a window */
#define W2L_MAX_CLASSES 9
#define W2L_MAX_FRAMES 4096

/* transposed, C_in, C_out, kernel (h, w), stride (h, w), padding, residual, halo of the output map, CAT buffer it ends in (or -1) */
typedef struct W2lBlock {
    int tr, cin, cout, kh, kw, sh, sw, pad, residual, opad, cat;
} W2lBlock;

static const W2lBlock W2L_TABLE[W2L_BLOCKS] = {
    /* face encoder: [6, 96, 96] -> [512, 1, 1]; the last block of each of its seven groups is a skip feature */
    {0, 6, 16, 7, 7, 1, 1, 3, 0, 1, 6},
    {0, 16, 32, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 32, 32, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 32, 32, 3, 3, 1, 1, 1, 1, 1, 5},
    {0, 32, 64, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 64, 64, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 64, 64, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 64, 64, 3, 3, 1, 1, 1, 1, 1, 4},
    {0, 64, 128, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 128, 128, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 128, 128, 3, 3, 1, 1, 1, 1, 1, 3},
    {0, 128, 256, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 256, 256, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 256, 256, 3, 3, 1, 1, 1, 1, 1, 2},
    {0, 256, 512, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 512, 512, 3, 3, 1, 1, 1, 1, 1, 1},
    {0, 512, 512, 3, 3, 1, 1, 0, 0, 0, -1},
    {0, 512, 512, 1, 1, 1, 1, 0, 0, 0, 0},
    /* audio encoder: [1, 80, 16] -> [512, 1, 1] */
    {0, 1, 32, 3, 3, 1, 1, 1, 0, 1, -1},
    {0, 32, 32, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 32, 32, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 32, 64, 3, 3, 3, 1, 1, 0, 1, -1},
    {0, 64, 64, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 64, 64, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 64, 128, 3, 3, 3, 3, 1, 0, 1, -1},
    {0, 128, 128, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 128, 128, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 128, 256, 3, 3, 3, 2, 1, 0, 1, -1},
    {0, 256, 256, 3, 3, 1, 1, 1, 1, 0, -1},
    {0, 256, 512, 3, 3, 1, 1, 0, 0, 0, -1},
    {0, 512, 512, 1, 1, 1, 1, 0, 0, 0, -1},
    /* decoder: the last block of each of its seven groups is followed by the concatenation */
    {0, 512, 512, 1, 1, 1, 1, 0, 0, 0, 0},
    {1, 1024, 512, 3, 3, 1, 1, 0, 0, 1, -1},
    {0, 512, 512, 3, 3, 1, 1, 1, 1, 1, 1},
    {1, 1024, 512, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 512, 512, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 512, 512, 3, 3, 1, 1, 1, 1, 1, 2},
    {1, 768, 384, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 384, 384, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 384, 384, 3, 3, 1, 1, 1, 1, 1, 3},
    {1, 512, 256, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 256, 256, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 256, 256, 3, 3, 1, 1, 1, 1, 1, 4},
    {1, 320, 128, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 128, 128, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 128, 128, 3, 3, 1, 1, 1, 1, 1, 5},
    {1, 160, 64, 3, 3, 2, 2, 1, 0, 1, -1},
    {0, 64, 64, 3, 3, 1, 1, 1, 1, 1, -1},
    {0, 64, 64, 3, 3, 1, 1, 1, 1, 1, 6},
    /* output block */
    {0, 80, 32, 3, 3, 1, 1, 1, 0, 0, -1},
    {0, 32, 3, 1, 1, 1, 1, 0, 0, 0, -1},
};

/* CAT j: channels of the decoder's part, channels in all, extent, halo */
static const int W2L_CAT_A[W2L_CATS] = {512, 512, 512, 384, 256, 128, 64};
static const int W2L_CAT_C[W2L_CATS] = {1024, 1024, 768, 512, 320, 160, 80};
static const int W2L_CAT_HW[W2L_CATS] = {1, 3, 6, 12, 24, 48, 96};
static const int W2L_CAT_HALO[W2L_CATS] = {0, 1, 1, 1, 1, 1, 1};

static inline size_t w2l_cat_elems(int j) {
    const size_t e = (size_t)(W2L_CAT_HW[j] + 2 * W2L_CAT_HALO[j]);
    return e * e * W2L_CAT_C[j];
}

/* one block's maps.  Input: extent Hi x Wi with halo ihalo >= pad in a buffer of Hp x Wp cells and row stride istride, read from
 * channel in_off on (in_cat: the CAT buffer it lies in, or -1 for a map of its own).  Output: Ho x Wo with halo opad in Hq x Wq
 * cells; in the chain it goes to CAT out_cat at channel out_off with row stride out_stride (a map of its own: -1, 0, cout).
 * np is C_out rounded up to 32: the packed matrix has np columns, of which cout are stored.  K = kh kw cinp. */
typedef struct W2lGeom {
    int tr, Hi, Wi, Ho, Wo, Hp, Wp, Hq, Wq, cin, cinp, cout, np, ihalo, opad, pad, kh, kw, sh, sw, K, residual;
    int in_cat, in_off, istride, out_cat, out_off, out_stride;
} W2lGeom;

static inline int w2l_out_extent(const W2lBlock* t, int n, int k, int s) {
    return t->tr ? (n - 1) * s - 2 * t->pad + k + (s == 2 ? 1 : 0) : cn_conv_out(n, k, s, t->pad);
}

static inline W2lGeom w2l_geom(int block) {
    const int first = block < W2L_FIRST_AUDIO ? 0 : block < W2L_FIRST_DEC ? W2L_FIRST_AUDIO : W2L_FIRST_DEC;
    int H = first == 0 ? W2L_IMG : first == W2L_FIRST_AUDIO ? SN_MEL_H : 1;
    int W = first == 0 ? W2L_IMG : first == W2L_FIRST_AUDIO ? SN_MEL_W : 1;
    for (int b = first; b < block; ++b) {
        H = w2l_out_extent(&W2L_TABLE[b], H, W2L_TABLE[b].kh, W2L_TABLE[b].sh);
        W = w2l_out_extent(&W2L_TABLE[b], W, W2L_TABLE[b].kw, W2L_TABLE[b].sw);
    }
    const W2lBlock t = W2L_TABLE[block];
    W2lGeom g;
    g.tr = t.tr;
    g.Hi = H;
    g.Wi = W;
    g.Ho = w2l_out_extent(&t, H, t.kh, t.sh);
    g.Wo = w2l_out_extent(&t, W, t.kw, t.sw);
    g.cin = t.cin;
    g.cinp = cn_round16(t.cin);
    g.cout = t.cout;
    g.np = cn_round32(t.cout);
    g.pad = t.pad;
    g.kh = t.kh;
    g.kw = t.kw;
    g.sh = t.sh;
    g.sw = t.sw;
    g.K = t.kh * t.kw * g.cinp;
    g.residual = t.residual;
    g.opad = t.opad;
    /* where the input lies: the two encoders' first blocks read a layout of the caller's tensor, every other block its predecessor */
    g.in_cat = -1;
    g.in_off = 0;
    g.istride = g.cinp;
    if (block == 0 || block == W2L_FIRST_AUDIO) {
        g.ihalo = t.pad;
    } else {
        const W2lBlock p = W2L_TABLE[block - 1];
        g.ihalo = p.opad;
        if (p.cat >= 0) {
            g.in_cat = p.cat;
            g.in_off = block < W2L_FIRST_AUDIO ? W2L_CAT_A[p.cat] : 0;
            g.istride = W2L_CAT_C[p.cat];
        }
    }
    g.Hp = H + 2 * g.ihalo;
    g.Wp = W + 2 * g.ihalo;
    g.Hq = g.Ho + 2 * g.opad;
    g.Wq = g.Wo + 2 * g.opad;
    g.out_cat = t.cat;
    g.out_off = t.cat >= 0 && block < W2L_FIRST_AUDIO ? W2L_CAT_A[t.cat] : 0;
    g.out_stride = t.cat >= 0 ? W2L_CAT_C[t.cat] : t.cout;
    return g;
}

/* elements of the block's input and output as maps of their own (the single-block entry point, the walker) */
static inline size_t w2l_in_elems(const W2lGeom* g, int n) { return (size_t)n * g->Hp * g->Wp * g->cinp; }
static inline size_t w2l_out_elems(const W2lGeom* g, int n) { return (size_t)n * g->Hq * g->Wq * g->cout; }

/* the largest map outside the CAT buffers that any block reads or writes, per window */
static inline size_t w2l_max_map_elems(void) {
    size_t m = 0;
    for (int b = 0; b < W2L_BLOCKS; ++b) {
        const W2lGeom g = w2l_geom(b);
        const size_t i = w2l_in_elems(&g, 1), o = w2l_out_elems(&g, 1);
        if (g.in_cat < 0 && i > m) m = i;
        if (o > m) m = o;  /* the single-block entry point writes every output to a map of its own */
    }
    return m;
}

/* bf16 elements of a block's packed weights: hi and lo matrices [K][np] over all its classes (the head keeps its 3 x 32 fp32
 * weights as they are and has none) */
static inline size_t w2l_packed_elems(int block) {
    const W2lGeom g = w2l_geom(block);
    return block == W2L_HEAD ? 0 : (size_t)2 * g.K * g.np;
}

/* ---- classes -------------------------------------------------------------------------------------------------------------------
 * Class c covers the cells (oy + step i, ox + step j), i < Hc, j < Wc, of every window's padded output map: Mc = n Hc Wc rows.
 * Its A operand is tkh x tkw taps at input cell (iy + ty, ix + tx), tap = ty tkw + tx, K step s = tap cinp / 16 + c0 / 16; tap
 * `tap` multiplies the weights w[.., kidx[tap] / kw, kidx[tap] % kw] (kidx is the tap itself for a Conv2d block).  Its packed
 * matrix (hi, then lo, Kc np elements each, Kc = tkh tkw cinp) begins woff elements into the block's; its wave tiles are
 * tile0 .. tile0 + tiles - 1 of the launch. */
typedef struct W2lClass {
    int oy, ox, Hc, Wc, step, tkh, tkw, kidx[4];
    long long tile0;
    long long woff;
} W2lClass;

CN_HD long long w2l_class_rows(const W2lClass* c, int n) { return (long long)n * c->Hc * c->Wc; }
CN_HD long long w2l_class_tiles(const W2lClass* c, int n, int ntn) { return (w2l_class_rows(c, n) + CN_TILE_M - 1) / CN_TILE_M * ntn; }

/* the classes of a block for n windows and wave tiles of 32 NT columns; returns their number and the launch's tiles in *tiles */
static inline int w2l_classes(const W2lGeom* g, int n, int NT, W2lClass* cls, long long* tiles) {
    const int ntn = g->np / (32 * NT);
    int count = 0;
    if (!g->tr) {
        W2lClass c = {0, 0, g->Hq, g->Wq, 1, g->kh, g->kw, {0, 1, 2, 3}, 0, 0};
        cls[count++] = c;
    } else if (g->sh == 2) {
        for (int qy = 0; qy < 2; ++qy)
            for (int qx = 0; qx < 2; ++qx) {
                const int py = (qy + g->opad) & 1, px = (qx + g->opad) & 1;  /* parity of the output pixel y = yq - opad */
                W2lClass c = {qy, qx, g->Hq / 2, g->Wq / 2, 2, 1 + py, 1 + px, {0, 0, 0, 0}, 0, 0};
                for (int ty = 0; ty <= py; ++ty)
                    for (int tx = 0; tx <= px; ++tx) {
                        const int ky = py ? (ty ? 0 : 2) : 1, kx = px ? (tx ? 0 : 2) : 1;
                        c.kidx[ty * c.tkw + tx] = ky * g->kw + kx;
                    }
                cls[count++] = c;
            }
    } else {
        for (int cy = 0; cy < g->Ho; ++cy)
            for (int cx = 0; cx < g->Wo; ++cx) {
                /* pixel (cy, cx) with the halo cells before the first and behind the last pixel of each axis */
                const int oy = cy == 0 ? 0 : cy + g->opad, ox = cx == 0 ? 0 : cx + g->opad;
                const int hc = 1 + (cy == 0 ? g->opad : 0) + (cy == g->Ho - 1 ? g->opad : 0);
                const int wc = 1 + (cx == 0 ? g->opad : 0) + (cx == g->Wo - 1 ? g->opad : 0);
                W2lClass c = {oy, ox, hc, wc, 1, 1, 1, {cy * g->kw + cx, 0, 0, 0}, 0, 0};
                cls[count++] = c;
            }
    }
    long long tile = 0, woff = 0;
    for (int i = 0; i < count; ++i) {
        cls[i].tile0 = tile;
        cls[i].woff = woff;
        tile += w2l_class_tiles(&cls[i], n, ntn);
        woff += (long long)2 * cls[i].tkh * cls[i].tkw * g->cinp * g->np;
    }
    *tiles = tile;
    return count;
}

/* 32-column tiles per wave: one where the matrix is 32 columns wide, and where two would leave fewer than 1024 waves; else two */
static inline int w2l_wave_ntiles(const W2lGeom* g, int n) {
    if (g->np % 64) return 1;
    W2lClass cls[W2L_MAX_CLASSES];
    long long tiles;
    (void)w2l_classes(g, n, 2, cls, &tiles);
    return tiles < 1024 ? 1 : 2;
}

/* ---- rows of the implicit GEMM -------------------------------------------------------------------------------------------------
 * Row m of class c is cell (img, yq, xq) of the padded output map; rows past Mc compute row Mc - 1 again and are never stored. */
CN_HD void w2l_row_cell(long long m, long long Mc, int oy, int ox, int Hc, int Wc, int step, int* img, int* yq, int* xq) {
    int i, j;
    cn_row_cell(m, Mc, Hc, Wc, img, &i, &j);
    *yq = oy + step * i;
    *xq = ox + step * j;
}

/* the input cell of tap (0, 0) of output pixel y (one axis): Conv2d y s + (ihalo - pad); the parity classes y / 2 + ihalo (the
 * halo cell behind the last row is what (y + 1) / 2 reads for the last odd y); the 1 x 1 map's only cell */
CN_HD int w2l_in_cell(int y, int tr, int s, int ihalo, int pad) { return tr ? (s == 2 ? (y >> 1) + ihalo : ihalo) : y * s + ihalo - pad; }

CN_HD size_t w2l_cell(int img, int y, int x, int H, int W, int stride) { return (((size_t)img * H + (size_t)y) * W + (size_t)x) * stride; }

CN_HD size_t w2l_tap_offset(int tap, int tkw, int Wp, int istride) { return ((size_t)(tap / tkw) * Wp + (size_t)(tap % tkw)) * istride; }

#endif
