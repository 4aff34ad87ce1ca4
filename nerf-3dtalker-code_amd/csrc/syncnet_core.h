/*
 * syncnet_core.h -- the geometry table and the index arithmetic of n3dt_syncnet (include/n3dt.h): Wav2Lip's lip-sync expert
 * SyncNet_color (the reference's wav_models/syncnet.py over wav_models/conv.py), frozen, inference only.
 *
 * Included by csrc/syncnet.hip, whose convolution, layout and prologue kernels take their addresses from the functions below, and
 * by tests/syncnet_core_host.cpp, which walks the very same functions over the convolution kernel's grid on the CPU (under the
 * address and undefined-behaviour sanitizers) for all 31 blocks.  The weight pack's fragment arithmetic and the epilogue's
 * register -> row map are conv_frag.h's, the rows of the GEMM, the halo test, tap offsets, the crop prologue's resample and the
 * wave-tile rule conv_net_core.h's, shared with the other networks and walked by the same program; the block / wave / lane /
 * K-step nest of the convolution kernel is re-typed there.  Compiles as host C++ on its own; the __host__ __device__
 * qualifiers exist only under hipcc.
 *
 * Maps.  Every activation is NHWC fp32 with C a multiple of 16 (the two first blocks' 15 and 1 input channels are padded with
 * zero channels, their weight rows are zero) and carries the zero halo the NEXT block's padding needs.  A block's GEMM has one row
 * per CELL of its padded output map, halo cells included: a halo row computes a clamped pixel and stores 0, so every cell of the
 * output buffer is written by exactly one row and no buffer is ever cleared.
 */
#ifndef N3DT_SYNCNET_CORE_H
#define N3DT_SYNCNET_CORE_H

#include <stddef.h>

#include "conv_net_core.h"

#define SN_BLOCKS 31
#define SN_FACE_BLOCKS 17      /* blocks 0..16: the face encoder; 17..30: the audio encoder */
#define SN_EMB 512
#define SN_FACE_FRAMES 5
#define SN_FACE_C 15           /* 5 frames x BGR */
#define SN_FACE_H 48           /* the lower half of a 96 x 96 crop */
#define SN_FACE_W 96
#define SN_CROP 96
#define SN_MEL_H 80
#define SN_MEL_W 16
#define SN_MAX_WINDOWS 1024
#define SN_BN_EPS 1e-5

/* C_in, C_out, kernel (h, w), stride (h, w), padding, residual */
typedef struct SnBlock {
    int cin, cout, kh, kw, sh, sw, pad, residual;
} SnBlock;

static const SnBlock SN_TABLE[SN_BLOCKS] = {
    /* face encoder: [15, 48, 96] -> 512 */
    {15, 32, 7, 7, 1, 1, 3, 0},
    {32, 64, 5, 5, 1, 2, 1, 0},
    {64, 64, 3, 3, 1, 1, 1, 1},
    {64, 64, 3, 3, 1, 1, 1, 1},
    {64, 128, 3, 3, 2, 2, 1, 0},
    {128, 128, 3, 3, 1, 1, 1, 1},
    {128, 128, 3, 3, 1, 1, 1, 1},
    {128, 128, 3, 3, 1, 1, 1, 1},
    {128, 256, 3, 3, 2, 2, 1, 0},
    {256, 256, 3, 3, 1, 1, 1, 1},
    {256, 256, 3, 3, 1, 1, 1, 1},
    {256, 512, 3, 3, 2, 2, 1, 0},
    {512, 512, 3, 3, 1, 1, 1, 1},
    {512, 512, 3, 3, 1, 1, 1, 1},
    {512, 512, 3, 3, 2, 2, 1, 0},
    {512, 512, 3, 3, 1, 1, 0, 0},
    {512, 512, 1, 1, 1, 1, 0, 0},
    /* audio encoder: [1, 80, 16] -> 512 */
    {1, 32, 3, 3, 1, 1, 1, 0},
    {32, 32, 3, 3, 1, 1, 1, 1},
    {32, 32, 3, 3, 1, 1, 1, 1},
    {32, 64, 3, 3, 3, 1, 1, 0},
    {64, 64, 3, 3, 1, 1, 1, 1},
    {64, 64, 3, 3, 1, 1, 1, 1},
    {64, 128, 3, 3, 3, 3, 1, 0},
    {128, 128, 3, 3, 1, 1, 1, 1},
    {128, 128, 3, 3, 1, 1, 1, 1},
    {128, 256, 3, 3, 3, 2, 1, 0},
    {256, 256, 3, 3, 1, 1, 1, 1},
    {256, 256, 3, 3, 1, 1, 1, 1},
    {256, 512, 3, 3, 1, 1, 0, 0},
    {512, 512, 1, 1, 1, 1, 0, 0},
};

/* one block's maps: input [n, Hp, Wp, cinp] with halo ipad (its own padding), output [n, Hq, Wq, cout] with halo opad (the next
 * block's padding; 0 behind the last block of an encoder).  K = kh kw cinp is a multiple of 16. */
typedef struct SnGeom {
    int Hi, Wi, Ho, Wo, Hp, Wp, Hq, Wq, cinp, cout, ipad, opad, kh, kw, sh, sw, K, residual;
} SnGeom;

static inline SnGeom sn_geom(int block) {
    const int first = block < SN_FACE_BLOCKS ? 0 : SN_FACE_BLOCKS;
    const int last = block < SN_FACE_BLOCKS ? SN_FACE_BLOCKS - 1 : SN_BLOCKS - 1;
    int H = block < SN_FACE_BLOCKS ? SN_FACE_H : SN_MEL_H, W = block < SN_FACE_BLOCKS ? SN_FACE_W : SN_MEL_W;
    for (int b = first; b < block; ++b) {
        H = cn_conv_out(H, SN_TABLE[b].kh, SN_TABLE[b].sh, SN_TABLE[b].pad);
        W = cn_conv_out(W, SN_TABLE[b].kw, SN_TABLE[b].sw, SN_TABLE[b].pad);
    }
    const SnBlock t = SN_TABLE[block];
    SnGeom g;
    g.Hi = H;
    g.Wi = W;
    g.Ho = cn_conv_out(H, t.kh, t.sh, t.pad);
    g.Wo = cn_conv_out(W, t.kw, t.sw, t.pad);
    g.ipad = t.pad;
    g.opad = block == last ? 0 : SN_TABLE[block + 1].pad;
    g.Hp = H + 2 * g.ipad;
    g.Wp = W + 2 * g.ipad;
    g.Hq = g.Ho + 2 * g.opad;
    g.Wq = g.Wo + 2 * g.opad;
    g.cinp = cn_round16(t.cin);
    g.cout = t.cout;
    g.kh = t.kh;
    g.kw = t.kw;
    g.sh = t.sh;
    g.sw = t.sw;
    g.K = t.kh * t.kw * g.cinp;
    g.residual = t.residual;
    return g;
}

static inline size_t sn_in_elems(const SnGeom* g, int n) { return (size_t)n * g->Hp * g->Wp * g->cinp; }
static inline size_t sn_out_elems(const SnGeom* g, int n) { return (size_t)n * g->Hq * g->Wq * g->cout; }

/* the largest map any block reads or writes, per window */
static inline size_t sn_max_map_elems(void) {
    size_t m = 0;
    for (int b = 0; b < SN_BLOCKS; ++b) {
        const SnGeom g = sn_geom(b);
        const size_t i = sn_in_elems(&g, 1), o = sn_out_elems(&g, 1);
        if (i > m) m = i;
        if (o > m) m = o;
    }
    return m;
}

/* ---- addresses (the rows of the implicit GEMM, the halo test and the tap offsets are conv_net_core.h's) ----------------------------
 * first element of the receptive field of output pixel (img, y, x) in the padded NHWC input [n, Hp, Wp, cinp] */
CN_HD size_t sn_field_base(int img, int y, int x, int sh, int sw, int Hp, int Wp, int cinp) {
    return (((size_t)img * Hp + (size_t)y * sh) * Wp + (size_t)x * sw) * cinp;
}

/* a residual block (stride 1, C_in = C_out, same extent) adds its own input at the same pixel: where that pixel begins */
CN_HD size_t sn_residual_pixel(int img, int y, int x, int Hp, int Wp, int ipad, int cinp) {
    return (((size_t)img * Hp + (size_t)(y + ipad)) * Wp + (size_t)(x + ipad)) * cinp;
}

#endif
