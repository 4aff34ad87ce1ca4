/*
 * fan_core.h -- the convolution table, the launch plan and the index arithmetic of n3dt_fan (include/n3dt.h): the AWing stacked
 * hourglass landmark detector (the reference's s_face3d/util/my_awing_arch.py, FAN over HourGlass / ConvBlock / CoordConvTh, with
 * calculate_points behind it as get_landmarks calls it), frozen, inference only.
 *
 * Included by csrc/fan.hip, whose kernels take their sizes and addresses from the functions below, and by tests/fan_core_host.cpp,
 * which walks the same plan and the same functions over the kernels' grids on the CPU under the address and undefined-behaviour
 * sanitizers.  The rows of the implicit GEMM, the stem's row order and the wave-tile rule are conv_net_core.h's; the fragment arithmetic is conv_frag.h's.  Compiles as host C++
 * on its own.
 *
 * Maps.  NHWC fp32 WITHOUT halos: the pre-activation relu(g x + b) of a ConvBlock sits in the convolution's A-operand fetch, and a
 * tap outside the map is predicated to zero there, behind the activation as the reference pads.  A convolution reads a channel
 * slice [c0, c0 + cin) of a map cs channels wide and writes a slice of another.
 *
 * Convolutions.  12 in front of the stacks (the stem CoordConv; conv2 = ConvBlock(64, 128): conv1, conv2, conv3, downsample;
 * conv3 = ConvBlock(128, 128); conv4 = ConvBlock(128, 256) with its downsample) and 47 per stack (the hourglass CoordConv, 14
 * ConvBlock(256, 256) -- the hourglass's 13 in state-dict order, then top_m -- of 3 each, conv_last, l, bl, al).
 */
#ifndef N3DT_FAN_CORE_H
#define N3DT_FAN_CORE_H

#include <stdint.h>

#include "conv_net_core.h"

#define FAN_MAX_MODULES 4
#define FAN_MAX_LANDMARKS 127
#define FAN_FRONT_CONVS 12
#define FAN_STACK_CONVS 47
#define FAN_MAX_CONVS (FAN_FRONT_CONVS + FAN_MAX_MODULES * FAN_STACK_CONVS)
#define FAN_IMG 256
#define FAN_STEM_HW 128
#define FAN_HEAT 64
#define FAN_CELLS 4096
#define FAN_MAX_IMAGES 1024
#define FAN_WS_BUDGET ((size_t)4 << 30)
#define FAN_BN_EPS 1e-5
#define FAN_NONE ((size_t)-1)
#define FAN_GATE_LEVEL 0.05f

/* blocks of the single-block entry: 6 in front (stem, conv2, conv3, conv4, the 2 x 2 average pool, the upsample-add) and 19 per
 * stack (coordconv, 13 hourglass ConvBlocks, top_m, conv_last, l, bl, al) */
#define FAN_FRONT_BLOCKS 6
#define FAN_STACK_BLOCKS 19
#define FAN_POOL_BLOCK 4
#define FAN_UPADD_BLOCK 5
#define FAN_MAX_BLOCKS (FAN_FRONT_BLOCKS + FAN_MAX_MODULES * FAN_STACK_BLOCKS)

enum { FAN_STEM = 0, FAN_CB1, FAN_CB2, FAN_CB3, FAN_DOWN, FAN_COORD, FAN_LAST, FAN_L, FAN_BL, FAN_AL };

/* C_in, C_out, kernel, stride, kind; bias: the convolution has one; pre: a BatchNorm + ReLU in front of it; post: a BatchNorm (+
 * ReLU) behind it, folded into the weights */
typedef struct FanConv {
    int cin, cout, k, stride, kind, bias, pre, post;
} FanConv;

static inline FanConv fan_cb(int cin, int cout, int r) {
    const FanConv c1 = {cin, cout / 2, 3, 1, FAN_CB1, 0, 1, 0}, c2 = {cout / 2, cout / 4, 3, 1, FAN_CB2, 0, 1, 0};
    const FanConv c3 = {cout / 4, cout / 4, 3, 1, FAN_CB3, 0, 1, 0}, cd = {cin, cout, 1, 1, FAN_DOWN, 0, 1, 0};
    return r == 0 ? c1 : r == 1 ? c2 : r == 2 ? c3 : cd;
}

/* convolution j of FAN(num_landmarks = N) */
static inline FanConv fan_conv(int j, int N) {
    const FanConv stem = {3, 64, 7, 2, FAN_STEM, 1, 0, 1};
    if (j == 0) return stem;
    if (j < 5) return fan_cb(64, 128, j - 1);
    if (j < 8) return fan_cb(128, 128, j - 5);
    if (j < 12) return fan_cb(128, 256, j - 8);
    const int t = (j - FAN_FRONT_CONVS) % FAN_STACK_CONVS;
    const FanConv coord = {256, 256, 1, 1, FAN_COORD, 1, 0, 0}, last = {256, 256, 1, 1, FAN_LAST, 1, 0, 1};
    const FanConv l = {256, N + 1, 1, 1, FAN_L, 1, 0, 0}, bl = {256, 256, 1, 1, FAN_BL, 1, 0, 0}, al = {N + 1, 256, 1, 1, FAN_AL, 1, 0, 0};
    if (t == 0) return coord;
    if (t < 43) return fan_cb(256, 256, (t - 1) % 3);
    return t == 43 ? last : t == 44 ? l : t == 45 ? bl : al;
}

static inline int fan_convs(int modules) { return FAN_FRONT_CONVS + modules * FAN_STACK_CONVS; }
static inline int fan_stack_conv(int stack, int t) { return FAN_FRONT_CONVS + stack * FAN_STACK_CONVS + t; }
/* the last stack has no bl and no al */
static inline int fan_conv_exists(int j, int modules) {
    if (j < FAN_FRONT_CONVS) return 1;
    const int s = (j - FAN_FRONT_CONVS) / FAN_STACK_CONVS, t = (j - FAN_FRONT_CONVS) % FAN_STACK_CONVS;
    return s < modules && (t < 45 || s < modules - 1);
}

/* channels of the K loop (the stem: its flattened K), rows of the packed matrix, its columns */
static inline int fan_cinp(const FanConv* c) { return c->kind == FAN_STEM ? 3 : cn_round16(c->cin); }
static inline int fan_K(const FanConv* c) { return c->kind == FAN_STEM ? CN_STEM_KP : c->k * c->k * cn_round16(c->cin); }
static inline int fan_np(const FanConv* c) { return cn_round32(c->cout); }
/* channels a heat map is stored with: N + 1 padded to al's K */
static inline int fan_heat_cs(int N) { return cn_round16(N + 1); }

/* input pixel of output pixel o at tap t; whether it lies inside a map of `in` pixels */
CN_HD int fan_tap_pixel(int o, int t, int stride, int pad) { return o * stride + t - pad; }
CN_HD int fan_inside(int y, int x, int H, int W) { return y >= 0 && y < H && x >= 0 && x < W; }

/* ---- the plan ----------------------------------------------------------------------------------------------------------------------
 * what a forward (or one block alone) launches, in order.  Offsets are floats PER IMAGE into the workspace, multiples of 64: a
 * map of an n-image call begins at n * offset floats, a multiple of 256 bytes. */
enum { FAN_OP_CONV = 0, FAN_OP_POOL, FAN_OP_UPADD };

typedef struct FanStep {
    int op, conv, stack;     /* stack: whose gates a COORD convolution takes (0: none) */
    int H, W, C;             /* the input map's extent (POOL, UPADD: of the output's larger side, see below) and, for these two, C */
    size_t in, out, skip, raw;
    int in_cs, in_c0, out_cs, out_c0, skip_cs, skip_c0, raw_cs;
} FanStep;

#define FAN_MAX_STEPS 1024

typedef struct FanPlan {
    FanStep step[FAN_MAX_STEPS];
    int steps;
    size_t top, peak;            /* bump allocator, floats per image */
    size_t heat[FAN_MAX_MODULES]; /* where each stack's heat map [64, 64, heat_cs] lies */
    size_t image;                /* [256, 256, 3] */
} FanPlan;

static inline size_t fan_alloc(FanPlan* p, size_t elems) {
    const size_t at = p->top;
    p->top += (elems + 63) / 64 * 64;
    if (p->top > p->peak) p->peak = p->top;
    return at;
}

static inline FanStep fan_step_init(int op, int conv, int H, int W) {
    FanStep s;
    s.op = op; s.conv = conv; s.stack = 0; s.H = H; s.W = W; s.C = 0;
    s.in = s.out = s.skip = s.raw = FAN_NONE;
    s.in_cs = s.in_c0 = s.out_cs = s.out_c0 = s.skip_cs = s.skip_c0 = s.raw_cs = 0;
    return s;
}

/* one plain convolution: in [H, W, cs_in] -> out [Ho, Wo, cs_out], whole maps */
static inline void fan_emit_conv(FanPlan* p, int j, int H, int W, size_t in, int in_cs, size_t out, int out_cs, size_t skip, int stack) {
    FanStep s = fan_step_init(FAN_OP_CONV, j, H, W);
    s.in = in; s.in_cs = in_cs; s.out = out; s.out_cs = out_cs; s.stack = stack;
    if (skip != FAN_NONE) { s.skip = skip; s.skip_cs = out_cs; }
    p->step[p->steps++] = s;
}

/* ConvBlock(cin, cout) whose first convolution is j: x [H, W, cin] -> y [H, W, cout] = cat(out1, out2, out3) + residual.  conv1
 * and conv2 leave their raw outputs in two temporaries for their successors; the residual (x itself, or the downsample branch's
 * map) is added slice by slice in the three epilogues. */
static inline void fan_emit_convblock(FanPlan* p, int j, int cin, int cout, int H, int W, size_t x, size_t y) {
    const size_t cells = (size_t)H * W, keep = p->top;
    size_t res = x;
    if (cin != cout) {
        res = fan_alloc(p, cells * cout);
        fan_emit_conv(p, j + 3, H, W, x, cin, res, cout, FAN_NONE, 0);
    }
    const size_t t1 = fan_alloc(p, cells * (cout / 2)), t2 = fan_alloc(p, cells * (cout / 4));
    FanStep s = fan_step_init(FAN_OP_CONV, j, H, W);
    s.in = x; s.in_cs = cin; s.out = y; s.out_cs = cout; s.skip = res; s.skip_cs = cout; s.raw = t1; s.raw_cs = cout / 2;
    p->step[p->steps++] = s;
    s = fan_step_init(FAN_OP_CONV, j + 1, H, W);
    s.in = t1; s.in_cs = cout / 2; s.out = y; s.out_cs = cout; s.out_c0 = cout / 2; s.skip = res; s.skip_cs = cout; s.skip_c0 = cout / 2;
    s.raw = t2; s.raw_cs = cout / 4;
    p->step[p->steps++] = s;
    s = fan_step_init(FAN_OP_CONV, j + 2, H, W);
    s.in = t2; s.in_cs = cout / 4; s.out = y; s.out_cs = cout; s.out_c0 = 3 * cout / 4; s.skip = res; s.skip_cs = cout; s.skip_c0 = 3 * cout / 4;
    p->step[p->steps++] = s;
    p->top = keep; /* the temporaries are free again: the stream orders their next writer behind these readers */
}

/* in [H, W, C] -> out [H / 2, W / 2, C], H and W even */
static inline void fan_emit_pool(FanPlan* p, int H, int W, int C, size_t in, size_t out) {
    FanStep s = fan_step_init(FAN_OP_POOL, -1, H, W);
    s.C = C; s.in = in; s.out = out;
    p->step[p->steps++] = s;
}

/* out [H, W, C] = up [H, W, C] (skip) + nearest x 2 of low [H / 2, W / 2, C] (in) */
static inline void fan_emit_upadd(FanPlan* p, int H, int W, int C, size_t low, size_t up, size_t out) {
    FanStep s = fan_step_init(FAN_OP_UPADD, -1, H, W);
    s.C = C; s.in = low; s.skip = up; s.out = out;
    p->step[p->steps++] = s;
}

/* HourGlass._forward(level, inp) -> the map it returns.  cb: the stack's first ConvBlock convolution; ConvBlocks in state-dict
 * order: b1_4, b2_4, b1_3, b2_3, b1_2, b2_2, b1_1, b2_1, b2_plus_1, b3_1, b3_2, b3_3, b3_4 */
static inline size_t fan_emit_hourglass(FanPlan* p, int cb, int level, int hw, size_t inp) {
    const size_t cells = (size_t)hw * hw, half = cells / 4;
    const int b1 = 2 * (4 - level), b2 = b1 + 1, b3 = 8 + level; /* b3_1 is 9 */
    const size_t up1 = fan_alloc(p, cells * 256), low0 = fan_alloc(p, half * 256), low1 = fan_alloc(p, half * 256);
    fan_emit_convblock(p, cb + 3 * b1, 256, 256, hw, hw, inp, up1);
    fan_emit_pool(p, hw, hw, 256, inp, low0);
    fan_emit_convblock(p, cb + 3 * b2, 256, 256, hw / 2, hw / 2, low0, low1);
    size_t low2;
    if (level > 1) {
        low2 = fan_emit_hourglass(p, cb, level - 1, hw / 2, low1);
    } else {
        low2 = fan_alloc(p, half * 256);
        fan_emit_convblock(p, cb + 3 * 8, 256, 256, hw / 2, hw / 2, low1, low2);
    }
    const size_t low3 = fan_alloc(p, half * 256), out = fan_alloc(p, cells * 256);
    fan_emit_convblock(p, cb + 3 * b3, 256, 256, hw / 2, hw / 2, low2, low3);
    fan_emit_upadd(p, hw, hw, 256, low3, up1, out);
    return out;
}

/* the whole forward.  The stacks share their maps (stack s + 1 writes where stack s wrote); `previous` alternates. */
static inline void fan_plan_forward(FanPlan* p, int modules, int N) {
    p->steps = 0;
    p->top = p->peak = 0;
    const int hcs = fan_heat_cs(N);
    p->image = fan_alloc(p, (size_t)FAN_IMG * FAN_IMG * 3);
    for (int s = 0; s < modules; ++s) p->heat[s] = fan_alloc(p, (size_t)FAN_CELLS * hcs);
    const size_t c128 = (size_t)FAN_STEM_HW * FAN_STEM_HW, c64 = FAN_CELLS;
    const size_t prev[2] = {fan_alloc(p, c64 * 256), fan_alloc(p, c64 * 256)};
    const size_t front = p->top;
    const size_t stem = fan_alloc(p, c128 * 64), x2 = fan_alloc(p, c128 * 128), xp = fan_alloc(p, c64 * 128), x3 = fan_alloc(p, c64 * 128);
    fan_emit_conv(p, 0, FAN_IMG, FAN_IMG, p->image, 3, stem, 64, FAN_NONE, 0);
    fan_emit_convblock(p, 1, 64, 128, FAN_STEM_HW, FAN_STEM_HW, stem, x2);
    fan_emit_pool(p, FAN_STEM_HW, FAN_STEM_HW, 128, x2, xp);
    fan_emit_convblock(p, 5, 128, 128, FAN_HEAT, FAN_HEAT, xp, x3);
    fan_emit_convblock(p, 8, 128, 256, FAN_HEAT, FAN_HEAT, x3, prev[0]);
    p->top = front;
    for (int s = 0; s < modules; ++s) {
        p->top = front;
        const int j0 = fan_stack_conv(s, 0);
        const size_t previous = prev[s & 1], cc = fan_alloc(p, c64 * 256);
        fan_emit_conv(p, j0, FAN_HEAT, FAN_HEAT, previous, 256, cc, 256, FAN_NONE, s);
        const size_t hg = fan_emit_hourglass(p, j0 + 1, 4, FAN_HEAT, cc);
        const size_t top = fan_alloc(p, c64 * 256), ll = fan_alloc(p, c64 * 256);
        fan_emit_convblock(p, j0 + 1 + 3 * 13, 256, 256, FAN_HEAT, FAN_HEAT, hg, top);
        fan_emit_conv(p, j0 + 43, FAN_HEAT, FAN_HEAT, top, 256, ll, 256, FAN_NONE, 0);
        fan_emit_conv(p, j0 + 44, FAN_HEAT, FAN_HEAT, ll, 256, p->heat[s], hcs, FAN_NONE, 0);
        if (s < modules - 1) {
            const size_t sum = fan_alloc(p, c64 * 256);
            fan_emit_conv(p, j0 + 45, FAN_HEAT, FAN_HEAT, ll, 256, sum, 256, previous, 0);
            fan_emit_conv(p, j0 + 46, FAN_HEAT, FAN_HEAT, p->heat[s], hcs, prev[(s + 1) & 1], 256, sum, 0);
        }
    }
}

/* ---- one block alone ---------------------------------------------------------------------------------------------------------------
 * block b -> (C_in, C_out, the input's divisor: output extent = input / div); conv: its first convolution or -1 */
typedef struct FanBlock {
    int cin, cout, div, conv, convblock, takes_skip, fixed_hw; /* fixed_hw: the only input extent it takes, or 0 */
} FanBlock;

static inline int fan_block_exists(int b, int modules) {
    if (b < 0) return 0;
    if (b < FAN_FRONT_BLOCKS) return 1;
    const int s = (b - FAN_FRONT_BLOCKS) / FAN_STACK_BLOCKS, t = (b - FAN_FRONT_BLOCKS) % FAN_STACK_BLOCKS;
    return s < modules && (t < 17 || s < modules - 1);
}

static inline FanBlock fan_block(int b, int N) {
    FanBlock k = {0, 0, 1, -1, 0, 0, 0};
    if (b == 0) { k.cin = 3; k.cout = 64; k.div = 2; k.conv = 0; k.fixed_hw = FAN_IMG; return k; }
    if (b == 1) { k.cin = 64; k.cout = 128; k.conv = 1; k.convblock = 1; return k; }
    if (b == 2) { k.cin = 128; k.cout = 128; k.conv = 5; k.convblock = 1; return k; }
    if (b == 3) { k.cin = 128; k.cout = 256; k.conv = 8; k.convblock = 1; return k; }
    if (b == FAN_POOL_BLOCK) { k.cin = k.cout = 256; k.div = 2; return k; }
    if (b == FAN_UPADD_BLOCK) { k.cin = k.cout = 256; k.div = -2; k.takes_skip = 1; return k; } /* the output is twice the input */
    const int s = (b - FAN_FRONT_BLOCKS) / FAN_STACK_BLOCKS, t = (b - FAN_FRONT_BLOCKS) % FAN_STACK_BLOCKS, j0 = fan_stack_conv(s, 0);
    k.cin = k.cout = 256;
    if (t == 0) { k.conv = j0; k.fixed_hw = FAN_HEAT; }
    else if (t < 15) { k.conv = j0 + 1 + 3 * (t - 1); k.convblock = 1; }
    else if (t == 15) k.conv = j0 + 43;
    else if (t == 16) { k.conv = j0 + 44; k.cout = N + 1; }
    else if (t == 17) { k.conv = j0 + 45; k.takes_skip = 1; }
    else { k.conv = j0 + 46; k.cin = N + 1; k.takes_skip = 1; }
    return k;
}

/* the plan of block b alone on an H x W input: the input map at 0, the output map and the skip map behind it */
typedef struct FanBlockMaps {
    size_t in, out, skip;
    int in_cs, out_cs, Ho, Wo;
} FanBlockMaps;

static inline FanBlockMaps fan_plan_block(FanPlan* p, int b, int N, int H, int W) {
    const FanBlock k = fan_block(b, N);
    FanBlockMaps m;
    p->steps = 0;
    p->top = p->peak = 0;
    m.Ho = k.div > 0 ? H / k.div : H * 2;
    m.Wo = k.div > 0 ? W / k.div : W * 2;
    m.in_cs = k.cin == 3 ? 3 : cn_round16(k.cin);
    m.out_cs = cn_round16(k.cout);
    m.in = fan_alloc(p, (size_t)H * W * m.in_cs);
    m.out = fan_alloc(p, (size_t)m.Ho * m.Wo * m.out_cs);
    m.skip = k.takes_skip ? fan_alloc(p, (size_t)m.Ho * m.Wo * m.out_cs) : FAN_NONE;
    if (b == FAN_POOL_BLOCK) fan_emit_pool(p, H, W, 256, m.in, m.out);
    else if (b == FAN_UPADD_BLOCK) fan_emit_upadd(p, m.Ho, m.Wo, 256, m.in, m.skip, m.out);
    else if (k.convblock) fan_emit_convblock(p, k.conv, k.cin, k.cout, H, W, m.in, m.out);
    else {
        const int s = b < FAN_FRONT_BLOCKS ? 0 : (b - FAN_FRONT_BLOCKS) / FAN_STACK_BLOCKS;
        fan_emit_conv(p, k.conv, H, W, m.in, m.in_cs, m.out, m.out_cs, m.skip, fan_conv(k.conv, N).kind == FAN_COORD ? s : 0);
    }
    return m;
}

static inline size_t fan_ws_bytes_of(const FanPlan* p, int n) { return p->peak * (size_t)n * sizeof(float); }

/* ---- the decode ----------------------------------------------------------------------------------------------------------------------
 * numpy's argmax order: a NaN beats everything, the first index wins ties */
CN_HD int fan_better(float v, int i, float bv, int bi) {
    const int vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (vn || v == bv) return i < bi;
    return v > bv;
}

/* calculate_points' neighbours of flat index i (i < 4095): literal flat indices, -1 wrapping to the map's last cell */
CN_HD int fan_x_up(int i) { return i + 1; }
CN_HD int fan_x_down(int i) { return i == 0 ? FAN_CELLS - 1 : i - 1; }
CN_HD int fan_y_up(int i, int any_up) { return any_up ? FAN_CELLS - 1 : i + FAN_HEAT; }
CN_HD int fan_y_down(int i, int any_down) { return any_down ? 0 : i - FAN_HEAT; }
CN_HD int fan_flag_up(int i) { return i + FAN_HEAT >= FAN_CELLS; }
CN_HD int fan_flag_down(int i) { return i - FAN_HEAT <= 0; }
CN_HD double fan_sign(double d) { return d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d; /* 0 stays 0, NaN stays NaN */ }

/* a crop box (y1, y2, x1, x2) inside an H x W frame: fine, or the status bit 2 */
CN_HD int fan_box_ok(const int* box, int H, int W) { return box[0] >= 0 && box[2] >= 0 && box[1] > box[0] && box[3] > box[2] && box[1] <= H && box[3] <= W; }

#endif
