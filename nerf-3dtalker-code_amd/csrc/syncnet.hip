// Wav2Lip's lip-sync expert SyncNet_color, frozen and inference-only (include/n3dt.h, n3dt_syncnet_*; the reference's
// wav_models/syncnet.py over wav_models/conv.py).  The geometry table and every address that can go wrong at
// an edge -- the rows of the GEMM, the halo cells, taps, residual reads and stores -- come from syncnet_core.h, which
// tests/syncnet_core_host.cpp also compiles and walks over the same grid for all 31 blocks.  That program re-types the loop nest of
// the convolution kernel below (block / wave / lane / K step): a change to that loop here must be made there too.  The epilogue's
// register -> row map, the pack kernel's element decode and the address the MFMA step reads its weights at are not re-typed:
// they are conv_frag.h's functions, which that program calls too, walking the pack of every block.  The flat element decodes of
// the layout, prologue and tail kernels are written inline.
//
//   faces      frames [F,3,H,W] fp32 RGB + crop boxes -> face windows [n,15,48,96]: crop, bilinear resample to 96 x 96 with
//              half-pixel centres in float64, rows 48..95, BGR, channel 3 t + c for frame t of the window
//   layout     [n,C,H,W] -> NHWC with C padded to 16 and the first block's zero halo
//   conv x31   Conv2d + folded BatchNorm2d (+ the block's own input) + ReLU as an implicit GEMM on v_mfma_f32_32x32x16_bf16
//              (M = cells of the padded output map, N = C_out, k = tap * C_in + c_in), every operand split x = hi + lo into two
//              bf16s and three products hi*hi + hi*lo + lo*hi accumulated in fp32: conv_mfma.h's step, which vgg_loss.hip and
//              lpips.hip share, in its split form.  There is no other mode.
//   tail       per window x / max(||x||_2, 1e-12) of both 512-vectors and their dot product, in float64, in a fixed order
//
// Every window goes through identical code with the same K order, no split-K and no atomics: a window's embeddings depend
// neither on its position in the batch nor on the batch size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/n3dt.h"
#include "conv_mfma.h"
#include "conv_net.h"
#include "syncnet_core.h"
#include "n3dt_launch.h"

// ---- packed weights ------------------------------------------------------------------------------------------------------------
// Per block one B matrix in conv_frag.h's fragment order, [K/16][C_out/32] fragments of 64 lanes x 8 bf16: element e holds
// B[k][n] = w'[n][ci][ky][kx] with (k, n) = cf_pack_decode(e), k = (ky kw + kx) cinp + ci; rows of the padded channels are
// zero.  The lo matrix lies right behind the hi matrix.  Then the folded fp32 biases.
struct SnPackLayout {
    size_t w[SN_BLOCKS], elems[SN_BLOCKS], bias[SN_BLOCKS], total;
};

static SnPackLayout sn_layout() {
    SnPackLayout L;
    size_t off = 0;
    for (int b = 0; b < SN_BLOCKS; ++b) {
        const SnGeom g = sn_geom(b);
        L.elems[b] = (size_t)g.K * g.cout;
        L.w[b] = off;
        off = rup(off + L.elems[b] * 2 * sizeof(__bf16), 256);
    }
    for (int b = 0; b < SN_BLOCKS; ++b) {
        L.bias[b] = off;
        off = rup(off + SN_TABLE[b].cout * sizeof(float), 256);
    }
    L.total = off;
    return L;
}

// batch norm folded in float64 by conv_net.hip's pack and bias kernels: s = gamma / sqrt(var + eps), w' = fp32(w s),
// b' = fp32((b - mean) s + beta)

// ---- face-window prologue ------------------------------------------------------------------------------------------------------
// one thread per element of faces [n, 15, 48, 96].  boxes: [n + 4, 4] or, with box_stride 0, one box for every frame.
__global__ __launch_bounds__(256) void syncnet_faces_kernel(int n, int height, int width, const float* __restrict__ frames,
                                                            const int* __restrict__ boxes, int box_stride, float* __restrict__ faces) {
    const size_t total = (size_t)n * SN_FACE_C * SN_FACE_H * SN_FACE_W;
    const size_t plane = (size_t)height * width;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int x = (int)(e % SN_FACE_W);
        size_t t = e / SN_FACE_W;
        const int y = (int)(t % SN_FACE_H);
        t /= SN_FACE_H;
        const int ch = (int)(t % SN_FACE_C), win = (int)(t / SN_FACE_C);
        const int frame = win + ch / 3, c = 2 - ch % 3;  // BGR: output channel 0 is the frame's blue
        int y1, h, x1, w;
        cn_clamp_box(boxes + (size_t)frame * box_stride, height, width, &y1, &h, &x1, &w);
        int ya, yb, xa, xb;
        double wy, wx;
        cn_bilinear(SN_CROP - SN_FACE_H + y, h, SN_CROP, &ya, &yb, &wy);
        cn_bilinear(x, w, SN_CROP, &xa, &xb, &wx);
        const float* src = frames + ((size_t)frame * 3 + c) * plane;
        double v[4];
        const size_t at[4] = {(size_t)(y1 + ya) * width + (x1 + xa), (size_t)(y1 + ya) * width + (x1 + xb),
                              (size_t)(y1 + yb) * width + (x1 + xa), (size_t)(y1 + yb) * width + (x1 + xb)};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float u = src[at[i]];
            if (!(u > 0.0f)) u = 0.0f;  // negative, -0 and NaN
            if (u > 1.0f) u = 1.0f;
            v[i] = (double)u;
        }
        const double uy = 1.0 - wy, ux = 1.0 - wx;
        faces[e] = (float)(uy * (ux * v[0] + wx * v[1]) + wy * (ux * v[2] + wx * v[3]));
    }
}

// layouts: conv_net.hip's -- [n,C,H,W] -> NHWC with C padded to 16 and the first block's zero halo, and back

// ---- implicit-GEMM convolution ---------------------------------------------------------------------------------------------------
struct SnConvArgs {
    const float* in;     // [n, Hp, Wp, cinp], zero halo included in Hp, Wp
    const __bf16* whi;   // packed B matrix (hi), [K/16][cout/32][64][8]
    const __bf16* wlo;
    const float* bias;   // [cout], batch norm folded in
    float* out;          // [n, Hq, Wq, cout], every cell written
    int n, Ho, Wo, Hp, Wp, Hq, Wq, cinp, cout, kh, kw, sh, sw, ipad, opad, residual;
};

// 256 threads = 4 waves; wave tile t = 4 blockIdx.x + wave computes CN_TILE_M cells x 32 NT channels: the tiles are numbered with
// the channel tile fastest, so the waves of a workgroup share their rows where C_out has several tiles, and a map of a few cells
// still spreads over C_out / (32 NT) waves.  A k-step is 16 channels of one tap (cinp % 16 == 0).
template <int NT>
__global__ __launch_bounds__(256) void syncnet_conv_kernel(SnConvArgs a) {
    const ConvWaveTile t = conv_wave_tile<NT>(a.cout, a.n, a.Hq, a.Wq);
    if (t.idle()) return;  // no barriers in this kernel: an idle wave may leave
    const int lane = t.lane, r = t.r, h = t.h, nt0 = t.nt0(NT);
    const long long Mq = t.M, m0 = t.m0;
    const float* base[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int img, yq, xq;
        cn_row_cell(m0 + mt * 32 + r, Mq, a.Hq, a.Wq, &img, &yq, &xq);  // rows past Mq compute the last cell again and are never stored
        const int y = cn_clampi(yq - a.opad, 0, a.Ho - 1), x = cn_clampi(xq - a.opad, 0, a.Wo - 1);
        base[mt] = a.in + sn_field_base(img, y, x, a.sh, a.sw, a.Hp, a.Wp, a.cinp);
    }
    conv_f32x16 acc[2][NT];
    CONV_ZERO_ACC(acc, NT);
    float av[2][8];

    int s = 0;
    for (int tap = 0; tap < a.kh * a.kw; ++tap) {
        const size_t toff = cn_tap_offset(tap, a.kw, a.Wp, a.cinp) + 8 * h;
        for (int c0 = 0; c0 < a.cinp; c0 += 16, ++s) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) conv_load8(base[mt] + toff + c0, av[mt]);
            conv_mma_step<true, NT>(a.whi, a.wlo, a.cout, s, nt0, lane, av, acc);
        }
    }

    // epilogue: accumulator register i of lane (r, h) is output row cf_acc_row(i, h), column r.
    // conv + folded bias, then the block's own input, then ReLU (wav_models/conv.py:15-19); 0 in the halo.
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long m = m0 + mt * 32 + cf_acc_row(i, h);
            if (m >= Mq) continue;
            int img, yq, xq;
            cn_row_cell(m, Mq, a.Hq, a.Wq, &img, &yq, &xq);
            const bool inside = cn_interior(yq, xq, a.Ho, a.Wo, a.opad);
            float* o = a.out + (size_t)m * a.cout;
            const float* res = nullptr;
            if (inside && a.residual) res = a.in + sn_residual_pixel(img, yq - a.opad, xq - a.opad, a.Hp, a.Wp, a.ipad, a.cinp);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int co = (nt0 + nt) * 32 + r;  // cout is a multiple of 32 NT: always inside
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

// ---- tail ------------------------------------------------------------------------------------------------------------------------
// one wave per window: lane l owns entries l, l + 64, ... of both vectors
__global__ __launch_bounds__(64) void syncnet_tail_kernel(const float* __restrict__ audio, const float* __restrict__ face,
                                                          float* __restrict__ audio_emb, float* __restrict__ face_emb, double* __restrict__ cosv) {
    const int lane = threadIdx.x;
    const size_t w = (size_t)blockIdx.x * SN_EMB;
    double sa = 0.0, sf = 0.0;
    for (int c = lane; c < SN_EMB; c += 64) {
        const double u = (double)audio[w + c], v = (double)face[w + c];
        sa += u * u;
        sf += v * v;
    }
    const double na = fmax(sqrt(conv_wave_sum(sa)), 1e-12), nf = fmax(sqrt(conv_wave_sum(sf)), 1e-12);
    double d = 0.0;
    for (int c = lane; c < SN_EMB; c += 64) {
        const double u = (double)audio[w + c] / na, v = (double)face[w + c] / nf;
        if (audio_emb) audio_emb[w + c] = (float)u;
        if (face_emb) face_emb[w + c] = (float)v;
        d += u * v;
    }
    d = conv_wave_sum(d);
    if (cosv && lane == 0) cosv[blockIdx.x] = d;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// workspace: the face windows [n,15,48,96], two maps that the blocks alternate between, the two raw 512-vectors per window
struct SnWorkspace {
    size_t faces, map[2], raw[2], total;  // byte offsets
};

static SnWorkspace sn_workspace(int n) {
    SnWorkspace w;
    size_t off = 0;
    auto take = [&off](size_t floats) {
        const size_t at = off;
        off += rup(floats * sizeof(float), 256);
        return at;
    };
    w.faces = take((size_t)n * SN_FACE_C * SN_FACE_H * SN_FACE_W);
    w.map[0] = take((size_t)n * sn_max_map_elems());
    w.map[1] = take((size_t)n * sn_max_map_elems());
    w.raw[0] = take((size_t)n * SN_EMB);
    w.raw[1] = take((size_t)n * SN_EMB);
    w.total = off;
    return w;
}

extern "C" size_t n3dt_syncnet_packed_layout_bytes(void) { return sn_layout().total; }
extern "C" size_t n3dt_syncnet_ws_bytes(int n) { return sn_workspace(n).total; }

extern "C" void n3dt_launch_syncnet_pack(const N3dtSyncnetParams* p, void* packed, hipStream_t st) {
    const SnPackLayout L = sn_layout();
    char* base = (char*)packed;
    for (int b = 0; b < SN_BLOCKS; ++b) {
        const SnGeom g = sn_geom(b);
        __bf16* hi = (__bf16*)(base + L.w[b]);
        const size_t n = L.elems[b];
        conv_net_pack(p->weight[b], p->bn_weight[b], p->bn_var[b], SN_BN_EPS, SN_TABLE[b].cin, SN_TABLE[b].cin, g.cinp, g.cout, g.cout, g.kh * g.kw, g.K,
                      0, hi, hi + n, st);
        conv_net_bias_bn(p->bias[b], p->bn_weight[b], p->bn_bias[b], p->bn_mean[b], p->bn_var[b], SN_BN_EPS, g.cout, (float*)(base + L.bias[b]), st);
    }
}

extern "C" void n3dt_launch_syncnet_faces(int n, int height, int width, const float* frames, const int* boxes, int box_stride, float* faces,
                                          hipStream_t st) {
    syncnet_faces_kernel<<<conv_grid((size_t)n * SN_FACE_C * SN_FACE_H * SN_FACE_W), 256, 0, st>>>(n, height, width, frames, boxes, box_stride, faces);
}

static void sn_conv(int block, int n, const void* packed, const float* in, float* out, hipStream_t st) {
    const SnPackLayout L = sn_layout();
    const SnGeom g = sn_geom(block);
    const char* pk = (const char*)packed;
    SnConvArgs a;
    a.in = in;
    a.whi = (const __bf16*)(pk + L.w[block]);
    a.wlo = a.whi + L.elems[block];
    a.bias = (const float*)(pk + L.bias[block]);
    a.out = out;
    a.n = n;
    a.Ho = g.Ho; a.Wo = g.Wo; a.Hp = g.Hp; a.Wp = g.Wp; a.Hq = g.Hq; a.Wq = g.Wq;
    a.cinp = g.cinp; a.cout = g.cout; a.kh = g.kh; a.kw = g.kw; a.sh = g.sh; a.sw = g.sw;
    a.ipad = g.ipad; a.opad = g.opad; a.residual = g.residual;
    const size_t Mq = (size_t)n * g.Hq * g.Wq;
    const size_t mtiles = (Mq + CN_TILE_M - 1) / CN_TILE_M;
    const int nt = cn_wave_ntiles((long long)Mq, g.cout);
    const size_t tiles = mtiles * (g.cout / (32 * nt));
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    if (nt == 1) syncnet_conv_kernel<1><<<grid, 256, 0, st>>>(a);
    else syncnet_conv_kernel<2><<<grid, 256, 0, st>>>(a);
}

// blocks first .. last on `src` [n, C, H, W]; the last block's output (halo 0) goes to `final`
static void sn_encoder(int first, int last, int n, const void* packed, const float* src, float* map0, float* map1, float* final, hipStream_t st) {
    const SnGeom g0 = sn_geom(first);
    conv_net_to_nhwc(src, n, SN_TABLE[first].cin, g0.Hi, g0.Wi, g0.ipad, g0.cinp, map0, g0.cinp, st);
    float* in = map0;
    float* out = map1;
    for (int b = first; b <= last; ++b) {
        float* dst = b == last ? final : out;
        sn_conv(b, n, packed, in, dst, st);
        out = in;
        in = dst;
    }
}

extern "C" void n3dt_launch_syncnet_fwd(int n, const void* packed, const float* mel, const float* faces, float* audio_emb, float* face_emb,
                                        double* cosv, void* workspace, hipStream_t st) {
    const SnWorkspace w = sn_workspace(n);
    char* ws = (char*)workspace;
    float* map0 = (float*)(ws + w.map[0]);
    float* map1 = (float*)(ws + w.map[1]);
    float* raw_face = (float*)(ws + w.raw[0]);
    float* raw_audio = (float*)(ws + w.raw[1]);
    sn_encoder(0, SN_FACE_BLOCKS - 1, n, packed, faces, map0, map1, raw_face, st);
    sn_encoder(SN_FACE_BLOCKS, SN_BLOCKS - 1, n, packed, mel, map0, map1, raw_audio, st);
    syncnet_tail_kernel<<<n, 64, 0, st>>>(raw_audio, raw_face, audio_emb, face_emb, cosv);
}

extern "C" float* n3dt_syncnet_ws_faces(int n, void* workspace) { return (float*)((char*)workspace + sn_workspace(n).faces); }

// one block alone: in [n, C_in, Hi, Wi] -> out [n, C_out, Ho, Wo]
extern "C" void n3dt_launch_syncnet_block(int block, int n, const void* packed, const float* in, float* out, void* workspace, hipStream_t st) {
    const SnWorkspace w = sn_workspace(n);
    const SnGeom g = sn_geom(block);
    char* ws = (char*)workspace;
    float* map0 = (float*)(ws + w.map[0]);
    float* map1 = (float*)(ws + w.map[1]);
    conv_net_to_nhwc(in, n, SN_TABLE[block].cin, g.Hi, g.Wi, g.ipad, g.cinp, map0, g.cinp, st);
    sn_conv(block, n, packed, map0, map1, st);
    conv_net_to_nchw(map1, g.cout, n, g.cout, g.Ho, g.Wo, g.opad, out, st);
}
