// LPIPS with AlexNet features (include/n3dt.h, n3dt_lpips): the third number of the reference's validation pass
// (talker_trainer.py:1087-1150 -> Utils/Eval_utils.py:43-47,108-115).  The addresses that can go wrong at
// an edge -- the reinterpretation, the convolutions' rows, taps and stores, the pool windows, the halo cells -- come from
// lpips_core.h, which tests/lpips_core_host.cpp also compiles and walks over the same grids.  That program re-types the loop
// nests of the convolution, pool and halo kernels below (block / wave / lane / K step, the pool's and the halo kernel's element
// decodes): a change to one of those loops here must be made there too.  The epilogue's register -> row map, the pack kernel's
// element decode and the address the MFMA step reads its weights at are not re-typed: they are conv_frag.h's functions, which
// that program calls too, walking the pack of every layer.  The flat element decodes of the prologue and the distance kernel
// are written inline and are not walked.
//
//   prologue   pred, gt [B,3,H,W] fp32 -> in0: one batch of 2B images (predictions first, then targets), NHWC with a 2-pixel zero
//              halo.  reference mode: quantise to bytes (evm_quantise), read them as the reference's reshape(-1,3,h,w) of the HWC
//              image does, values 0..255; standard mode: 2 clamp(x,0,1) - 1, channels as given.  Then (v - shift) / scale in fp32.
//   conv x5    torchvision alexnet().features convolutions + bias + ReLU as implicit GEMMs on v_mfma_f32_32x32x16_bf16
//              (M = output pixels, N = C_out, k = tap * C_in + c_in), every operand split x = hi + lo into two bf16s and three
//              products hi*hi + hi*lo + lo*hi accumulated in fp32: conv_mfma.h's step, which vgg_loss.hip and syncnet.hip share,
//              in its split form (there is no other mode here).
//              conv1 (C_in = 3, 11x11, stride 4) gathers its operand element by element; the others read 8 channels at a time.
//   pool x2    3x3 / stride 2 max-pool of relu1 and relu2 into a halo-padded map of their own (relu1 and relu2 stay: they are
//              LPIPS features).
//   distance   per layer, one wave per pixel pair: n = f / (sqrt(sum_c f^2) + 1e-10), d = sum_c w_c (n0_c - n1_c)^2 in float64;
//              LP_PARTS fixed partial sums per image PAIR and layer, finished in index order: mean over pixels, then the five
//              layers added in layer order.
//
// Every image goes through identical code with the same K order, no split-K and no atomics, and a pair's partial sums are laid
// out by pair-local indices only, so lpips(x, x) is exactly 0, lpips(a, b) == lpips(b, a) bit for bit, and a pair's score depends
// neither on its position in the batch nor on the batch size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/n3dt.h"
#include "eval_metrics_core.h"
#include "conv_mfma.h"
#include "conv_net.h"
#include "lpips_core.h"
#include "n3dt_launch.h"

// ---- packed weights ------------------------------------------------------------------------------------------------------------
// Per conv one B matrix in conv_frag.h's fragment order, [Kp/16][Np/32] fragments of 64 lanes x 8 bf16: element e holds
// B[k][n] = W[n][ci][ky][kx] with (k, n) = cf_pack_decode(e), k = (ky * ksize + kx) * C_in + ci; rows k >= K are zero.  The lo
// matrix lies right behind the hi matrix.  Then the fp32 biases, then the fp32 lin weights.
struct LpPackLayout {
    size_t w[LP_LAYERS], elems[LP_LAYERS], bias[LP_LAYERS], lin[LP_LAYERS], total;
};

static LpPackLayout lp_layout() {
    LpPackLayout L;
    size_t off = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        L.elems[l] = (size_t)lp_kp(l) * lp_cout(l);
        L.w[l] = off;
        off = rup(off + L.elems[l] * 2 * sizeof(__bf16), 256);
    }
    for (int l = 0; l < LP_LAYERS; ++l) {
        L.bias[l] = off;
        off = rup(off + lp_cout(l) * sizeof(float), 256);
    }
    for (int l = 0; l < LP_LAYERS; ++l) {
        L.lin[l] = off;
        off = rup(off + lp_cout(l) * sizeof(float), 256);
    }
    L.total = off;
    return L;
}

__global__ __launch_bounds__(256) void lpips_pack_kernel(const float* __restrict__ W, int cin, int cout, int ksize, int kp,
                                                         __bf16* __restrict__ hi, __bf16* __restrict__ lo) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)kp * cout) return;
    int k, n;
    cf_pack_decode(e, cout / 32, &k, &n);
    float w = 0.0f;
    if (k < ksize * ksize * cin) {
        const int tap = k / cin, ci = k - tap * cin;
        w = W[((size_t)n * cin + ci) * (ksize * ksize) + tap];
    }
    const __bf16 h = (__bf16)w;
    hi[e] = h;
    lo[e] = conv_lo(w, h);
}

// ---- prologue --------------------------------------------------------------------------------------------------------------------
__constant__ float c_lp_shift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float c_lp_scale[3] = {0.458f, 0.448f, 0.450f};

// one thread per pixel of the padded in0 [2B, H + 4, W + 4, 3]: the halo is written as 0 (the convolution pads AFTER the scaling)
__global__ __launch_bounds__(256) void lpips_prologue_kernel(int B, int height, int width, int standard, const float* __restrict__ pred,
                                                             const float* __restrict__ gt, float* __restrict__ in0) {
    const int Hp = height + 4, Wp = width + 4;
    const size_t total = (size_t)2 * B * Hp * Wp;
    const size_t image = (size_t)3 * height * width, plane = (size_t)height * width;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int xp = (int)(e % Wp);
        const size_t t = e / Wp;
        const int yp = (int)(t % Hp), img = (int)(t / Hp);
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (xp >= 2 && xp < Wp - 2 && yp >= 2 && yp < Hp - 2) {
            const int y = yp - 2, x = xp - 2;
            const float* src = (img < B ? pred + (size_t)img * image : gt + (size_t)(img - B) * image);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float u;
                if (standard) {
                    u = src[c * plane + (size_t)y * width + x];
                    if (!(u > 0.0f)) u = 0.0f;  // negative, -0 and NaN
                    if (u > 1.0f) u = 1.0f;
                    u = 2.0f * u - 1.0f;
                } else {
                    u = (float)evm_quantise(src[lp_reinterpret_src(c, y, x, height, width)]);
                }
                v[c] = (u - c_lp_shift[c]) / c_lp_scale[c];
            }
        }
        float* o = in0 + e * 3;
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
    }
}

// ---- implicit-GEMM convolution ---------------------------------------------------------------------------------------------------
struct LpConvArgs {
    const float* in;     // [n_img, Hp, Wp, cin], zero halo included in Hp, Wp
    const __bf16* whi;   // packed B matrix (hi), [kp/16][np/32][64][8]
    const __bf16* wlo;
    const float* bias;   // [cout]
    float* out;          // [n_img, Ho + 2 out_pad, Wo + 2 out_pad, cout], interior only
    int n_img, Ho, Wo, Hp, Wp, cin, ksize, stride, K, kp, cout, out_pad;
};

// 256 threads = 4 waves; a wave computes LP_TILE_M output pixels x LP_TILE_N output channels (2 x 2 tiles of 32 x 32).
// GATHER false: cin % 16 == 0, a k-step is 16 channels of one tap;  GATHER true: conv1 (C_in = 3, 11x11), k decoded per element
// with the layer's constants folded in.
template <bool GATHER>
__global__ __launch_bounds__(256) void lpips_conv_kernel(LpConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long long M = (long long)a.n_img * a.Ho * a.Wo;
    const long long m0 = ((long long)blockIdx.x * 4 + wave) * LP_TILE_M;
    if (m0 >= M) return;  // no barriers in this kernel: an idle wave may leave
    const int nt0 = blockIdx.y * 2;
    const float* base[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int img, y, x;
        lp_row_pixel(m0 + mt * 32 + r, M, a.Ho, a.Wo, &img, &y, &x);  // rows past M compute a clamped pixel and are never stored
        base[mt] = a.in + lp_field_base(img, y, x, a.stride, a.Hp, a.Wp, a.cin);
    }
    conv_f32x16 acc[2][2];
    CONV_ZERO_ACC(acc, 2);
    float av[2][8];

    if constexpr (!GATHER) {
        int s = 0;
        for (int tap = 0; tap < a.ksize * a.ksize; ++tap) {
            const size_t toff = lp_tap_offset(tap, a.ksize, a.Wp, a.cin) + 8 * h;
            for (int c0 = 0; c0 < a.cin; c0 += 16, ++s) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) conv_load8(base[mt] + toff + c0, av[mt]);
                conv_mma_step<true, 2>(a.whi, a.wlo, a.cout, s, nt0, lane, av, acc);
            }
        }
    } else {
        for (int s = 0; s < (a.kp >> 4); ++s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * h + j;
                const bool ok = k < a.K;
                const size_t off = ok ? lp_gather_offset(k, lp_ksize(0), a.Wp, lp_cin(0)) : 0;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) av[mt][j] = ok ? base[mt][off] : 0.0f;
            }
            conv_mma_step<true, 2>(a.whi, a.wlo, a.cout, s, nt0, lane, av, acc);
        }
    }

    // epilogue: accumulator register i of lane (r, h) is output row cf_acc_row(i, h), column r
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long m = m0 + mt * 32 + cf_acc_row(i, h);
            if (m >= M) continue;
            int img, y, x;
            lp_row_pixel(m, M, a.Ho, a.Wo, &img, &y, &x);
            float* o = a.out + lp_out_pixel(img, y, x, a.Ho, a.Wo, a.out_pad, a.cout);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int co = (nt0 + nt) * 32 + r;  // cout is a multiple of LP_TILE_N: always inside
                const float v = acc[mt][nt][i] + a.bias[co];
                o[co] = v > 0.0f ? v : 0.0f;
            }
        }
}

// ---- pool, halo ----------------------------------------------------------------------------------------------------------------
// in [n, Hi, Wi, C] -> out [n, Ho + 2 pad, Wo + 2 pad, C]: the 3x3 / 2 maximum inside, 0 in the halo.  One thread per 4 channels.
__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* __restrict__ in, int n_img, int Hi, int Wi, int C, int Ho, int Wo, int pad,
                                                         float* __restrict__ out) {
    const int C4 = C >> 2, Hq = Ho + 2 * pad, Wq = Wo + 2 * pad;
    const size_t total = (size_t)n_img * Hq * Wq * C4;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c4 = (int)(e % C4);
        size_t t = e / C4;
        const int xq = (int)(t % Wq);
        t /= Wq;
        const int yq = (int)(t % Hq), img = (int)(t / Hq);
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (xq >= pad && xq < Wq - pad && yq >= pad && yq < Hq - pad) {
            const int oy = yq - pad, ox = xq - pad;
            m = *reinterpret_cast<const float4*>(in + lp_pool_src(img, oy, ox, 0, 0, Hi, Wi, C) + 4 * c4);
#pragma unroll
            for (int d = 1; d < 9; ++d) {
                const float4 q = *reinterpret_cast<const float4*>(in + lp_pool_src(img, oy, ox, d / 3, d % 3, Hi, Wi, C) + 4 * c4);
                m.x = fmaxf(m.x, q.x); m.y = fmaxf(m.y, q.y); m.z = fmaxf(m.z, q.z); m.w = fmaxf(m.w, q.w);
            }
        }
        *reinterpret_cast<float4*>(out + e * 4) = m;
    }
}

// zero the 1-pixel halo of a [n, H + 2, W + 2, C] map; blockIdx.y picks the map
struct LpHaloList {
    float* p[2];
    int C[2];
};

__global__ __launch_bounds__(256) void lpips_halo_kernel(LpHaloList L, int n_img, int H, int W) {
    float* p = L.p[blockIdx.y];
    const int C = L.C[blockIdx.y];
    const int cells = lp_halo_cells(H, W);
    const size_t total = (size_t)n_img * cells * C;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % C);
        const size_t t = e / C;
        const int cell = (int)(t % cells), img = (int)(t / cells);
        int y, x;
        lp_halo_cell(cell, H, W, &y, &x);
        p[(((size_t)img * (H + 2) + y) * (W + 2) + x) * C + c] = 0.0f;
    }
}

// ---- distance --------------------------------------------------------------------------------------------------------------------
// grid (LP_PARTS, B): workgroup (p, b) owns pixels i = 4 p + wave, stepping 4 LP_PARTS, of pair b (images b and B + b) -- pair-local
// indices only.  feat [2B, H + 2 pad, W + 2 pad, C], C a multiple of 64.  partial[b * LP_PARTS + p] = the workgroup's sum of d.
__global__ __launch_bounds__(256) void lpips_dist_kernel(const float* __restrict__ feat, int B, int H, int W, int C, int pad,
                                                         const float* __restrict__ lin, double* __restrict__ partial) {
    __shared__ double s_w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int npix = H * W;
    double acc = 0.0;
    for (int i = blockIdx.x * 4 + wave; i < npix; i += LP_PARTS * 4) {
        const int y = i / W, x = i - y * W;
        const float* f0 = feat + lp_out_pixel(b, y, x, H, W, pad, C);
        const float* f1 = feat + lp_out_pixel(B + b, y, x, H, W, pad, C);
        double s0 = 0.0, s1 = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double u = (double)f0[c], v = (double)f1[c];
            s0 += u * u;
            s1 += v * v;
        }
        const double n0 = sqrt(conv_wave_sum(s0)) + 1e-10, n1 = sqrt(conv_wave_sum(s1)) + 1e-10;
        double d = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double t = (double)f0[c] / n0 - (double)f1[c] / n1;
            d += (double)lin[c] * (t * t);
        }
        acc += conv_wave_sum(d);
    }
    if (lane == 0) s_w[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)b * LP_PARTS + blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

struct LpCounts {
    double npix[LP_LAYERS];
};

// one workgroup per pair: thread l adds layer l's LP_PARTS partials in index order; thread 0 adds the five layers in layer order
__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* __restrict__ partial, int B, LpCounts cnt, double* __restrict__ out,
                                                          double* __restrict__ layers) {
    __shared__ double s_l[LP_LAYERS];
    const int b = blockIdx.x;
    if (threadIdx.x < LP_LAYERS) {
        const double* p = partial + ((size_t)threadIdx.x * B + b) * LP_PARTS;
        double s = 0.0;
        for (int i = 0; i < LP_PARTS; ++i) s += p[i];
        s /= cnt.npix[threadIdx.x];
        s_l[threadIdx.x] = s;
        if (layers) layers[(size_t)threadIdx.x * B + b] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[b] = (((s_l[0] + s_l[1]) + s_l[2]) + s_l[3]) + s_l[4];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// workspace: in0, relu1, pool1, relu2, pool2, relu3, relu4, relu5 (floats, each rounded up to 64), then [5][B][LP_PARTS] doubles
struct LpWorkspace {
    size_t in0, relu[LP_LAYERS], pool[2], partial, total;  // byte offsets
};

static LpWorkspace lp_workspace(int batch, int height, int width) {
    const LpMaps g = lp_maps(2 * batch, height, width);
    LpWorkspace w;
    size_t off = 0;
    auto take = [&off](size_t floats) {
        const size_t at = off;
        off += rup(floats, 64) * sizeof(float);
        return at;
    };
    w.in0 = take(g.in0);
    w.relu[0] = take(g.relu[0]);
    w.pool[0] = take(g.pool[0]);
    w.relu[1] = take(g.relu[1]);
    w.pool[1] = take(g.pool[1]);
    for (int l = 2; l < LP_LAYERS; ++l) w.relu[l] = take(g.relu[l]);
    w.partial = off;
    w.total = off + (size_t)LP_LAYERS * batch * LP_PARTS * sizeof(double);
    return w;
}

extern "C" size_t n3dt_lpips_packed_layout_bytes(void) { return lp_layout().total; }
extern "C" size_t n3dt_lpips_ws_bytes(int batch, int height, int width) { return lp_workspace(batch, height, width).total; }

extern "C" void n3dt_launch_lpips_pack(const N3dtLpipsParams* p, void* packed, hipStream_t st) {
    const LpPackLayout L = lp_layout();
    char* base = (char*)packed;
    for (int l = 0; l < LP_LAYERS; ++l) {
        __bf16* hi = (__bf16*)(base + L.w[l]);
        const size_t n = L.elems[l];
        lpips_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(p->weight[l], lp_cin(l), lp_cout(l), lp_ksize(l), lp_kp(l), hi, hi + n);
        conv_net_copy(p->bias[l], (size_t)lp_cout(l), (float*)(base + L.bias[l]), st);
        conv_net_copy(p->lin[l], (size_t)lp_cout(l), (float*)(base + L.lin[l]), st);
    }
}

extern "C" void n3dt_launch_lpips(int batch, int height, int width, int input_mode, const void* packed, const float* pred, const float* gt,
                                  double* out, double* layers, void* workspace, hipStream_t st) {
    const LpPackLayout L = lp_layout();
    const LpWorkspace w = lp_workspace(batch, height, width);
    const int n_img = 2 * batch;
    const LpMaps g = lp_maps(n_img, height, width);
    char* ws = (char*)workspace;
    const char* pk = (const char*)packed;
    float* in0 = (float*)(ws + w.in0);
    float* relu[LP_LAYERS];
    for (int l = 0; l < LP_LAYERS; ++l) relu[l] = (float*)(ws + w.relu[l]);
    float* pool[2] = {(float*)(ws + w.pool[0]), (float*)(ws + w.pool[1])};
    double* partial = (double*)(ws + w.partial);

    lpips_prologue_kernel<<<conv_grid(g.in0 / 3), 256, 0, st>>>(batch, height, width, input_mode == N3DT_LPIPS_STANDARD, pred, gt, in0);
    const float* in = in0;
    int Hp = height + 4, Wp = width + 4;
    for (int l = 0; l < LP_LAYERS; ++l) {
        if (l == 1 || l == 2) {  // the pool in front of conv2 and conv3, padded for that convolution
            const int pad = lp_pad(l);
            lpips_pool_kernel<<<conv_grid(g.pool[l - 1] / 4), 256, 0, st>>>(relu[l - 1], n_img, g.fh[l - 1], g.fw[l - 1], lp_cout(l - 1), g.fh[l], g.fw[l],
                                                                          pad, pool[l - 1]);
            in = pool[l - 1];
            Hp = g.fh[l] + 2 * pad;
            Wp = g.fw[l] + 2 * pad;
        }
        if (l == 2) {
            LpHaloList hl;
            hl.p[0] = relu[2];
            hl.C[0] = lp_cout(2);
            hl.p[1] = relu[3];
            hl.C[1] = lp_cout(3);
            lpips_halo_kernel<<<dim3(64, 2), 256, 0, st>>>(hl, n_img, g.fh[2], g.fw[2]);
        }
        LpConvArgs a;
        a.in = in;
        a.whi = (const __bf16*)(pk + L.w[l]);
        a.wlo = a.whi + L.elems[l];
        a.bias = (const float*)(pk + L.bias[l]);
        a.out = relu[l];
        a.n_img = n_img;
        a.Ho = g.fh[l];
        a.Wo = g.fw[l];
        a.Hp = Hp;
        a.Wp = Wp;
        a.cin = lp_cin(l);
        a.ksize = lp_ksize(l);
        a.stride = lp_stride(l);
        a.K = lp_k(l);
        a.kp = lp_kp(l);
        a.cout = lp_cout(l);
        a.out_pad = lp_feat_pad(l);
        const size_t M = (size_t)n_img * a.Ho * a.Wo;
        const dim3 grid((unsigned)((M + LP_WG_M - 1) / LP_WG_M), (unsigned)(a.cout / LP_TILE_N));
        if (l == 0) lpips_conv_kernel<true><<<grid, 256, 0, st>>>(a);
        else lpips_conv_kernel<false><<<grid, 256, 0, st>>>(a);
        in = relu[l];  // relu3 and relu4 carry the next convolution's halo themselves
        Hp = a.Ho + 2 * a.out_pad;
        Wp = a.Wo + 2 * a.out_pad;
    }
    LpCounts cnt;
    for (int l = 0; l < LP_LAYERS; ++l) {
        lpips_dist_kernel<<<dim3(LP_PARTS, batch), 256, 0, st>>>(relu[l], batch, g.fh[l], g.fw[l], lp_cout(l), lp_feat_pad(l),
                                                                 (const float*)(pk + L.lin[l]), partial + (size_t)l * batch * LP_PARTS);
        cnt.npix[l] = (double)g.fh[l] * (double)g.fw[l];
    }
    lpips_finish_kernel<<<batch, 64, 0, st>>>(partial, batch, cnt, out, layers);
}
