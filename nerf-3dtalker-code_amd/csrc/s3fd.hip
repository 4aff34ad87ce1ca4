// The S3FD face detector, frozen and inference-only (include/n3dt.h, n3dt_s3fd_*; the reference's
// face_detection/detection/sfd/{net_s3fd,detect,bbox,sfd_detector}.py under face_detection/api.py).  The
// table, every map's size -- known only at run time, a function of the frame's (H, W) -- and every address that can go wrong at an
// edge come from s3fd_core.h, which tests/s3fd_core_host.cpp also compiles and walks over the same grids.  That program re-types
// the loop nest of the convolution kernel below (block / wave / lane / K step): a change to that loop here must be made there too.
//
//   frames     frames [n,3,H,W] fp32 RGB in [0,1] -> the network's padded NHWC input, 255 u - (104, 117, 123)[c] in float64
//   conv x25   Conv2d (+ ReLU) as an implicit GEMM on v_mfma_f32_32x32x16_bf16 (M = cells of the padded output map, N = C_out,
//              k = tap * C_in + c_in), every operand split x = hi + lo into two bf16s, three products accumulated in fp32:
//              conv_mfma.h's step in its split form.  19 backbone convolutions and six head pairs (conf + loc as one matrix of 32
//              columns of which the first 8 or 6 are stored) go through the one kernel.
//   pool x5    2 x 2 / 2 max with floor, writing the next map with its halo
//   norm x3    x / (sqrt(sum_c x^2) + 1e-10) weight[c], the sum in float64 in channel order
//   tail       scores (level 1's max-out, two-way softmax), decode, greedy NMS, crop boxes: float64, fixed order, no atomics
//
// Every image goes through identical code with the same K order, no split-K and no atomics: an image's result depends neither on
// its position in the batch nor on the batch size.  Every element of every map, halo included, is written exactly once per
// forward; nothing is cleared.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/n3dt.h"
#include "conv_mfma.h"
#include "conv_net.h"
#include "s3fd_core.h"
#include "n3dt_launch.h"

// ---- packed weights ------------------------------------------------------------------------------------------------------------
// Per GEMM one B matrix in conv_frag.h's fragment order, hi then lo, then the fp32 biases (32 per head pair, the unused ones 0).
struct S3PackLayout {
    size_t w[S3_GEMMS], elems[S3_GEMMS], bias[S3_GEMMS], norm[S3_NORMS], total;
};

static S3PackLayout s3_layout() {
    S3PackLayout L;
    size_t off = 0;
    for (int j = 0; j < S3_GEMMS; ++j) {
        const S3Geom g = s3_gemm_geom(j, S3_MIN_HW, S3_MIN_HW);  // K and np do not depend on the size
        L.elems[j] = (size_t)g.K * g.np;
        L.w[j] = off;
        off = rup(off + L.elems[j] * 2 * sizeof(__bf16), 256);
    }
    for (int j = 0; j < S3_GEMMS; ++j) {
        const S3Geom g = s3_gemm_geom(j, S3_MIN_HW, S3_MIN_HW);
        L.bias[j] = off;
        off = rup(off + g.np * sizeof(float), 256);
    }
    for (int l = 0; l < S3_NORMS; ++l) {
        L.norm[l] = off;
        off = rup(off + s3_level_c(l) * sizeof(float), 256);
    }
    L.total = off;
    return L;
}

// columns 0 .. c0 - 1 come from W0 [c0, cin, taps], columns c0 .. c0 + c1 - 1 from W1 [c1, cin, taps] (a head pair: conf, loc);
// the rest of the np columns and the rows of the padded channels are zero
__global__ __launch_bounds__(256) void s3fd_pack_kernel(const float* __restrict__ W0, int c0, const float* __restrict__ W1, int c1, int cin,
                                                        int cinp, int np, int taps, int K, __bf16* __restrict__ hi, __bf16* __restrict__ lo) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)K * np) return;
    int k, n;
    cf_pack_decode(e, np / 32, &k, &n);
    const int tap = k / cinp, ci = k - tap * cinp;
    float w = 0.0f;
    if (ci < cin) {
        if (n < c0) w = W0[((size_t)n * cin + ci) * taps + tap];
        else if (n < c0 + c1) w = W1[((size_t)(n - c0) * cin + ci) * taps + tap];
    }
    const __bf16 h = (__bf16)w;
    hi[e] = h;
    lo[e] = conv_lo(w, h);
}

__global__ __launch_bounds__(256) void s3fd_bias_kernel(const float* __restrict__ b0, int c0, const float* __restrict__ b1, int c1, int np,
                                                        float* __restrict__ dst) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < np) dst[n] = n < c0 ? b0[n] : n < c0 + c1 ? b1[n - c0] : 0.0f;
}

// ---- prologue and layouts ------------------------------------------------------------------------------------------------------
// frames [n,3,H,W] fp32 RGB in [0,1] -> dst [n, H + 2 pad, W + 2 pad, 16]: channel c = 255 u - mean[c] with the Caffe means
// (104, 117, 123) on R, G, B in that order (api.py:65 reverses BGR to RGB, detect.py:59 subtracts the BGR means: the
// reference's own quirk), in float64, rounded once; zero in the halo and in channels 3..15.  One thread per cell.
__global__ __launch_bounds__(256) void s3fd_frames_kernel(const float* __restrict__ frames, int n, int H, int W, int pad, float* __restrict__ dst) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const size_t total = (size_t)n * Hp * Wp, plane = (size_t)H * W;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        int img, yp, xp;
        cn_cell(e, Hp, Wp, &img, &yp, &xp);
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (xp >= pad && xp < Wp - pad && yp >= pad && yp < Hp - pad) {
            const double mean[3] = {104.0, 117.0, 123.0};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float u = frames[((size_t)img * 3 + c) * plane + (size_t)(yp - pad) * W + (xp - pad)];
                if (!(u > 0.0f)) u = 0.0f;  // negative, -0 and NaN
                if (u > 1.0f) u = 1.0f;
                v[c] = (float)(255.0 * (double)u - mean[c]);
            }
        }
        float4* o = reinterpret_cast<float4*>(dst + e * 16);
        o[0] = make_float4(v[0], v[1], v[2], 0.0f);
        o[1] = o[2] = o[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// the plain layouts [n,C,H,W] <-> padded NHWC are conv_net.hip's

// level 1's confidences: src [n, H, W, Cs] (no halo) -> dst [n, 2, H, W], channel 0 = max(max(s0, s1), s2) and channel 1 = s3 of the
// first four source channels (net_s3fd.py:124-127)
__global__ __launch_bounds__(256) void s3fd_maxout_nchw_kernel(const float* __restrict__ src, int n, int Cs, int H, int W, float* __restrict__ dst) {
    const int C = 2;
    const size_t total = (size_t)n * C * H * W;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int x = (int)(e % W);
        size_t t = e / W;
        const int y = (int)(t % H);
        t /= H;
        const int c = (int)(t % C), img = (int)(t / C);
        const float* s = src + (((size_t)img * H + y) * W + x) * Cs;
        dst[e] = c == 0 ? fmaxf(fmaxf(s[0], s[1]), s[2]) : s[3];
    }
}

// ---- implicit-GEMM convolution ---------------------------------------------------------------------------------------------------
struct S3ConvArgs {
    const float* in;     // [n, Hp, Wp, cinp], halo included in Hp, Wp
    const __bf16* whi;   // packed B matrix (hi), [K/16][np/32][64][8]
    const __bf16* wlo;
    const float* bias;   // [np]
    float* out;          // [n, Hq, Wq, cstore], every cell written
    int n, Ho, Wo, Hp, Wp, Hq, Wq, cinp, np, cstore, k, stride, ioff, opad, relu;
};

// 256 threads = 4 waves; wave tile t = 4 blockIdx.x + wave computes CN_TILE_M cells x 32 NT columns, the column tile fastest.
// A k-step is 16 channels of one tap (cinp % 16 == 0).  Every dimension, stride and halo width is a run-time argument; the row
// index is 64-bit (n Hq Wq reaches tens of millions at 512 x 512).
template <int NT>
__global__ __launch_bounds__(256) void s3fd_conv_kernel(S3ConvArgs a) {
    const ConvWaveTile t = conv_wave_tile<NT>(a.np, a.n, a.Hq, a.Wq);
    if (t.idle()) return;  // no barriers in this kernel: an idle wave may leave
    const int lane = t.lane, r = t.r, h = t.h, nt0 = t.nt0(NT);
    const long long Mq = t.M, m0 = t.m0;
    const float* base[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int img, yq, xq;
        cn_row_cell(m0 + mt * 32 + r, Mq, a.Hq, a.Wq, &img, &yq, &xq);  // rows past Mq compute the last cell again and are never stored
        const int y = cn_clampi(yq - a.opad, 0, a.Ho - 1), x = cn_clampi(xq - a.opad, 0, a.Wo - 1);
        base[mt] = a.in + s3_field_base(img, y, x, a.stride, a.ioff, a.Hp, a.Wp, a.cinp);
    }
    conv_f32x16 acc[2][NT];
    CONV_ZERO_ACC(acc, NT);
    float av[2][8];

    int s = 0;
    for (int tap = 0; tap < a.k * a.k; ++tap) {
        const size_t toff = cn_tap_offset(tap, a.k, a.Wp, a.cinp) + 8 * h;
        for (int c0 = 0; c0 < a.cinp; c0 += 16, ++s) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) conv_load8(base[mt] + toff + c0, av[mt]);
            conv_mma_step<true, NT>(a.whi, a.wlo, a.np, s, nt0, lane, av, acc);
        }
    }

    // epilogue: accumulator register i of lane (r, h) is output row cf_acc_row(i, h), column r.  conv + bias (+ ReLU); 0 in the
    // halo; columns cstore .. np - 1 of a head pair are never stored.
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long m = m0 + mt * 32 + cf_acc_row(i, h);
            if (m >= Mq) continue;
            int img, yq, xq;
            cn_row_cell(m, Mq, a.Hq, a.Wq, &img, &yq, &xq);
            const bool inside = cn_interior(yq, xq, a.Ho, a.Wo, a.opad);
            float* o = a.out + (size_t)m * a.cstore;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int co = (nt0 + nt) * 32 + r;
                if (co >= a.cstore) continue;
                float v = 0.0f;
                if (inside) {
                    v = acc[mt][nt][i] + a.bias[co];
                    if (a.relu) v = v > 0.0f ? v : 0.0f;
                }
                o[co] = v;
            }
        }
}

// ---- pool and norm -----------------------------------------------------------------------------------------------------------------
// in [n, Hi + 2 ihalo, Wi + 2 ihalo, C] -> out [n, Ho + 2 opad, Wo + 2 opad, C], Ho = Hi / 2, Wo = Wi / 2 (floor): one thread per
// four channels of a cell of the padded output; 0 in the halo
__global__ __launch_bounds__(256) void s3fd_pool_kernel(const float* __restrict__ in, int n, int Hi, int Wi, int ihalo, int C, int opad,
                                                        float* __restrict__ out) {
    const int Ho = Hi / 2, Wo = Wi / 2, Hq = Ho + 2 * opad, Wq = Wo + 2 * opad, C4 = C / 4;
    const size_t total = (size_t)n * Hq * Wq * C4;
    const size_t row = (size_t)(Wi + 2 * ihalo) * C;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % C4) * 4;
        int img, yq, xq;
        cn_cell(e / C4, Hq, Wq, &img, &yq, &xq);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (cn_interior(yq, xq, Ho, Wo, opad)) {
            const float* p = in + s3_pool_base(img, yq - opad, xq - opad, Hi, Wi, ihalo, C) + c;
            const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + C);
            const float4 d = *reinterpret_cast<const float4*>(p + row), f = *reinterpret_cast<const float4*>(p + row + C);
            v.x = fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, f.x));
            v.y = fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, f.y));
            v.z = fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, f.z));
            v.w = fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, f.w));
        }
        *reinterpret_cast<float4*>(out + e * 4) = v;
    }
}

// in [n, H, W, C] (no halo) -> out [n, H + 2, W + 2, C]: x / (sqrt(sum_c x^2) + 1e-10) * weight[c], the sum in float64 in channel
// order, the quotient and product in float64, rounded once; 0 in the halo.  One thread per cell.
__global__ __launch_bounds__(256) void s3fd_norm_kernel(const float* __restrict__ in, const float* __restrict__ weight, int n, int H, int W, int C,
                                                        float* __restrict__ out) {
    const int Hq = H + 2, Wq = W + 2;
    const size_t total = (size_t)n * Hq * Wq;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        int img, yq, xq;
        cn_cell(e, Hq, Wq, &img, &yq, &xq);
        float4* o = reinterpret_cast<float4*>(out + e * C);
        if (!cn_interior(yq, xq, H, W, 1)) {
            for (int c = 0; c < C / 4; ++c) o[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            continue;
        }
        const float4* x = reinterpret_cast<const float4*>(in + (((size_t)img * H + (yq - 1)) * W + (xq - 1)) * C);
        const float4* wv = reinterpret_cast<const float4*>(weight);
        double s = 0.0;
        for (int c = 0; c < C / 4; ++c) {
            const float4 v = x[c];
            s += (double)v.x * (double)v.x;
            s += (double)v.y * (double)v.y;
            s += (double)v.z * (double)v.z;
            s += (double)v.w * (double)v.w;
        }
        const double nrm = sqrt(s) + S3_NORM_EPS;
        for (int c = 0; c < C / 4; ++c) {
            const float4 v = x[c], g = wv[c];
            o[c] = make_float4((float)((double)v.x / nrm * (double)g.x), (float)((double)v.y / nrm * (double)g.y),
                               (float)((double)v.z / nrm * (double)g.z), (float)((double)v.w / nrm * (double)g.w));
        }
    }
}

// ---- tail ------------------------------------------------------------------------------------------------------------------------
struct S3Levels {
    const float* head[S3_LEVELS];  // [n, lh, lw, cols]
    int first[S3_LEVELS + 1], lh[S3_LEVELS], lw[S3_LEVELS];
};

// one thread per (image, position): the face score and the decoded box, float64
__global__ __launch_bounds__(256) void s3fd_score_kernel(S3Levels L, int n, double* __restrict__ score, double* __restrict__ box) {
    const int P = L.first[S3_LEVELS];
    const size_t total = (size_t)n * P;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int img = (int)(e / P), p = (int)(e - (size_t)img * P);
        int l, y, x;
        s3_position(p, L.first, L.lw, &l, &y, &x);
        const int cols = s3_level_cols(l);
        const float* hm = L.head[l] + (((size_t)img * L.lh[l] + y) * L.lw[l] + x) * cols;
        double c0, c1;
        if (l == 0) {
            c0 = (double)fmaxf(fmaxf(hm[0], hm[1]), hm[2]);
            c1 = (double)hm[3];
        } else {
            c0 = (double)hm[0];
            c1 = (double)hm[1];
        }
        const float* lp = hm + s3_level_conf(l);
        const double loc[4] = {(double)lp[0], (double)lp[1], (double)lp[2], (double)lp[3]};
        double b[4];
        s3_decode(s3_level_stride(l), y, x, loc, b);
        score[e] = s3_score(c0, c1);
#pragma unroll
        for (int i = 0; i < 4; ++i) box[e * 4 + i] = b[i];
    }
}

// greedy NMS, one workgroup of 1024 threads per image: the highest remaining score > 0.5 (ties: the lowest position) is kept, every
// remaining position whose overlap with it is > 0.3 is suppressed, until none is left or max_faces are kept.
// dets [n, max_faces, 5] (x1, y1, x2, y2, score; unused rows 0), count [n], left [n] (positions still standing when the cap cut)
#define S3_NMS_THREADS 1024
__global__ __launch_bounds__(S3_NMS_THREADS) void s3fd_nms_kernel(int P, int max_faces, const double* __restrict__ score,
                                                                  const double* __restrict__ box, unsigned char* __restrict__ sup,
                                                                  double* __restrict__ dets, int* __restrict__ count, int* __restrict__ left) {
    __shared__ double s_val[S3_NMS_THREADS / 64];
    __shared__ int s_idx[S3_NMS_THREADS / 64];
    __shared__ int s_best;
    const int tid = threadIdx.x, img = blockIdx.x;
    const double* sc = score + (size_t)img * P;
    const double* bx = box + (size_t)img * P * 4;
    unsigned char* sp = sup + (size_t)img * P;
    double* out = dets + (size_t)img * max_faces * 5;
    for (int p = tid; p < P; p += S3_NMS_THREADS) sp[p] = sc[p] > S3_SCORE_THRESH ? 0 : 1;
    __syncthreads();
    int kept = 0;
    while (kept < max_faces) {
        double bv = -1.0;
        int bi = 0x7fffffff;
        for (int p = tid; p < P; p += S3_NMS_THREADS)
            if (!sp[p] && sc[p] > bv) {  // ascending p: a tie keeps the lower one
                bv = sc[p];
                bi = p;
            }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
            const double ov = __shfl_xor(bv, w, 64);
            const int oi = __shfl_xor(bi, w, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            s_val[tid >> 6] = bv;
            s_idx[tid >> 6] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < S3_NMS_THREADS / 64; ++w)
                if (s_val[w] > bv || (s_val[w] == bv && s_idx[w] < bi)) {
                    bv = s_val[w];
                    bi = s_idx[w];
                }
            s_best = bi;
        }
        __syncthreads();
        const int best = s_best;
        if (best == 0x7fffffff) break;  // uniform: s_best is the same for every thread
        double bb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bb[i] = bx[(size_t)best * 4 + i];
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) out[kept * 5 + i] = bb[i];
            out[kept * 5 + 4] = sc[best];
        }
        for (int p = tid; p < P; p += S3_NMS_THREADS)
            if (!sp[p] && (p == best || s3_overlap(bb, bx + (size_t)p * 4) > S3_NMS_THRESH)) sp[p] = 1;
        ++kept;
        __syncthreads();
    }
    for (int i = kept * 5 + tid; i < max_faces * 5; i += S3_NMS_THREADS) out[i] = 0.0;
    // how many still stand (0 unless the cap cut it short): an integer sum, exact in any order
    int standing = 0;
    for (int p = tid; p < P; p += S3_NMS_THREADS) standing += sp[p] ? 0 : 1;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) standing += __shfl_xor(standing, w, 64);
    __syncthreads();
    if ((tid & 63) == 0) s_idx[tid >> 6] = standing;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < S3_NMS_THREADS / 64; ++w) t += s_idx[w];
        count[img] = kept;
        left[img] = t;
    }
}

// ---- crop boxes ------------------------------------------------------------------------------------------------------------------
// raw [F,4] (x1, y1, x2, y2) from each frame's top detection; a frame without one gets the whole frame and found = 0
__global__ __launch_bounds__(256) void s3fd_raw_boxes_kernel(int F, int H, int W, int max_faces, const double* __restrict__ dets,
                                                             const int* __restrict__ count, int4 pads, int* __restrict__ raw,
                                                             int* __restrict__ found) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int pd[4] = {pads.x, pads.y, pads.z, pads.w};
    int b[4] = {0, 0, W, H};
    const int have = count[f] > 0;
    if (have) s3_pad_box(dets + (size_t)f * max_faces * 5, H, W, pd, b);
    found[f] = have;
#pragma unroll
    for (int i = 0; i < 4; ++i) raw[f * 4 + i] = b[i];
}

// get_smoothened_boxes's parallel part: entries with i + T <= F read only entries that are not smoothed yet; the others are copied
__global__ __launch_bounds__(256) void s3fd_smooth_kernel(int F, int T, const int* __restrict__ raw, int* __restrict__ sm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    if (i + T > F) {
#pragma unroll
        for (int c = 0; c < 4; ++c) sm[i * 4 + c] = raw[i * 4 + c];
        return;
    }
    int a, b;
    s3_smooth_window(i, F, T, &a, &b);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        long long s = 0;
        for (int j = a; j < b; ++j) s += raw[j * 4 + c];
        sm[i * 4 + c] = s3_trunc_mean(s, b - a);
    }
}

// its sequential part -- the last T - 1 entries (all of them where F < T) read entries smoothed before them, in place, so one
// thread does them in order
__global__ __launch_bounds__(64) void s3fd_smooth_tail_kernel(int F, int T, int* __restrict__ sm) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && T > 0) {
        int i0 = F - T + 1;
        if (i0 < 0) i0 = 0;
        for (int i = i0; i < F; ++i) {
            int a, b;
            s3_smooth_window(i, F, T, &a, &b);
            for (int c = 0; c < 4; ++c) {
                long long s = 0;
                for (int j = a; j < b; ++j) s += sm[j * 4 + c];
                sm[i * 4 + c] = s3_trunc_mean(s, b - a);
            }
        }
    }
}

// (x1, y1, x2, y2) -> boxes (y1, y2, x1, x2)
__global__ __launch_bounds__(256) void s3fd_box_order_kernel(int F, const int* __restrict__ sm, int* __restrict__ boxes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    boxes[i * 4 + 0] = sm[i * 4 + 1];
    boxes[i * 4 + 1] = sm[i * 4 + 3];
    boxes[i * 4 + 2] = sm[i * 4 + 0];
    boxes[i * 4 + 3] = sm[i * 4 + 2];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
extern "C" size_t n3dt_s3fd_packed_layout_bytes(void) { return s3_layout().total; }
extern "C" size_t n3dt_s3fd_ws_bytes(int n, int H, int W) { return s3_workspace(n, H, W).total; }

extern "C" void n3dt_launch_s3fd_pack(const N3dtS3fdParams* p, void* packed, hipStream_t st) {
    const S3PackLayout L = s3_layout();
    char* base = (char*)packed;
    for (int j = 0; j < S3_GEMMS; ++j) {
        const S3Geom g = s3_gemm_geom(j, S3_MIN_HW, S3_MIN_HW);
        const float *w0, *w1 = nullptr, *b0, *b1 = nullptr;
        int c0, c1 = 0;
        if (j < S3_CONVS) {
            w0 = p->weight[j];
            b0 = p->bias[j];
            c0 = g.np;
        } else {
            const int l = j - S3_CONVS;
            w0 = p->weight[S3_CONVS + 2 * l];
            b0 = p->bias[S3_CONVS + 2 * l];
            w1 = p->weight[S3_CONVS + 2 * l + 1];
            b1 = p->bias[S3_CONVS + 2 * l + 1];
            c0 = s3_level_conf(l);
            c1 = 4;
        }
        __bf16* hi = (__bf16*)(base + L.w[j]);
        const size_t n = L.elems[j];
        s3fd_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(w0, c0, w1, c1, g.cin, g.cinp, g.np, g.k * g.k, g.K, hi, hi + n);
        s3fd_bias_kernel<<<(g.np + 255) / 256, 256, 0, st>>>(b0, c0, b1, c1, g.np, (float*)(base + L.bias[j]));
    }
    for (int l = 0; l < S3_NORMS; ++l)
        conv_net_copy(p->norm_weight[l], (size_t)s3_level_c(l), (float*)(base + L.norm[l]), st);
}

static void s3_conv(int j, int n, int Hi, int Wi, const void* packed, const float* in, float* out, hipStream_t st) {
    const S3PackLayout L = s3_layout();
    const S3Geom g = s3_gemm_geom(j, Hi, Wi);
    const char* pk = (const char*)packed;
    S3ConvArgs a;
    a.in = in;
    a.whi = (const __bf16*)(pk + L.w[j]);
    a.wlo = a.whi + L.elems[j];
    a.bias = (const float*)(pk + L.bias[j]);
    a.out = out;
    a.n = n;
    a.Ho = g.Ho; a.Wo = g.Wo; a.Hp = g.Hp; a.Wp = g.Wp; a.Hq = g.Hq; a.Wq = g.Wq;
    a.cinp = g.cinp; a.np = g.np; a.cstore = g.cstore; a.k = g.k; a.stride = g.stride;
    a.ioff = g.ioff; a.opad = g.opad; a.relu = g.relu;
    const size_t Mq = (size_t)n * g.Hq * g.Wq;
    const size_t mtiles = (Mq + CN_TILE_M - 1) / CN_TILE_M;
    const int nt = cn_wave_ntiles((long long)Mq, g.np);
    const size_t tiles = mtiles * (g.np / (32 * nt));
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    if (nt == 1) s3fd_conv_kernel<1><<<grid, 256, 0, st>>>(a);
    else s3fd_conv_kernel<2><<<grid, 256, 0, st>>>(a);
}

static void s3_pool(int n, int Hi, int Wi, int ihalo, int C, int opad, const float* in, float* out, hipStream_t st) {
    const size_t work = (size_t)n * (Hi / 2 + 2 * opad) * (Wi / 2 + 2 * opad) * (C / 4);
    s3fd_pool_kernel<<<conv_grid(work), 256, 0, st>>>(in, n, Hi, Wi, ihalo, C, opad, out);
}

static void s3_norm(int l, int n, int H, int W, const void* packed, const float* in, float* out, hipStream_t st) {
    const S3PackLayout L = s3_layout();
    s3fd_norm_kernel<<<conv_grid((size_t)n * (H + 2) * (W + 2)), 256, 0, st>>>(in, (const float*)((const char*)packed + L.norm[l]), n, H, W,
                                                                             s3_level_c(l), out);
}

// the halo of the map a pool writes: the padding of the convolution behind it
static int s3_pool_opad(int c) { return S3_TABLE[c + 1].pad; }

// the chain from the padded NHWC input in map[0] to the six head maps
static void s3_chain(int n, int H, int W, const void* packed, char* ws, const S3Workspace& w, hipStream_t st) {
    const S3Sizes s = s3_sizes(H, W);
    float* in = (float*)(ws + w.map[0]);
    float* out = (float*)(ws + w.map[1]);
    float* nrm = (float*)(ws + w.norm);
    for (int c = 0; c < S3_CONVS; ++c) {
        const S3Conv t = S3_TABLE[c];
        s3_conv(c, n, s.h[c], s.w[c], packed, in, out, st);
        float* tmp = in;
        in = out;
        out = tmp;
        if (t.level) {
            const int l = t.level - 1;
            const float* src = in;
            if (l < S3_NORMS) {
                s3_norm(l, n, s.lh[l], s.lw[l], packed, in, nrm, st);
                src = nrm;
            }
            s3_conv(S3_CONVS + l, n, s.lh[l], s.lw[l], packed, src, (float*)(ws + w.head[l]), st);
        }
        if (t.pool) {
            const S3Geom g = s3_gemm_geom(c, s.h[c], s.w[c]);
            s3_pool(n, g.Ho, g.Wo, g.opad, t.cout, s3_pool_opad(c), in, out, st);
            tmp = in;
            in = out;
            out = tmp;
        }
    }
}

static S3Levels s3_levels(int H, int W, char* ws, const S3Workspace& w) {
    const S3Sizes s = s3_sizes(H, W);
    S3Levels L;
    s3_positions(&s, L.first);
    for (int l = 0; l < S3_LEVELS; ++l) {
        L.head[l] = (const float*)(ws + w.head[l]);
        L.lh[l] = s.lh[l];
        L.lw[l] = s.lw[l];
    }
    return L;
}

extern "C" void n3dt_launch_s3fd_heads(int n, int H, int W, const void* packed, const float* x, float* const* out, void* workspace,
                                       hipStream_t st) {
    const S3Workspace w = s3_workspace(n, H, W);
    char* ws = (char*)workspace;
    conv_net_to_nhwc(x, n, 3, H, W, 1, 16, (float*)(ws + w.map[0]), 16, st);
    s3_chain(n, H, W, packed, ws, w, st);
    const S3Levels L = s3_levels(H, W, ws, w);
    for (int l = 0; l < S3_LEVELS; ++l) {
        const int cols = s3_level_cols(l), conf = s3_level_conf(l);
        const size_t px = (size_t)n * L.lh[l] * L.lw[l];
        if (l == 0) s3fd_maxout_nchw_kernel<<<conv_grid(px * 2), 256, 0, st>>>(L.head[l], n, cols, L.lh[l], L.lw[l], out[2 * l]);
        else conv_net_to_nchw(L.head[l], cols, n, 2, L.lh[l], L.lw[l], 0, out[2 * l], st);
        conv_net_to_nchw(L.head[l] + conf, cols, n, 4, L.lh[l], L.lw[l], 0, out[2 * l + 1], st);
    }
}

extern "C" void n3dt_launch_s3fd_detect(int n, int H, int W, const void* packed, const float* frames, int max_faces, double* scores,
                                        double* dets, int* count, int* left, void* workspace, hipStream_t st) {
    const S3Workspace w = s3_workspace(n, H, W);
    char* ws = (char*)workspace;
    s3fd_frames_kernel<<<conv_grid((size_t)n * (H + 2) * (W + 2)), 256, 0, st>>>(frames, n, H, W, 1, (float*)(ws + w.map[0]));
    s3_chain(n, H, W, packed, ws, w, st);
    const S3Levels L = s3_levels(H, W, ws, w);
    const int P = L.first[S3_LEVELS];
    double* score = scores ? scores : (double*)(ws + w.score);  // [n, P], the caller's where it wants them
    double* box = (double*)(ws + w.box);
    s3fd_score_kernel<<<conv_grid((size_t)n * P), 256, 0, st>>>(L, n, score, box);
    s3fd_nms_kernel<<<n, S3_NMS_THREADS, 0, st>>>(P, max_faces, score, box, (unsigned char*)(ws + w.sup), dets, count, left);
}

extern "C" void n3dt_launch_s3fd_boxes(int F, int H, int W, int max_faces, const double* dets, const int* count, const int* pads, int T,
                                       int* boxes, int* found, int* scratch, hipStream_t st) {
    const unsigned grid = (unsigned)((F + 255) / 256);
    int* raw = scratch;
    int* sm = scratch + (size_t)F * 4;
    s3fd_raw_boxes_kernel<<<grid, 256, 0, st>>>(F, H, W, max_faces, dets, count, make_int4(pads[0], pads[1], pads[2], pads[3]), raw, found);
    if (T > 0) {
        s3fd_smooth_kernel<<<grid, 256, 0, st>>>(F, T, raw, sm);
        s3fd_smooth_tail_kernel<<<1, 64, 0, st>>>(F, T, sm);
    } else {
        sm = raw;
    }
    s3fd_box_order_kernel<<<grid, 256, 0, st>>>(F, sm, boxes);
}

// ---- one block alone ---------------------------------------------------------------------------------------------------------------
// in [n, C_in, Hi, Wi] -> out [n, C_out, Ho, Wo] through two maps laid out as the chain holds them; a head pair gives its stored
// columns (conf, then loc) without the max-out
struct S3BlockShape {
    int cin, cout, Ho, Wo, opad;
    size_t in_elems, out_elems;  // of the padded NHWC maps, per image
};

static S3BlockShape s3_block_shape(int block, int Hi, int Wi) {
    S3BlockShape b;
    if (block < S3_FIRST_POOL || block >= S3_FIRST_HEAD) {
        const S3Geom g = s3_gemm_geom(block < S3_FIRST_POOL ? block : S3_CONVS + block - S3_FIRST_HEAD, Hi, Wi);
        b.cin = g.cin; b.cout = g.cstore; b.Ho = g.Ho; b.Wo = g.Wo; b.opad = g.opad;
        b.in_elems = s3_in_elems(&g, 1);
        b.out_elems = s3_out_elems(&g, 1);
    } else if (block < S3_FIRST_NORM) {
        int c = 0;
        for (int k = block - S3_FIRST_POOL; ; ++c)
            if (S3_TABLE[c].pool && k-- == 0) break;
        const int op = b.opad = s3_pool_opad(c);
        b.cin = b.cout = S3_TABLE[c].cout; b.Ho = Hi / 2; b.Wo = Wi / 2;
        b.in_elems = (size_t)Hi * Wi * b.cin;
        b.out_elems = (size_t)(b.Ho + 2 * op) * (b.Wo + 2 * op) * b.cout;
    } else {
        const int l = block - S3_FIRST_NORM;
        b.cin = b.cout = s3_level_c(l); b.Ho = Hi; b.Wo = Wi; b.opad = 1;
        b.in_elems = (size_t)Hi * Wi * b.cin;
        b.out_elems = s3_norm_elems(Hi, Wi, b.cin);
    }
    return b;
}

extern "C" size_t n3dt_s3fd_block_ws_bytes(int block, int n, int Hi, int Wi) {
    const S3BlockShape b = s3_block_shape(block, Hi, Wi);
    return cn_rup256((size_t)n * b.in_elems * sizeof(float)) + cn_rup256((size_t)n * b.out_elems * sizeof(float));
}

extern "C" void n3dt_launch_s3fd_block(int block, int n, int Hi, int Wi, const void* packed, const float* in, float* out, void* workspace,
                                       hipStream_t st) {
    const S3BlockShape b = s3_block_shape(block, Hi, Wi);
    float* map0 = (float*)workspace;
    float* map1 = (float*)((char*)workspace + cn_rup256((size_t)n * b.in_elems * sizeof(float)));
    if (block < S3_FIRST_POOL || block >= S3_FIRST_HEAD) {
        const int j = block < S3_FIRST_POOL ? block : S3_CONVS + block - S3_FIRST_HEAD;
        const S3Geom g = s3_gemm_geom(j, Hi, Wi);
        conv_net_to_nhwc(in, n, g.cin, Hi, Wi, g.ihalo, g.cinp, map0, g.cinp, st);
        s3_conv(j, n, Hi, Wi, packed, map0, map1, st);
        conv_net_to_nchw(map1, g.cstore, n, g.cstore, g.Ho, g.Wo, g.opad, out, st);
    } else if (block < S3_FIRST_NORM) {
        const int op = b.opad;
        conv_net_to_nhwc(in, n, b.cin, Hi, Wi, 0, b.cin, map0, b.cin, st);
        s3_pool(n, Hi, Wi, 0, b.cin, op, map0, map1, st);
        conv_net_to_nchw(map1, b.cout, n, b.cout, b.Ho, b.Wo, op, out, st);
    } else {
        conv_net_to_nhwc(in, n, b.cin, Hi, Wi, 0, b.cin, map0, b.cin, st);
        s3_norm(block - S3_FIRST_NORM, n, Hi, Wi, packed, map0, map1, st);
        conv_net_to_nchw(map1, b.cout, n, b.cout, Hi, Wi, 1, out, st);
    }
}
