// Audio2style encoder (talker_trainer.py:407-461), forward and backward, fp32 (include/n3dt.h, n3dt_a2s_*).
//
// The frames of a batch are ONE sequence: mel [T, 1280] -> 2-layer bidirectional LSTM (hidden 640) -> [T, 1280] -> three
// Linear + LeakyReLU(0.2) + Dropout(0.5) layers -> [T, 64].
//
// Forward, per LSTM layer:
//   * input projection xp[dir] = X W_ih[dir]^T + b_ih[dir]: one fp32 MFMA GEMM per direction (gemm32.h), every weight byte
//     read once;
//   * T recurrent steps, one launch each, both directions in the same launch (forward at t = s, reverse at t = T-1-s).  A
//     workgroup owns A2S_UF hidden units (all four gates of them), so it reads the same 32 rows of W_hh at every step: they
//     stay in its L2.  The step adds W_hh h_prev + b_hh to xp, applies the cell update and keeps the activated gates, c and
//     h for the backward.
// Head: GEMM with bias + LeakyReLU epilogue, then the dropout scale (2 * keep mask, or 1 without masks).
//
// Backward: the head in reverse (dropout / LeakyReLU gate, dW = dZ^T Y, db = column sums, dY = dZ W), then BPTT per layer in
// reverse, one launch per step: dh_t = dH_out[t] + W_hh^T dgates_next, then the cell backward.  The weight gradients are
// GEMMs with K = T (dW_ih = dgates^T X, dW_hh = dgates^T h_prev), the bias gradients column sums in a fixed order.  Every
// gradient is written (not accumulated) into its slice of the caller's arena.  No atomics, no split-K: bitwise reproducible.
#include <hip/hip_runtime.h>

#include "../../include/n3dt.h"
#include "gemm32.h"
#include "n3dt_device.h"
#include "n3dt_launch.h"

#define A2S_IN 1280
#define A2S_H 640
#define A2S_G 2560
#define A2S_UF 8                  // hidden units per workgroup in a recurrent step (forward and backward)
#define A2S_NB (A2S_H / A2S_UF)   // workgroups per direction

// grad arena layout (include/n3dt.h)
#define A2S_K_STRIDE 4920320L     // 2560*1280 + 2560*640 + 2560 + 2560
#define A2S_OFF_WHH 3276800L
#define A2S_OFF_BIH 4915200L
#define A2S_OFF_BHH 4917760L
#define A2S_HEAD 19681280L
static const long a2s_lin_w_off[3] = {0L, 819840L, 1024960L};
static const long a2s_lin_b_off[3] = {819200L, 1024640L, 1045440L};
static const int a2s_lin_in[3] = {1280, 640, 320};
static const int a2s_lin_out[3] = {640, 320, 64};

// per-T layouts, in floats (every piece a multiple of 64 T floats: 256-byte aligned for any T)
struct A2sSaved {
    float *X0, *H[2], *G[2], *C[2], *A[3], *S[3], *Y[2];
};
static A2sSaved a2s_saved(float* b, int T) {
    A2sSaved s;
    const long t = T;
    s.X0 = b;           b += A2S_IN * t;
    s.H[0] = b;         b += 2 * A2S_H * t;
    s.H[1] = b;         b += 2 * A2S_H * t;
    s.G[0] = b;         b += 2 * A2S_G * t;
    s.G[1] = b;         b += 2 * A2S_G * t;
    s.C[0] = b;         b += 2 * A2S_H * t;
    s.C[1] = b;         b += 2 * A2S_H * t;
    for (int k = 0; k < 3; ++k) { s.A[k] = b; b += a2s_lin_out[k] * t; }
    for (int k = 0; k < 3; ++k) { s.S[k] = b; b += a2s_lin_out[k] * t; }
    for (int k = 0; k < 2; ++k) { s.Y[k] = b; b += a2s_lin_out[k] * t; }
    return s;
}
// Workspace: XP[l] [2][T][2560] (layer l's input projections, forward) and DC[l] [2][T][640] (its cell-state gradients) per
// LSTM layer, then DH1, DH0 [T][1280], DZ3 [T][64], DY2 [T][320], DY1 [T][640]: 16384 T floats.  The backward writes layer l's
// pre-activation gradients DG[l] over XP[l] (the forward is done with it), so after a forward + backward every intermediate of
// both layers is still there: XP[l] after n3dt_a2s_fwd, DG[l] and DC[l] after n3dt_a2s_bwd.
struct A2sWs {
    float *XP[2], *DC[2], *DH1, *DH0, *DZ3, *DY2, *DY1;
};
static A2sWs a2s_ws(float* b, int T) {
    A2sWs w;
    const long t = T;
    for (int l = 0; l < 2; ++l) { w.XP[l] = b; b += 2 * A2S_G * t; }
    for (int l = 0; l < 2; ++l) { w.DC[l] = b; b += 2 * A2S_H * t; }
    w.DH1 = b; b += 2 * A2S_H * t;
    w.DH0 = b; b += 2 * A2S_H * t;
    w.DZ3 = b; b += 64 * t;
    w.DY2 = b; b += 320 * t;
    w.DY1 = b; b += 640 * t;
    return w;
}

extern "C" size_t n3dt_a2s_saved_floats(int T) { return (size_t)T * (A2S_IN + 4 * A2S_H + 4 * A2S_G + 4 * A2S_H + 2 * 1024 + 960); }
extern "C" size_t n3dt_a2s_ws_floats(int T) { return (size_t)T * (4 * A2S_G + 8 * A2S_H + 1024); }

__device__ __forceinline__ float a2s_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float a2s_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One forward step of both directions.  Block -> (direction, A2S_UF units); wave q -> gate q of those units; each row's dot
// product with h_prev is spread over the 64 lanes (10 elements each, float2 loads) and reduced by a butterfly.
__global__ __launch_bounds__(256) void a2s_step_fwd(int T, int s, const float* __restrict__ xp, const float* __restrict__ whh0,
                                                    const float* __restrict__ whh1, const float* __restrict__ bhh0,
                                                    const float* __restrict__ bhh1, float* __restrict__ Hout, float* __restrict__ G,
                                                    float* __restrict__ C) {
    __shared__ float pre[4][A2S_UF];
    const int dir = blockIdx.x / A2S_NB, u0 = (blockIdx.x % A2S_NB) * A2S_UF;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int t = dir ? T - 1 - s : s;
    const int tp = dir ? t + 1 : t - 1;  // the step before this one in this direction's order
    const bool has_prev = s > 0;
    const float* __restrict__ whh = dir ? whh1 : whh0;
    const float* __restrict__ bhh = dir ? bhh1 : bhh0;
    float hv[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) hv[i] = 0.0f;
    if (has_prev) {
        const float* hp = Hout + (long)tp * (2 * A2S_H) + dir * A2S_H;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float2 v = *reinterpret_cast<const float2*>(hp + 2 * lane + 128 * i);
            hv[2 * i] = v.x;
            hv[2 * i + 1] = v.y;
        }
    }
#pragma unroll
    for (int j = 0; j < A2S_UF; ++j) {
        const int row = q * A2S_H + u0 + j;
        float acc = 0.0f;
        if (has_prev) {
            const float* w = whh + (long)row * A2S_H;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const float2 v = *reinterpret_cast<const float2*>(w + 2 * lane + 128 * i);
                acc = fmaf(v.x, hv[2 * i], acc);
                acc = fmaf(v.y, hv[2 * i + 1], acc);
            }
            acc = a2s_wave_sum(acc);
        }
        // (x W_ih^T + b_ih) + (h W_hh^T + b_hh), the reference's grouping
        if (lane == 0) pre[q][j] = xp[((long)dir * T + t) * A2S_G + row] + (acc + bhh[row]);
    }
    __syncthreads();
    if (threadIdx.x < A2S_UF) {
        const int j = threadIdx.x, u = u0 + j;
        const float ig = a2s_sigmoid(pre[0][j]), fg = a2s_sigmoid(pre[1][j]), gg = tanhf(pre[2][j]), og = a2s_sigmoid(pre[3][j]);
        const float cp = has_prev ? C[((long)dir * T + tp) * A2S_H + u] : 0.0f;
        const float c = fg * cp + ig * gg;
        const float h = og * tanhf(c);
        float* g = G + ((long)dir * T + t) * A2S_G;
        g[u] = ig;
        g[A2S_H + u] = fg;
        g[2 * A2S_H + u] = gg;
        g[3 * A2S_H + u] = og;
        C[((long)dir * T + t) * A2S_H + u] = c;
        Hout[(long)t * (2 * A2S_H) + dir * A2S_H + u] = h;
    }
}

// One BPTT step of both directions: direction 0 walks t = T-1 .. 0, direction 1 t = 0 .. T-1.  Block -> (direction,
// A2S_UF units); thread -> rows r = tid + 256 i of W_hh, the block's A2S_UF columns of each (two float4), against the
// previous backward step's pre-activation gradients; a fixed-order wave + block reduction gives W_hh^T dgates_next.
__global__ __launch_bounds__(256) void a2s_step_bwd(int T, int s, const float* __restrict__ whh0, const float* __restrict__ whh1,
                                                    const float* __restrict__ G, const float* __restrict__ C,
                                                    const float* __restrict__ dHout, float* __restrict__ DG, float* __restrict__ DC) {
    __shared__ float part[4][A2S_UF];
    const int dir = blockIdx.x / A2S_NB, u0 = (blockIdx.x % A2S_NB) * A2S_UF;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = dir ? s : T - 1 - s;
    const int tn = dir ? t - 1 : t + 1;  // the step whose gradients were formed just before (later in the forward order)
    const bool has_next = s > 0;
    const float* __restrict__ whh = dir ? whh1 : whh0;
    float acc[A2S_UF];
#pragma unroll
    for (int j = 0; j < A2S_UF; ++j) acc[j] = 0.0f;
    if (has_next) {
        const float* dgn = DG + ((long)dir * T + tn) * A2S_G;
        for (int r = threadIdx.x; r < A2S_G; r += 256) {
            const float d = dgn[r];
            const float* w = whh + (long)r * A2S_H + u0;
            const f32x4 a = *reinterpret_cast<const f32x4*>(w), b = *reinterpret_cast<const f32x4*>(w + 4);
            acc[0] = fmaf(a.x, d, acc[0]);
            acc[1] = fmaf(a.y, d, acc[1]);
            acc[2] = fmaf(a.z, d, acc[2]);
            acc[3] = fmaf(a.w, d, acc[3]);
            acc[4] = fmaf(b.x, d, acc[4]);
            acc[5] = fmaf(b.y, d, acc[5]);
            acc[6] = fmaf(b.z, d, acc[6]);
            acc[7] = fmaf(b.w, d, acc[7]);
        }
#pragma unroll
        for (int j = 0; j < A2S_UF; ++j) acc[j] = a2s_wave_sum(acc[j]);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < A2S_UF; ++j) part[wave][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < A2S_UF) {
        const int j = threadIdx.x, u = u0 + j;
        const float dh_rec = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
        const float* g = G + ((long)dir * T + t) * A2S_G;
        const float ig = g[u], fg = g[A2S_H + u], gg = g[2 * A2S_H + u], og = g[3 * A2S_H + u];
        const float c = C[((long)dir * T + t) * A2S_H + u];
        const float tc = tanhf(c);
        const float dh = dHout[(long)t * (2 * A2S_H) + dir * A2S_H + u] + dh_rec;
        float dc = (dh * og) * (1.0f - tc * tc);
        if (has_next)
            dc = dc + DC[((long)dir * T + tn) * A2S_H + u] * G[((long)dir * T + tn) * A2S_G + A2S_H + u];
        const bool has_prev = dir ? t < T - 1 : t > 0;
        const int tp = dir ? t + 1 : t - 1;
        const float cp = has_prev ? C[((long)dir * T + tp) * A2S_H + u] : 0.0f;
        float* dg = DG + ((long)dir * T + t) * A2S_G;
        dg[u] = (dc * gg) * (ig * (1.0f - ig));
        dg[A2S_H + u] = (dc * cp) * (fg * (1.0f - fg));
        dg[2 * A2S_H + u] = (dc * ig) * (1.0f - gg * gg);
        dg[3 * A2S_H + u] = (dh * tc) * (og * (1.0f - og));
        DC[((long)dir * T + t) * A2S_H + u] = dc;
    }
}

// dropout after LeakyReLU: S = 2 * keep mask (no mask: 1), Y = A * S
__global__ __launch_bounds__(256) void a2s_dropout_fwd(int n, const float* __restrict__ A, const float* __restrict__ mask,
                                                       float* __restrict__ S, float* __restrict__ Y) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float sc = mask ? mask[i] * 2.0f : 1.0f;
    S[i] = sc;
    Y[i] = A[i] * sc;
}

// dZ = (dY * S) * lrelu'(A), the order of the reference's autograd (Dropout, then LeakyReLU); dY and dZ may alias
__global__ __launch_bounds__(256) void a2s_dropout_bwd(int n, const float* dY, const float* __restrict__ A, const float* __restrict__ S,
                                                       float* dZ) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = dY[i] * S[i];
    dZ[i] = A[i] > 0.0f ? v : v * 0.2f;
}

// bias gradient: column sums over the T rows, in row order; written to dst0 and (if given) dst1
__global__ __launch_bounds__(256) void a2s_colsum(int T, int n, const float* __restrict__ src, int ld, float* __restrict__ dst0,
                                                  float* __restrict__ dst1) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    float acc = 0.0f;
    for (int t = 0; t < T; ++t) acc += src[(long)t * ld + c];
    dst0[c] = acc;
    if (dst1) dst1[c] = acc;
}

// C[M,N] = A B (gemm32.h operand conventions), nothing else
static Gemm32 a2s_mm(int M, int N, int K, const float* A, long lda, int ak, const float* B, long ldb, int bk, float* C, long ldc) {
    Gemm32 g = {};
    g.M = M; g.N = N; g.K = K;
    g.A = A; g.lda = lda; g.a_kmajor = ak;
    g.B = B; g.ldb = ldb; g.b_kmajor = bk;
    g.C = C; g.ldc = ldc;
    g.act = G32_ACT_NONE;
    g.gate_act = G32_ACT_NONE;
    g.split_k = 1;
    return g;
}

static inline unsigned a2s_blocks(long n) { return (unsigned)((n + 255) / 256); }

extern "C" void n3dt_launch_a2s_fwd(int T, const N3dtA2sParams* p, const float* mel, const float* const masks[3], float* out,
                                    void* saved, void* ws, hipStream_t st) {
    const A2sSaved sv = a2s_saved(static_cast<float*>(saved), T);
    const A2sWs w = a2s_ws(static_cast<float*>(ws), T);
    (void)hipMemcpyAsync(sv.X0, mel, sizeof(float) * A2S_IN * (size_t)T, hipMemcpyDeviceToDevice, st);
    for (int l = 0; l < 2; ++l) {
        const float* X = l ? sv.H[0] : sv.X0;
        for (int d = 0; d < 2; ++d) {
            Gemm32 g = a2s_mm(T, A2S_G, A2S_IN, X, A2S_IN, 0, p->w_ih[2 * l + d], A2S_IN, 0, w.XP[l] + (long)d * T * A2S_G, A2S_G);
            g.bias = p->b_ih[2 * l + d];
            n3dt_gemm32(g, st);
        }
        for (int s = 0; s < T; ++s)
            hipLaunchKernelGGL(a2s_step_fwd, dim3(2 * A2S_NB), dim3(256), 0, st, T, s, w.XP[l], p->w_hh[2 * l], p->w_hh[2 * l + 1],
                               p->b_hh[2 * l], p->b_hh[2 * l + 1], sv.H[l], sv.G[l], sv.C[l]);
    }
    const float* X = sv.H[1];
    for (int k = 0; k < 3; ++k) {
        const int ni = a2s_lin_in[k], no = a2s_lin_out[k];
        Gemm32 g = a2s_mm(T, no, ni, X, ni, 0, p->lin_w[k], ni, 0, sv.A[k], no);
        g.bias = p->lin_b[k];
        g.act = G32_ACT_LRELU;
        n3dt_gemm32(g, st);
        float* Y = k < 2 ? sv.Y[k] : out;
        hipLaunchKernelGGL(a2s_dropout_fwd, dim3(a2s_blocks((long)T * no)), dim3(256), 0, st, T * no, sv.A[k], masks[k], sv.S[k], Y);
        X = Y;
    }
}

extern "C" void n3dt_launch_a2s_bwd(int T, const N3dtA2sParams* p, const float* g_out, const void* saved, float* arena, void* ws,
                                    hipStream_t st) {
    const A2sSaved sv = a2s_saved(const_cast<float*>(static_cast<const float*>(saved)), T);
    const A2sWs w = a2s_ws(static_cast<float*>(ws), T);
    float* head = arena + A2S_HEAD;
    // head, last layer first: dZ_k = dropout / LeakyReLU gate of dY_k; dW_k = dZ_k^T X_k; db_k = sum_t dZ_k; dY_{k-1} = dZ_k W_k
    float* dz[3] = {w.DY1, w.DY2, w.DZ3};
    const float* xin[3] = {sv.H[1], sv.Y[0], sv.Y[1]};
    float* dx_out[3] = {w.DH1, w.DY1, w.DY2};
    const float* dy = g_out;
    for (int k = 2; k >= 0; --k) {
        const int ni = a2s_lin_in[k], no = a2s_lin_out[k];
        hipLaunchKernelGGL(a2s_dropout_bwd, dim3(a2s_blocks((long)T * no)), dim3(256), 0, st, T * no, dy, sv.A[k], sv.S[k], dz[k]);
        n3dt_gemm32(a2s_mm(no, ni, T, dz[k], no, 1, xin[k], ni, 1, head + a2s_lin_w_off[k], ni), st);
        hipLaunchKernelGGL(a2s_colsum, dim3(a2s_blocks(no)), dim3(256), 0, st, T, no, dz[k], no, head + a2s_lin_b_off[k], (float*)nullptr);
        n3dt_gemm32(a2s_mm(T, ni, no, dz[k], no, 0, p->lin_w[k], ni, 1, dx_out[k], ni), st);
        dy = dx_out[k];
    }
    for (int l = 1; l >= 0; --l) {
        float* DG = w.XP[l];
        const float* dHout = l ? w.DH1 : w.DH0;
        for (int s = 0; s < T; ++s)
            hipLaunchKernelGGL(a2s_step_bwd, dim3(2 * A2S_NB), dim3(256), 0, st, T, s, p->w_hh[2 * l], p->w_hh[2 * l + 1], sv.G[l], sv.C[l],
                               dHout, DG, w.DC[l]);
        const float* X = l ? sv.H[0] : sv.X0;
        for (int d = 0; d < 2; ++d) {
            const int k = 2 * l + d;
            float* gk = arena + k * A2S_K_STRIDE;
            const float* dgd = DG + (long)d * T * A2S_G;
            // dW_ih = dgates^T X
            n3dt_gemm32(a2s_mm(A2S_G, A2S_IN, T, dgd, A2S_G, 1, X, A2S_IN, 1, gk, A2S_IN), st);
            // dW_hh = sum_t dgates_t h_prev(t)^T: direction 0 pairs t = 1..T-1 with h[t-1], direction 1 t = 0..T-2 with h[t+1]
            if (T > 1) {
                const float* a = d ? dgd : dgd + A2S_G;
                const float* hb = d ? sv.H[l] + 2 * A2S_H + A2S_H : sv.H[l];
                n3dt_gemm32(a2s_mm(A2S_G, A2S_H, T - 1, a, A2S_G, 1, hb, 2 * A2S_H, 1, gk + A2S_OFF_WHH, A2S_H), st);
            } else {
                (void)hipMemsetAsync(gk + A2S_OFF_WHH, 0, sizeof(float) * A2S_G * A2S_H, st);
            }
            hipLaunchKernelGGL(a2s_colsum, dim3(a2s_blocks(A2S_G)), dim3(256), 0, st, T, A2S_G, dgd, A2S_G, gk + A2S_OFF_BIH, gk + A2S_OFF_BHH);
        }
        if (l == 1) {
            // the gradient reaching layer 0's output: dgates[0] W_ih[2] + dgates[1] W_ih[3] (the mel input takes none)
            for (int d = 0; d < 2; ++d) {
                Gemm32 g = a2s_mm(T, A2S_IN, A2S_G, DG + (long)d * T * A2S_G, A2S_G, 0, p->w_ih[2 + d], A2S_IN, 1, w.DH0, 2 * A2S_H);
                g.accumulate = d;
                n3dt_gemm32(g, st);
            }
        }
    }
}
