// One neural-renderer block as ONE kernel (16-bit path; included by neural_render_x16.inc).
//
// Per input pixel the block is a chain of three 1x1 convolutions (reference: NetWorks/PixelShuffleUpsample.py:36-45,
// NetWorks/neural_renderer.py:79-81):
//     t1   = lrelu(W1 x + b1)                                   [2C]
//     y_q  = lrelu(W2[4c+q, :] t1 + b2[4c+q]) + x[(4c+q) % C]   [C]   q = 2di+dj: the four sub-pixels of pixel_shuffle(2)
//     hid_q = Wf y_q                                            [CO]  feat_layers BEFORE the blur (commuted, see above)
// and no pixel talks to another until the blur.  The layered version moved t1 and y through HBM (32 C bytes per input
// pixel, against 6 C for x in and hid out) and its three GEMMs ran at 12 % of the matrix peak.  Here one wavefront carries
// 32 pixels through the whole chain the way the fused NeRF kernel carries samples (nerf_fwd_x16.hip): activations stay
// in registers as transposed accumulator tiles that are re-packed into the next product's B operand, and the weights of
// the whole block arrive as one stream of 1 KiB MFMA A fragments, staged L2 -> LDS by LDS-DMA (x16_core.h WeightStream).
//
// The residual never touches the accumulators (its channel (4c+q) % C sits on another lane half): it is pushed through
// feat_layers instead, hid_q = Wf lrelu(.) + R_q x with R_q[o][k] = sum of Wf[o][c] over the four c with (4c+q) % C == k
// (zero unless k % 4 == q).  Only a quarter of x's channels carry weight for a given q, so the wave regroups its x
// fragments per sub-pixel (same lane, 16-bit elements q and q+4 of four consecutive fragments: four v_perm per fragment)
// and the residual costs C/64 extra k-steps of the last product instead of C/16.
//
// hid is written as four sub-pixel planes [q][M][CO] (one wavefront's rows of a plane are contiguous, so its 8-byte stores
// complete whole cache lines); blur_act_rgb_q_kernel reads that layout.
#include "x16_core.h"

#ifndef NRF_NBUF
#define NRF_NBUF 3  // ring depth (4 measured no faster)
#endif

struct NrfDims {
    int s1, s2, s3, body, total, padded, kxq, regroup;
};
__host__ __device__ constexpr NrfDims nrf_dims(const int C, const int CO) {
    NrfDims d = {0, 0, 0, 0, 0, 0, 0, 0};
    // the residual operand is regrouped per sub-pixel where that pays (C >= 128: 183 / 174 us against 200 / 179); at C = 64
    // the sub-pixel body would no longer be whole chunks, the four unrolled copies push the kernel past 128 registers and it
    // loses its second workgroup per CU (189 us against 160), so the small blocks keep x in natural order
    d.regroup = C >= 128 ? 1 : 0;
    d.kxq = d.regroup ? C / 64 : C / 16;  // k-steps of the residual operand
    d.s1 = (2 * C / 32) * (C / 16);
    d.s2 = (C / 32) * (C / 8);
    d.s3 = (CO / 32) * (C / 16 + d.kxq);
    d.body = d.s2 + d.s3;
    d.total = d.s1 + 4 * d.body;
    d.padded = ((d.total + X16_CH - 1) / X16_CH) * X16_CH;
    return d;
}
// bias table behind the pieces: b1 [2C] | b2 of sub-pixel q, [C] each
static inline size_t nrf_packed_bytes(const int C, const int CO) {
    return (size_t)nrf_dims(C, CO).padded * X16_PIECE + (size_t)6 * C * sizeof(float);
}
static inline bool nrf_supported(const int C, const int CO) {
    return (C == 256 && CO == 128) || (C == 128 && CO == 64) || (C == 64 && CO == 32) || (C == 32 && CO == 32);
}

// The piece stream of one block, in execution order, and its bias table.  One thread = one lane's 16 bytes of a piece.
__device__ __forceinline__ void nrf_pack_body(const int C, const int CO, const int precision, const float* __restrict__ W1,
                                              const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
                                              const float* __restrict__ Wf, unsigned char* __restrict__ out, const int i) {
    const NrfDims d = nrf_dims(C, CO);
    float* bias = reinterpret_cast<float*>(out + (size_t)d.padded * X16_PIECE);
    if (i < 6 * C) {
        if (i < 2 * C) bias[i] = b1[i];
        else {
            const int q = (i - 2 * C) / C, c = (i - 2 * C) % C;
            bias[i] = b2[4 * c + q];
        }
    }
    if (i >= d.padded * 64) return;
    const int P = i >> 6, lane = i & 63, r = lane & 31, hh = lane >> 5;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int nat = 8 * hh + j;                          // k slot inside a 16-wide step, natural order (x fragments)
        const int perm = 8 * (j >> 2) + 4 * hh + (j & 3);    // ... and the order a packed accumulator tile has (x16_core.h)
        float w = 0.0f;
        if (P < d.s1) {
            const int ot = P / (C / 16), ks = P % (C / 16);
            w = W1[(size_t)(32 * ot + r) * C + 16 * ks + nat];
        } else if (P < d.total) {
            const int q = (P - d.s1) / d.body;
            int pp = (P - d.s1) % d.body;
            if (pp < d.s2) {
                const int ot = pp / (C / 8), ks = pp % (C / 8);
                w = W2[(size_t)(4 * (32 * ot + r) + q) * (2 * C) + 16 * ks + perm];
            } else {
                pp -= d.s2;
                const int ks3 = C / 16 + d.kxq;
                const int ot = pp / ks3, ks = pp % ks3;
                const float* wr = Wf + (size_t)(32 * ot + r) * C;
                if (ks < C / 16) {
                    w = wr[16 * ks + perm];
                } else {
                    // regrouped x operand: slot j of step ks' is element q + 4 (j & 1) of natural fragment 4 ks' + (j >> 1);
                    // natural order otherwise (three slots in four then carry a zero weight)
                    const int k = d.regroup ? 16 * (4 * (ks - C / 16) + (j >> 1)) + 8 * hh + q + 4 * (j & 1) : 16 * (ks - C / 16) + nat;
                    if ((k & 3) == q) {
                        const int c0 = (k - q) >> 2;
                        w = (wr[c0] + wr[c0 + C / 4]) + (wr[c0 + C / 2] + wr[c0 + 3 * (C / 4)]);
                    }
                }
            }
        }
        v[j] = w;
    }
    const u16x8 o = precision == N3DT_BF16 ? x16_pack8<N3DT_BF16, u16x8>(v) : x16_pack8<N3DT_F16, u16x8>(v);  // two values per conversion
    *reinterpret_cast<u16x8*>(out + (size_t)P * X16_PIECE + lane * 16) = o;
}
__global__ void nrf_pack_kernel(const int C, const int CO, const int precision, const float* __restrict__ W1, const float* __restrict__ b1,
                                const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ Wf,
                                unsigned char* __restrict__ out) {
    nrf_pack_body(C, CO, precision, W1, b1, W2, b2, Wf, out, blockIdx.x * blockDim.x + threadIdx.x);
}
// every block of a renderer in one launch (blockIdx.y = block; the training forward packs all of them on every step)
struct NrfPackAll {
    const float* W1[N3DT_MAX_BLOCKS];
    const float* b1[N3DT_MAX_BLOCKS];
    const float* W2[N3DT_MAX_BLOCKS];
    const float* b2[N3DT_MAX_BLOCKS];
    const float* Wf[N3DT_MAX_BLOCKS];
    unsigned char* out[N3DT_MAX_BLOCKS];
    int C[N3DT_MAX_BLOCKS], CO[N3DT_MAX_BLOCKS];
};
__global__ void nrf_pack_all_kernel(const NrfPackAll a, const int precision) {
    const int k = blockIdx.y;
    const int n = nrf_dims(a.C[k], a.CO[k]).padded * 64;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n || i < 6 * a.C[k]; i += gridDim.x * blockDim.x)
        nrf_pack_body(a.C[k], a.CO[k], precision, a.W1[k], a.b1[k], a.W2[k], a.b2[k], a.Wf[k], a.out[k], i);
}

// One product of the chain: NT output tiles of 32 channels, each summed over KH k-steps of `hin` (packed accumulator
// tiles of the previous product) and then KX k-steps of `xin` (the input fragments, natural channel order).
//   MODE 0: out = lrelu(acc + bias), packed into hout (two k-steps of the next product per tile)
//   MODE 1: out = acc, stored 16-bit at st + 32 * tile (+ 8 per register group; st carries the lane's 4h offset)
// P0: index of the stage's first piece in the stream (compile time: the fragment prefetch needs its ring position).
// END: the stage's last piece is the last of the whole stream (no prefetch behind it, x16_core.h).
// SAVE (MODE 0, training forward): the activation is ALSO stored 16-bit, row-major, at st + 32 * tile -- what the
// backward reads as GEMM operand and as LeakyReLU gate (st as in MODE 1: the pixel's row, + 4 h).
template <int PREC, int WAVES, int NCH, int P0, int KH, int KX, int NT, int MODE, bool END, bool SAVE = false, class WS, int NHIN, int NXIN, int NHOUT>
__device__ __forceinline__ void nrf_stage(WS& ws, const unsigned bias /* LDS byte address of the stage's table + 4 c */,
                                          const typename X16<PREC>::frag (&hin)[NHIN], const typename X16<PREC>::frag (&xin)[NXIN],
                                          typename X16<PREC>::frag (&hout)[NHOUT], unsigned short* const st, const bool live, const int lane) {
    typedef typename X16<PREC>::frag frag;
    constexpr int KS = KH + KX;
    // two accumulator sets: the epilogue of tile t-1 issues under the MFMAs of tile t.  Only at one wave per SIMD: with two,
    // the partner wave's MFMAs cover the epilogue and the 16 registers are needed elsewhere.
    constexpr bool DEFER = WAVES == 4;
    const int h = lane >> 5;
    const frag ones = X16<PREC>::ones_frag();
    // Biases come from an LDS copy of the block's table (filled in the kernel prologue), read a tile ahead with an asm
    // ds_read_b32: LDS returns in order, so the value has landed once a later weight fragment has been awaited.  As global loads
    // they sat on vmcnt, which retires in order -- hipcc's wait for a bias also waited for every `hid` store issued before it
    // (x16_core.h, nerf_fwd_x16.hip: the same finding in the training forward).
    float bias_cur = 0.0f, bias_nxt = 0.0f;
    if (MODE == 0) {
        x16_bias_read<0>(bias_cur, bias);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bias_cur));  // once per stage
    }
    f32x16 acc[DEFER ? 2 : 1];
    u32x4 stash;  // MODE 1 / SAVE: half 0 of the tile being stored
    auto finish = [&](const int t, const int half) {
        const int set = DEFER ? (t & 1) : 0;
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float a = acc[set][8 * half + r];
            // (the two-instruction form where the epilogue's VALU is exposed: one wave per SIMD.  In the 8-wave kernels it
            // costs registers -- 127 -> 132 at C = 64, one workgroup per CU instead of two: 145 -> 165 us)
            v[r] = MODE == 0 ? (WAVES == 4 ? x16_lrelu02(a) : fmaxf(a, 0.2f * a)) : a;
        }
        const frag f = X16<PREC>::pack(v);
        if (MODE == 0) hout[(2 * t + half) < NHOUT ? (2 * t + half) : 0] = f;
        if (MODE == 1 || SAVE) {
            // A lane holds four 8-byte groups of the tile's 32 channels: 4h + {0, 8, 16, 24} + 0..3 (half 0: the first two,
            // half 1: the others).  Stored as they stand that is four 8-byte stores per lane, each instruction touching 16 of
            // every 64+ bytes of 32 pixel rows.  Instead the two lanes of a pixel trade groups (v_permlane32_swap: the upper
            // half-wave's copy of one register against the lower half-wave's copy of another): lane (c, 0) ends up with
            // channels 0..15, lane (c, 1) with 16..31, contiguous -- two 16-byte stores per lane, whole rows per instruction.
            const u32x4 d = __builtin_bit_cast(u32x4, f);
            if (half == 0) {
                stash = d;
            } else {
                const u32x4 a = stash;  // a[0..1]: ch 4h+0..3, a[2..3]: 8+4h+0..3;  d[0..1]: 16+4h+0..3, d[2..3]: 24+4h+0..3
                const auto s0 = __builtin_amdgcn_permlane32_swap(a[0], d[0], false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(a[1], d[1], false, false);
                const auto s2 = __builtin_amdgcn_permlane32_swap(a[2], d[2], false, false);
                const auto s3 = __builtin_amdgcn_permlane32_swap(a[3], d[3], false, false);
                if (live) {
                    unsigned short* dst = st + 32 * t + 12 * h;  // st carries 4 h: the lane's 16 channels start at 16 h
                    *reinterpret_cast<u32x4*>(dst) = u32x4{s0[0], s1[0], s0[1], s1[1]};
                    *reinterpret_cast<u32x4*>(dst + 8) = u32x4{s2[0], s3[0], s2[1], s3[1]};
                }
            }
        }
    };
    constexpr int E0 = KS >= 8 ? 2 : 1, E1 = KS >= 8 ? 5 : (KS - 1);
    static_for<0, NT>([&](auto ot_c) {
        constexpr int ot = decltype(ot_c)::value;
        constexpr int cur = DEFER ? (ot & 1) : 0;
        {
            f32x16 zero;
#pragma unroll
            for (int r = 0; r < 16; ++r) zero[r] = 0.0f;
            f32x16 binit = zero;
            if (MODE == 0) {  // acc = bias broadcast over the pixels, by one extra MFMA (hi/lo split, x16_core.h)
                const frag bf = X16<PREC>::bias_frag(bias_cur, h == 0);
                if constexpr (ot + 1 < NT) x16_bias_read<(ot + 1) * 128>(bias_nxt, bias);
                binit = X16<PREC>::mfma(bf, ones, zero);
            }
            acc[cur] = binit;
        }
        static_for<0, KS>([&](auto ks_c) {
            constexpr int ks = decltype(ks_c)::value;
            const frag a_cur = ws.template next<END, P0 + NT * KS, P0 + ot * KS + ks>();
            const frag b = ks < KH ? hin[ks < KH ? ks : 0] : xin[ks >= KH ? ks - KH : 0];
            acc[cur] = X16<PREC>::mfma(a_cur, b, acc[cur]);
            if (DEFER && ot > 0 && ks == E0) finish(ot - 1, 0);
            if (DEFER && ot > 0 && ks == E1) finish(ot - 1, 1);
        });
        if constexpr (MODE == 0 && ot + 1 < NT) {
            // landed: older than every fragment read awaited in the k-loop above.  The accumulator rides along so that this
            // statement cannot be scheduled ahead of the loop's last MFMA (and with it the waits on its fragments): where the
            // fragments are plain loads (ResidentStream) nothing else orders it behind them -- seen: biases read too early
            asm volatile("" : "+v"(bias_nxt), "+v"(acc[cur]));
            bias_cur = bias_nxt;
        }
        if (!DEFER || ot == NT - 1) {
            finish(ot, 0);
            finish(ot, 1);
        }
    });
}

// sub-pixel q of the block: y_q from t1, then hid_q from y_q and x
template <int PREC, int C, int CO, int WAVES, int NCH, int PB, bool FINAL, bool SAVE = false, class WS>
__device__ __forceinline__ void nrf_subpixel(WS& ws, const unsigned bias, const int q,
                                             const typename X16<PREC>::frag (&t1)[C / 8], const typename X16<PREC>::frag (&xf)[C / 16],
                                             unsigned short* const plane0, const size_t plane_stride, const bool live, const int lane,
                                             unsigned short* const ysave0, const size_t ysave_stride) {
    typedef typename X16<PREC>::frag frag;
    constexpr NrfDims D = nrf_dims(C, CO);
    frag y[C / 16];
    // x regrouped for this sub-pixel: elements q and q + 4 of four consecutive natural fragments (same lane)
    frag xq[D.kxq];
    if constexpr (!D.regroup) {
#pragma unroll
        for (int k = 0; k < D.kxq; ++k) xq[k] = xf[k];
    } else {
        const bool hi_dw = (q & 2) != 0;
        const unsigned sel = (q & 1) ? 0x07060302u : 0x05040100u;
#pragma unroll
        for (int k = 0; k < D.kxq; ++k) {
            u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                if (4 * k + dd < C / 16) {
                    const u32x4 src = __builtin_bit_cast(u32x4, xf[(4 * k + dd) < C / 16 ? (4 * k + dd) : 0]);
                    const unsigned lo = hi_dw ? src[1] : src[0], hi = hi_dw ? src[3] : src[2];
                    o[dd] = __builtin_amdgcn_perm(hi, lo, sel);
                }
            }
            xq[k] = __builtin_bit_cast(frag, o);
        }
    }
    unsigned short* const ysv = SAVE ? ysave0 + (size_t)q * ysave_stride : nullptr;  // y_q of plane q (training forward)
    unsigned short* const st = plane0 + (size_t)q * plane_stride;
    nrf_stage<PREC, WAVES, NCH, PB, C / 8, 0, C / 32, 0, false, SAVE>(ws, bias + 4u * (2 * C + q * C), t1, xf, y, ysv, live, lane);
    nrf_stage<PREC, WAVES, NCH, PB + D.s2, C / 16, D.kxq, CO / 32, 1, FINAL>(ws, bias, y, xq, y, st, live, lane);
}

// SAVE (training forward): t1 [M][2C] and the four y_q planes [4][M][C] are stored as well (16-bit rows).
template <int PREC, int C, int CO, int WAVES, bool IN32, bool SAVE = false>
__global__ __launch_bounds__(WAVES * 64) void nr_level_x16_kernel(const int M_, const void* __restrict__ xv, const unsigned char* __restrict__ packed_,
                                                           unsigned short* __restrict__ hid_, unsigned short* __restrict__ t1_save_,
                                                           unsigned short* __restrict__ y_save_) {
    int M = M_;
    const unsigned char* packed = packed_;
    unsigned short* hid = hid_;
    unsigned short* t1_save = t1_save_;
    unsigned short* y_save = y_save_;
    x16_pin(M);  // no scalar loads once the fragment stream runs (x16_core.h)
    x16_pin(packed);
    x16_pin(hid);
    if (SAVE) {
        x16_pin(t1_save);
        x16_pin(y_save);
    }
    typedef typename X16<PREC>::frag frag;
    constexpr NrfDims D = nrf_dims(C, CO);
    constexpr int NCH = D.padded / X16_CH;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const float* bias = reinterpret_cast<const float*>(packed + (size_t)D.padded * X16_PIECE);

    WeightStream<PREC, WAVES, NCH, NRF_NBUF> ws;
    ws.gsrc = packed + (size_t)wave * WeightStream<PREC, WAVES, NCH, NRF_NBUF>::PPW * X16_PIECE + lane * 16;
    ws.ring = lds;
    ws.lds_addr0 = (unsigned)(size_t)(LDS_AS unsigned char*)lds + lane * 16;
    ws.wave = wave;
    ws.prologue_issue();  // the input loads below run under these

    frag xf[C / 16];
    long m = ((long)blockIdx.x * WAVES + wave) * 32 + c;
    const bool live = m < M;
    if (!live) m = M - 1;
    unsigned short* plane0 = hid + (size_t)m * CO + 4 * h;
    unsigned short* t1sv = SAVE ? t1_save + (size_t)m * (2 * C) + 4 * h : nullptr;
    unsigned short* ysv0 = SAVE ? y_save + (size_t)m * C + 4 * h : nullptr;
    if (IN32) {
        const float* xr = reinterpret_cast<const float*>(xv) + (size_t)m * C + 8 * h;
#pragma unroll
        for (int ks = 0; ks < C / 16; ++ks) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(xr + 16 * ks), b = *reinterpret_cast<const f32x4*>(xr + 16 * ks + 4);
            const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
            xf[ks] = X16<PREC>::pack(v);
        }
    } else {
        const unsigned short* xr = reinterpret_cast<const unsigned short*>(xv) + (size_t)m * C + 8 * h;
#pragma unroll
        for (int ks = 0; ks < C / 16; ++ks) xf[ks] = __builtin_bit_cast(frag, *reinterpret_cast<const u16x8*>(xr + 16 * ks));
    }
    // the block's 6 C biases -> LDS (behind the weight ring), visible after prologue_wait()'s barrier
    float* const bias_s = reinterpret_cast<float*>(lds + NRF_NBUF * X16_CH * X16_PIECE);
    for (int i = threadIdx.x; i < 6 * C; i += WAVES * 64) bias_s[i] = bias[i];
    const unsigned bias_lane = (unsigned)(size_t)(LDS_AS unsigned char*)bias_s + 4 * c;
    x16_pin_v(plane0);
    if (SAVE) {
        x16_pin_v(t1sv);
        x16_pin_v(ysv0);
    }
    size_t plane_stride = (size_t)M * CO;
    x16_pin(plane_stride);
    size_t ysave_stride = (size_t)M * C;
    if (SAVE) x16_pin(ysave_stride);
    ws.prologue_wait();

    frag t1[C / 8];
    nrf_stage<PREC, WAVES, NCH, 0, 0, C / 16, 2 * C / 32, 0, false, SAVE>(ws, bias_lane, xf, xf, t1, t1sv, live, lane);
    if constexpr (D.body % X16_CH == 0) {
        // every sub-pixel starts at the same ring position: one rolled body
#pragma unroll 1
        for (int q = 0; q < 4; ++q)
            nrf_subpixel<PREC, C, CO, WAVES, NCH, D.s1, false, SAVE>(ws, bias_lane, q, t1, xf, plane0, plane_stride, live, lane, ysv0, ysave_stride);
    } else {
        static_for<0, 4>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            nrf_subpixel<PREC, C, CO, WAVES, NCH, D.s1 + q * D.body, q == 3, SAVE>(ws, bias_lane, q, t1, xf, plane0, plane_stride, live, lane, ysv0,
                                                                                      ysave_stride);
        });
    }
    // the rolled loop's last pass prefetched a piece nobody reads; its registers stay reserved up to here (x16_core.h)
    ws.settle();
}

template <int PREC, int C, int CO, int WAVES, bool SAVE = false>
static void nrf_launch_level(const int M, const void* x, const bool x_is_16, const unsigned char* packed, unsigned short* hid, hipStream_t s,
                             unsigned short* t1_save = nullptr, unsigned short* y_save = nullptr) {
    const size_t lds_bytes = NRF_NBUF * X16_CH * X16_PIECE + 6 * C * sizeof(float);  // weight ring + the bias table
    const int per_wg = WAVES * 32;
    const dim3 grid((unsigned)((M + per_wg - 1) / per_wg));
    if (x_is_16) {
        auto kern = nr_level_x16_kernel<PREC, C, CO, WAVES, false, SAVE>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL(kern, grid, dim3(WAVES * 64), lds_bytes, s, M, x, packed, hid, t1_save, y_save);
    } else {
        auto kern = nr_level_x16_kernel<PREC, C, CO, WAVES, true, SAVE>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL(kern, grid, dim3(WAVES * 64), lds_bytes, s, M, x, packed, hid, t1_save, y_save);
    }
}

#include "nr_fused_lat_x16.inc"

// pack the block's weights (the renderer takes raw fp32 parameters: pack_mode 0 packs on every call, 1 trusts the stream
// a previous call left in the caller's workspace, 2 only packs) and run it
// the training forward: the same block with t1 and the four y_q planes saved for the backward (bf16 maps; packs on every call --
// the weights moved since the last step)
static void nrf_run_level_train(const int C, const int CO, const int M, const void* x, const bool x_is_16, unsigned char* packed,
                                unsigned short* hid, unsigned short* t1_save, unsigned short* y_save, hipStream_t s);

template <int PREC>
static void nrf_run_level(const int C, const int CO, const int M, const void* x, const bool x_is_16, const float* W1, const float* b1,
                          const float* W2, const float* b2, const float* Wf, unsigned char* packed, unsigned short* hid, const int pack_mode,
                          hipStream_t s) {
    const int nthr = nrf_dims(C, CO).padded * 64;
    if (pack_mode != 1) hipLaunchKernelGGL(nrf_pack_kernel, dim3((nthr + 255) / 256), dim3(256), 0, s, C, CO, PREC, W1, b1, W2, b2, Wf, packed);
    if (pack_mode == 2) return;
    // one 32-pixel tile per wavefront (two measured slower at every block size: 172 us against ~130 at C = 128, 232 against 165
    // at C = 64); wavefronts per workgroup, measured per block size (us at 16 frames, 64^2 feature map):
    //   C 256: 4 (378 registers: t1 alone is 128) 194
    //   C 128: 4  ~130  (252 registers, two workgroups per CU; 8: hipcc spills at the 256 budget, 217)
    //   C  64: 8  165   (119 registers, two workgroups per CU; 4: 207)
    //   C  32: 8
    // few tiles: the launch's time is one tile's chain -- the four waves of a workgroup share a tile (nr_fused_lat_x16.inc)
    static const int lat = [] {
        const char* e = getenv("N3DT_NR_LAT");
        return e ? atoi(e) : 1;
    }();
    if (lat && C >= 64 && (M + 31) / 32 <= NRF_LAT_MAX_TILES) {
        if (C == 256) nrf_launch_level_lat<PREC, 256, 128>(M, x, x_is_16, packed, hid, s);
        else if (C == 128) nrf_launch_level_lat<PREC, 128, 64>(M, x, x_is_16, packed, hid, s);
        else nrf_launch_level_lat<PREC, 64, 32>(M, x, x_is_16, packed, hid, s);
        return;
    }
    if (C == 256) nrf_launch_level<PREC, 256, 128, 4>(M, x, x_is_16, packed, hid, s);
    else if (C == 128) nrf_launch_level<PREC, 128, 64, 4>(M, x, x_is_16, packed, hid, s);
    else if (C == 64) nrf_launch_level<PREC, 64, 32, 8>(M, x, x_is_16, packed, hid, s);
    else nrf_launch_level<PREC, 32, 32, 8>(M, x, x_is_16, packed, hid, s);
}

static void nrf_run_level_train(const int C, const int CO, const int M, const void* x, const bool x_is_16, unsigned char* packed,
                                unsigned short* hid, unsigned short* t1_save, unsigned short* y_save, hipStream_t s) {
    constexpr int PREC = N3DT_BF16;  // (`packed` was filled by nrf_pack_all_kernel at the top of the forward)
    if (C >= 64 && (M + 31) / 32 <= NRF_LAT_MAX_TILES) {
        if (C == 256) nrf_launch_level_lat<PREC, 256, 128, true>(M, x, x_is_16, packed, hid, s, t1_save, y_save);
        else if (C == 128) nrf_launch_level_lat<PREC, 128, 64, true>(M, x, x_is_16, packed, hid, s, t1_save, y_save);
        else nrf_launch_level_lat<PREC, 64, 32, true>(M, x, x_is_16, packed, hid, s, t1_save, y_save);
        return;
    }
    if (C == 256) nrf_launch_level<PREC, 256, 128, 4, true>(M, x, x_is_16, packed, hid, s, t1_save, y_save);
    else if (C == 128) nrf_launch_level<PREC, 128, 64, 4, true>(M, x, x_is_16, packed, hid, s, t1_save, y_save);
    else if (C == 64) nrf_launch_level<PREC, 64, 32, 8, true>(M, x, x_is_16, packed, hid, s, t1_save, y_save);
    else nrf_launch_level<PREC, 32, 32, 8, true>(M, x, x_is_16, packed, hid, s, t1_save, y_save);
}
