// Mixed-precision training path of the volumetric render (bf16 MFMA products, fp32 accumulation, fp32
// parameters and gradients) -- the fused counterpart of the layer-by-layer fp32 path in train_mlp.hip.
// Included by train_mlp.hip (one translation unit, so the small head / folding kernels are shared).
//
//   forward   nerf_fwd_x16_train_kernel (nerf_fwd_x16.hip): the fused render kernel, leaving per 32-sample block
//             the layer inputs as [sample][channel] tile images (xT; x16_core.h), relu(RGB_layer_1) (gS) and sigma / dist (geo)
//   backward  1. head (RGB_layer_2 per ray, merge)            train_head_bwd_kernel, train_bg_b2_grad_kernel, gemm
//             2. compositing adjoint per ray                  train16_composite_bwd_kernel  -> d sigma per sample
//             3. the dX chain, fused over all layers          nerf_bwd_x16_kernel: per block dZ_l = (W_{l+1}^T dZ_{l+1}) * relu'(H_l)
//                kept in registers as MFMA operands; every dZ_l is also written as tile images (dzT)
//             4. weight gradients dW_l = sum_samples dZ_l (x) X_l   dw_x16_body: both operands are pieces, streamed HBM -> LDS
//                once per block of tiles; bias gradients are the row sums of the same pieces.  Three launches: dw_x16_kernel
//                (the merged RGB product), dw_x16_flat_kernel twice (the seven hidden products, then the two PE products)
//             5. un-merge RGB_layer_0 / RGB_layer_1, density row, latent folding adjoint
// RGB_layer_0 and RGB_layer_1 run merged (W_m = Wr1[:, :384] Wr0, no activation between them, models.py:79-81);
// the chain rule through the product gives dWr1a = dW_m Wr0^T + db_m (x) br0, dWr0 = Wr1a^T dW_m, dbr0 = Wr1a^T db_m.
// Camera gradients (single-image fitting) add two small stages to the dX chain: d PE through the skip layer and layer 0.
#include <stdlib.h>
#include <string.h>

#include "x16_core.h"
#include "n3dt_launch.h"

#define T16_DZ_TILES 103  // per block: [dG (6) | d sigma row (1)] | dZ0 .. dZ7 (12 each), tile offset of dZ_l = 7 + 12 l
#define T16_BWD_PIECES (168 + 7 * 288)
#define T16_BWD_NCHUNK (T16_BWD_PIECES / X16_CH)
// with camera gradients two more stages ride in the stream: d PE = W5[:, 0:63]^T dZ5 and W0[:, 0:63]^T dZ0 (48 pieces each)
#define T16_BWD_PIECES_CAM (T16_BWD_PIECES + 2 * 48)
#define T16_BWD_NCHUNK_CAM (T16_BWD_PIECES_CAM / X16_CH)
#define T16_BWD_WAVES 4

#define DW_XCDS 8           // partial buffers per weight-gradient launch (indexed by the hardware XCC id, masked to 0..7)
#define DW_PACE_SLOTS 4096  // per product: [slice][2], slices <= 2048
#define DW_MAX_LAUNCHES 10  // merged RGB, FeaExt_module_7..1 (5 twice: hidden and PE columns), FeaExt_module_0
struct Train16Saved {  // byte offsets into the saved buffer
    size_t fold, xT, gS, geo, weight, ray, gates, wm, total;
};
#define T16_GATE_WORDS (8 * 6 * 64)  // per block: 8 layers x 12 tiles x 16 sign bits per lane, two tiles per 32-bit word
struct Train16Ws {  // byte offsets into the workspace
    size_t part, wlocal, packT, dzT, dsig, ddist, dpe5, dpe0, dfg, dgray, dwsum, dfold, rsrgb, dwm, dwpart, pace, total;
};
static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline long t16_blocks(const N3dtGeom* g) { return (long)g->batch * g->n_rays * ((g->n_samples + 31) / 32); }

static Train16Saved saved16_layout(const N3dtGeom* g) {
    Train16Saved s;
    const size_t blocks = (size_t)t16_blocks(g), R = (size_t)g->batch * g->n_rays;
    size_t o = 0;
    s.fold = o; o += al256(sizeof(float) * n3dt_fold_region_floats(g->batch, g->n_rays, g->vd_dim));  // (+ the per-ray table of include_vd)
    s.xT = o; o += al256((blocks + 1) * X16_XT_TILES * 2 * X16_PIECE);  // + 1: the dump record dead waves write (x16_core.h: counted waits)
    s.gS = o; o += al256((blocks + 1) * 12 * X16_PIECE);
    s.geo = o; o += al256(blocks * 64 * sizeof(float));
    s.weight = o; o += al256(R * g->n_samples * sizeof(float));
    s.ray = o; o += al256(R * N3DT_PART_STRIDE * sizeof(float));
    s.gates = o; o += al256((blocks + 1) * T16_GATE_WORDS * sizeof(unsigned));
    s.wm = o; o += al256(sizeof(float) * 192 * 384);  // the forward's merged RGB matrix W_m, for the backward's transposed stream
    s.total = o;
    return s;
}
static Train16Ws ws16_layout(const N3dtGeom* g) {
    Train16Ws w;
    const size_t blocks = (size_t)t16_blocks(g), R = (size_t)g->batch * g->n_rays;
    size_t o = 0;
    w.part = o; o += al256(blocks * N3DT_PART_STRIDE * sizeof(float));
    w.wlocal = o; o += al256(blocks * 32 * sizeof(float));
    w.packT = o; o += al256((size_t)T16_BWD_PIECES_CAM * X16_PIECE);
    w.dzT = o; o += al256((blocks + 1) * T16_DZ_TILES * 2 * X16_PIECE);
    w.dsig = o; o += al256(blocks * 32 * sizeof(float));
    w.ddist = o; o += al256(blocks * 32 * sizeof(float));
    w.dpe5 = o; o += al256(blocks * 32 * 64 * sizeof(float));  // camera gradients only: d PE from the skip layer ...
    w.dpe0 = o; o += al256(blocks * 32 * 64 * sizeof(float));  // ... and from layer 0, [block * 32 + sample][64]
    w.dfg = o; o += al256(R * 256 * sizeof(float));
    w.dgray = o; o += al256(R * 192 * sizeof(float));
    w.dwsum = o; o += al256(R * sizeof(float));
    w.dfold = o; o += al256(sizeof(float) * g->batch * N3DT_FOLD_STRIDE);
    w.rsrgb = o; o += al256(sizeof(float) * g->batch * 224);
    w.dwm = o; o += al256(sizeof(float) * 224 * 384);
    w.dwpart = o; o += al256(sizeof(float) * (size_t)DW_MAX_LAUNCHES * DW_XCDS * 384 * 384);  // per-XCD partial weight gradients
    w.pace = o; o += al256(sizeof(unsigned) * (size_t)DW_MAX_LAUNCHES * DW_PACE_SLOTS);       // progress counters of paired workgroups
    w.total = o;
    return w;
}
extern "C" size_t n3dt_train16_saved_bytes(const N3dtGeom* g) { return saved16_layout(g).total; }
extern "C" size_t n3dt_train16_ws_bytes(const N3dtGeom* g) { return ws16_layout(g).total; }

// ---------------------------------------------------------------------------------------------
// Transposed weight stream of the backward chain, bf16, in execution order:
//   RGB   [W_m ; w_density ; 0]^T   384 x 224   (rows = H7 channels, k = RGB_layer_1 rows | density | pad)
//   W_l^T for l = 7, 6, 5 (the H4 columns of FeaExt_module_5), 4, 3, 2, 1           384 x 384 each
//   cam only: PE5 = W5[:, 0:63]^T (64 x 384, row 63 zero) right behind W6^T (when dZ5 exists), PE0 = W0[:, 0:63]^T last
// Piece (ot, ks) of a stage, lane, element j  ->  row ot*32 + (lane&31), k as in nerf_aux.hip (accumulator-tile order).
// grid (64, 8 or 10)
// ---------------------------------------------------------------------------------------------
__global__ void train16_pack_bwd_kernel(N3dtMlpParams p, int S, int U, int cam, const float* __restrict__ wm /*[192][384]*/,
                                        unsigned char* __restrict__ out) {
    // stage table: kind 0 = RGB, 1..7 = W_kind^T, 8 = PE5, 9 = PE0
    const int order_plain[8] = {0, 7, 6, 5, 4, 3, 2, 1};
    const int order_cam[10] = {0, 7, 6, 8, 5, 4, 3, 2, 1, 9};
    const int q = blockIdx.y;
    size_t base = 0;  // elements before this stage
    int kind = 0;
    for (int i = 0; i <= q; ++i) {
        kind = cam ? order_cam[i] : order_plain[i];
        if (i < q) base += (size_t)(kind == 0 ? 168 : (kind >= 8 ? 48 : 288)) * 512;
    }
    const int K = kind == 0 ? 224 : 384;
    const int rows = kind >= 8 ? 64 : 384;
    const int in0 = N3DT_PE_DIM + S + U, in5 = N3DT_PE_DIM + S + N3DT_HID;
    const size_t n = (size_t)rows * K;
    unsigned short* o16 = reinterpret_cast<unsigned short*>(out);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int j = e & 7, lane = (e >> 3) & 63;
        const size_t t = e >> 9;
        const int ks = (int)(t % (K / 16)), ot = (int)(t / (K / 16));
        const int row = ot * 32 + (lane & 31);
        const int k = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
        float v;
        if (kind == 0) {
            if (k < 192) v = wm[(size_t)k * N3DT_HID + row];
            else v = k == 192 ? p.weight[8][row] : 0.0f;
        } else if (kind == 5) {
            v = p.weight[5][(size_t)k * in5 + N3DT_PE_DIM + S + row];
        } else if (kind == 8) {
            v = row < N3DT_PE_DIM ? p.weight[5][(size_t)k * in5 + row] : 0.0f;
        } else if (kind == 9) {
            v = row < N3DT_PE_DIM ? p.weight[0][(size_t)k * in0 + row] : 0.0f;
        } else {
            v = p.weight[kind][(size_t)k * N3DT_HID + row];
        }
        __bf16 hv = (__bf16)v;
        o16[base + e] = __builtin_bit_cast(unsigned short, hv);
    }
}

// ---------------------------------------------------------------------------------------------
// Compositing adjoint, one wave per ray, walking its 32-sample blocks back to front (same algebra as
// train_composite_bwd_kernel above; reference NetWorks/utils.py:273-309):
//   dw_s = dGray . g_s + d_wsum ;  dalpha_s = dw_s T_s - (sum_{t>s} dw_t w_t) / x_s ;  dsigma_s = dalpha_s dist_s (1 - alpha_s) [sigma_pre > 0]
// g comes as the lane = sample fragments the forward left (lane (c, h) element j of fragment ks = channel
// 16 ks + 8 (j>>2) + 4 h + (j&3) of sample c).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void train16_composite_bwd_kernel(N3dtGeom g, int bpr, const unsigned char* __restrict__ gS,
                                                                    const float* __restrict__ geo, const float* __restrict__ weight,
                                                                    const float* __restrict__ dgray, const float* __restrict__ dwsum,
                                                                    float* __restrict__ dsig, float* __restrict__ ddist) {
    const long R = (long)g.batch * g.n_rays;
    const long ray = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    if (ray >= R) return;
    const int Ns = g.n_samples;
    float dfv[12][8];
#pragma unroll
    for (int ks = 0; ks < 12; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) dfv[ks][j] = dgray[ray * 192 + 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)];
    const float dws = dwsum[ray];
    float carry = 0.0f;
    for (int sb = bpr - 1; sb >= 0; --sb) {
        const size_t blk = (size_t)ray * bpr + sb;
        const unsigned char* gb = gS + blk * 12 * X16_PIECE + lane * 16;
        float dot = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 12; ++ks) {
            const bf16x8 f = *reinterpret_cast<const bf16x8*>(gb + ks * X16_PIECE);
#pragma unroll
            for (int j = 0; j < 8; ++j) dot = fmaf(dfv[ks][j], (float)f[j], dot);
        }
        dot += __shfl_xor(dot, 32, 64);
        const float dw = dot + dws;
        const int s = sb * 32 + c;
        const bool valid = s < Ns;
        const float w = valid ? weight[(size_t)ray * Ns + s] : 0.0f;
        const float sig = geo[blk * 64 + c], dist = geo[blk * 64 + 32 + c];
        const float sigma = fmaxf(sig, 0.0f);
        const float e = expf(-sigma * dist);
        const float alpha = 1.0f - e;
        const float x = e + 1e-10f;
        const float v = valid ? dw * w : 0.0f;
        float incl = v;  // inclusive suffix sum over the 32 lanes of the half
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            const float o = __shfl_down(incl, off, 32);
            if (c + off < 32) incl += o;
        }
        const float suf = incl - v + carry;
        float dalpha = 0.0f;
        if (alpha > 0.0f) dalpha = dw * (w / alpha) - suf / x;
        float ds = dalpha * dist * e;
        if (!(sig > 0.0f) || !valid) ds = 0.0f;
        if (h == 0) {
            dsig[blk * 32 + c] = ds;
            if (ddist) ddist[blk * 32 + c] = valid ? dalpha * sigma * e : 0.0f;  // d dist, for the camera backward
        }
        carry += __shfl(incl, 0, 32);
    }
}

// ---------------------------------------------------------------------------------------------
// The fused dX chain.  One wave = one 32-sample block, T16_BWD_WAVES waves per workgroup sharing the
// transposed weight stream through the LDS ring of x16_core.h.
// ---------------------------------------------------------------------------------------------
// Gate words of one layer for one wave sit in LDS (a single 1.5 KiB slot per wave; T16_GATE_SLOT): vmcnt retires in order, so
// hipcc's wait for a gate word LOADED from global memory also waited for every dZ store issued before the load -- 0.3 ms of the
// 1.36 ms chain (diagnostic build without the loads).  The slot is filled by LDS-DMA (x16_gate_stage_in): for the first stage in
// the kernel prologue, for stage l+1 three tiles before the end of stage l, when stage l's six words have all been read into
// registers (three rendezvous then retire the copy); words are read with asm ds_read_b32 a pair ahead -- LDS returns in order, so a
// word has landed once a later weight fragment has been awaited.
#define T16_GATE_SLOT 1536
__device__ __forceinline__ void x16_gate_stage_in(const unsigned* src /* layer's words of this block + lane */, unsigned char* slot) {
#pragma unroll
    for (int p = 0; p < 6; ++p)
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(src + p * 64), (LDS_AS void*)(slot + p * 256), 4, 0, 0);
}
template <int OFF>
__device__ __forceinline__ void x16_gate_read(unsigned& dst, const unsigned addr) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF) : "memory");
}
template <class WS, int KS, int NT, bool LAST>
__device__ __forceinline__ void x16_bwd_stage(WS& ws, const bf16x8 (&hin)[24], bf16x8 (&hout)[24], const unsigned gate_addr,
                                              unsigned char* save_dst, unsigned char* gate_slot, const unsigned* gate_next) {
    typedef X16<N3DT_BF16> X;
    // ReLU gates: the sign bits the forward left for the layer below, in THIS accumulator order (bit r of the tile's
    // half-word = register r of this lane) -- 6 words per lane and layer instead of the 48 KiB of activation pieces the
    // first version re-read (and transposed with two MFMAs per tile) to rebuild them: the chain's reads fall 3.3 GB -> 0.2 GB
    // (all six words up front cost 6 registers and the second workgroup per CU with them).
    static_assert(NT == 12, "six gate words per stage");
    unsigned g_cur = 0, g_nxt = 0;
    x16_gate_read<0>(g_cur, gate_addr);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(g_cur));  // once per stage
    static_for<0, NT>([&](auto ot_c) {
        constexpr int ot = decltype(ot_c)::value;
        if constexpr ((ot & 1) == 0) {
            if constexpr (ot > 0) g_cur = g_nxt;  // (pinned behind the previous tile's k-loop)
            if constexpr (ot + 2 < NT) x16_gate_read<((ot >> 1) + 1) * 256>(g_nxt, gate_addr);
        }
        if constexpr (ot == NT - 3) {
            // all six words of this stage are in registers (the last one was read at tile NT - 4 and pinned behind that tile's
            // k-loop): the slot is free.  Three rendezvous follow before the next stage reads it, so the copy has retired whether
            // the rendezvous waits vmcnt(0) (the __syncthreads() fence) or only for what is older than the last tiles' stores
            if (gate_next) x16_gate_stage_in(gate_next, gate_slot);
        }
        const unsigned gm = g_cur >> (16 * (ot & 1));
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        static_for<0, KS>([&](auto ks_c) {
            constexpr int ks = decltype(ks_c)::value;
            const bf16x8 a_cur = ws.template next<LAST, NT * KS, ot * KS + ks>();
            acc = X::mfma(a_cur, hin[ks], acc);
        });
        // landed: older than the fragments awaited above (tied to the accumulator so that it stays behind the loop's last MFMA)
        if constexpr ((ot & 1) == 0 && ot + 2 < NT) asm volatile("" : "+v"(g_nxt), "+v"(acc));
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = ((gm >> (8 * half + r)) & 1u) ? acc[8 * half + r] : 0.0f;
            hout[2 * ot + half] = X::pack(v);
        }
#ifndef X16_DIAG_NODZ
        x16_image_store<N3DT_BF16>(hout[2 * ot], hout[2 * ot + 1], save_dst + ot * 2 * X16_PIECE);  // unconditional: counted
        ws.note_stores(2);
#endif
    });
}

// d PE [64 x 32] = W[:, 0:63]^T dZ for the camera gradients: two output tiles, no gate, written point-major fp32
// dpe[(block * 32 + sample) * 64 + channel] (4-byte stores at a 256-byte stride: the rare path, kept simple)
template <class WS, bool LAST>
__device__ __forceinline__ void x16_bwd_pe_stage(WS& ws, const bf16x8 (&hin)[24], float* dpe_blk, const int lane) {
    typedef X16<N3DT_BF16> X;
    const int c = lane & 31, h = lane >> 5;
    static_for<0, 2>([&](auto ot_c) {
        constexpr int ot = decltype(ot_c)::value;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        static_for<0, 24>([&](auto ks_c) {
            constexpr int ks = decltype(ks_c)::value;
            const bf16x8 a_cur = ws.template next<LAST, 48, ot * 24 + ks>();
            acc = X::mfma(a_cur, hin[ks], acc);
        });
        if (dpe_blk) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dpe_blk[c * 64 + 32 * ot + (r & 3) + 8 * (r >> 2) + 4 * h] = acc[r];
        }
    });
}

// (two 4-wave workgroups per CU, two waves per SIMD: a 256-register budget)
template <int WAVES, bool CAM>
__global__ __launch_bounds__(WAVES * 64, 2) void nerf_bwd_x16_kernel(N3dtGeom g, const unsigned char* __restrict__ packT,
                                                                     const unsigned* __restrict__ gates,
                                                                     const unsigned char* __restrict__ gS,
                                                                     const float* __restrict__ weight, const float* __restrict__ dsig,
                                                                     const float* __restrict__ dgray, unsigned char* __restrict__ dzT_,
                                                                     float* __restrict__ dpe5_, float* __restrict__ dpe0_, int bpr,
                                                                     long total_blocks) {
    // the arguments first used deep inside the stream are fetched here (x16_core.h: no scalar loads beside counted LDS waits)
    unsigned char* dzT = dzT_;
    float* dpe5 = dpe5_;
    float* dpe0 = dpe0_;
    x16_pin(dzT);
    x16_pin(dpe5);
    x16_pin(dpe0);
    typedef X16<N3DT_BF16> X;
    typedef WeightStream<N3DT_BF16, WAVES, CAM ? T16_BWD_NCHUNK_CAM : T16_BWD_NCHUNK> WS;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    WS ws;
    ws.gsrc = packT + (size_t)wave * WS::PPW * X16_PIECE + lane * 16;
    ws.ring = lds;
    ws.lds_addr0 = (unsigned)(size_t)(LDS_AS unsigned char*)lds + lane * 16;
    ws.wave = wave;
    ws.prologue_issue();

    long blk = (long)blockIdx.x * WAVES + wave;
    const bool live = blk < total_blocks;
    if (!live) blk = total_blocks - 1;
    const int sb = (int)(blk % bpr);
    const long ray = blk / bpr;
    const int s = sb * 32 + c;
    const float w = s < g.n_samples ? weight[(size_t)ray * g.n_samples + s] : 0.0f;
    const float ds = dsig[(size_t)blk * 32 + c];
    const unsigned* gtb = gates + (size_t)blk * T16_GATE_WORDS + lane;
    const unsigned char* gb = gS + (size_t)blk * 12 * X16_PIECE + lane * 16;
    // (a dead wave writes the dump record behind the last block: the stream's counted waits need every wave to issue its stores)
    unsigned char* const zb = dzT + (size_t)(live ? blk : total_blocks) * T16_DZ_TILES * 2 * X16_PIECE + x16_image_lane_offset(lane);

    bf16x8 ha[24], hb[24];
    // dG[ch][s] = w_s dGray[ch] [g > 0]: a rank-1 product on the matrix pipe (bf16 hi/lo split of both factors)
    {
        const __bf16 w_hi = (__bf16)w;
        const __bf16 w_lo = (__bf16)(w - (float)w_hi);
        bf16x8 wf;
#pragma unroll
        for (int j = 0; j < 8; ++j) wf[j] = (__bf16)0.0f;
        wf[0] = w_hi;
        wf[1] = w_hi;
        wf[2] = w_lo;
        const float* dgr = dgray + (size_t)ray * 192;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const float df = dgr[32 * t + c];
            const __bf16 d_hi = (__bf16)df;
            const __bf16 d_lo = (__bf16)(df - (float)d_hi);
            bf16x8 af;
#pragma unroll
            for (int j = 0; j < 8; ++j) af[j] = (__bf16)0.0f;
            if (h == 0) {
                af[0] = d_hi;
                af[1] = d_lo;
                af[2] = d_hi;
            }
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = 0.0f;
            const f32x16 acc = X::mfma(af, wf, z);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const s16x8 gs = *reinterpret_cast<const s16x8*>(gb + (2 * t + half) * X16_PIECE);
                float v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = acc[8 * half + r];
                const s16x8 m = gs != (s16x8)(0);  // all-ones where the forward activation is non-zero (it is relu'd, so > 0)
                ha[2 * t + half] = __builtin_bit_cast(bf16x8, (s16x8)(__builtin_bit_cast(s16x8, X::pack(v)) & m));
            }
        }
        // tile 6: row 0 = d sigma (the density head rides in the same product), the rest zero
        bf16x8 zf;
#pragma unroll
        for (int j = 0; j < 8; ++j) zf[j] = (__bf16)0.0f;
        ha[13] = zf;
        if (h == 0) zf[0] = (__bf16)ds;
        ha[12] = zf;
#pragma unroll
        for (int t = 0; t < 7; ++t) x16_image_store<N3DT_BF16>(ha[2 * t], ha[2 * t + 1], zb + t * 2 * X16_PIECE);
    }
    auto gate = [&](const int l) { return gtb + l * 6 * 64; };  // gate words of H_l (global memory, + lane)
    unsigned char* const gate_slot = lds + (size_t)X16_NBUF * X16_CH * X16_PIECE + (size_t)wave * T16_GATE_SLOT;  // this wave's slot
    const unsigned gate_addr = (unsigned)(size_t)(LDS_AS unsigned char*)gate_slot + lane * 4;
    x16_gate_stage_in(gate(7), gate_slot);
    ws.prologue_wait();
    auto dz = [&](const int l) -> unsigned char* { return zb + (size_t)(7 + 12 * l) * 2 * X16_PIECE; };
    x16_bwd_stage<WS, 14, 12, false>(ws, ha, hb, gate_addr, dz(7), gate_slot, gate(6));  // [RGB_layer_1 . RGB_layer_0 ; density]^T
    x16_bwd_stage<WS, 24, 12, false>(ws, hb, ha, gate_addr, dz(6), gate_slot, gate(5));  // FeaExt_module_7^T
    x16_bwd_stage<WS, 24, 12, false>(ws, ha, hb, gate_addr, dz(5), gate_slot, gate(4));  // 6
    if constexpr (CAM) x16_bwd_pe_stage<WS, false>(ws, hb, live ? dpe5 + (size_t)blk * 32 * 64 : nullptr, lane);  // skip layer's PE columns
    x16_bwd_stage<WS, 24, 12, false>(ws, hb, ha, gate_addr, dz(4), gate_slot, gate(3));  // 5 (H4 columns)
    x16_bwd_stage<WS, 24, 12, false>(ws, ha, hb, gate_addr, dz(3), gate_slot, gate(2));  // 4
    x16_bwd_stage<WS, 24, 12, false>(ws, hb, ha, gate_addr, dz(2), gate_slot, gate(1));  // 3
    x16_bwd_stage<WS, 24, 12, false>(ws, ha, hb, gate_addr, dz(1), gate_slot, gate(0));  // 2
    x16_bwd_stage<WS, 24, 12, !CAM>(ws, hb, ha, gate_addr, dz(0), gate_slot, nullptr);   // 1
    if constexpr (CAM) x16_bwd_pe_stage<WS, true>(ws, ha, live ? dpe0 + (size_t)blk * 32 * 64 : nullptr, lane);   // layer 0's PE columns
}

// Camera backward of the fused path: the algebra of train_camera_bwd_kernel (above), with the encoder's sin / cos
// recomputed from the sample position (accurate sinf / cosf) and d PE = dpe5 + dpe0 in block-padded point order.
template <bool KX>
__global__ void train16_camera_bwd_kernel(N3dtGeom g, int bpr, const float* __restrict__ xy, const float* __restrict__ R,
                                          const float* __restrict__ T, const float* __restrict__ Kinv,
                                          const float* __restrict__ t_rand, const float* __restrict__ dpe5,
                                          const float* __restrict__ dpe0, const float* __restrict__ ddist, float* __restrict__ d_R,
                                          float* __restrict__ d_T, float* __restrict__ d_Kinv, float* __restrict__ d_xy,
                                          const int cam_rays) {
    // block = cam_rays (<= CAM_RAYS, n3dt_cam_rays_per_block) consecutive rays of ONE frame (blockIdx.y), 4 waves taking rays in turn;
    // the 12 results are summed in registers and LDS and leave as 12 atomics per block (KX: 21, and d_xy per ray, as in the fp32 kernel)
    __shared__ float cam_red[4][21];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y, Ns = g.n_samples;
    float sum_R[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sum_T[3] = {0.f, 0.f, 0.f};
    float sum_K[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int ray_end = min(g.n_rays, (int)(blockIdx.x + 1) * cam_rays);
    for (int ray = blockIdx.x * cam_rays + wave; ray < ray_end; ray += 4) {
    const long rayg = (long)b * g.n_rays + ray;
    const float* Rb = R + b * 9;
    const float* Kb = Kinv + b * 9;
    const float* Tb = T + b * 3;
    const float x = xy[(int64_t)b * g.xy_stride_b + (int64_t)ray * g.xy_stride_r];
    const float y = xy[(int64_t)b * g.xy_stride_b + g.xy_stride_c + (int64_t)ray * g.xy_stride_r];
    float cc[3], w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) cc[i] = Kb[i * 3 + 0] * x + Kb[i * 3 + 1] * y + Kb[i * 3 + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = Rb[i * 3 + 0] * cc[0] + Rb[i * 3 + 1] * cc[1] + Rb[i * 3 + 2] * cc[2];
    const float n = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const float dh[3] = {w[0] / n, w[1] / n, w[2] / n};
    const float l = -1.0f / dh[2];
    const float dl[3] = {dh[0] * l, dh[1] * l, dh[2] * l};
    const float rz1 = Tb[2] - g.world_z1, rz2 = Tb[2] - g.world_z2;
    const float* tr = t_rand ? t_rand + ((int64_t)b * g.n_rays + ray) * (Ns + 1) : nullptr;
    float g_dl[3] = {0.f, 0.f, 0.f}, g_T[3] = {0.f, 0.f, 0.f}, g_l = 0.0f, g_tz = 0.0f;
    for (int s = lane; s < Ns; s += 64) {
        const size_t pt = ((size_t)rayg * bpr + (s >> 5)) * 32 + (s & 31);
        const float* q5 = dpe5 + pt * 64;
        const float* q0 = dpe0 + pt * 64;
        // hierarchical pass: the planes are given.  They are affine combinations (weights summing to 1, placed by the DETACHED
        // coarse weights, NetWorks/utils.py:219-252) of the coarse planes o_z + const, so d plane / d T_z = 1 as in the coarse pass
        const float z_lo = g.z_planes_given ? tr[s] : n3dt_edge_z(rz1, rz2, s, Ns, tr);
        const float z_hi = g.z_planes_given ? tr[s + 1] : n3dt_edge_z(rz1, rz2, s + 1, Ns, tr);
        float dp[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float pd = Tb[d] + dl[d] * z_lo;
            float acc = q5[d] + q0[d];
            float f = 1.0f;
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const float sn = sinf(pd * f), cs = cosf(pd * f);
                const int is = 3 + 6 * k + d, ic = 3 + 6 * k + 3 + d;
                acc += f * (cs * (q5[is] + q0[is]) - sn * (q5[ic] + q0[ic]));
                f *= 2.0f;
            }
            dp[d] = acc;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            g_dl[d] += dp[d] * z_lo;
            g_T[d] += dp[d];
        }
        g_tz += dp[0] * dl[0] + dp[1] * dl[1] + dp[2] * dl[2];
        g_l += ddist[pt] * (z_hi - z_lo);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            g_dl[d] += __shfl_xor(g_dl[d], off, 64);
            g_T[d] += __shfl_xor(g_T[d], off, 64);
        }
        g_l += __shfl_xor(g_l, off, 64);
        g_tz += __shfl_xor(g_tz, off, 64);
    }
    {
        const float gl = g_l + g_dl[0] * dh[0] + g_dl[1] * dh[1] + g_dl[2] * dh[2];
        float g_dh[3] = {g_dl[0] * l, g_dl[1] * l, g_dl[2] * l + gl * l * l};
        const float dot = g_dh[0] * dh[0] + g_dh[1] * dh[1] + g_dh[2] * dh[2];
        [[maybe_unused]] float gwv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float gw = (g_dh[i] - dh[i] * dot) / n;
#pragma unroll
            for (int j = 0; j < 3; ++j) sum_R[i * 3 + j] += gw * cc[j];
            if constexpr (KX) gwv[i] = gw;
        }
        if constexpr (KX) {
            // gradient at c = Kinv [x, y, 1]: gc = R^T gw (gw carries |w|, l and the sample distances already), then
            // d Kinv[i][j] = gc[i] h[j] with h = [x, y, 1] and d (x, y) = the first two columns of Kinv against gc
            float gc[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) gc[j] = Rb[j] * gwv[0] + Rb[3 + j] * gwv[1] + Rb[6 + j] * gwv[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                sum_K[i * 3 + 0] += gc[i] * x;
                sum_K[i * 3 + 1] += gc[i] * y;
                sum_K[i * 3 + 2] += gc[i];
            }
            if (d_xy && lane == 0) {
                float* o = d_xy + (size_t)b * 2 * g.n_rays + ray;
                o[0] = gc[0] * Kb[0] + gc[1] * Kb[3] + gc[2] * Kb[6];
                o[g.n_rays] = gc[0] * Kb[1] + gc[1] * Kb[4] + gc[2] * Kb[7];
            }
        }
        sum_T[0] += g_T[0];
        sum_T[1] += g_T[1];
        sum_T[2] += g_T[2] + g_tz;
    }
    }  // rays of this wave
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) cam_red[wave][i] = sum_R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) cam_red[wave][9 + i] = sum_T[i];
        if constexpr (KX) {
#pragma unroll
            for (int i = 0; i < 9; ++i) cam_red[wave][12 + i] = sum_K[i];
        }
    }
    __syncthreads();
    if (threadIdx.x < (KX ? 21 : 12)) {
        const float v = (cam_red[0][threadIdx.x] + cam_red[1][threadIdx.x]) + (cam_red[2][threadIdx.x] + cam_red[3][threadIdx.x]);
        if (threadIdx.x < 9) {
            if (d_R) atomicAdd(&d_R[b * 9 + threadIdx.x], v);
        } else if (threadIdx.x < 12) {
            if (d_T) atomicAdd(&d_T[b * 3 + threadIdx.x - 9], v);
        } else if (d_Kinv) {
            atomicAdd(&d_Kinv[b * 9 + threadIdx.x - 12], v);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Weight gradients: out[row][col] += sum over blocks and samples of A[row][sample] * B[col][sample], both operands
// stored as [sample][channel] tile images and read transposed from LDS (A = a dZ tensor, B = a layer input).  One workgroup (8 waves as WO x WI, each
// TO x TI tiles) owns (WO*TO) x (WI*TI) tiles of the result for one slice of blocks of one frame: per block it stages
// the 2 (WO*TO + WI*TI) pieces HBM -> LDS by LDS-DMA (3 stages in flight) and every wave reads its fragments from
// there.  HBM-bound: 128 FLOP per operand byte at best.  Row sums of A (the bias gradients) ride along on the
// waves of the first column group.  Results are combined across slices with fp32 atomics.
// ---------------------------------------------------------------------------------------------
struct DwArgs {
    const unsigned char* A;  // + block * strideA bytes; tile t, k-step s at ((a_tile0 + t) * 2 + s) KiB
    size_t strideA;
    int a_tile0, nA;
    const unsigned char* B;
    size_t strideB;
    int b_tile0, nB;
    float* out;
    long ld;
    int rows_valid, cols_valid;
    float* part;    // [DW_XCDS][rows_valid][cols_valid] partial sums of this launch (zeroed by the caller)
    float* rowsum;  // + frame * rs_stride, row index; nullptr: none
    long rs_stride;
    int blocks_per_frame, slices_per_frame, frames, gy;
    unsigned* pace;  // PACE: progress counters of the workgroups that share a slice, [slice][gy] (zeroed by the caller); else unused
    // Row-major operands (the 2-D renderer's weight gradients, train_nr.hip): rowmajor != 0 -> A and B are 16-bit matrices
    // [pixel][channel] with ldA / ldB elements per row; a "block" is 32 consecutive pixels and piece (tile t, half s) of it is
    // the 16 x 32 sub-block rows 16 s .., channels 32 t ..: lane l fetches the 16 bytes at row l / 4, channel 8 (l % 4), which
    // lands in LDS as the same [sample][channel] image the MLP's producers store.  A may be several planes side by side
    // (a_plane_tiles tiles each, a_plane_bytes apart): the four sub-pixel planes of a gradient as one wide operand.
    // row_perm > 0: output row r (= q * row_perm + c) belongs at row 4 c + q of `out` / `rowsum` (pixel_shuffle's channel order).
    int rowmajor;
    long ldA, ldB;
    int a_plane_tiles;
    size_t a_plane_bytes;
    int row_perm;
};

#ifndef DW_STAGES
#define DW_STAGES 4
#endif
#define DW_NBUF(npp) (((DW_STAGES) * (npp) * X16_PIECE <= 160 * 1024) ? (DW_STAGES) : 3)

// One product, one workgroup: the body of dw_x16_kernel (a launch of its own) and of dw_x16_flat_kernel (several products in one
// launch, which picks the workgroup's place itself: y_in, slice_in).  `a` is __restrict__: without it the epilogue re-reads
// its fields from the kernel arguments behind every atomic (300 scalar loads and waits in the 9-tile kernel).
// RM: row-major operands (a compile-time switch: as run-time branches on a.rowmajor the extra live values cost the 12-tile
// MLP kernel its last registers -- 132 bytes of scratch, 210 -> 650 us)
// In-kernel stamps (diagnostic build only: hipcc ... -DN3DT_DW_STAMPS -c csrc/train_mlp.hip, linked into a library of its own and
// picked with N3DT_LIB; never timed, never shipped): where a block's cycles go, per wave of one workgroup -- the source of the
// two constants of launch_dw_multi's cost model (docs/tuning_log.md, round 4).
#ifdef N3DT_DW_STAMPS
#define DW_STAMP(k)                                                                \
    {                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                         \
        unsigned long long t_;                                                     \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                         \
        st_sum[k] += t_ - st_prev;                                                 \
        st_prev = t_;                                                              \
    }
#else
#define DW_STAMP(k)
#endif
// PACE: the two workgroups of a gy = 2 slice keep in step (see below).  DW_PACE_LEAD: blocks of lead tolerated; DW_PACE_SLEEPS: the
// most sleeps of ~0.25 us taken per check, one per block of lead beyond that.
#define DW_PACE_LEAD 0
#define DW_PACE_SLEEPS 12
template <int WO, int WI, int TO, int TI, bool RM = false, bool PACE = false>
__device__ __forceinline__ void dw_x16_body(const DwArgs& __restrict__ a, const int y_in = -1, const int slice_in = -1) {
    static_assert(WO * WI == 8, "8 waves");
    // NBUF stages of one block's pieces in LDS, NBUF - 1 of them in flight.  The kernel is HBM-latency bound (one workgroup
    // per CU, 36-40 KiB per block): the bytes in flight set the bandwidth.  4 stages where they fit the 160 KiB of LDS.
    constexpr int NA = WO * TO, NBT = WI * TI, NP = 2 * (NA + NBT), NPP = (NP + 7) / 8 * 8, PPW = NPP / 8;
    constexpr int NBUF = DW_NBUF(NPP);
    constexpr int STAGE = NPP * X16_PIECE;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wo = wave / WI, wi = wave % WI;
    const int ny_in = (a.nB + NBT - 1) / NBT;
    // XCD-aware 1-D grid: workgroup L runs on XCD L % 8.  The gy workgroups that share a slice (same A or B pieces)
    // get ids 8 apart -- same XCD, dispatched together -- so that the second reader of a piece hits that XCD's L2.
    const int gy = a.gy;
    const int L = blockIdx.x, tq = L >> 3;
    const int y = y_in >= 0 ? y_in : tq % gy, slice = slice_in >= 0 ? slice_in : (tq / gy) * 8 + (L & 7);  // (the flat kernel picks them)
    if (slice >= a.slices_per_frame * a.frames) return;  // padding of the slice count to a multiple of 8 (uniform)
    const int oy = y / ny_in, iy = y % ny_in;
    const int f = slice / a.slices_per_frame, sl = slice % a.slices_per_frame;
    const int per = (a.blocks_per_frame + a.slices_per_frame - 1) / a.slices_per_frame;
    const long b0 = (long)f * a.blocks_per_frame + (long)sl * per;
    long b1 = b0 + per;
    if (b1 > (long)(f + 1) * a.blocks_per_frame) b1 = (long)(f + 1) * a.blocks_per_frame;
    if (b0 >= b1) return;  // uniform over the workgroup

    // this wave's share of a stage: pieces q = wave + 8 i
    const unsigned char* src[PPW];
    size_t stride[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        int q = wave + 8 * i;
        if (q >= NP) q = NP - 1;  // padding slots re-load the last piece
        const bool isA = q < 2 * NA;
        const int qq = isA ? q : q - 2 * NA;
        int tile = (isA ? oy * NA : iy * NBT) + (qq >> 1);
        const int nt = isA ? a.nA : a.nB;
        if (tile >= nt) tile = nt - 1;  // dead tiles re-load a valid one; their results are not written
        if constexpr (RM) {
            const long ld = isA ? a.ldA : a.ldB;
            const int t = (isA ? a.a_tile0 : a.b_tile0) + tile;
            size_t off = ((size_t)(16 * (qq & 1) + (lane >> 2)) * ld + 8 * (lane & 3)) * 2;
            if (isA && a.a_plane_tiles > 0) off += (size_t)(t / a.a_plane_tiles) * a.a_plane_bytes + (size_t)(t % a.a_plane_tiles) * 64;
            else off += (size_t)t * 64;
            src[i] = (isA ? a.A : a.B) + off;
            stride[i] = (size_t)32 * ld * 2;
        } else {
            const size_t off = ((size_t)((isA ? a.a_tile0 : a.b_tile0) + tile) * 2 + (qq & 1)) * X16_PIECE;
            src[i] = (isA ? a.A : a.B) + off + lane * 16;
            stride[i] = isA ? a.strideA : a.strideB;
        }
    }
    // A stage has NP real pieces in NPP = 8 PPW slots: the last slot of waves >= LAST_REAL is padding, and they do not load it.  What
    // a CU can take into LDS is what bounds this kernel (tools/lds_fill_probe.hip: 23 B/clk per CU by LDS-DMA, 25 - 28 through
    // registers, L2-resident source; the seven-product launch moves 20), so the 4 padding pieces of a 36-piece stage were 10 % of
    // its time.  Those waves then count one piece fewer per stage in stage_ready.
    constexpr int LAST_REAL = NP - 8 * (PPW - 1);  // 1 .. 8
    const bool full = LAST_REAL == 8 || wave < LAST_REAL;  // (uniform)
    auto issue = [&](const long b) {
        unsigned char* dst = lds + (size_t)(b % NBUF) * STAGE;
        static_for<0, PPW>([&](auto i_c) {
            constexpr int i = decltype(i_c)::value;
            if (i < PPW - 1 || full)
                __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(src[i] + (size_t)b * stride[i]),
                                                 (LDS_AS void*)(dst + (wave + 8 * i) * X16_PIECE), 16, 0, 0);
        });
    };

    f32x16 acc[TO][TI];
    float rs[TO];
    bool do_rs = false;
    const unsigned tr_off = RM ? x16_tr_lane_offset_natural(lane) : x16_tr_lane_offset(lane);
    const unsigned lds_base = (unsigned)(size_t)(LDS_AS unsigned char*)lds;

    // PACE: the gy = 2 workgroups of a slice stream the SAME A pieces; the second reader hits L2 only while it stays within a few
    // microseconds of the first (a line lives ~6 us in an XCD's 4 MiB at 700 GB/s), and the two drift apart: measured 1.42x the
    // algorithmic bytes fetched (1.5x = no sharing at all).  Every four blocks wave 0 publishes the workgroup's progress and looks
    // at its partner's (same XCD, same L2: a plain store and a glc scalar load); whoever is more than DW_PACE_LEAD blocks ahead sleeps
    // a little before the stage barrier.  Purely a pacing heuristic: a stale or missing value only changes who sleeps, never a
    // result, and every sleep is bounded, so a partner that is not resident yet cannot hold anyone up for long.
    unsigned* pace_mine = nullptr;
    const unsigned* pace_other = nullptr;
    unsigned other_progress = 0;
    if (PACE && gy == 2 && a.pace) {
        pace_mine = a.pace + (size_t)slice * 2 + y;
        pace_other = a.pace + (size_t)slice * 2 + (y ^ 1);
    }
    // One half block (k-step sp: 16 samples) of this wave's operand tiles: two transposed 64-bit reads per tile.
    struct Half {
        x16_u32x2 a[TO][2], b[TI][2];
    };
    auto read_half = [&](Half& hf, const unsigned buf, auto sp_c) {
        constexpr int sp = decltype(sp_c)::value;
        static_for<0, TO>([&](auto i_c) {
            constexpr int i = decltype(i_c)::value;
            x16_tr_issue<i * 2 * X16_PIECE + sp * 1024>(hf.a[i][0], buf + wo * TO * 2 * X16_PIECE);
            x16_tr_issue<i * 2 * X16_PIECE + sp * 1024 + 256>(hf.a[i][1], buf + wo * TO * 2 * X16_PIECE);
        });
        static_for<0, TI>([&](auto j_c) {
            constexpr int j = decltype(j_c)::value;
            x16_tr_issue<(2 * NA + j * 2) * X16_PIECE + sp * 1024>(hf.b[j][0], buf + wi * TI * 2 * X16_PIECE);
            x16_tr_issue<(2 * NA + j * 2) * X16_PIECE + sp * 1024 + 256>(hf.b[j][1], buf + wi * TI * 2 * X16_PIECE);
        });
    };
    auto pin_half = [&](Half& hf) {  // the destinations stay reserved up to the wait (x16_tr_settle)
#pragma unroll
        for (int i = 0; i < TO; ++i) asm volatile("" : "+v"(hf.a[i][0]), "+v"(hf.a[i][1]));
#pragma unroll
        for (int j = 0; j < TI; ++j) asm volatile("" : "+v"(hf.b[j][0]), "+v"(hf.b[j][1]));
    };
    auto mfma_half = [&](const Half& hf) {
        bf16x8 fa[TO], fb[TI];
#pragma unroll
        for (int i = 0; i < TO; ++i) fa[i] = __builtin_bit_cast(bf16x8, x16_u32x4{hf.a[i][0][0], hf.a[i][0][1], hf.a[i][1][0], hf.a[i][1][1]});
#pragma unroll
        for (int j = 0; j < TI; ++j) fb[j] = __builtin_bit_cast(bf16x8, x16_u32x4{hf.b[j][0][0], hf.b[j][0][1], hf.b[j][1][0], hf.b[j][1][1]});
#pragma unroll
        for (int i = 0; i < TO; ++i)
#pragma unroll
            for (int j = 0; j < TI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        if (do_rs) {
#pragma unroll
            for (int i = 0; i < TO; ++i) {
                float t = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) t += (float)fa[i][j];
                rs[i] += t;
            }
        }
    };
    // Stage s has landed when at most the loads of the younger stages in flight are outstanding (loads return in order);
    // near the end fewer stages follow: wait for everything (uniform branch).  Then everyone's pieces of it are visible and
    // everyone has left the buffer the next issue() refills.  A raw s_barrier: __syncthreads() carries a workgroup release
    // fence, for which hipcc waits vmcnt(0) -- i.e. for EVERY stage of the LDS-DMA stream in flight, not just stage s: the
    // ring was one stage deep whatever NBUF said (seen in the ISA).
    auto stage_ready = [&](const long st) {
        // (wait and barrier in ONE asm statement: as separate statements hipcc is free to schedule scalar address arithmetic
        //  between them -- harmless, but the ISA gate looks for the wait right in front of the barrier)
        if (st + NBUF - 2 >= b1) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        else if (full) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"((NBUF - 2) * PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"((NBUF - 2) * (PPW - 1)) : "memory");
        asm volatile("" ::: "memory");
    };
    auto buf_of = [&](const long st) { return lds_base + (unsigned)(st % NBUF) * STAGE + tr_off; };
    // The tiles sit in LDS as the producers stored them ([sample][channel] images, x16_core.h); the transposed reads hand
    // every lane 8 samples of one channel -- the operand form of a product over samples.
    // SOFTWARE PIPELINE over half blocks: the reads of the NEXT half (96 KiB of LDS traffic per block and workgroup) are in
    // flight under the 9 MFMAs per wave of the CURRENT half.  In the first version every wave read a whole block, waited, then
    // multiplied -- all eight waves in step behind the stage barrier, so the CU alternated between an LDS phase and an MFMA
    // phase (~1.5 us per block against 0.6 us of MFMA time; the launch was bound by that sequence, not by HBM: removing 22 %
    // of its fetches changed nothing).  Same registers: two halves in flight instead of one block.
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i)
        if (b0 + i < b1) issue(b0 + i);
    const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11)) & (DW_XCDS - 1);  // HW_REG_XCC_ID, bits 3:0 (see the epilogue)
#pragma unroll
    for (int i = 0; i < TO; ++i) {
        rs[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < TI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    }
    do_rs = a.rowsum != nullptr && iy == 0 && wi == 0;
    Half cur, nxt;
#ifdef N3DT_DW_STAMPS
    unsigned long long st_sum[7] = {0, 0, 0, 0, 0, 0, 0}, st_prev = 0, st_begin;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_begin)::"memory");
#endif
    stage_ready(b0);
    if (b0 + NBUF - 1 < b1) issue(b0 + NBUF - 1);
    read_half(cur, buf_of(b0), std::integral_constant<int, 0>{});
    x16_tr_settle();
    pin_half(cur);
    for (long b = b0; b < b1; ++b) {
        if (PACE && pace_mine && wave == 0) {
            const unsigned mine = (unsigned)(b - b0);
            if ((mine & 3u) == 1u) {  // the value requested at the previous multiple of four has landed (the settle below waited)
                const int lead = (int)mine - (int)other_progress - DW_PACE_LEAD;
                if (lead > 0) {
                    const int n = lead < DW_PACE_SLEEPS ? lead : DW_PACE_SLEEPS;
                    for (int k = 0; k < n; ++k) __builtin_amdgcn_s_sleep(8);  // 8 x 64 cycles = ~0.25 us each
                }
            }
            if ((mine & 3u) == 0u) {
                if (lane == 0) __hip_atomic_store(pace_mine, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_load_dword %0, %1, 0x0 glc" : "=s"(other_progress) : "s"(pace_other) : "memory");
            }
        }
        // second half of block b on its way; first half through the matrix pipe
        DW_STAMP(0)
        read_half(nxt, buf_of(b), std::integral_constant<int, 1>{});
        mfma_half(cur);
        x16_tr_settle();
        pin_half(nxt);
        DW_STAMP(1)
        // block b + 1: landed and visible, the buffer of block b free for stage b + NBUF (every wave has settled its reads of it)
        const bool more = b + 1 < b1;
        if (more) {
            stage_ready(b + 1);
            DW_STAMP(2)
            if (b + NBUF < b1) issue(b + NBUF);
            DW_STAMP(3)
        }
        // first half of block b + 1 on its way (the last block re-reads its own buffer: the read is unconditional, because a
        // fragment defined under a branch becomes a phi and hipcc copies its not-yet-landed registers ahead of the wait)
        read_half(cur, buf_of(more ? b + 1 : b), std::integral_constant<int, 0>{});
        mfma_half(nxt);
        x16_tr_settle();
        pin_half(cur);
        DW_STAMP(4)
    }
    // Combine across slices.  Device-scope fp32 atomics from 256 workgroups onto one 384 x 384 result cost 60-70 us of a
    // 250 us launch (measured by disabling them): the eight XCDs' L2s are not coherent with each other, so those atomics
    // are served at the memory side.  Instead every XCD accumulates into ITS OWN partial buffer with atomics that stay in
    // its L2 (all workgroups of an XCD share that one L2), picked by the hardware XCC id -- not by an assumed dispatch order, so a
    // different workgroup-to-XCD mapping cannot make two L2s own the same buffer.  The kernel boundary writes the L2s
    // back; dw_reduce_kernel then adds the eight partials into the gradient.
    // The atomics are written with AGENT scope (formally race-free under the HIP memory model, ADVICE r2).  That costs
    // nothing: for a relaxed, non-returning fp32 RMW hipcc emits the same `global_atomic_add_f32 v, v, off` -- no sc0 / sc1
    // bit -- at workgroup and at agent scope (checked in build/train_mlp.s), so what made the difference measured above was
    // never the scope but the eight-fold spread of the same-address traffic.  XCC_ID names the XCC a wave runs on in every
    // partition mode of this part (SPX: 0..7; DPX / QPX: 0..3 / 0..1; CPX: one XCC per device, id 0): `& 7` never aliases,
    // and whichever buffer a workgroup picks, the sum over the eight buffers is the gradient.
    float* const part = a.part + (size_t)xcc * a.rows_valid * a.cols_valid;
#pragma unroll
    for (int i = 0; i < TO; ++i) {
        const int to = oy * NA + wo * TO + i;
        if (to >= a.nA) continue;
#pragma unroll
        for (int j = 0; j < TI; ++j) {
            const int ti = iy * NBT + wi * TI + j;
            if (ti >= a.nB) continue;
            const int col = ti * 32 + c;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = to * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < a.rows_valid && col < a.cols_valid)
                    __hip_atomic_fetch_add(part + (size_t)row * a.cols_valid + col, acc[i][j][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (do_rs) {
            const float t = rs[i] + __shfl_xor(rs[i], 32, 64);
            const int row = to * 32 + c;
            const int rrow = (RM && a.row_perm > 0) ? 4 * (row % a.row_perm) + row / a.row_perm : row;
            if (h == 0 && row < a.rows_valid) atomicAdd(a.rowsum + (size_t)f * a.rs_stride + rrow, t);
        }
    }
#ifdef N3DT_DW_STAMPS
    DW_STAMP(5)  // epilogue issued
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    DW_STAMP(6)  // ... and drained
    if (TO == 3 && TI == 3 && blockIdx.x == 9 && lane == 0)
        printf("dw stamps wave %d blocks %ld: half0 %llu ready %llu issue %llu half1 %llu | epilogue issue %llu drain %llu | whole %llu\n", wave,
               (long)(b1 - b0), st_sum[1], st_sum[2], st_sum[3], st_sum[4], st_sum[5], st_sum[6], st_prev - st_begin);
#endif
}

template <int WO, int WI, int TO, int TI, bool RM = false>
__global__ __launch_bounds__(512, 1) void dw_x16_kernel(DwArgs a) {
    dw_x16_body<WO, WI, TO, TI, RM>(a);
}
// Several weight-gradient products of one shape in ONE launch, as one flat, XCD-balanced list of workgroups: the seven 384 x 384
// hidden layers used to be seven launches of 256 workgroups, each ending in its atomic phase with the HBM idle; in one grid the
// workgroups of the next product stream while the previous one's atomics drain (different resources: L2 atomics vs HBM).
// Workgroup L runs on XCD L % 8 whatever the grid's shape (the dispatcher deals workgroup ids round-robin over the eight XCDs), so a
// (workgroups, products) grid balances the XCDs only when the real workgroups of EVERY product are a multiple of 8 x gy: with the
// slice count padded to a multiple of 8 the padding lands on the same XCDs in every product (36 workgroups per product = 18
// slices: XCDs 0 and 1 get 42 workgroups, the others 28 -- two rounds on a quarter of the chip).  Here unit k (a pair of column
// halves when gy = 2, else one workgroup) of the n x slices units goes to XCD k % 8:
// L = 16 (k / 8) + 8 y + k % 8 (gy = 2) or L = k (gy = 1); every XCD gets the same number of real workgroups to within one unit, and
// the two halves of a pair still sit 8 ids apart on one XCD.  With that, ONE round of long slices is possible: a workgroup's
// fixed cost (first stages, 144 atomic instructions per wave: ~45 k cycles, 16 % of a 128-block slice) is paid once per CU
// instead of seven times.
#define DW_MULTI_MAX 8
struct DwArgsN {
    DwArgs a[DW_MULTI_MAX];
    int n;
};
template <int WO, int WI, int TO, int TI, bool PACE>
__global__ __launch_bounds__(512, 1) void dw_x16_flat_kernel(DwArgsN m) {
    const int L = blockIdx.x;
    const int gy = m.a[0].gy;  // 1 or 2
    const int k = gy == 2 ? (L >> 4) * 8 + (L & 7) : L;
    const int y = gy == 2 ? (L >> 3) & 1 : 0;
    const int total = m.a[0].slices_per_frame * m.a[0].frames;
    if (k >= m.n * total) return;
    dw_x16_body<WO, WI, TO, TI, false, PACE>(m.a[k / total], y, k % total);
}

// n products of the same shape (and therefore the same plan) in one launch.  GY: the workgroups that share a slice, i.e. the
// products' tiles over a workgroup's -- 2 for 12 x 12 tiles in 12 x 6, 1 for 12 x 2 in 12 x 2; the flat kernel knows no other.
template <int WO, int WI, int TO, int TI, int GY>
static void launch_dw_multi(const N3dtGeom* g, const DwArgs* list, int n, hipStream_t s) {
    static_assert(GY == 1 || GY == 2, "one workgroup per slice, or a paced pair");
    constexpr int NA = WO * TO, NBT = WI * TI, NPP = (2 * (NA + NBT) + 7) / 8 * 8, gy = GY;
    const int bpf = g->n_rays * ((g->n_samples + 31) / 32), B = g->batch;
    const size_t lds_bytes = (size_t)DW_NBUF(NPP) * NPP * X16_PIECE;
    // slices per frame: the count that minimises rounds x (blocks per slice x cycles per block + a workgroup's fixed cost);
    // a round = 256 workgroups, one per CU (measured, in-kernel stamps: ~2 450 cycles per block, ~45 000 per workgroup)
    int best = 1;
    double best_t = 1e30;
    const int max_spf = bpf / 8 > 1 ? bpf / 8 : 1;
    for (int spf = 1; spf <= max_spf && (long)n * B * spf * gy <= 8 * 256; ++spf) {
        const long units = (long)n * B * spf, wg = units * gy;
        const long rounds = (wg + 255) / 256;
        const double t = (double)rounds * ((double)((bpf + spf - 1) / spf) * 2450.0 + 45000.0);
        if (t < best_t * 0.995) best_t = t, best = spf;   // (ties go to the smaller count: fewer atomics)
    }
    DwArgsN m;
    m.n = n;
    for (int i = 0; i < n; ++i) {
        m.a[i] = list[i];
        m.a[i].blocks_per_frame = bpf;
        m.a[i].slices_per_frame = best;
        m.a[i].frames = B;
        m.a[i].gy = gy;
    }
    const long units = (long)n * B * best;
    const int grid = gy == 2 ? (int)((units + 7) / 8) * 16 : (int)units;
    // Paced where two workgroups share a slice: a pair walks ~900 blocks and drifts apart completely without it (FETCH_SIZE 8.30 GB =
    // 1.47x the algorithmic bytes: no sharing at all); paced it fetches 6.51 GB (1.15x) in the same time -- 1.8 GB of HBM reads per
    // step for nothing.  (In the same time: the kernel is bound by its per-block sequence, not by HBM bytes.)
    auto fk = dw_x16_flat_kernel<WO, WI, TO, TI, GY == 2>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(fk, dim3(grid), dim3(512), lds_bytes, s, m);
}

// Slices of a single-product launch: about one workgroup per CU in total (the fp32 atomics that combine the slices cost ~0.1 ms
// per launch per extra 256 workgroups), at least 8 blocks per slice.  Fills the plan in; returns the grid (slices padded to 8, x gy).
static int dw_plan_slices(DwArgs& a, int blocks_per_frame, int frames, int gy) {
    int spf = (256 + frames * gy - 1) / (frames * gy);
    if (spf > blocks_per_frame / 8) spf = blocks_per_frame / 8;
    if (spf < 1) spf = 1;
    a.blocks_per_frame = blocks_per_frame;
    a.slices_per_frame = spf;
    a.frames = frames;
    a.gy = gy;
    return (spf * frames + 7) / 8 * 8 * gy;
}
template <int WO, int WI, int TO, int TI>
static void launch_dw(const N3dtGeom* g, DwArgs a, hipStream_t s) {
    constexpr int NA = WO * TO, NBT = WI * TI, NPP = (2 * (NA + NBT) + 7) / 8 * 8;
    const int gy = ((a.nA + NA - 1) / NA) * ((a.nB + NBT - 1) / NBT);
    const int grid = dw_plan_slices(a, g->n_rays * ((g->n_samples + 31) / 32), g->batch, gy);
    const size_t lds_bytes = (size_t)DW_NBUF(NPP) * NPP * X16_PIECE;
    auto kern = dw_x16_kernel<WO, WI, TO, TI>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds_bytes, s, a);
}

// out[row][col] += sum over the XCDs' partial buffers, for every weight-gradient launch of the step in one pass
struct DwReduce {
    const float* part[DW_MAX_LAUNCHES];
    float* out[DW_MAX_LAUNCHES];
    long ld[DW_MAX_LAUNCHES];
    int rows[DW_MAX_LAUNCHES], cols[DW_MAX_LAUNCHES];
    int perm[DW_MAX_LAUNCHES];  // row_perm of the product (0: rows as they are)
    int n;
};
__global__ __launch_bounds__(256) void dw_reduce_kernel(DwReduce d) {
    const int e = blockIdx.y;
    if (e >= d.n) return;
    const int rows = d.rows[e], cols = d.cols[e];
    const size_t n = (size_t)rows * cols;
    const float* p = d.part[e];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float acc = 0.0f;
#pragma unroll
        for (int x = 0; x < DW_XCDS; ++x) acc += p[(size_t)x * n + i];
        int row = (int)(i / cols);
        const int col = (int)(i % cols);
        if (d.perm[e] > 0) row = 4 * (row % d.perm[e]) + row / d.perm[e];
        d.out[e][(size_t)row * d.ld[e] + col] += acc;
    }
}

// ---------------------------------------------------------------------------------------------
// Finishing: distribute the per-frame row sums and the merged-RGB / density rows.
//   rs_rgb[f][0:192] = db_m[f] (merged RGB bias), rs_rgb[f][192] = d b_density;  dwm[0:192] = dW_m, dwm[192] = d w_density
//   dfold[f][stage l] holds the per-frame row sums of dZ_l (l = 0..7)
// grid 1 x block 384
// ---------------------------------------------------------------------------------------------
__global__ void train16_finish_kernel(N3dtMlpParams p, N3dtMlpGrads gp, int B, int A, float* __restrict__ dfold,
                                      const float* __restrict__ rs_rgb, const float* __restrict__ dwm, float* __restrict__ dbm_out) {
    const int t = threadIdx.x;  // 384
    __shared__ float dbm[192];
    (void)A;
    (void)p;
    // plain (unfolded) biases: sum the frames
    const int plain[6] = {1, 2, 3, 4, 6, 7};
    for (int i = 0; i < 6; ++i) {
        float acc = 0.0f;
        for (int f = 0; f < B; ++f) acc += dfold[(size_t)f * N3DT_FOLD_STRIDE + n3dt_bias_offset(plain[i]) + t];
        gp.bias[plain[i]][t] += acc;
    }
    // density head
    gp.weight[8][t] += dwm[(size_t)192 * 384 + t];
    if (t == 0) {
        float acc = 0.0f;
        for (int f = 0; f < B; ++f) acc += rs_rgb[(size_t)f * 224 + 192];
        gp.bias[8][0] += acc;
    }
    // merged RGB bias: per frame into the folding table (train_fold_bwd_kernel turns it into d br1, d Wr1[:, 384:], d appea)
    if (t < 192) {
        float acc = 0.0f;
        for (int f = 0; f < B; ++f) {
            const float v = rs_rgb[(size_t)f * 224 + t];
            dfold[(size_t)f * N3DT_FOLD_STRIDE + n3dt_bias_offset(10) + t] = v;
            acc += v;
        }
        dbm[t] = acc;
    }
    __syncthreads();
    if (t < 192) dbm_out[t] = dbm[t];
}

// b_m = Wr1a br0 + ... :  d br0[j] = sum_o Wr1a[o][j] db_m[o] ;  dWr1a[o][j] += db_m[o] br0[j]      grid 192 (o), block 384 (j)
__global__ void train16_unmerge_bias_kernel(N3dtMlpParams p, N3dtMlpGrads gp, int A, const float* __restrict__ dbm) {
    const int o = blockIdx.x, j = threadIdx.x, inr = N3DT_HID + A;
    const float d = dbm[o];
    gp.weight[10][(size_t)o * inr + j] += d * p.bias[9][j];
    atomicAdd(&gp.bias[9][j], p.weight[10][(size_t)o * inr + j] * d);
}


// ---------------------------------------------------------------------------------------------
// Per-frame row sums of three stages of dZ straight from the saved tile images (frozen network: see n3dt_launch_train16_bwd):
//   stage 0: the merged RGB rows (tiles 0 .. 5 = 192 rows)     -> dfold[f][bias_offset(10) + row]
//   stage 1: dZ_5 (12 tiles)                                   -> dfold[f][bias_offset(5) + row]
//   stage 2: dZ_0 (12 tiles)                                   -> dfold[f][bias_offset(0) + row]
// A tile image is [32 samples][32 channels] 16-bit, 64-byte rows, channels of a row in the order
// [0-3, 8-11 | 4-7, 12-15 | 16-19, 24-27 | 20-23, 28-31] (x16_core.h): lane l reads the 16-byte unit l % 4 of rows l / 4 and
// 16 + l / 4.  grid (slices, 3, frames), block 256: wave w takes tiles w, w + 4, w + 8 of its stage over the slice's blocks.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dz_rowsum_kernel(const unsigned char* __restrict__ dzT, size_t strideZ, long blocks_per_frame, int slices,
                                                        float* __restrict__ dfold) {
    const int stage = blockIdx.y, f = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile0 = stage == 0 ? 0 : (stage == 1 ? 7 + 12 * 5 : 7), ntile = stage == 0 ? 6 : 12;
    const int out0 = n3dt_bias_offset(stage == 0 ? 10 : (stage == 1 ? 5 : 0));
    const long per = (blocks_per_frame + slices - 1) / slices;
    const long b0 = (long)f * blocks_per_frame + (long)blockIdx.x * per;
    const long b1 = min((long)(f + 1) * blocks_per_frame, b0 + per);
    float acc[3][8];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
    const size_t lane_off = (size_t)(lane >> 2) * 64 + (size_t)(lane & 3) * 16;
    for (long b = b0; b < b1; ++b) {
        const unsigned char* blk = dzT + (size_t)b * strideZ;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int t = wave + 4 * i;
            if (t < ntile) {
                const unsigned char* img = blk + (size_t)(tile0 + t) * 2 * X16_PIECE + lane_off;
                const bf16x8 r0 = *reinterpret_cast<const bf16x8*>(img), r1 = *reinterpret_cast<const bf16x8*>(img + X16_PIECE);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] += (float)r0[j] + (float)r1[j];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int t = wave + 4 * i;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = acc[i][j];
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lane < 4 && t < ntile) {
                const int k = lane;  // the row's 16-byte unit
                const int ch = 16 * (k >> 1) + 4 * (k & 1) + (j < 4 ? j : j + 4);
                atomicAdd(dfold + (size_t)f * N3DT_FOLD_STRIDE + out0 + 32 * t + ch, v);
            }
        }
    }
}
// include_vd: dL/d(ray_bias)[ray][row] = sum over the ray's blocks and samples of the merged RGB rows of dZ (tiles 0 .. 5).
// One wave per ray; tile image layout as dz_rowsum_kernel above.
__global__ __launch_bounds__(256) void dz_ray_rowsum_kernel(const unsigned char* __restrict__ dzT, size_t strideZ, int bpr, long n_rays_total,
                                                            float* __restrict__ d_ray_bias) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long ray = (long)blockIdx.x * 4 + wave;
    if (ray >= n_rays_total) return;
    const size_t lane_off = (size_t)(lane >> 2) * 64 + (size_t)(lane & 3) * 16;
    for (int t = 0; t < 6; ++t) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < bpr; ++b) {
            const unsigned char* img = dzT + (size_t)(ray * bpr + b) * strideZ + (size_t)t * 2 * X16_PIECE + lane_off;
            const bf16x8 r0 = *reinterpret_cast<const bf16x8*>(img), r1 = *reinterpret_cast<const bf16x8*>(img + X16_PIECE);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += (float)r0[j] + (float)r1[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = acc[j];
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lane < 4) {
                const int ch = 16 * (lane >> 1) + 4 * (lane & 1) + (j < 4 ? j : j + 4);
                d_ray_bias[(size_t)ray * N3DT_RAYFOLD_STRIDE + 32 * t + ch] = v;
            }
        }
    }
}
static void launch_dz_rowsum(const N3dtGeom* g, const unsigned char* dzT, size_t strideZ, int bpr, float* dfold, hipStream_t s) {
    const long bpf = (long)g->n_rays * bpr;
    int slices = (int)(512 / (3 * g->batch));
    if (slices > bpf / 4) slices = (int)(bpf / 4);
    if (slices < 1) slices = 1;
    hipLaunchKernelGGL(dz_rowsum_kernel, dim3(slices, 3, g->batch), dim3(256), 0, s, dzT, strideZ, bpf, slices, dfold);
}

// ---------------------------------------------------------------------------------------------
// orchestration
// ---------------------------------------------------------------------------------------------
// (n3dt_prof_span_begin / _end below: bench.py's measurement hook, n3dt_api.hip)
extern "C" void n3dt_launch_train16_fwd(const N3dtGeom* g, const N3dtMlpParams* p, const void* packed_bf16, const float* tail,
                                        const float* xy, const float* R, const float* T, const float* Kinv, const float* shape,
                                        const float* appea, const float* audio, const float* t_rand, const float* bg_featmap,
                                        float* fg_feat, float* bg_alpha, float* depth, float* merge_feat, void* saved, void* wsv,
                                        const float* ray_bias, hipStream_t s) {
    const Train16Saved sv = saved16_layout(g);
    const Train16Ws wl = ws16_layout(g);
    unsigned char* sb = reinterpret_cast<unsigned char*>(saved);
    unsigned char* ws = reinterpret_cast<unsigned char*>(wsv);
    float* fold = reinterpret_cast<float*>(sb + sv.fold);
    float* part = reinterpret_cast<float*>(ws + wl.part);
    float* wlocal = reinterpret_cast<float*>(ws + wl.wlocal);
    const int bpr = (g->n_samples + 31) / 32;
    n3dt_launch_fold(g, p, shape, appea, audio, fold, 1, s);
    if (ray_bias) n3dt_launch_rayfold(g, fold, ray_bias, s);  // include_vd: the merged RGB bias per ray
    // W_m = Wr1[:, 0:384] Wr0 was formed by n3dt_mlp_pack (fp32, in the packed buffer's tail): keep it for the backward, which
    // used to rebuild it with a 43 us product
    (void)hipMemcpyAsync(sb + sv.wm, tail + (size_t)N3DT_G * N3DT_C + N3DT_C, sizeof(float) * 192 * 384, hipMemcpyDeviceToDevice, s);
    const int span = n3dt_prof_span_begin(s);  // bench.py's measurement hook: span 1 of 3 of a training step
    n3dt_launch_nerf_fwd_x16_train(g, packed_bf16, fold, xy, R, T, Kinv, t_rand, part, wlocal, sb + sv.xT, sb + sv.gS,
                                   reinterpret_cast<float*>(sb + sv.geo), sb + sv.gates, s);
    n3dt_prof_span_end(span, s);
    n3dt_launch_ray_head_rec(g, bpr, 32, part, wlocal, tail, bg_featmap, fg_feat, bg_alpha, depth, reinterpret_cast<float*>(sb + sv.weight),
                             merge_feat, reinterpret_cast<float*>(sb + sv.ray), s);
}

extern "C" void n3dt_launch_train16_bwd(const N3dtGeom* g, const N3dtMlpParams* p, const N3dtMlpGrads* gp, const float* shape,
                                        const float* appea, const float* audio, const float* bg_featmap, const float* d_merge,
                                        const float* d_fg, const float* d_ba, const void* saved, float* d_bg_featmap, float* d_shape,
                                        float* d_appea, float* d_audio, const float* xy, const float* Rm, const float* Tv,
                                        const float* Kinv, const float* t_rand, float* d_R, float* d_T, float* d_Kinv, float* d_xy,
                                        void* wsv, float* d_ray_bias, hipStream_t s) {
    const Train16Saved sv = saved16_layout(g);
    const Train16Ws wl = ws16_layout(g);
    const unsigned char* sb = reinterpret_cast<const unsigned char*>(saved);
    unsigned char* ws = reinterpret_cast<unsigned char*>(wsv);
    const int S = g->shape_dim, A = g->appea_dim, U = g->audio_dim, B = g->batch;
    const long Rr = (long)B * g->n_rays;
    const int bpr = (g->n_samples + 31) / 32;
    const long blocks = t16_blocks(g);
    const float* rayrec = reinterpret_cast<const float*>(sb + sv.ray);
    const float* weight = reinterpret_cast<const float*>(sb + sv.weight);
    const float* geo = reinterpret_cast<const float*>(sb + sv.geo);
    const unsigned char* xT = sb + sv.xT;
    const unsigned char* gS = sb + sv.gS;
    unsigned char* packT = ws + wl.packT;
    unsigned char* dzT = ws + wl.dzT;
    float* dsig = reinterpret_cast<float*>(ws + wl.dsig);
    const bool cam = d_R || d_T || d_Kinv || d_xy;
    float* ddist = cam ? reinterpret_cast<float*>(ws + wl.ddist) : nullptr;
    float* dpe5 = reinterpret_cast<float*>(ws + wl.dpe5);
    float* dpe0 = reinterpret_cast<float*>(ws + wl.dpe0);
    float* dfg_total = reinterpret_cast<float*>(ws + wl.dfg);
    float* dgray = reinterpret_cast<float*>(ws + wl.dgray);
    float* dwsum = reinterpret_cast<float*>(ws + wl.dwsum);
    float* dfold = reinterpret_cast<float*>(ws + wl.dfold);
    float* rs_rgb = reinterpret_cast<float*>(ws + wl.rsrgb);
    float* dwm = reinterpret_cast<float*>(ws + wl.dwm);

    // every accumulator of this backward sits at the end of the workspace (dfold | rs_rgb | dW_m | the per-XCD partial weight
    // gradients): ONE memset; the three code gradients in one more when the caller allocated them side by side
    (void)hipMemsetAsync(ws + wl.dfold, 0, wl.total - wl.dfold, s);
    {
        float* const zp[3] = {d_shape, d_appea, U > 0 ? d_audio : nullptr};
        const size_t zc[3] = {(size_t)B * S, (size_t)B * A, (size_t)B * U};
        zero_runs(zp, zc, 3, s);
    }
    // the transposed stream packs W_m = Wr1[:, 0:384] Wr0 as the forward formed it (saved copy)
    hipLaunchKernelGGL(train16_pack_bwd_kernel, dim3(64, cam ? 10 : 8), dim3(256), 0, s, *p, S, U, cam ? 1 : 0,
                       reinterpret_cast<const float*>(sb + sv.wm), packT);
    // ---- head: RGB_layer_2 once per ray + merge (models.py:82, HeadNeRFNet.py:103-112)
    hipLaunchKernelGGL(train_head_bwd_kernel, dim3((unsigned)((Rr + HB_RAYS - 1) / HB_RAYS)), dim3(256), 0, s, *g, p->weight[11], p->bias[11], bg_featmap, d_merge,
                       d_fg, d_ba, dfg_total, dgray, dwsum, (long)Rr);
    if (gp || d_bg_featmap)
        hipLaunchKernelGGL(train_bg_b2_grad_kernel, dim3((g->n_rays + BG_RAYS - 1) / BG_RAYS), dim3(256), 0, s, *g, rayrec, d_merge, dfg_total, d_bg_featmap,
                           gp ? gp->bias[11] : nullptr);
    if (gp) {   // dW2[256][192] += dfg_total^T Gray
        Gemm32 q = mk(256, 192, (int)Rr, dfg_total, 256, 1, rayrec, N3DT_PART_STRIDE, 1, gp->weight[11], 192);
        long sp = Rr / 128;  // 4 output tiles: split the rays widely
        q.split_k = (int)(sp < 1 ? 1 : (sp > 128 ? 128 : sp));
        q.accumulate = q.split_k <= 1 ? 1 : 0;
        n3dt_gemm32(q, s);
    }
    // ---- compositing adjoint
    hipLaunchKernelGGL(train16_composite_bwd_kernel, dim3((unsigned)((Rr + 3) / 4)), dim3(256), 0, s, *g, bpr, gS, geo, weight, dgray,
                       dwsum, dsig, ddist);
    // ---- fused dX chain
    const int span_dx = n3dt_prof_span_begin(s);  // span 2 of 3
    {
        const size_t lds_bytes = (size_t)X16_NBUF * X16_CH * X16_PIECE + (size_t)T16_BWD_WAVES * T16_GATE_SLOT;  // ring + one gate-word slot per wave
        auto kern = cam ? nerf_bwd_x16_kernel<T16_BWD_WAVES, true> : nerf_bwd_x16_kernel<T16_BWD_WAVES, false>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL(kern, dim3((unsigned)((blocks + T16_BWD_WAVES - 1) / T16_BWD_WAVES)), dim3(T16_BWD_WAVES * 64), lds_bytes, s, *g, packT,
                           reinterpret_cast<const unsigned*>(sb + sv.gates), gS, weight, dsig, dgray, dzT, dpe5, dpe0, bpr, blocks);
    }
    n3dt_prof_span_end(span_dx, s);
    if (d_ray_bias)  // include_vd: per-ray sums of the merged RGB rows of dZ (the caller's autograd turns them into d W_vd, d R)
        hipLaunchKernelGGL(dz_ray_rowsum_kernel, dim3((unsigned)((Rr + 3) / 4)), dim3(256), 0, s, dzT, (size_t)T16_DZ_TILES * 2 * X16_PIECE, bpr, (long)Rr,
                           d_ray_bias);
    if (cam) {
        if (d_R) (void)hipMemsetAsync(d_R, 0, sizeof(float) * 9 * B, s);
        if (d_T) (void)hipMemsetAsync(d_T, 0, sizeof(float) * 3 * B, s);
        const int cr = n3dt_cam_rays_per_block(g->n_rays, B);
        auto ckern = (d_Kinv || d_xy) ? train16_camera_bwd_kernel<true> : train16_camera_bwd_kernel<false>;
        hipLaunchKernelGGL(ckern, dim3((g->n_rays + cr - 1) / cr, B), dim3(256), 0, s, *g, bpr, xy, Rm, Tv, Kinv, t_rand, dpe5,
                           dpe0, ddist, d_R, d_T, d_Kinv, d_xy, cr);
    }
    if (!gp) {
        // Frozen network (single-image fitting, FittingSingleImage_new.py:826-859: only codes and cameras are optimised): no weight
        // gradients.  The latent-code gradients still need the per-frame row sums of dZ_0, dZ_5 and of the merged RGB rows, which
        // otherwise ride on the weight-gradient kernels: one pass over those 31 of the 103 dZ tiles per block instead of the three
        // weight-gradient launches, their reduction and the un-merging (0.64 of a 2.6 ms fitting iteration at config 4's geometry).
        const size_t strideZ0 = (size_t)T16_DZ_TILES * 2 * X16_PIECE;
        launch_dz_rowsum(g, dzT, strideZ0, bpr, dfold, s);
        launch_fold_bwd(p, gp, S, A, U, B, shape, appea, audio, dfold, d_shape, d_appea, d_audio, s, /*codes_zeroed=*/true);
        return;
    }
    // ---- weight gradients (per-XCD partial sums, reduced once at the end: see dw_x16_body)
    const size_t strideX = (size_t)X16_XT_TILES * 2 * X16_PIECE, strideZ = (size_t)T16_DZ_TILES * 2 * X16_PIECE;
    float* dwpart = reinterpret_cast<float*>(ws + wl.dwpart);
    DwReduce red;
    red.n = 0;
    auto args = [&](int a_tile0, int nA, int b_tile0, int nB, float* out, long ld, int rows, int cols, float* rowsum, long rs_stride) {
        DwArgs a;
        a.A = dzT; a.strideA = strideZ; a.a_tile0 = a_tile0; a.nA = nA;
        a.B = xT; a.strideB = strideX; a.b_tile0 = b_tile0; a.nB = nB;
        a.out = out; a.ld = ld; a.rows_valid = rows; a.cols_valid = cols;
        a.part = dwpart + (size_t)red.n * DW_XCDS * 384 * 384;
        a.pace = reinterpret_cast<unsigned*>(ws + wl.pace) + (size_t)red.n * DW_PACE_SLOTS;
        red.part[red.n] = a.part; red.out[red.n] = out; red.ld[red.n] = ld; red.rows[red.n] = rows; red.cols[red.n] = cols;
        red.perm[red.n] = 0;
        ++red.n;
        a.rowmajor = 0; a.ldA = a.ldB = 0; a.a_plane_tiles = 0; a.a_plane_bytes = 0; a.row_perm = 0;
        a.rowsum = rowsum; a.rs_stride = rs_stride;
        a.blocks_per_frame = 0; a.slices_per_frame = 0; a.frames = 0; a.gy = 1;
        return a;
    };
    const int in0 = N3DT_PE_DIM + S + U, in5 = N3DT_PE_DIM + S + N3DT_HID;
    auto xh = [](int l) { return 2 + 12 * l; };   // H_l tiles in xT
    auto zl = [](int l) { return 7 + 12 * l; };   // dZ_l tiles in dzT
    // merged RGB (+ density row) against H7
    const int span_dw = n3dt_prof_span_begin(s);  // span 3 of 3: the three weight-gradient launches and their reduction
    launch_dw<2, 4, 4, 3>(g, args(0, 7, xh(7), 12, dwm, 384, 224, 384, rs_rgb, 224), s);
    {   // the seven 384 x 384 products (FeaExt_module_7 .. 1; module 5: its H4 columns) in one launch
        DwArgs hid[7];
        int n = 0;
        for (int l = 7; l >= 1; --l) {
            if (l == 5)
                hid[n++] = args(zl(5), 12, xh(4), 12, gp->weight[5] + N3DT_PE_DIM + S, in5, 384, 384, dfold + n3dt_bias_offset(5), N3DT_FOLD_STRIDE);
            else
                hid[n++] = args(zl(l), 12, xh(l - 1), 12, gp->weight[l], 384, 384, 384, dfold + n3dt_bias_offset(l), N3DT_FOLD_STRIDE);
        }
        launch_dw_multi<4, 2, 3, 3, 2>(g, hid, n, s);
    }
    // the PE columns of the skip layer and layer 0 (two products of one shape)
    {
        DwArgs pe[2] = {args(zl(5), 12, 0, 2, gp->weight[5], in5, 384, N3DT_PE_DIM, nullptr, 0),
                        args(zl(0), 12, 0, 2, gp->weight[0], in0, 384, N3DT_PE_DIM, dfold + n3dt_bias_offset(0), N3DT_FOLD_STRIDE)};
        launch_dw_multi<4, 2, 3, 1, 1>(g, pe, 2, s);
    }
    hipLaunchKernelGGL(dw_reduce_kernel, dim3(72, red.n), dim3(256), 0, s, red);
    n3dt_prof_span_end(span_dw, s);
    // ---- un-merge RGB_layer_0 / RGB_layer_1, density row, bias sums
    float* dbm = dwm + (size_t)193 * 384;  // rows 193.. of the scratch are unused
    hipLaunchKernelGGL(train16_finish_kernel, dim3(1), dim3(384), 0, s, *p, *gp, B, A, dfold, rs_rgb, dwm, dbm);
    hipLaunchKernelGGL(train16_unmerge_bias_kernel, dim3(192), dim3(384), 0, s, *p, *gp, A, dbm);
    // dWr1[o][j] += sum_c dW_m[o][c] Wr0[j][c]   (j < 384)
    n3dt_launch_small_gemm(192, 384, 384, dwm, 384, 1, p->weight[9], 384, 1, gp->weight[10], 384 + A, 1, s);
    // dWr0[j][c] += sum_o Wr1[o][j] dW_m[o][c]
    n3dt_launch_small_gemm(384, 384, 192, p->weight[10], 1, 384 + A, dwm, 1, 384, gp->weight[9], 384, 1, s);
    launch_fold_bwd(p, gp, S, A, U, B, shape, appea, audio, dfold, d_shape, d_appea, d_audio, s, /*codes_zeroed=*/true);
}

// ---------------------------------------------------------------------------------------------
// The same weight-gradient kernel for the 2-D renderer's row-major 16-bit maps (train_nr.hip, nr_bwd16): a batch of products
// out_e[rows_e][cols_e] += A_e^T B_e over M_e pixels, each with its own per-XCD partial buffer inside `part` (zeroed here by one
// memset), all reduced by ONE dw_reduce_kernel at the end.  Replaces the 2-byte-gather kernel (nrt_dw16_kernel) where the
// pixel count is a multiple of 32 and the operands are 16-bit: the gathers issue 48 loads per 8 MFMAs.
// ---------------------------------------------------------------------------------------------
#include "dw_rowmajor.h"
extern "C" size_t n3dt_dw_rowmajor_part_bytes(const N3dtDwRm* e, int n) {
    size_t b = 0;
    for (int i = 0; i < n; ++i) b += al256(sizeof(float) * (size_t)DW_XCDS * e[i].rows * e[i].cols);
    return b;
}
extern "C" bool n3dt_dw_rowmajor_ok(const N3dtDwRm* e) {
    return e->M % 32 == 0 && e->M >= 256 && e->rows % 32 == 0 && e->cols % 32 == 0 && e->ldA % 8 == 0 && e->ldB % 8 == 0 &&
           (e->rows / e->a_planes) % 32 == 0;
}
template <int WO, int WI, int TO, int TI>
static void launch_dw_rm(DwArgs a, long blocks, hipStream_t s) {
    constexpr int NA = WO * TO, NBT = WI * TI, NPP = (2 * (NA + NBT) + 7) / 8 * 8;
    const int gy = ((a.nA + NA - 1) / NA) * ((a.nB + NBT - 1) / NBT);
    const int grid = dw_plan_slices(a, (int)blocks, 1, gy);
    const size_t lds_bytes = (size_t)DW_NBUF(NPP) * NPP * X16_PIECE;
    auto kern = dw_x16_kernel<WO, WI, TO, TI, true>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds_bytes, s, a);
}
// zero every product's partial buffers (one memset) / launch product `index` / reduce them all into their outputs (one launch)
extern "C" void n3dt_launch_dw_rowmajor_zero(const N3dtDwRm* e, int n, float* part, hipStream_t s) {
    (void)hipMemsetAsync(part, 0, n3dt_dw_rowmajor_part_bytes(e, n), s);
}
extern "C" void n3dt_launch_dw_rowmajor_one(const N3dtDwRm* e, int index, float* part, hipStream_t s) {
    const N3dtDwRm& q = e[index];
    DwArgs a;
    a.A = reinterpret_cast<const unsigned char*>(q.A); a.strideA = 0; a.a_tile0 = 0; a.nA = q.rows / 32;
    a.B = reinterpret_cast<const unsigned char*>(q.B); a.strideB = 0; a.b_tile0 = 0; a.nB = q.cols / 32;
    a.out = q.out; a.ld = q.ld_out; a.rows_valid = q.rows; a.cols_valid = q.cols;
    a.part = part + n3dt_dw_rowmajor_part_bytes(e, index) / sizeof(float);
    a.rowsum = q.rowsum; a.rs_stride = 0;
    a.pace = nullptr;
    a.rowmajor = 1; a.ldA = q.ldA; a.ldB = q.ldB;
    a.a_plane_tiles = q.a_planes > 1 ? (q.rows / q.a_planes) / 32 : 0;
    a.a_plane_bytes = q.a_plane_elems * 2;
    a.row_perm = q.row_perm;
    a.blocks_per_frame = 0; a.slices_per_frame = 0; a.frames = 0; a.gy = 1;
    const long blocks = q.M / 32;
    if (a.nA <= 4 && a.nB <= 2) launch_dw_rm<4, 2, 1, 1>(a, blocks, s);
    else launch_dw_rm<4, 2, 2, 2>(a, blocks, s);
}
extern "C" void n3dt_launch_dw_rowmajor_reduce(const N3dtDwRm* e, int n, float* part, hipStream_t s) {
    DwReduce red;
    red.n = 0;
    for (int i = 0; i < n && i < DW_MAX_LAUNCHES; ++i) {
        red.part[i] = part + n3dt_dw_rowmajor_part_bytes(e, i) / sizeof(float);
        red.out[i] = e[i].out; red.ld[i] = e[i].ld_out; red.rows[i] = e[i].rows; red.cols[i] = e[i].cols; red.perm[i] = e[i].row_perm;
        ++red.n;
    }
    hipLaunchKernelGGL(dw_reduce_kernel, dim3(72, red.n), dim3(256), 0, s, red);
}
