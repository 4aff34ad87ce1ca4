// conv_mfma.h -- the inner machinery the implicit-GEMM convolutions share -- vgg_loss.hip, lpips.hip and the six frozen networks
// syncnet.hip, wav2lip.hip, s3fd.hip, face_recon.hip, fan.hip and head_mask.hip: one K step of 16 on v_mfma_f32_32x32x16_bf16 with
// fp32 operands split into two bf16s, and the small helpers around it (DESIGN sections 3.10 and 3.22).  Each family keeps its own
// kernel, argument struct, A-operand gather and epilogue; conv_net.hip holds the pack, layout and pool kernels the six share.
//
// The order of the products is a contract: the bitwise properties the tests assert (lpips(x, x) == 0, symmetry, batch-position
// independence, VGG's exactly zero loss and gradient for equal images, SyncNet's window-position independence) rest on every
// image meeting the same products in the same order, and that order is written here and nowhere else.  nerf_aux.hip's split
// products use another order (hi*hi, hi*lo, lo*hi) and are not this step.
#ifndef N3DT_CONV_MFMA_H
#define N3DT_CONV_MFMA_H

#include <hip/hip_runtime.h>

#include "conv_frag.h"
#include "conv_net_core.h"

typedef __bf16 conv_bf16x8 __attribute__((ext_vector_type(8)));
typedef float conv_f32x16 __attribute__((ext_vector_type(16)));

static inline size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }

// 1-D grid of 256-thread workgroups for a grid-stride loop over `work` items
static inline unsigned conv_grid(size_t work) {
    const size_t blocks = (work + 255) / 256;
    return (unsigned)(blocks < 65536 ? (blocks ? blocks : 1) : 65536);
}

__device__ __forceinline__ void conv_load8(const float* p, float* v) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    const float4 y = *reinterpret_cast<const float4*>(p + 4);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
}

// Zero the acc[2][NT] tiles.  A macro, not a function: through a function (tried: by reference, through a float pointer,
// whole-vector assignment) every conv kernel comes out with 8 to 20 more registers than with these loops in its own body
// (docs/tuning_log.md, 2026-10-19).
#define CONV_ZERO_ACC(acc, NT)                            \
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)      \
    _Pragma("unroll") for (int nt = 0; nt < (NT); ++nt)   \
    _Pragma("unroll") for (int i = 0; i < 16; ++i) (acc)[mt][nt][i] = 0.0f

// eval-mode BatchNorm2d's scale of column n, float64: gamma / sqrt(var + eps); 1 where the convolution has no BatchNorm behind it
// (gamma NULL).  The one definition every weight pack and bias fold uses.
__device__ __forceinline__ double conv_bn_scale(const float* gamma, const float* var, double eps, int n) {
    return gamma ? (double)gamma[n] / sqrt((double)var[n] + eps) : 1.0;
}

// the split x = hi + lo: hi = bf16(x), lo = conv_lo(x, hi); the A operand's in the step below and the weights' in the pack kernels
__device__ __forceinline__ __bf16 conv_lo(float x, __bf16 hi) { return (__bf16)(x - (float)hi); }

// One K step of 16: two 32-row A tiles (av: the 8 values of this lane's row, k = 16 s + 8 (lane >> 5) + j) against the 32-column
// tiles nt0 .. nt0 + NT - 1 of a packed B matrix np columns wide (conv_frag.h).  SPLIT: both operands split, and per tile the
// products lo*hi, hi*lo, hi*hi in that order; else hi*hi alone, and wlo is not read.  np is the argument struct's own field,
// taken by reference so that it is loaded here, behind the A split: passed by value, vgg_conv_kernel loads its arguments in
// another order and allocates its scalar registers differently (same log entry).
template <bool SPLIT, int NT>
__device__ __forceinline__ void conv_mma_step(const __bf16* whi, const __bf16* wlo, const int& np, int s, int nt0, int lane,
                                              const float (&av)[2][8], conv_f32x16 (&acc)[2][NT]) {
    conv_bf16x8 ahi[2], alo[2], bhi[NT], blo[NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const __bf16 h = (__bf16)av[mt][j];
            ahi[mt][j] = h;
            if (SPLIT) alo[mt][j] = conv_lo(av[mt][j], h);
        }
    const int ntiles = np >> 5;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const size_t f = cf_frag_group(s, ntiles, nt0, nt, lane);
        bhi[nt] = reinterpret_cast<const conv_bf16x8*>(whi)[f];
        if (SPLIT) blo[nt] = reinterpret_cast<const conv_bf16x8*>(wlo)[f];
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (SPLIT) {
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo[mt], bhi[nt], acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi[mt], blo[nt], acc[mt][nt], 0, 0, 0);
            }
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi[mt], bhi[nt], acc[mt][nt], 0, 0, 0);
        }
}

// ---- the wave's tile in the conv-net kernels ----------------------------------------------------------------
// Shared by the conv kernels of syncnet, s3fd, face_recon, fan and head_mask, whose instruction streams it leaves as they were;
// wav2lip looks its class up from the tile first and keeps its own decode.  The dense tap loop and the stem gather were tried as
// functions too and change the emitted code (docs/tuning_log.md, 2026-10-21): the kernels keep those loops in their bodies.
//
// 256 threads = 4 waves; wave tile t = 4 blockIdx.x + wave computes rows m0 .. m0 + CN_TILE_M - 1 of the M = n H W rows of the GEMM
// (the cells of n output maps of H x W) against the 32-column tiles nt0 .. nt0 + NT - 1 of the np, the column tile fastest: the
// waves of a workgroup share their rows where there are several column tiles.  idle: the tile lies past the last row; the kernels
// have no barriers, so such a wave may leave.  nt0 is a function the kernel calls behind the idle test, where the private copies
// formed it: formed in front of it, syncnet_conv_kernel comes out with two registers numbered the other way round.
struct ConvWaveTile {
    int lane, r, h, ntn;
    long long M, tile, m0;
    __device__ __forceinline__ bool idle() const { return m0 >= M; }
    __device__ __forceinline__ int nt0(int NT) const { return (int)(tile % ntn) * NT; }
};

template <int NT>
__device__ __forceinline__ ConvWaveTile conv_wave_tile(int np, int n, int H, int W) {
    ConvWaveTile t;
    t.lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    t.r = t.lane & 31;
    t.h = t.lane >> 5;
    t.M = (long long)n * H * W;
    t.ntn = np / (32 * NT);
    t.tile = (long long)blockIdx.x * 4 + wave;
    t.m0 = t.tile / t.ntn * CN_TILE_M;
    return t;
}

__device__ __forceinline__ double conv_wave_sum(double v) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);  // a butterfly: every lane ends with the same bits
    return v;
}

#endif
