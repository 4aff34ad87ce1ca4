// conv_net.h -- the launch functions of csrc/conv_net.hip: the weight pack, bias fold, layout, copy and pool kernels that the
// frozen convolutional networks (syncnet, wav2lip, s3fd, face_recon, fan, head_mask) share, each defined once (DESIGN section
// 3.22).  Plain C++ functions inside libn3dt.so, not part of the C ABI.  None of them is on a hot path: the packs run once per
// set of weights, the layouts at the two ends of a forward.
#ifndef N3DT_CONV_NET_H
#define N3DT_CONV_NET_H

#include <hip/hip_runtime.h>

// W [cout, wc, taps] -> B [K][np] in conv_frag.h's fragment order, hi then its lo part: row k = tap * cinp + ci, or with `stem`
// the flattened 7 x 7 x 3 order of conv_net_core.h's cn_stem_tap (wc >= 3, taps = 49, K = 160); zero for ci >= cin, n >= cout and
// the stem's rows from 147 on.  Each weight times gamma / sqrt(var + eps) of its column in float64 (gamma NULL: times 1), rounded
// once to fp32, then split.
void conv_net_pack(const float* W, const float* gamma, const float* var, double eps, int wc, int cin, int cinp, int cout, int np, int taps, int K,
                   int stem, __bf16* hi, __bf16* lo, hipStream_t st);

// dst [cout] = fp32((bias - mean) s + beta), s = gamma / sqrt(var + eps), float64: a convolution with a bias under a BatchNorm
void conv_net_bias_bn(const float* bias, const float* gamma, const float* beta, const float* mean, const float* var, double eps, int cout, float* dst,
                      hipStream_t st);
// dst [np] = fp32(beta - mean s): a convolution without a bias under a BatchNorm; 0 where gamma is NULL (no BatchNorm)
void conv_net_shift_bn(const float* gamma, const float* beta, const float* mean, const float* var, double eps, int np, float* dst, hipStream_t st);

// src [n, C, H, W] -> channels 0 .. Cp - 1 of dst [n, H + 2 pad, W + 2 pad, .] whose cells are dstride floats apart: zero in the halo
// and in channels C .. Cp - 1
void conv_net_to_nhwc(const float* src, int n, int C, int H, int W, int pad, int Cp, float* dst, int dstride, hipStream_t st);
// channels 0 .. C - 1 of src [n, H + 2 pad, W + 2 pad, .] whose cells are sstride floats apart -> dst [n, C, H, W]
void conv_net_to_nchw(const float* src, int sstride, int n, int C, int H, int W, int pad, float* dst, hipStream_t st);

void conv_net_copy(const float* src, size_t n, float* dst, hipStream_t st);

// in [n, Hi, Wi, C] -> out [n, cn_pool_out(Hi), cn_pool_out(Wi), C]: the 3 x 3 / 2 maximum over the taps inside the map, C % 4 == 0
void conv_net_max_pool(const float* in, int n, int Hi, int Wi, int C, float* out, hipStream_t st);

#endif
