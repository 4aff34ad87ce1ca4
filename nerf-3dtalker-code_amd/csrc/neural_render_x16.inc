// 2-D neural renderer, 16-bit path (bf16 or f16 activations in HBM, MFMA with fp32 accumulate).
// Same mathematics as neural_render.hip (reference: NetWorks/neural_renderer.py:72-91,
// NetWorks/PixelShuffleUpsample.py:36-45), re-arranged for HBM traffic, which is what bounds it:
//   * every intermediate map is stored 16-bit;
//   * pixel-shuffle + residual is the second GEMM's store-address permutation (columns walked in
//     shuffled order, so a half-wave stores one output pixel's contiguous channels);
//   * the Blur after the shuffle is commuted past the next 1x1 conv (both are linear and act on
//     different axes): feat_layers runs on the un-blurred map and the blur is applied to its HALF-width
//     output, fused with the bias, LeakyReLU and the feat_2_rgb projection in one stencil kernel.
// The RGB skip pyramid stays planar fp32.
// (included by neural_render.hip)

typedef __bf16 hx_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int PREC>
__device__ __forceinline__ unsigned short f2h(float v) {
    if (PREC == N3DT_BF16) return __builtin_bit_cast(unsigned short, (__bf16)v);
    return __builtin_bit_cast(unsigned short, (_Float16)v);
}
template <int PREC>
__device__ __forceinline__ float h2f(unsigned short u) {
    if (PREC == N3DT_BF16) return __builtin_bit_cast(float, (unsigned)u << 16);
    return (float)__builtin_bit_cast(_Float16, u);
}

#define HG_BM 128
#define HG_BN 128
#define HG_BK 32
#define HG_LD (HG_BK + 8)  // 80-byte LDS rows: the 16-byte fragment reads spread over the banks

#define HEPI_PLAIN 0  // y[m][n] = act(acc + bias)
#define HEPI_PSU 1    // y(shuffled) = lrelu(acc + bias) + x.repeat(1,4,1,1)
#define HEPI_GATE 2   // training backward: y[m][n] = acc * lrelu'(res[m][n])   (res = the forward activation, 16-bit [M][N])
#define HEPI_ADD 3    // training backward: y[m][n] = acc + res[m][n]           (res 16-bit [M][N])

struct HGemm {
    unsigned short* y;
    const void* res;   // HEPI_PSU: block input x [M][C], fp32 (RES16 = false) or 16-bit
    int C, H, W;       // HEPI_PSU: channels and resolution of x (N == 4C, M == nb*H*W)
    float slope;       // LeakyReLU slope, < 0: identity
    int has_bias;
    int cshift;        // log2(C) (C is a power of two: featmap_nc == 256 halved per stage, floor 32)
    int wshift, hshift;  // log2(W), log2(H) when both are powers of two, else -1 (index math falls back to divisions)
    // MULTI (training backward): the A operand is the row-wise concatenation of up to five 16-bit matrices -- region r covers
    // k in [xr_k0[r], xr_k0[r+1]) and is stored [M][xr_ld[r]] at xr_base[r] (the four sub-pixel planes of a gradient, or
    // d_t1 followed by the planes of d_hid).  Region widths are multiples of HG_BK.
    const unsigned short* xr_base[5];
    int xr_k0[6];
    int xr_ld[5];
    int xr_n;
};

// Index decompositions of the pixel-shuffle epilogue.  They used to be runtime integer divisions (~35 VALU operations
// each, 80 per thread and tile: the second PixelShuffleUpsample GEMM spent 3 300 VALU instructions per wave on them and
// was VALU-bound at 1.7 TB/s); with power-of-two extents they are shifts and masks.
__device__ __forceinline__ int hg_shuffled_col(const HGemm& ea, const int n) {  // 4 * (n % C) + n / C
    return 4 * (n & (ea.C - 1)) + (n >> ea.cshift);
}
__device__ __forceinline__ void hg_pixel(const HGemm& ea, const int m, int& w, int& hh, int& img) {
    if (ea.wshift >= 0) {
        w = m & (ea.W - 1);
        hh = (m >> ea.wshift) & (ea.H - 1);
        img = m >> (ea.wshift + ea.hshift);
    } else {
        w = m % ea.W;
        hh = (m / ea.W) % ea.H;
        img = m / (ea.W * ea.H);
    }
}
static inline int hg_log2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}

// (MULTI -- the training backward's instantiations -- fits 128 registers without a spill: four waves per SIMD instead of the three
//  hipcc settles for unasked; the others spill 1 - 33 registers under that cap and keep their 148 - 156)
template <int EPI, int PREC, bool IN16, bool RES16, bool MULTI = false>
__global__ __launch_bounds__(256, MULTI ? 4 : 1) void gemm_h_kernel(int M, int N, int K, const void* __restrict__ Xv, const float* __restrict__ Wt,
                                                     const float* __restrict__ bias, HGemm ea) {
    static_assert(!MULTI || IN16, "the multi-region A operand is 16-bit");
    __shared__ __attribute__((aligned(16))) unsigned short smem[(HG_BM + HG_BN) * HG_LD];
    unsigned short* As = smem;
    unsigned short* Bs = smem + HG_BM * HG_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // XCD-aware tile order: workgroup L (dispatch order: x fastest) runs on XCD L % 8.  The N tiles of one 128-row slab of
    // the activation map get ids 8 apart -- same XCD, dispatched together -- so the slab is read from HBM once and the
    // other N tiles hit that XCD's L2 (with the plain 2-D order the second N tile comes a whole grid row later).
    int mt = blockIdx.x, nt = blockIdx.y;
    if (gridDim.y > 1) {
        const int MT = gridDim.x, NT = gridDim.y, full = MT & ~7;
        const int L = blockIdx.y * MT + blockIdx.x;
        if (L < full * NT) {
            const int r = L % (8 * NT);
            mt = (L / (8 * NT)) * 8 + (r & 7);
            nt = r >> 3;
        } else {
            const int Lt = L - full * NT, rem = MT - full;
            mt = full + Lt % rem;
            nt = Lt / rem;
        }
    }
    const int m0 = mt * HG_BM, n0 = nt * HG_BN;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    // Software pipeline: the global loads of k-step k+1 are issued before the MFMAs of k-step k and land in registers
    // while those run (one LDS buffer, two barriers per step; the loads no longer sit in front of a barrier).
    u16x8 a16[2];
    f32x4 a32[4];
    f32x4 bv[4];
    auto load_tile = [&](const int k0) {
        // A: 128 rows x 32 k.  16-bit input: 2 x 16-byte loads per thread; fp32 input: 4 x float4, converted when staged
        if (IN16) {
            const unsigned short* X = reinterpret_cast<const unsigned short*>(Xv);
            int ldx = K, kk = k0;
            if (MULTI) {  // (wave-uniform: scalar work)
                int r = 0;
                while (r + 1 < ea.xr_n && k0 >= ea.xr_k0[r + 1]) ++r;
                X = ea.xr_base[r];
                ldx = ea.xr_ld[r];
                kk = k0 - ea.xr_k0[r];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + 256 * i, row = idx >> 2, kq = idx & 3;
                a16[i] = (u16x8)(0);
                if (m0 + row < M) a16[i] = *reinterpret_cast<const u16x8*>(X + (size_t)(m0 + row) * ldx + kk + 8 * kq);
            }
        } else {
            const float* X = reinterpret_cast<const float*>(Xv);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = tid + 256 * i, row = idx >> 3, kq = idx & 7;
                a32[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (m0 + row < M) a32[i] = *reinterpret_cast<const f32x4*>(X + (size_t)(m0 + row) * K + k0 + 4 * kq);
            }
        }
        // B: weights stay fp32 in HBM (tiny, L2-resident), converted while staging
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, kq = idx & 7;
            bv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            int n = n0 + row;
            if (n < N) {
                if (EPI == HEPI_PSU) n = hg_shuffled_col(ea, n);  // pixel-shuffled column order
                bv[i] = *reinterpret_cast<const f32x4*>(Wt + (size_t)n * K + k0 + 4 * kq);
            }
        }
    };
    load_tile(0);
    for (int k0 = 0; k0 < K; k0 += HG_BK) {
        __syncthreads();  // previous tile fully consumed
        if (IN16) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + 256 * i, row = idx >> 2, kq = idx & 3;
                *reinterpret_cast<u16x8*>(As + row * HG_LD + 8 * kq) = a16[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = tid + 256 * i, row = idx >> 3, kq = idx & 7;
                u16x4 v = {f2h<PREC>(a32[i][0]), f2h<PREC>(a32[i][1]), f2h<PREC>(a32[i][2]), f2h<PREC>(a32[i][3])};
                *reinterpret_cast<u16x4*>(As + row * HG_LD + 4 * kq) = v;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, kq = idx & 7;
            u16x4 v = {f2h<PREC>(bv[i][0]), f2h<PREC>(bv[i][1]), f2h<PREC>(bv[i][2]), f2h<PREC>(bv[i][3])};
            *reinterpret_cast<u16x4*>(Bs + row * HG_LD + 4 * kq) = v;
        }
        __syncthreads();
        if (k0 + HG_BK < K) load_tile(k0 + HG_BK);
#pragma unroll
        for (int ks = 0; ks < HG_BK / 16; ++ks) {
            u16x8 af[2], bf[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                af[t] = *reinterpret_cast<const u16x8*>(As + (wr * 64 + t * 32 + (lane & 31)) * HG_LD + 16 * ks + 8 * (lane >> 5));
                bf[t] = *reinterpret_cast<const u16x8*>(Bs + (wc * 64 + t * 32 + (lane & 31)) * HG_LD + 16 * ks + 8 * (lane >> 5));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (PREC == N3DT_BF16)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(hx_bf16x8, af[i]),
                                                                            __builtin_bit_cast(hx_bf16x8, bf[j]), acc[i][j], 0, 0, 0);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[i]),
                                                                           __builtin_bit_cast(f16x8, bf[j]), acc[i][j], 0, 0, 0);
                }
        }
    }
    // Epilogue through LDS: the accumulator layout has the output column on the lane, so direct stores would be
    // 2 bytes per lane; instead each wave stages its 32 x 64 half-tile as [row][col] 16-bit and writes 16-byte chunks.
    __syncthreads();  // every wave is done with As / Bs
    constexpr int SLD = 72;  // halves per staged row (64 + 8 pad)
    unsigned short* stg = smem + wave * 32 * SLD;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wc * 64 + j * 32 + (lane & 31);
            int o = n;
            if (EPI == HEPI_PSU) o = hg_shuffled_col(ea, n);
            const float bn = (ea.has_bias && n < N) ? bias[o] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                float v = acc[i][j][reg] + bn;
                if (ea.slope >= 0.0f) v = fmaxf(v, v * ea.slope);  // LeakyReLU, 0 <= slope < 1
                stg[r * SLD + j * 32 + (lane & 31)] = f2h<PREC>(v);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int chunk = it * 64 + lane, r = chunk >> 3, c8 = chunk & 7;
            const int m = m0 + wr * 64 + i * 32 + r, n = n0 + wc * 64 + 8 * c8;
            if (m >= M || n >= N) continue;
            u16x8 v = *reinterpret_cast<const u16x8*>(stg + r * SLD + 8 * c8);
            if (EPI == HEPI_PLAIN) {
                *reinterpret_cast<u16x8*>(ea.y + (size_t)m * N + n) = v;
            } else if (EPI == HEPI_GATE || EPI == HEPI_ADD) {
                const u16x8 rv = *reinterpret_cast<const u16x8*>(reinterpret_cast<const unsigned short*>(ea.res) + (size_t)m * N + n);
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const float a = h2f<PREC>(v[t]), r = h2f<PREC>(rv[t]);
                    v[t] = f2h<PREC>(EPI == HEPI_ADD ? a + r : (r > 0.0f ? a : 0.2f * a));
                }
                *reinterpret_cast<u16x8*>(ea.y + (size_t)m * N + n) = v;
            } else {
                // pixel_shuffle(2): shuffled column n = q*C + c  ->  out[c, 2h+di, 2w+dj], q = 2di+dj
                const int c = n & (ea.C - 1), q = n >> ea.cshift, di = q >> 1, dj = q & 1;
                // + x.repeat(1,4,1,1): output channel c+t takes x[(4(c+t)+q) % C].  c is a multiple of 8, so the 8
                // sources sit at stride 4 inside ONE 32-channel block of the row: 64 contiguous bytes (16-bit x),
                // fetched as four 16-byte loads here instead of 64 two-byte gathers in the accumulator phase
                // (measured: the gathers tripled this GEMM's time)
                const int b0 = (4 * c) & (ea.C - 1);
                if (RES16) {
                    const unsigned short* xr = reinterpret_cast<const unsigned short*>(ea.res) + (size_t)m * ea.C + b0;
                    u16x8 x4[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) x4[u] = *reinterpret_cast<const u16x8*>(xr + 8 * u);
                    // element q + 4 (t & 1) of the 16-byte block t >> 1: dword (q >> 1) + 2 (t & 1), half q & 1 -- two selects
                    // (a compare-select chain over the 8 elements cost 14 VALU operations per value here)
                    const bool hi_dw = (q & 2) != 0, hi_half = (q & 1) != 0;
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const u32x4 blk = __builtin_bit_cast(u32x4, x4[t >> 1]);
                        const unsigned d = (t & 1) ? (hi_dw ? blk[3] : blk[2]) : (hi_dw ? blk[1] : blk[0]);
                        const unsigned short xv = (unsigned short)(hi_half ? (d >> 16) : (d & 0xFFFFu));
                        v[t] = f2h<PREC>(h2f<PREC>(v[t]) + h2f<PREC>(xv));
                    }
                } else {
                    const float* xr = reinterpret_cast<const float*>(ea.res) + (size_t)m * ea.C + b0 + q;
#pragma unroll
                    for (int t = 0; t < 8; ++t) v[t] = f2h<PREC>(h2f<PREC>(v[t]) + xr[4 * t]);
                }
                int w, hh, img;
                hg_pixel(ea, m, w, hh, img);
                *reinterpret_cast<u16x8*>(ea.y + (((size_t)img * 2 * ea.H + 2 * hh + di) * 2 * ea.W + 2 * w + dj) * ea.C + c) = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

__device__ __forceinline__ int hreflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// net = lrelu(Blur(hid) + b)  [16-bit out]  and  rgb (+)= feat_2_rgb(net)  [planar fp32], one thread = pixel x 8 channels
template <int PREC>
__global__ void blur_act_rgb_kernel(int nb, int H, int W, int K, const unsigned short* __restrict__ hid, const float* __restrict__ bias,
                                    unsigned short* __restrict__ net, const float* __restrict__ Wrgb, const float* __restrict__ brgb,
                                    const float* __restrict__ rgb_in, float* __restrict__ rgb_out, int final_sigmoid, int wshift) {
    extern __shared__ float wl[];  // [3][K] feat_2_rgb weights, then bias[K]
    for (int i = threadIdx.x; i < 3 * K; i += blockDim.x) wl[i] = Wrgb[i];
    for (int i = threadIdx.x; i < K; i += blockDim.x) wl[3 * K + i] = bias[i];
    __syncthreads();
    const int k8 = K / 8;  // threads per pixel: 16, 8 or 4 (K = 128, 64, 32) -- a power of two <= 64
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)nb * H * W * k8;
    const bool valid = i < total;
    if (!valid) i = total - 1;  // keep the lane for the shuffles below
    const int k8s = 31 - __builtin_clz(k8);
    const int kq = (int)(i & (k8 - 1));
    const size_t pix = i >> k8s;
    int w, h, img;
    if (wshift >= 0) {  // power-of-two resolution: no integer divisions on the hot path
        w = (int)(pix & (W - 1));
        h = (int)((pix >> wshift) & (H - 1));
        img = (int)(pix >> (2 * wshift));
    } else {
        w = (int)(pix % W);
        h = (int)((pix / W) % H);
        img = (int)(pix / ((size_t)W * H));
    }
    const float kk[3] = {0.25f, 0.5f, 0.25f};
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) {
            const int hh = hreflect1(h + di, H), ww = hreflect1(w + dj, W);
            const u16x8 v = *reinterpret_cast<const u16x8*>(hid + (((size_t)img * H + hh) * W + ww) * K + 8 * kq);
            const float wgt = kk[di + 1] * kk[dj + 1];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += wgt * h2f<PREC>(v[j]);
        }
    u16x8 out;
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v = acc[j] + wl[3 * K + 8 * kq + j];
        v = v > 0.0f ? v : 0.2f * v;
        out[j] = f2h<PREC>(v);
        const float vq = h2f<PREC>(out[j]);  // feat_2_rgb sees the stored (rounded) activation, like the next stage does
        r0 = fmaf(wl[8 * kq + j], vq, r0);
        r1 = fmaf(wl[K + 8 * kq + j], vq, r1);
        r2 = fmaf(wl[2 * K + 8 * kq + j], vq, r2);
    }
    if (valid && net) *reinterpret_cast<u16x8*>(net + pix * K + 8 * kq) = out;  // net == nullptr: last block, only the image is wanted
    for (int off = k8 >> 1; off > 0; off >>= 1) {
        r0 += __shfl_xor(r0, off, 64);
        r1 += __shfl_xor(r1, off, 64);
        r2 += __shfl_xor(r2, off, 64);
    }
    if (valid && kq == 0) {
        const size_t HW = (size_t)H * W, p = (size_t)h * W + w, o = (size_t)img * 3 * HW + p;
        r0 += brgb[0];
        r1 += brgb[1];
        r2 += brgb[2];
        if (rgb_in) {
            r0 += rgb_in[o];
            r1 += rgb_in[o + HW];
            r2 += rgb_in[o + 2 * HW];
        }
        if (final_sigmoid) {
            r0 = 1.0f / (1.0f + expf(-r0));
            r1 = 1.0f / (1.0f + expf(-r1));
            r2 = 1.0f / (1.0f + expf(-r2));
        }
        rgb_out[o] = r0;
        rgb_out[o + HW] = r1;
        rgb_out[o + 2 * HW] = r2;
    }
}

// The same stage for the sub-pixel-plane layout of the fused block kernel (hid [4][nb*H*W][K], H x W = the block's INPUT
// resolution): one thread = one input pixel x 8 channels = the 2 x 2 output pixels born from it.  Their four 3x3 stencils
// share a 4 x 4 neighbourhood, so 16 loads serve 4 outputs (the per-output kernel above issues 9 each) and the index
// arithmetic is done once.  Reflection (Blur pads by reflect, PixelShuffleUpsample.py:31) acts on OUTPUT coordinates.
template <int PREC>
__global__ __launch_bounds__(256) void blur_act_rgb_q_kernel(int nb, int H, int W, int K, const unsigned short* __restrict__ hid,
                                                             const float* __restrict__ bias, unsigned short* __restrict__ net,
                                                             const float* __restrict__ Wrgb, const float* __restrict__ brgb,
                                                             const float* __restrict__ rgb_lo, float* __restrict__ rgb_out, int final_sigmoid,
                                                             int wshift, float* __restrict__ rgb_out2 = nullptr) {
    // rgb_out2 (nullable): a second copy of the output (the training forward keeps the sigmoid image for the backward).
    // rgb_lo: the RGB pyramid at this block's INPUT resolution, planar [nb*3][H][W].  Its `rgb_upsample` (bilinear x2 + Blur,
    // neural_renderer.py:54-55,84) is evaluated here, per output pixel, as the 3 x 3 low-resolution taps of n3dt_up_blur_w3
    // in rgb_up_kernel's summation order -- the stand-alone upsample pass (write 4x, read 4x) is gone from the fused path.
    extern __shared__ float wl[];  // [3][K] feat_2_rgb weights, then bias[K]
    for (int i = threadIdx.x; i < 3 * K; i += blockDim.x) wl[i] = Wrgb[i];
    for (int i = threadIdx.x; i < K; i += blockDim.x) wl[3 * K + i] = bias[i];
    __syncthreads();
    const int k8 = K / 8;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t Mq = (size_t)nb * H * W, total = Mq * k8;
    const bool valid = i < total;
    if (!valid) i = total - 1;  // keep the lane for the shuffles below
    const int k8s = 31 - __builtin_clz(k8);
    const int kq = (int)(i & (k8 - 1));
    const size_t pix = i >> k8s;
    int w, h, img;
    if (wshift >= 0) {
        w = (int)(pix & (W - 1));
        h = (int)((pix >> wshift) & (H - 1));
        img = (int)(pix >> (2 * wshift));
    } else {
        w = (int)(pix % W);
        h = (int)((pix / W) % H);
        img = (int)(pix / ((size_t)W * H));
    }
    const int H2 = 2 * H, W2 = 2 * W;
    // Tap addresses.  The sub-pixel plane of a tap is a COMPILE-TIME constant: reflection preserves parity (hreflect1 maps i to -i
    // or 2n - 2 - i), so row tap rr sits in a plane of row parity (rr + 1) & 1 and column tap t in one of column parity (t + 1) & 1.
    // Plane bases are therefore wave-uniform (scalar registers) and a tap costs one 32-bit add of an in-plane row offset and an
    // in-plane column offset (the host keeps Mq * K below 2^31: run_x16).  (With the plane folded into 64-bit per-lane offsets
    // the sixteen taps cost ~70 64-bit adds and ~40 multiplies per thread.)
    unsigned coff[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) coff[t] = (unsigned)(hreflect1(2 * w - 1 + t, W2) >> 1) * K + 8 * kq;
    float acc[2][2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[a][b][j] = 0.0f;
    const size_t plane_elems = Mq * K;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = hreflect1(2 * h - 1 + rr, H2);
        const unsigned roff = ((unsigned)img * H + (unsigned)(r >> 1)) * W * K;
        float t4[4][8];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned short* pl = hid + (size_t)(2 * ((rr + 1) & 1) + ((t + 1) & 1)) * plane_elems;
            const u16x8 v = *reinterpret_cast<const u16x8*>(pl + (roff + coff[t]));
#pragma unroll
            for (int j = 0; j < 8; ++j) t4[t][j] = h2f<PREC>(v[j]);
        }
        // horizontal 1-2-1 for the two output columns, then into the output rows this input row feeds
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float h0 = t4[0][j] + 2.0f * t4[1][j] + t4[2][j], h1 = t4[1][j] + 2.0f * t4[2][j] + t4[3][j];
            const float w0 = rr == 0 ? 1.0f : (rr == 1 ? 2.0f : (rr == 2 ? 1.0f : 0.0f));  // weight in output row 2h
            const float w1 = rr == 1 ? 1.0f : (rr == 2 ? 2.0f : (rr == 3 ? 1.0f : 0.0f));  // ... in output row 2h+1
            if (rr < 3) {
                acc[0][0][j] = fmaf(w0, h0, acc[0][0][j]);
                acc[0][1][j] = fmaf(w0, h1, acc[0][1][j]);
            }
            if (rr > 0) {
                acc[1][0][j] = fmaf(w1, h0, acc[1][0][j]);
                acc[1][1][j] = fmaf(w1, h1, acc[1][1][j]);
            }
        }
    }
    const size_t HW2 = (size_t)H2 * W2;
    // rgb_upsample of the pyramid (bilinear x2 + Blur = 3 x 3 low-resolution taps, n3dt_up_blur_w3): lane kq < 3 of this pixel's
    // K / 8 >= 4 lanes evaluates CHANNEL kq for the four outputs (nine loads, the separable 3 x 3 form: 30 FMAs, every tap index a
    // compile-time constant), and the butterfly that sums the feat_2_rgb projection carries it.  (One lane doing all 27 loads made
    // the kernel 1.5x slower; spreading the nine TAPS over the lanes needed ~180 compares / selects per thread to pick a lane's
    // row and column weights.)
    float pyr[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    const float m0 = kq == 0 ? 1.0f : 0.0f, m1 = kq == 1 ? 1.0f : 0.0f, m2 = kq == 2 ? 1.0f : 0.0f;
    if (rgb_lo) {
        float wr[2][3], wc[2][3];
        n3dt_up_blur_w3(2 * h, H, wr[0]);
        n3dt_up_blur_w3(2 * h + 1, H, wr[1]);
        n3dt_up_blur_w3(2 * w, W, wc[0]);
        n3dt_up_blur_w3(2 * w + 1, W, wc[1]);
        const float* xp = rgb_lo + ((size_t)img * 3 + min(kq, 2)) * H * W;
        int ro[3], co[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            ro[a] = min(max(h - 1 + a, 0), H - 1) * W;
            co[a] = min(max(w - 1 + a, 0), W - 1);
        }
        float tmp[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const float v = xp[ro[a] + co[b]];
                tmp[0][b] = fmaf(wr[0][a], v, tmp[0][b]);
                tmp[1][b] = fmaf(wr[1][a], v, tmp[1][b]);
            }
#pragma unroll
        for (int di = 0; di < 2; ++di)
#pragma unroll
            for (int dj = 0; dj < 2; ++dj)
#pragma unroll
                for (int b = 0; b < 3; ++b) pyr[di][dj] = fmaf(wc[dj][b], tmp[di][b], pyr[di][dj]);
    }
#pragma unroll
    for (int di = 0; di < 2; ++di)
#pragma unroll
        for (int dj = 0; dj < 2; ++dj) {
            u16x8 out;
            float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = acc[di][dj][j] * 0.0625f + wl[3 * K + 8 * kq + j];
                v = fmaxf(v, 0.2f * v);  // LeakyReLU(0.2)
                out[j] = f2h<PREC>(v);
                const float vq = h2f<PREC>(out[j]);  // feat_2_rgb sees the stored (rounded) activation, like the next stage does
                r0 = fmaf(wl[8 * kq + j], vq, r0);
                r1 = fmaf(wl[K + 8 * kq + j], vq, r1);
                r2 = fmaf(wl[2 * K + 8 * kq + j], vq, r2);
            }
            const size_t p = (size_t)(2 * h + di) * W2 + (2 * w + dj);
            if (valid && net) *reinterpret_cast<u16x8*>(net + ((size_t)img * HW2 + p) * K + 8 * kq) = out;
            // this lane's share of the upsampled pyramid value (summed with the projection below): its channel's, lanes 0..2
            r0 = fmaf(m0, pyr[di][dj], r0);
            r1 = fmaf(m1, pyr[di][dj], r1);
            r2 = fmaf(m2, pyr[di][dj], r2);
            for (int off = k8 >> 1; off > 0; off >>= 1) {
                r0 += __shfl_xor(r0, off, 64);
                r1 += __shfl_xor(r1, off, 64);
                r2 += __shfl_xor(r2, off, 64);
            }
            if (valid && kq == 0) {
                const size_t o = (size_t)img * 3 * HW2 + p;
                r0 += brgb[0];
                r1 += brgb[1];
                r2 += brgb[2];
                if (final_sigmoid) {  // v_rcp_f32 (1 ulp) instead of an IEEE division: 2e-7 on a value in (0, 1)
                    r0 = __builtin_amdgcn_rcpf(1.0f + expf(-r0));
                    r1 = __builtin_amdgcn_rcpf(1.0f + expf(-r1));
                    r2 = __builtin_amdgcn_rcpf(1.0f + expf(-r2));
                }
                rgb_out[o] = r0;
                rgb_out[o + HW2] = r1;
                rgb_out[o + 2 * HW2] = r2;
                if (rgb_out2) {
                    rgb_out2[o] = r0;
                    rgb_out2[o + HW2] = r1;
                    rgb_out2[o + 2 * HW2] = r2;
                }
            }
        }
}

// to_rgb_kernel / rgb_up_kernel: shared with the fp32 path, defined above in neural_render.hip (this file is included there)

static inline int w_of(int h) { return h; }  // square maps
static inline int nr_ch16(int C, int i) {
    int v = C >> i;
    return v < 32 ? 32 : v;
}

#include "nr_fused_x16.inc"
#include "nr_blur_mfma.inc"

// floats reserved at the end of the renderer workspace for the packed weights of the fused blocks
static inline size_t nrf_pack_floats(const N3dtGeom* g) {
    size_t n = 0;
    for (int i = 0; i < g->n_blocks; ++i) {
        const int ci = nr_ch16(g->feat_nc, i), co = nr_ch16(g->feat_nc, i + 1);
        if (nrf_supported(ci, co)) n += (nrf_packed_bytes(ci, co) + 255) / 256 * 64;
    }
    return n;
}
static inline bool nrf_enabled() {
    static const int v = [] {
        const char* e = getenv("N3DT_NR_FUSED");
        return e ? atoi(e) : 1;
    }();
    return v != 0;
}

template <int PREC>
static void run_x16(const N3dtGeom* g, int nb, const N3dtRenderParams* p, const void* featmap, float* img, float* ws, size_t ws_floats,
                    const int pack_mode, hipStream_t s, const float* rgb0 = nullptr) {
    // rgb0 != nullptr: `featmap` is already the 16-bit map and rgb0 [nb][3][fs*fs] its level-0 projection (both from the ray
    // head, n3dt_render_fwd16): no projection pass, and the first block reads 16-bit rows
    const int C = g->feat_nc, fs = g->featmap_size, nblk = g->n_blocks;
    // carve (in 16-bit elements for the maps): t1 | ps | hid | netA | netB, then planar fp32 rgbA | rgbB
    size_t e_t1 = 0, e_ps = 0, e_hid = 0, e_net = 0;
    for (int i = 0; i < nblk; ++i) {
        const size_t h = (size_t)fs << i, M = (size_t)nb * h * h, ci = nr_ch16(C, i), co = nr_ch16(C, i + 1);
        if (M * 2 * ci > e_t1) e_t1 = M * 2 * ci;
        if (4 * M * ci > e_ps) e_ps = 4 * M * ci;
        if (4 * M * co > e_hid) e_hid = 4 * M * co;
    }
    e_net = e_hid;
    auto al = [](size_t n) { return (n + 127) & ~(size_t)127; };
    unsigned short* base = reinterpret_cast<unsigned short*>(ws);
    unsigned short* t1 = base;
    unsigned short* ps = t1 + al(e_t1);
    unsigned short* hid = ps + al(e_ps);
    unsigned short* netA = hid + al(e_hid);
    unsigned short* netB = netA + al(e_net);
    const size_t P = (size_t)fs << nblk;
    float* rgbA = reinterpret_cast<float*>(netB + al(e_net));
    float* rgbB = rgbA + (size_t)nb * 3 * P * P;
    unsigned char* packw = reinterpret_cast<unsigned char*>(ws + (ws_floats - nrf_pack_floats(g)));

    int h = fs;
    if (pack_mode == 2) {  // only refresh the packed block weights in the workspace tail
        for (int i = 0; i < nblk; ++i) {
            const int ci = nr_ch16(C, i), co = nr_ch16(C, i + 1);
            if (!(nrf_enabled() && nrf_supported(ci, co))) continue;
            nrf_run_level<PREC>(ci, co, 0, nullptr, false, p->psu1_w[i], p->psu1_b[i], p->psu2_w[i], p->psu2_b[i], p->feat_w[i], packw, nullptr, 2, s);
            packw += (nrf_packed_bytes(ci, co) + 255) / 256 * 256;
        }
        return;
    }
    if (!rgb0) {
        const size_t npix = (size_t)nb * h * h;
        const float* f32map = reinterpret_cast<const float*>(featmap);
        if (C % 64 == 0)
            hipLaunchKernelGGL(to_rgb16_kernel, dim3((unsigned)((npix * 16 + 255) / 256)), dim3(256), 3 * C * sizeof(float), s, nb, h * h, C, f32map,
                               p->to_rgb_w[0], p->to_rgb_b[0], rgbB);
        else
            hipLaunchKernelGGL(to_rgb_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 3 * C * sizeof(float), s, nb, h * h, C, f32map,
                               p->to_rgb_w[0], p->to_rgb_b[0], (const float*)nullptr, rgbB, 0);
    }
    // the RGB pyramid: `lo` holds it at the current block's INPUT resolution; a fused block upsamples it on the fly, the
    // layered fallback needs the stand-alone rgb_up pass first.  (A caller's rgb0 is only ever read: the first level writes
    // into the workspace, and from then on the two workspace planes alternate as before.)
    const float* lo = rgb0 ? rgb0 : rgbB;
    float* spare = rgbA;
    const void* x = featmap;
    bool x16 = rgb0 != nullptr;
    unsigned short* cur = netA;
    unsigned short* oth = netB;
    for (int i = 0; i < nblk; ++i) {
        const int ci = nr_ch16(C, i), co = nr_ch16(C, i + 1), M = nb * h * h;
        dim3 g1((M + HG_BM - 1) / HG_BM, (2 * ci + HG_BN - 1) / HG_BN), g2((M + HG_BM - 1) / HG_BM, (4 * ci + HG_BN - 1) / HG_BN);
        const bool fused = nrf_enabled() && nrf_supported(ci, co);
        if (fused) {
            // the whole block up to the blur in one kernel (nr_fused_x16.inc); hid comes out as four sub-pixel planes
            nrf_run_level<PREC>(ci, co, M, x, x16, p->psu1_w[i], p->psu1_b[i], p->psu2_w[i], p->psu2_b[i], p->feat_w[i], packw, hid, pack_mode, s);
            packw += (nrf_packed_bytes(ci, co) + 255) / 256 * 256;
        }
        const int hs = hg_log2(h);
        HGemm e1 = {t1, nullptr, 0, 0, 0, 0.2f, 1, 0, -1, -1};
        HGemm e2 = {ps, x, ci, h, h, 0.2f, 1, hg_log2(ci), hs, hs};
        if (fused) {
        } else if (x16) {
            hipLaunchKernelGGL((gemm_h_kernel<HEPI_PLAIN, PREC, true, false>), g1, dim3(256), 0, s, M, 2 * ci, ci, x, p->psu1_w[i], p->psu1_b[i], e1);
            hipLaunchKernelGGL((gemm_h_kernel<HEPI_PSU, PREC, true, true>), g2, dim3(256), 0, s, M, 4 * ci, 2 * ci, (const void*)t1, p->psu2_w[i],
                               p->psu2_b[i], e2);
        } else {
            hipLaunchKernelGGL((gemm_h_kernel<HEPI_PLAIN, PREC, false, false>), g1, dim3(256), 0, s, M, 2 * ci, ci, x, p->psu1_w[i], p->psu1_b[i], e1);
            hipLaunchKernelGGL((gemm_h_kernel<HEPI_PSU, PREC, true, false>), g2, dim3(256), 0, s, M, 4 * ci, 2 * ci, (const void*)t1, p->psu2_w[i],
                               p->psu2_b[i], e2);
        }
        h *= 2;
        const int M4 = nb * h * h;
        // feat_layers on the un-blurred map (Blur commuted behind it), no bias / activation yet
        HGemm e3 = {hid, nullptr, 0, 0, 0, -1.0f, 0, 0, -1, -1};
        dim3 g3((M4 + HG_BM - 1) / HG_BM, (co + HG_BN - 1) / HG_BN);
        if (!fused)
            hipLaunchKernelGGL((gemm_h_kernel<HEPI_PLAIN, PREC, true, false>), g3, dim3(256), 0, s, M4, co, ci, (const void*)ps, p->feat_w[i],
                               p->feat_b[i], e3);
        const bool last = i == nblk - 1;
        const size_t nthr = (size_t)M4 * (co / 8);
        if (fused) {
            launch_blur_q<PREC>(nb, h / 2, h / 2, co, hid, p->feat_b[i], last ? (unsigned short*)nullptr : cur, p->to_rgb_w[i + 1],
                                p->to_rgb_b[i + 1], lo, last ? img : spare, last ? 1 : 0, (float*)nullptr, s);
            float* t2 = lo == rgb0 ? rgbB : const_cast<float*>(lo);
            lo = spare;
            spare = t2;
        } else {
            float* low = lo == rgb0 ? rgbB : const_cast<float*>(lo);  // this level's pyramid output, in the workspace
            const size_t nout = (size_t)nb * 3 * h * h;  // h is the OUTPUT resolution here
            hipLaunchKernelGGL(rgb_up_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, nb * 3, h / 2, h / 2, lo, spare);
            hipLaunchKernelGGL(blur_act_rgb_kernel<PREC>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 4 * co * sizeof(float), s, nb, h, h, co,
                               hid, p->feat_b[i], last ? (unsigned short*)nullptr : cur, p->to_rgb_w[i + 1], p->to_rgb_b[i + 1], (const float*)spare,
                               last ? img : low, last ? 1 : 0, (h == w_of(h)) ? hg_log2(h) : -1);
            lo = low;
        }
        x = cur;
        x16 = true;
        unsigned short* t = cur;
        cur = oth;
        oth = t;
    }
}

// ---- training forward of the fused mixed-precision path (bf16 maps) ------------------------------------------------
// The inference sequence above -- one fused block kernel + one blur / activation / RGB kernel per level -- with what the
// backward needs kept (nr_train16.h): t1 and the y planes from the block kernel's SAVE epilogue, every level's activation
// map, the sigmoid image.  7 launches + 3 weight packs for three levels (the layered training forward it replaces: 24).
#include "nr_train16.h"
#include "n3dt_launch.h"
size_t nrf_packed_bytes_for(int C, int CO) { return nrf_packed_bytes(C, CO); }
bool nr16_supported(const N3dtGeom* g) {
    if (g->feat_nc != 256 || g->n_blocks < 1) return false;
    for (int i = 0; i < g->n_blocks; ++i)
        if (!nrf_supported(nr16_ch(g->feat_nc, i), nr16_ch(g->feat_nc, i + 1))) return false;
    const size_t side = (size_t)g->featmap_size << g->n_blocks;
    return side * side * 32 < ((size_t)1 << 31);
}
extern "C" void n3dt_launch_nr_train16_fwd(const N3dtGeom* g, int nb, const N3dtRenderParams* p, const float* featmap, float* img,
                                           unsigned char* saved, unsigned char* ws, hipStream_t s) {
    constexpr int PREC = N3DT_BF16;
    const int C = g->feat_nc, fs = g->featmap_size, nblk = g->n_blocks;
    const Nr16Saved sv = nr16_saved_layout(g, nb);
    const Nr16Ws wl = nr16_ws_layout(g, nb);
    unsigned short* hid = reinterpret_cast<unsigned short*>(ws + wl.hid);
    float* lo = reinterpret_cast<float*>(ws + wl.rgbB);
    float* spare = reinterpret_cast<float*>(ws + wl.rgbA);
    unsigned char* packw = ws + wl.packw;
    int h = fs;
    {
        const size_t npix = (size_t)nb * h * h;
        hipLaunchKernelGGL(to_rgb16_kernel, dim3((unsigned)((npix * 16 + 255) / 256)), dim3(256), 3 * C * sizeof(float), s, nb, h * h, C, featmap,
                           p->to_rgb_w[0], p->to_rgb_b[0], lo);
    }
    {   // the weights moved since the last step: every block's piece stream, one launch
        NrfPackAll pa;
        unsigned char* pw = packw;
        for (int i = 0; i < nblk; ++i) {
            pa.C[i] = nr16_ch(C, i); pa.CO[i] = nr16_ch(C, i + 1);
            pa.W1[i] = p->psu1_w[i]; pa.b1[i] = p->psu1_b[i]; pa.W2[i] = p->psu2_w[i]; pa.b2[i] = p->psu2_b[i]; pa.Wf[i] = p->feat_w[i];
            pa.out[i] = pw;
            pw += nr16_al(nrf_packed_bytes(pa.C[i], pa.CO[i]));
        }
        hipLaunchKernelGGL(nrf_pack_all_kernel, dim3(200, nblk), dim3(256), 0, s, pa, PREC);
    }
    const void* x = featmap;
    bool x16 = false;
    for (int i = 0; i < nblk; ++i) {
        const int ci = nr16_ch(C, i), co = nr16_ch(C, i + 1), M = nb * h * h;
        unsigned short* net = reinterpret_cast<unsigned short*>(saved + sv.net[i]);
        nrf_run_level_train(ci, co, M, x, x16, packw, hid, reinterpret_cast<unsigned short*>(saved + sv.t1[i]),
                            reinterpret_cast<unsigned short*>(saved + sv.y[i]), s);
        packw += nr16_al(nrf_packed_bytes(ci, co));
        const bool last = i == nblk - 1;
        launch_blur_q<PREC>(nb, h, h, co, (const unsigned short*)hid, p->feat_b[i], net, p->to_rgb_w[i + 1], p->to_rgb_b[i + 1], (const float*)lo,
                            last ? img : spare, last ? 1 : 0, last ? reinterpret_cast<float*>(saved + sv.img) : (float*)nullptr, s);
        float* t2 = lo;
        lo = spare;
        spare = t2;
        h *= 2;
        x = net;
        x16 = true;
    }
}

// The backward's input-gradient GEMMs (train_nr.hip, nr_bwd16): y[M][N] (bf16) = A[M][K] . Wt[N][K]^T with A the row-wise
// concatenation of n_regions 16-bit matrices; gate != nullptr: y *= lrelu'(gate[M][N]).
extern "C" void n3dt_launch_gemm_regions_bf16(int M, int N, int K, int n_regions, const void* const* base, const int* width, const int* ld,
                                              const float* Wt, const void* gate, void* y, hipStream_t s) {
    HGemm e = {reinterpret_cast<unsigned short*>(y), gate, 0, 0, 0, -1.0f, 0, 0, -1, -1, {nullptr, nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0, 0, 0},
               {0, 0, 0, 0, 0}, n_regions};
    int k = 0;
    for (int r = 0; r < n_regions; ++r) {
        e.xr_base[r] = reinterpret_cast<const unsigned short*>(base[r]);
        e.xr_k0[r] = k;
        e.xr_ld[r] = ld[r];
        k += width[r];
    }
    e.xr_k0[n_regions] = k;  // == K
    dim3 grid((M + HG_BM - 1) / HG_BM, (N + HG_BN - 1) / HG_BN);
    if (gate)
        hipLaunchKernelGGL((gemm_h_kernel<HEPI_GATE, N3DT_BF16, true, true, true>), grid, dim3(256), 0, s, M, N, K, base[0], Wt, (const float*)nullptr, e);
    else
        hipLaunchKernelGGL((gemm_h_kernel<HEPI_PLAIN, N3DT_BF16, true, false, true>), grid, dim3(256), 0, s, M, N, K, base[0], Wt, (const float*)nullptr, e);
}

static void n3dt_launch_neural_render_x16(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap,
                                              float* img, float* ws, size_t ws_floats, const int pack_mode, hipStream_t s) {
    if (precision == N3DT_BF16) run_x16<N3DT_BF16>(g, nb, p, featmap, img, ws, ws_floats, pack_mode, s);
    else run_x16<N3DT_F16>(g, nb, p, featmap, img, ws, ws_floats, pack_mode, s);
}
// the 16-bit input form (packed block weights already in the workspace tail)
static void n3dt_launch_neural_render_x16_in16(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const void* featmap16,
                                               const float* rgb0, float* img, float* ws, size_t ws_floats, hipStream_t s) {
    if (precision == N3DT_BF16) run_x16<N3DT_BF16>(g, nb, p, featmap16, img, ws, ws_floats, 1, s, rgb0);
    else run_x16<N3DT_F16>(g, nb, p, featmap16, img, ws, ws_floats, 1, s, rgb0);
}

// The pixel-major 1x1-conv GEMM of this file for the training path's forward (bf16 maps):
//   y[M][N] (bf16) = lrelu_slope(x[M][K] . Wt[N][K]^T + bias),  x bf16 or fp32
// training backward: y[M][N] (bf16) = (dy[M][K] . Wt[N][K]^T) gated by lrelu'(res) (mode 1) or + res (mode 2); plain for mode 0
extern "C" void n3dt_launch_conv1x1_bwd_bf16(int M, int N, int K, const void* dy, const float* Wt, int mode, const void* res, void* y,
                                             hipStream_t s) {
    HGemm e = {reinterpret_cast<unsigned short*>(y), res, 0, 0, 0, -1.0f, 0, 0, -1, -1};
    dim3 grid((M + HG_BM - 1) / HG_BM, (N + HG_BN - 1) / HG_BN);
    if (mode == 1) hipLaunchKernelGGL((gemm_h_kernel<HEPI_GATE, N3DT_BF16, true, true>), grid, dim3(256), 0, s, M, N, K, dy, Wt, (const float*)nullptr, e);
    else if (mode == 2) hipLaunchKernelGGL((gemm_h_kernel<HEPI_ADD, N3DT_BF16, true, true>), grid, dim3(256), 0, s, M, N, K, dy, Wt, (const float*)nullptr, e);
    else hipLaunchKernelGGL((gemm_h_kernel<HEPI_PLAIN, N3DT_BF16, true, false>), grid, dim3(256), 0, s, M, N, K, dy, Wt, (const float*)nullptr, e);
}

extern "C" void n3dt_launch_conv1x1_bf16(int M, int N, int K, const void* x, int x_is_16, const float* Wt, const float* bias, float slope,
                                         void* y, hipStream_t s) {
    HGemm e = {reinterpret_cast<unsigned short*>(y), nullptr, 0, 0, 0, slope, bias ? 1 : 0, 0, -1, -1};
    dim3 grid((M + HG_BM - 1) / HG_BM, (N + HG_BN - 1) / HG_BN);
    if (x_is_16) hipLaunchKernelGGL((gemm_h_kernel<HEPI_PLAIN, N3DT_BF16, true, false>), grid, dim3(256), 0, s, M, N, K, x, Wt, bias, e);
    else hipLaunchKernelGGL((gemm_h_kernel<HEPI_PLAIN, N3DT_BF16, false, false>), grid, dim3(256), 0, s, M, N, K, x, Wt, bias, e);
}
