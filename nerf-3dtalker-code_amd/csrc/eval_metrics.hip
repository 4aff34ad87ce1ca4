// Validation metrics (include/n3dt.h, n3dt_eval_metrics): SSIM and PSNR of rendered frames as the reference scores them after
// every epoch (talker_trainer.py:1087-1150 -> Utils/Eval_utils.py:11-48,54-66,101-106).  The arithmetic lives in
// eval_metrics_core.h, which a host program also compiles; this file is the two kernels that run it.
//
// Data path: pred, gt [n,3,H,W] fp32 -> (tile kernel) workspace [n][tiles] of (double, uint64) -> (finalise kernel) ssim[n], psnr[n].
//
// eval_tile_kernel: one workgroup of 256 threads per 32x32 tile of one image pair (grid-stride over n * tiles, so no grid limit
// bounds the image size).  The 38x38 region is read once, 24 B per pixel, and lives in LDS as grey BYTES (2 x 1444 B); the
// horizontal 7-sums take 5 x 38 x 32 int32 (23.75 KiB): about 29 KiB per workgroup, five workgroups per CU.  Everything up to
// the 7x7 window sums and the squared error is integer arithmetic and therefore exact; S is float64 from there.  The tile's
// values are added in a fixed pairwise order; one plain 16-byte store per tile, no atomics.
//
// eval_finalise_kernel: one workgroup per image.  The partials pass through LDS 256 at a time and thread 0 adds them in INDEX
// order, so the result depends neither on the grid nor on scheduling: two calls on the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include "eval_metrics_core.h"
#include "n3dt_launch.h"

#define EVM_MAX_GRID (1 << 20)

__global__ __launch_bounds__(EVM_THREADS) void eval_tile_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                int height, int width, long long tiles_x, long long tiles,
                                                                long long total, EvmPartial* __restrict__ partials) {
    __shared__ EvmTileMem m;
    const int tid = (int)threadIdx.x;
    const size_t image = (size_t)3 * (size_t)height * (size_t)width;
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const long long img = t / tiles, tile = t - img * tiles;
        const int y0 = (int)(tile / tiles_x) * EVM_TILE, x0 = (int)(tile % tiles_x) * EVM_TILE;
        const unsigned int sse = evm_stage(&m, tid, pred + (size_t)img * image, gt + (size_t)img * image, height, width, y0, x0);
        __syncthreads();
        evm_rows(&m, tid);
        __syncthreads();
        m.red[tid] = evm_cols(&m, tid, height, width, y0, x0);
        m.sse[tid] = sse;
        __syncthreads();
        for (int step = EVM_THREADS / 2; step >= 1; step >>= 1) {
            evm_reduce_step(&m, tid, step);
            __syncthreads();
        }
        if (tid == 0) {
            EvmPartial p;
            p.s = m.red[0];
            p.sse = m.sse[0];
            partials[t] = p;
        }
        __syncthreads();  // m is staged again by the next tile
    }
}

__global__ __launch_bounds__(EVM_THREADS) void eval_finalise_kernel(const EvmPartial* __restrict__ partials, long long tiles,
                                                                    int n_images, int height, int width,
                                                                    double* __restrict__ ssim, double* __restrict__ psnr) {
    __shared__ EvmPartial s_p[EVM_THREADS];
    for (int img = blockIdx.x; img < n_images; img += gridDim.x) {
        const EvmPartial* p = partials + (size_t)img * (size_t)tiles;
        double s = 0.0;
        unsigned long long sse = 0;
        for (long long base = 0; base < tiles; base += EVM_THREADS) {
            const int cnt = tiles - base < EVM_THREADS ? (int)(tiles - base) : EVM_THREADS;
            if ((int)threadIdx.x < cnt) s_p[threadIdx.x] = p[base + threadIdx.x];
            __syncthreads();
            if (threadIdx.x == 0)
                for (int i = 0; i < cnt; ++i) {
                    s += s_p[i].s;
                    sse += s_p[i].sse;
                }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            ssim[img] = evm_ssim_mean(s, height, width);
            psnr[img] = evm_psnr(sse, height, width);
        }
    }
}

extern "C" size_t n3dt_eval_metrics_ws_bytes(int n_images, int height, int width) {
    return (size_t)n_images * (size_t)(evm_tiles_x(width) * evm_tiles_y(height)) * sizeof(EvmPartial);
}

extern "C" void n3dt_launch_eval_metrics(int n_images, int height, int width, const float* pred, const float* gt, double* ssim,
                                         double* psnr, void* workspace, hipStream_t stream) {
    const long long tiles_x = evm_tiles_x(width), tiles = tiles_x * evm_tiles_y(height), total = tiles * n_images;
    const int grid = total < EVM_MAX_GRID ? (int)total : EVM_MAX_GRID;
    hipLaunchKernelGGL(eval_tile_kernel, dim3(grid), dim3(EVM_THREADS), 0, stream, pred, gt, height, width, tiles_x, tiles, total,
                       (EvmPartial*)workspace);
    hipLaunchKernelGGL(eval_finalise_kernel, dim3(n_images < 65536 ? n_images : 65536), dim3(EVM_THREADS), 0, stream,
                       (const EvmPartial*)workspace, tiles, n_images, height, width, ssim, psnr);
}
