// Host walk of n3dt_eval_metrics' tile grid (tests/test_eval_metrics_cpu.py builds this with the host compiler and the address
// and undefined-behaviour sanitizers and runs it on fixture inputs).  It includes the very header the kernels are compiled
// from, csrc/eval_metrics_core.h, and runs its phases in plain loops over `tid` where the kernel has one thread per tid and a
// barrier between phases -- so the tiling, the halo and every bound are exercised on the CPU before a GPU sees them.
//
// usage: eval_core_host FILE      FILE = int32 n, height, width; then pred and gt, each float32 [n][3][height][width]
// prints one line per image:  <index> <ssim %.17g> <psnr %.17g>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/eval_metrics_core.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    int32_t hdr[3];
    if (std::fread(hdr, sizeof(int32_t), 3, f) != 3) return 2;
    const int n = hdr[0], height = hdr[1], width = hdr[2];
    if (n < 1 || height < EVM_WIN || width < EVM_WIN || (long long)height * width >= EVM_MAX_HW) return 2;
    const size_t image = (size_t)3 * height * width;
    // exactly the bytes the entry point is given: the sanitizer sees any read past either image set
    std::vector<float> pred(n * image), gt(n * image);
    if (std::fread(pred.data(), sizeof(float), pred.size(), f) != pred.size()) return 2;
    if (std::fread(gt.data(), sizeof(float), gt.size(), f) != gt.size()) return 2;
    std::fclose(f);

    const long long tiles_x = evm_tiles_x(width), tiles = tiles_x * evm_tiles_y(height);
    std::vector<EvmPartial> partials((size_t)n * tiles);  // the workspace, at the size the library asks for
    auto m = std::make_unique<EvmTileMem>();               // one workgroup's LDS
    std::vector<unsigned int> sse(EVM_THREADS);
    for (long long t = 0; t < (long long)n * tiles; ++t) {
        const long long img = t / tiles, tile = t - img * tiles;
        const int y0 = (int)(tile / tiles_x) * EVM_TILE, x0 = (int)(tile % tiles_x) * EVM_TILE;
        for (int tid = 0; tid < EVM_THREADS; ++tid)
            sse[tid] = evm_stage(m.get(), tid, pred.data() + img * image, gt.data() + img * image, height, width, y0, x0);
        for (int tid = 0; tid < EVM_THREADS; ++tid) evm_rows(m.get(), tid);
        for (int tid = 0; tid < EVM_THREADS; ++tid) {
            m->red[tid] = evm_cols(m.get(), tid, height, width, y0, x0);
            m->sse[tid] = sse[tid];
        }
        for (int step = EVM_THREADS / 2; step >= 1; step >>= 1)
            for (int tid = 0; tid < EVM_THREADS; ++tid) evm_reduce_step(m.get(), tid, step);
        partials[t].s = m->red[0];
        partials[t].sse = m->sse[0];
    }
    for (int img = 0; img < n; ++img) {
        double s = 0.0;
        unsigned long long e = 0;
        for (long long i = 0; i < tiles; ++i) {
            s += partials[img * tiles + i].s;
            e += partials[img * tiles + i].sse;
        }
        std::printf("%d %.17g %.17g\n", img, evm_ssim_mean(s, height, width), evm_psnr(e, height, width));
    }
    return 0;
}
