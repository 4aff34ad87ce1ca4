// A stand-alone walk of csrc/head_mask_core.h on the CPU (tests/test_head_mask_cpu.py builds it with the host compiler under the
// address and undefined-behaviour sanitizers and runs it directly).  For every shape on the command line (n H W triples) and every
// step of the forward's chain with all three outputs selected it re-types the loop nest of head_mask_conv_kernel -- block, wave,
// lane, tap, K step -- and the grids of the pool, the small stage, the label and the upsample kernels, and checks that
//   - every load lies inside the map its step was handed (as its producer left it) or inside the haloed image,
//   - every cell of every output map is stored exactly once, inside its region of the workspace,
//   - the bilinear taps of the label rule lie inside the low-resolution map,
// then the single-block entry's carve, and, given a file of int32 [64][64][64] as --nearest FILE, that hm_nearest(dst, in, out)
// equals table[in - 1][out - 1][dst] for every in, out <= 64: the table torch's F.interpolate(mode='nearest') gives.
// Prints one line per shape: steps, convolutions walked, stores counted, loads checked.  Exit code 0: everything held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/conv_frag.h"
#include "../nerf-3dtalker-code_amd/csrc/head_mask_core.h"

static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (failures++ < 20) {                \
                fprintf(stderr, "FAIL %s: ", #cond); \
                fprintf(stderr, __VA_ARGS__);     \
                fprintf(stderr, "\n");            \
            }                                     \
        }                                         \
    } while (0)

struct Walk {
    long long stores = 0, loads = 0;
    int convs = 0;
};

// what a region holds: elements per image, as its last producer wrote them
struct Held {
    size_t elems = 0;
};

static void walk_conv(const HmStep& t, int n, const Held* held, const HmWorkspace& ws, Walk* wk) {
    const int j = t.block;
    const HmConv c = HM_TABLE[j];
    const int Ho = hm_out_h(j, t.Hi), Wo = hm_out_h(j, t.Wi), np = hm_np(j);
    const int csplit = t.in2 >= 0 ? c.cin / 2 : c.cin, c2 = c.cin - csplit;
    const long long M = (long long)n * Ho * Wo;
    const int NT = cn_wave_ntiles(M, np);
    CHECK((NT == 1 || NT == 2) && np % (32 * NT) == 0, "block %d: %d tiles a wave do not divide the %d columns", j, NT, np);
    const int ntn = np / (32 * NT);
    const long long tiles = (M + CN_TILE_M - 1) / CN_TILE_M * ntn;
    const long long grid = (tiles + 3) / 4;
    CHECK((np % (32 * NT) == 0 && c.cin % 16 == 0) || c.kind == HM_STEM, "block %d: np %d cin %d", j, np, c.cin);
    CHECK((size_t)M * np * sizeof(float) <= ws.bytes[t.out], "block %d: output larger than region %d", j, t.out);
    const size_t in_total = (size_t)n * held[t.in].elems;
    if (c.kind == HM_STEM) CHECK(held[t.in].elems == (size_t)(t.Hi + 6) * (t.Wi + 6) * 3, "stem image");
    else CHECK(held[t.in].elems == (size_t)t.Hs * t.Ws * csplit, "block %d: region %d holds %zu per image, wanted %zu", j, t.in, held[t.in].elems, (size_t)t.Hs * t.Ws * csplit);
    if (t.in2 >= 0) CHECK(held[t.in2].elems == (size_t)t.Hs * t.Ws * c2, "block %d: second source", j);
    if (t.addmap >= 0) CHECK(held[t.addmap].elems == (size_t)t.Hs * t.Ws * c.cin, "block %d: added map", j);
    if (t.skip >= 0) CHECK(held[t.skip].elems == (size_t)Ho * Wo * np && t.skip != t.out, "block %d: shortcut", j);
    CHECK(t.in != t.out && t.in2 != t.out && t.addmap != t.out, "block %d writes a map it reads", j);
    if (t.scale >= 0) CHECK(t.scale + c.cin <= HM_VEC && (t.addvec < 0 || t.addvec + c.cin <= HM_VEC), "block %d: vectors", j);
    std::vector<unsigned char> count((size_t)M * np, 0);
    for (long long blk = 0; blk < grid; ++blk)
        for (int wave = 0; wave < 4; ++wave) {
            const long long tile = blk * 4 + wave;
            const long long m0 = tile / ntn * CN_TILE_M;
            if (m0 >= M) continue;
            const int nt0 = (int)(tile % ntn) * NT;
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, h = lane >> 5;
                for (int mt = 0; mt < 2; ++mt) {
                    int img, yo, xo;
                    cn_row_cell(m0 + mt * 32 + r, M, Ho, Wo, &img, &yo, &xo);
                    CHECK(img >= 0 && img < n && yo >= 0 && yo < Ho && xo >= 0 && xo < Wo, "block %d: row", j);
                    if (c.kind == HM_STEM) {
                        const size_t base = cn_field_base(img, yo, xo, c.stride, t.Hi + 6, t.Wi + 6, 3);
                        for (int k = 8 * h; k < CN_STEM_KP; k += 16)
                            for (int jj = 0; jj < 8; ++jj) {
                                const size_t off = base + cn_stem_offset(k + jj < CN_STEM_K ? k + jj : 0, t.Wi + 6);
                                CHECK(off < in_total, "stem load %zu of %zu", off, in_total);
                                ++wk->loads;
                            }
                        continue;
                    }
                    for (int tap = 0; tap < c.k * c.k; ++tap) {
                        long long cell = 0;
                        if (!hm_tap_cell(img, yo, xo, tap, c.k, c.stride, c.pad, t.Hi, t.Wi, t.Hs, t.Ws, &cell)) continue;
                        CHECK(cell >= 0 && cell < (long long)n * t.Hs * t.Ws && cell / ((long long)t.Hs * t.Ws) == img, "block %d: cell", j);
                        for (int c0 = 0; c0 < c.cin; c0 += 16) {
                            const int ch = c0 + 8 * h;
                            if (ch < csplit) CHECK((size_t)cell * csplit + ch + 8 <= in_total, "block %d: load", j);
                            else CHECK((size_t)cell * c2 + (ch - csplit) + 8 <= (size_t)n * held[t.in2].elems, "block %d: second load", j);
                            if (t.scale >= 0) CHECK(ch + 8 <= c.cin, "block %d: vector load", j);
                            ++wk->loads;
                        }
                    }
                }
                // the epilogue
                for (int mt = 0; mt < 2; ++mt)
                    for (int i = 0; i < 16; ++i) {
                        const long long m = m0 + mt * 32 + cf_acc_row(i, h);
                        if (m >= M) continue;
                        for (int nt = 0; nt < NT; ++nt) {
                            const int co = (nt0 + nt) * 32 + r;
                            CHECK(co < np, "block %d: column", j);
                            ++count[(size_t)m * np + co];
                            ++wk->stores;
                        }
                    }
            }
        }
    for (size_t e = 0; e < count.size(); ++e)
        if (count[e] != 1) {
            CHECK(count[e] == 1, "block %d: element %zu stored %d times", j, e, (int)count[e]);
            break;
        }
    ++wk->convs;
}

static void walk_pool(const HmStep& t, int n, const Held* held, const HmWorkspace& ws, Walk* wk) {
    const int Ho = cn_pool_out(t.Hi), Wo = cn_pool_out(t.Wi);
    CHECK(held[t.in].elems == (size_t)t.Hi * t.Wi * 64, "pool input");
    CHECK((size_t)n * Ho * Wo * 64 * sizeof(float) <= ws.bytes[t.out], "pool output");
    const size_t total = (size_t)n * Ho * Wo * 16;
    for (size_t e = 0; e < total; ++e) {
        int img, yo, xo, ya, yb, xa, xb;
        cn_cell(e / 16, Ho, Wo, &img, &yo, &xo);
        cn_pool_range(yo, t.Hi, &ya, &yb);
        cn_pool_range(xo, t.Wi, &xa, &xb);
        CHECK(img < n && ya >= 0 && ya < yb && yb <= t.Hi && xa >= 0 && xa < xb && xb <= t.Wi, "pool window");
        ++wk->stores;
    }
}

static void walk_labels(int n, int H, int W, int h, int w, Walk* wk) {
    for (int Y = 0; Y < H; ++Y) {
        int i0, i1;
        double w1;
        hm_lerp(Y, h, H, &i0, &i1, &w1);
        CHECK(i0 >= 0 && i0 <= i1 && i1 < h && w1 >= 0.0 && w1 <= 1.0, "row taps %d of %d -> %d", Y, h, H);
    }
    for (int X = 0; X < W; ++X) {
        int i0, i1;
        double w1;
        hm_lerp(X, w, W, &i0, &i1, &w1);
        CHECK(i0 >= 0 && i0 <= i1 && i1 < w && w1 >= 0.0 && w1 <= 1.0, "column taps %d of %d -> %d", X, w, W);
    }
    wk->loads += (long long)n * (H + W);
}

static void walk_shape(int n, int H, int W) {
    CHECK(hm_hw_ok(H, W) && n >= 1 && n <= hm_max_images(H, W), "shape %d %d %d", n, H, W);
    const HmWorkspace ws = hm_workspace(n, H, W);
    for (int r = 0; r + 1 < HM_REGIONS; ++r) CHECK(ws.region[r] + ws.bytes[r] == ws.region[r + 1] && ws.region[r] % 256 == 0, "carve");
    CHECK(ws.region[HM_REGIONS - 1] + ws.bytes[HM_REGIONS - 1] == ws.total, "carve end");
    Walk wk;
    int steps_total = 0;
    for (int outputs = 1; outputs <= 7; ++outputs) {
        HmStep steps[HM_MAX_STEPS];
        const int count = hm_chain(H, W, outputs, steps);
        CHECK(count <= HM_MAX_STEPS, "steps");
        if (outputs != 7 && outputs != 4) {  // the other selections: the same launches, a subset; their count alone
            steps_total += count;
            continue;
        }
        Held held[HM_REGIONS];
        held[HM_R_IMG].elems = (size_t)(H + 6) * (W + 6) * 3;
        bool vec_written[HM_VEC] = {false};
        for (int s = 0; s < count; ++s) {
            const HmStep t = steps[s];
            if (t.block == HM_POOL_BLOCK) {
                walk_pool(t, n, held, ws, &wk);
            } else if (HM_TABLE[t.block].kind == HM_SMALL) {
                const HmConv c = HM_TABLE[t.block];
                if (t.invec >= 0) {
                    for (int k = 0; k < c.cin; ++k) CHECK(t.invec + k < HM_VEC && vec_written[t.invec + k], "small block %d reads an unwritten vector", t.block);
                } else {
                    CHECK(held[t.in].elems == (size_t)t.Hi * t.Wi * c.cin && c.cin <= 512, "small block %d input", t.block);
                }
                for (int k = 0; k < c.cout; ++k) {
                    CHECK(t.out + k < HM_VEC && !vec_written[t.out + k], "small block %d: vector element written twice", t.block);
                    vec_written[t.out + k] = true;
                }
                wk.stores += (long long)n * c.cout;
            } else {
                if (t.scale >= 0)
                    for (int k = 0; k < HM_TABLE[t.block].cin; ++k)
                        CHECK(vec_written[t.scale + k] && (t.addvec < 0 || vec_written[t.addvec + k]), "block %d reads an unwritten vector", t.block);
                walk_conv(t, n, held, ws, &wk);
            }
            if (t.block == HM_POOL_BLOCK || HM_TABLE[t.block].kind != HM_SMALL) held[t.out].elems = hm_step_out_elems(&t);
        }
        steps_total += count;
        for (int o = 0; o < 3; ++o) {
            if (!(outputs & (1 << o))) continue;
            int h, w;
            hm_logit_hw(H, W, o, &h, &w);
            CHECK(held[HM_R_LOG0 + o].elems == (size_t)h * w * HM_MAX_CLASSES, "logits %d", o);
            walk_labels(n, H, W, h, w, &wk);
        }
    }
    printf("%d %d %lld %lld\n", steps_total, wk.convs, wk.stores, wk.loads);
}

int main(int argc, char** argv) {
    int a = 1;
    if (argc > 2 && !strcmp(argv[1], "--nearest")) {
        FILE* f = fopen(argv[2], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[2]);
            return 2;
        }
        std::vector<int> table((size_t)64 * 64 * 64);
        const size_t got = fread(table.data(), sizeof(int), table.size(), f);
        fclose(f);
        CHECK(got == table.size(), "short table");
        for (int in = 1; in <= 64 && got == table.size(); ++in)
            for (int out = 1; out <= 64; ++out)
                for (int d = 0; d < out; ++d)
                    CHECK(hm_nearest(d, in, out) == table[((size_t)(in - 1) * 64 + (out - 1)) * 64 + d], "nearest %d of %d -> %d: %d", d, in, out, hm_nearest(d, in, out));
        a = 3;
    }
    // the table itself
    for (int j = 0; j < HM_CONVS; ++j) {
        const HmConv c = HM_TABLE[j];
        CHECK(hm_K(j) % 16 == 0 && hm_np(j) % 32 == 0, "block %d: K %d np %d", j, hm_K(j), hm_np(j));
        if (c.kind == HM_SMALL) CHECK(c.k == 1 && c.cin <= 512 && c.cout > 0, "small block %d", j);
    }
    // the hue: within range, and grey is 0
    for (int v = 0; v < 256; ++v) CHECK(hm_hue(v, v, v) == 0, "grey %d", v);
    for (int b = 0; b < 256; b += 5)
        for (int g = 0; g < 256; g += 3)
            for (int r = 0; r < 256; r += 7) CHECK(hm_hue(b, g, r) >= 0 && hm_hue(b, g, r) <= 180, "hue of %d %d %d", b, g, r);
    for (; a + 2 < argc; a += 3) walk_shape(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]));
    // the single-block carve: three disjoint maps
    for (int block = 0; block < HM_BLOCKS; ++block) {
        const HmBlockWs w = hm_block_ws(block, 2, 12, 10, block == HM_HEAD32 || block == HM_HEAD16 ? 6 : 12, block == HM_HEAD32 || block == HM_HEAD16 ? 5 : 10);
        CHECK(w.in < w.aux && w.aux < w.out && w.out < w.total && w.aux % 256 == 0 && w.out % 256 == 0, "block %d carve", block);
    }
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
