// Walks csrc/face_recon_core.h -- the functions csrc/face_recon.hip takes its sizes and addresses from -- over the kernels' grids on
// the CPU: the convolution kernel's block / wave / lane / K-step nest re-typed (a change to that loop in face_recon.hip must be made
// here too), the stem's flattened gather, the max pool, the average, the head and the pack, for every block of the chain, with the
// maps where the workspace carve holds them; and the resample's tap ranges.  A stand-alone program with its own main:
// tests/test_face_recon_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
//
//   face_recon_core_host N H W [N H W ...]
//
// Per (N, H, W) and block one line: N H W block Hi Wi Ho Wo C_out stores.  Exit status 1 and a message on stderr where a load
// leaves its map or is not the convolution's tap, an element of a map (halo included) is stored twice or never, a store leaves the
// carve, a block reads a region another live map still needs, or a packed weight is read where the pack did not write it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/conv_frag.h"
#include "../nerf-3dtalker-code_amd/csrc/face_recon_core.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");    \
            }                             \
        }                                 \
    } while (0)

// a region of the carve: `floats` elements, each counting its stores
struct Map {
    std::vector<unsigned char> count;
    size_t live = 0;  // elements of the map it holds now
    explicit Map(size_t floats) : count(floats, 0) {}
    void store(size_t at, const char* who) {
        CHECK(at < count.size(), "%s: store at %zu outside a region of %zu", who, at, count.size());
        if (at < count.size()) ++count[at];
    }
    // every one of the first `used` elements exactly once, none behind them
    size_t once(size_t used, const char* who, int block) {
        size_t bad = 0;
        for (size_t i = 0; i < count.size(); ++i) bad += count[i] != (i < used ? 1 : 0);
        CHECK(bad == 0, "%s block %d: %zu elements not stored exactly once", who, block, bad);
        for (size_t i = 0; i < count.size(); ++i) count[i] = 0;
        live = used;
        return used;
    }
};

// the pack kernel's decode over one matrix, its source index, and the reads of the MFMA step
static void walk_pack(int j) {
    const FrGeom g = fr_geom(j, FR_MIN_HW, FR_MIN_HW);
    const size_t elems = (size_t)g.K * g.cout, src = (size_t)g.cout * g.cin * g.k * g.k;
    std::vector<unsigned char> written(elems, 0), taken(src, 0);
    CHECK(g.K % 16 == 0 && g.cout % 64 == 0, "pack %d: K %d, C_out %d", j, g.K, g.cout);
    for (size_t e = 0; e < elems; ++e) {
        int k, n;
        cf_pack_decode(e, g.cout / 32, &k, &n);
        CHECK(k >= 0 && k < g.K && n >= 0 && n < g.cout, "pack %d: element %zu decodes to (%d, %d)", j, e, k, n);
        const size_t back = cf_frag_elem(k / 16, g.cout / 32, n / 32, 0, (n % 32) + 32 * ((k % 16) / 8), k % 8);
        CHECK(back == e, "pack %d: element %zu is read back at %zu", j, e, back);
        ++written[e];
        size_t at = src;
        if (g.role == FR_STEM) {
            if (k < CN_STEM_K) {
                int ky, kx, c;
                cn_stem_tap(k, &ky, &kx, &c);
                CHECK(ky >= 0 && ky < 7 && kx >= 0 && kx < 7 && c >= 0 && c < 3 && (ky * 7 + kx) * 3 + c == k, "stem row %d decodes to (%d, %d, %d)", k, ky, kx, c);
                at = ((size_t)n * 3 + c) * 49 + ky * 7 + kx;
            }
        } else {
            const int tap = k / g.cin, ci = k - tap * g.cin;
            at = ((size_t)n * g.cin + ci) * (g.k * g.k) + tap;
        }
        if (g.role != FR_STEM || k < CN_STEM_K) {
            CHECK(at < src, "pack %d: weight read at %zu of %zu", j, at, src);
            if (at < src) ++taken[at];
        }
    }
    size_t bad = 0;
    for (size_t i = 0; i < src; ++i) bad += taken[i] != 1;
    CHECK(bad == 0, "pack %d: %zu weights not packed exactly once", j, bad);
    for (int s = 0; s < g.K / 16; ++s)
        for (int t = 0; t < g.cout / 32; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int jj = 0; jj < 8; ++jj) {
                    const size_t e = cf_frag_elem(s, g.cout / 32, t, 0, lane, jj);
                    CHECK(e < elems && written[e] == 1, "pack %d: read at %zu not written", j, e);
                }
}

// the convolution kernel's grid: loads checked against the `in_floats` live elements of its input, stores counted in `out`
static void walk_conv(int j, int n, int Hi, int Wi, size_t in_floats, size_t skip_floats, bool has_skip, Map& out) {
    const FrGeom g = fr_geom(j, Hi, Wi);
    const long long Mq = (long long)n * g.Hq * g.Wq;
    const int NT = cn_wave_ntiles(Mq, g.cout);
    CHECK((NT == 1 || NT == 2) && g.cout % (32 * NT) == 0, "conv %d: %d tiles a wave do not divide C_out %d", j, NT, g.cout);
    const int ntn = g.cout / (32 * NT);
    const size_t mtiles = ((size_t)Mq + CN_TILE_M - 1) / CN_TILE_M, tiles = mtiles * ntn;
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    CHECK(fr_in_elems(&g, n) == in_floats, "conv %d: the input map has %zu elements, what was written %zu", j, fr_in_elems(&g, n), in_floats);
    CHECK((g.role == FR_CONV3) == has_skip, "conv %d: skip", j);
    if (has_skip) CHECK(g.opad == 0 && fr_out_elems(&g, n) == skip_floats, "conv %d: the skip map has %zu elements, the output %zu", j, skip_floats, fr_out_elems(&g, n));
    for (unsigned block = 0; block < grid; ++block)
        for (int wave = 0; wave < 4; ++wave) {
            const long long tile = (long long)block * 4 + wave;
            const long long m0 = tile / ntn * CN_TILE_M;
            if (m0 >= Mq) continue;
            const int nt0 = (int)(tile % ntn) * NT;
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, h = lane >> 5;
                if (nt0 == 0)  // the loads do not depend on the column tile
                    for (int mt = 0; mt < 2; ++mt) {
                        int img, yq, xq;
                        cn_row_cell(m0 + mt * 32 + r, Mq, g.Hq, g.Wq, &img, &yq, &xq);
                        const int y = cn_clampi(yq - g.opad, 0, g.Ho - 1), x = cn_clampi(xq - g.opad, 0, g.Wo - 1);
                        const size_t base = cn_field_base(img, y, x, g.stride, g.Hp, g.Wp, g.cinp);
                        if (g.role == FR_STEM) {
                            for (int s = 0; s < CN_STEM_KP / 16; ++s)
                                for (int jj = 0; jj < 8; ++jj) {
                                    const int k = 16 * s + 8 * h + jj;
                                    const size_t at = base + cn_stem_offset(k < CN_STEM_K ? k : 0, g.Wp);
                                    CHECK(at < in_floats, "stem: load at %zu of %zu", at, in_floats);
                                    if (k >= CN_STEM_K) continue;
                                    int ky, kx, c;
                                    cn_stem_tap(k, &ky, &kx, &c);
                                    const size_t cell = at / 3;
                                    const int xp = (int)(cell % g.Wp), yp = (int)(cell / g.Wp % g.Hp), im = (int)(cell / g.Wp / g.Hp);
                                    CHECK(im == img && yp == y * 2 + ky && xp == x * 2 + kx && (int)(at % 3) == c,
                                          "stem: pixel (%d, %d, %d) k %d reads cell (%d, %d, %d)", img, y, x, k, im, yp, xp);
                                }
                            continue;
                        }
                        int s = 0;
                        for (int tap = 0; tap < g.k * g.k; ++tap) {
                            const size_t toff = cn_tap_offset(tap, g.k, g.Wp, g.cinp) + 8 * h;
                            for (int c0 = 0; c0 < g.cinp; c0 += 16, ++s) {
                                const size_t at = base + toff + c0;
                                CHECK(at + 8 <= in_floats && at % 4 == 0, "conv %d: load at %zu of %zu", j, at, in_floats);
                                // the cell it reads is the convolution's tap (ky, kx) of pixel (y, x), in image img
                                const size_t cell = at / g.cinp;
                                const int xp = (int)(cell % g.Wp), yp = (int)(cell / g.Wp % g.Hp), im = (int)(cell / g.Wp / g.Hp);
                                CHECK(im == img && yp == y * g.stride + tap / g.k && xp == x * g.stride + tap % g.k && (int)(at % g.cinp) == c0 + 8 * h,
                                      "conv %d: pixel (%d, %d, %d) tap %d reads cell (%d, %d, %d)", j, img, y, x, tap, im, yp, xp);
                            }
                        }
                        CHECK(s == g.K / 16, "conv %d: %d K steps, %d expected", j, s, g.K / 16);
                    }
                for (int mt = 0; mt < 2; ++mt)
                    for (int i = 0; i < 16; ++i) {
                        const long long m = m0 + mt * 32 + cf_acc_row(i, h);
                        if (m >= Mq) continue;
                        for (int nt = 0; nt < NT; ++nt) {
                            const int co = (nt0 + nt) * 32 + r;
                            if (has_skip) CHECK((size_t)m * g.cout + co < skip_floats, "conv %d: skip load at %zu of %zu", j, (size_t)m * g.cout + co, skip_floats);
                            out.store((size_t)m * g.cout + co, "conv");
                        }
                    }
            }
        }
}

static void walk_pool(int n, int Hi, int Wi, int C, size_t in_floats, Map& out) {
    const int Ho = cn_pool_out(Hi), Wo = cn_pool_out(Wi), C4 = C / 4;
    const size_t total = (size_t)n * Ho * Wo * C4;
    CHECK((size_t)n * Hi * Wi * C == in_floats, "pool: the input map has %zu elements, what was written %zu", (size_t)n * Hi * Wi * C, in_floats);
    for (size_t e = 0; e < total; ++e) {
        const int c = (int)(e % C4) * 4;
        int img, yo, xo, ya, yb, xa, xb;
        cn_cell(e / C4, Ho, Wo, &img, &yo, &xo);
        cn_pool_range(yo, Hi, &ya, &yb);
        cn_pool_range(xo, Wi, &xa, &xb);
        CHECK(ya < yb && xa < xb && ya >= 0 && yb <= Hi && xa >= 0 && xb <= Wi && ya >= 2 * yo - 1 && yb <= 2 * yo + 2 && xa >= 2 * xo - 1 && xb <= 2 * xo + 2,
              "pool: cell (%d, %d) takes rows [%d, %d) columns [%d, %d)", yo, xo, ya, yb, xa, xb);
        // exactly the taps of the 3 x 3 window at (2 yo - 1, 2 xo - 1) that lie inside the map
        int want = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) want += 2 * yo + dy >= 0 && 2 * yo + dy < Hi && 2 * xo + dx >= 0 && 2 * xo + dx < Wi;
        CHECK((yb - ya) * (xb - xa) == want, "pool: cell (%d, %d) takes %d taps, %d lie inside", yo, xo, (yb - ya) * (xb - xa), want);
        for (int y = ya; y < yb; ++y)
            for (int x = xa; x < xb; ++x) {
                const size_t at = (((size_t)img * Hi + y) * Wi + x) * C + c;
                CHECK(at + 4 <= in_floats, "pool: load at %zu of %zu", at, in_floats);
            }
        for (int k = 0; k < 4; ++k) out.store(e * 4 + k, "pool");
    }
}

static void walk_avg(int n, int HW, int C, size_t in_floats, Map& out) {
    CHECK((size_t)n * HW * C == in_floats, "average: the input map has %zu elements, what was written %zu", (size_t)n * HW * C, in_floats);
    for (size_t e = 0; e < (size_t)n * C; ++e) {
        const size_t first = (e / C) * (size_t)HW * C + e % C;
        CHECK(first + (size_t)(HW - 1) * C < in_floats, "average: load at %zu of %zu", first + (size_t)(HW - 1) * C, in_floats);
        out.store(e, "average");
    }
}

static void line(int n, int H, int W, int block, int Hi, int Wi, int Ho, int Wo, int C, size_t stores) {
    printf("%d %d %d %d %d %d %d %d %d %zu\n", n, H, W, block, Hi, Wi, Ho, Wo, C, stores);
}

// the chain as n3dt_launch_face_recon_fwd launches it
static void walk_chain(int n, int H, int W) {
    const FrWorkspace w = fr_workspace(n, H, W);
    CHECK(fr_hw_ok(H, W) && n >= 1 && n <= fr_max_images(H, W) && w.total <= FR_WS_BUDGET, "%d x %d x %d is outside the limits", n, H, W);
    std::vector<Map> region;
    for (int r = 0; r < FR_REGIONS; ++r) {
        CHECK(w.region[r] % 256 == 0, "region %d is not 256-byte aligned", r);
        region.emplace_back(w.bytes[r] / sizeof(float));
    }
    // the prologue writes region 1: every cell of [n, H + 6, W + 6, 3]
    const size_t image = (size_t)n * (H + 6) * (W + 6) * 3;
    for (size_t e = 0; e < image; ++e) region[1].store(e, "image");
    region[1].once(image, "image", -1);
    FrStep steps[FR_STEPS];
    fr_chain(H, W, steps);
    int seen[FR_BLOCKS] = {0};
    for (int s = 0; s < FR_STEPS; ++s) {
        const FrStep t = steps[s];
        CHECK(t.in != t.out && t.skip != t.out && t.in >= 0 && t.in < FR_REGIONS && t.out >= 0 && t.out < FR_REGIONS, "step %d: regions %d, %d -> %d", s, t.in, t.skip, t.out);
        CHECK(t.block >= 0 && t.block < FR_BLOCKS && !seen[t.block], "step %d: block %d", s, t.block);
        seen[t.block] = 1;
        Map& out = region[t.out];
        if (t.block == FR_POOL_BLOCK) {
            walk_pool(n, t.Hi, t.Wi, 64, region[t.in].live, out);
            line(n, H, W, t.block, t.Hi, t.Wi, cn_pool_out(t.Hi), cn_pool_out(t.Wi), 64, out.once((size_t)n * fr_step_out_elems(&t), "pool", t.block));
        } else if (t.block == FR_AVG_BLOCK) {
            walk_avg(n, t.Hi * t.Wi, FR_FEAT, region[t.in].live, out);
            line(n, H, W, t.block, t.Hi, t.Wi, 1, 1, FR_FEAT, out.once((size_t)n * FR_FEAT, "average", t.block));
        } else {
            const FrGeom g = fr_geom(t.block, t.Hi, t.Wi);
            walk_conv(t.block, n, t.Hi, t.Wi, region[t.in].live, t.skip < 0 ? 0 : region[t.skip].live, t.skip >= 0, out);
            line(n, H, W, t.block, g.Hi, g.Wi, g.Ho, g.Wo, g.cout, out.once(fr_out_elems(&g, n), "conv", t.block));
        }
    }
    // the head reads the averages [n, 2048] and writes the caller's [n, 257]: one wave per output
    CHECK(region[5].live == (size_t)n * FR_FEAT, "the head's input has %zu elements", region[5].live);
    int cols = 0;
    for (int i = 0; i < FR_HEADS; ++i) cols += FR_HEAD_COLS[i];
    CHECK(cols == FR_COEFFS, "the heads have %d columns", cols);
    Map coeffs((size_t)n * FR_COEFFS);
    const size_t waves = ((size_t)n * FR_COEFFS + 3) / 4 * 4;
    for (size_t o = 0; o < waves; ++o) {
        if (o >= (size_t)n * FR_COEFFS) continue;
        CHECK((o / FR_COEFFS) * FR_FEAT + FR_FEAT <= region[5].live && o % FR_COEFFS < (size_t)FR_COEFFS, "head: output %zu", o);
        coeffs.store(o, "head");
    }
    line(n, H, W, FR_HEAD_BLOCK, 1, 1, 1, 1, FR_COEFFS, coeffs.once((size_t)n * FR_COEFFS, "head", FR_HEAD_BLOCK));
}

// the resample's taps for a resize in -> out: inside the source, never empty, the centre tap among them, the weights' sum positive
static void walk_taps(int in, int out) {
    for (int o = 0; o < out; ++o) {
        int lo, hi;
        double c, f;
        fr_taps(o, in, out, &lo, &hi, &c, &f);
        CHECK(lo >= 0 && lo < hi && hi <= in, "taps %d -> %d: output %d takes [%d, %d)", in, out, o, lo, hi);
        double sum = 0.0;
        for (int x = lo; x < hi; ++x) sum += fr_cubic(((double)x - c + 0.5) / f);
        CHECK(sum > 0.5, "taps %d -> %d: output %d's weights sum to %g", in, out, o, sum);
        CHECK((double)(hi - lo) <= 4.0 * f + 2.0, "taps %d -> %d: output %d takes %d taps", in, out, o, hi - lo);
    }
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: %s N H W [N H W ...]\n", argv[0]);
        return 2;
    }
    // the table: 53 convolutions, each bottleneck's roles in order, the channels chained
    int convs = 0;
    for (int b = 0; b < FR_BOTTLENECKS; ++b) {
        const int j = fr_bottleneck_first(b);
        CHECK(fr_conv(j).role == FR_CONV1 && fr_conv(j + 1).role == FR_CONV2 && fr_conv(j + 2).role == FR_CONV3, "bottleneck %d begins at %d", b, j);
        CHECK((fr_conv(j + 3).role == FR_DOWN) == (fr_bottleneck_down(b) != 0) || j + 3 >= FR_CONVS, "bottleneck %d: downsample", b);
        CHECK(fr_conv(j).cout == fr_conv(j + 1).cin && fr_conv(j + 1).cout == fr_conv(j + 2).cin, "bottleneck %d: channels", b);
        convs = j + (fr_bottleneck_down(b) ? 4 : 3);
    }
    CHECK(convs == FR_CONVS && fr_conv(FR_CONVS - 1).cout == FR_FEAT, "the table has %d convolutions", convs);
    for (int j = 0; j < FR_CONVS; ++j) walk_pack(j);
    for (int a = 1; a + 2 < argc; a += 3) walk_chain(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]));
    // the aligner: the fixture's resizes, the extremes of the scale range, and the similarity on a plain face
    const int resizes[][2] = {{64, 158}, {64, 40}, {80, 189}, {96, 227}, {80, 66}, {96, 79}, {80, 185}, {96, 222}, {2, 32}, {4096, 256}, {256, 4096}, {33, 2}, {5, 5}};
    for (size_t i = 0; i < sizeof(resizes) / sizeof(resizes[0]); ++i) walk_taps(resizes[i][0], resizes[i][1]);
    const double pinv[20] = {1, 0, 0, 0, -1, 0, 1, 0, -1, 0, 0, 0, 0, 0, 0, 0.2, 0.2, 0.2, 0.2, 0.2};
    const double lm5[5][2] = {{60, 70}, {30, 72}, {45, 50}, {32, 30}, {20, 31}};
    double trans[5];
    int geom[4];
    CHECK(fr_similarity(lm5, pinv, 96, 80, trans, geom) == 0 && geom[0] >= 1 && geom[1] >= 1, "the similarity of a plain face is refused");
    const double nan5[5][2] = {{60, 70}, {30, 72}, {nan(""), 50}, {32, 30}, {20, 31}};
    CHECK(fr_similarity(nan5, pinv, 96, 80, trans, geom) == 1 && geom[0] == 0, "a NaN landmark is not refused");
    const double far5[5][2] = {{6e12, 70}, {3e12, 72}, {4.5e12, 50}, {3.2e12, 30}, {2e12, 31}};
    CHECK(fr_similarity(far5, pinv, 96, 80, trans, geom) == 1, "a scale below 1/16 is not refused");
    if (failures) fprintf(stderr, "%d failures\n", failures);
    return failures ? 1 : 0;
}
