// Walks csrc/s3fd_core.h -- the functions csrc/s3fd.hip takes its sizes and addresses from -- over the kernels' grids on the CPU:
// the convolution kernel's block / wave / lane / K-step nest re-typed (a change to that loop in s3fd.hip must be made here too), the
// pool, the norm and the pack, for every block of the chain, with the maps where the workspace carve holds them.  A stand-alone
// program with its own main: tests/test_s3fd_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
//
//   s3fd_core_host N H W [N H W ...]
//
// Per (N, H, W) and block one line: N H W block Hi Wi Ho Wo C_out stores.  Exit status 1 and a message on stderr where a load
// leaves its map or is not the convolution's tap, an element of a map (halo included) is stored twice or never, a store leaves the
// carve, or a packed weight is read where the pack did not write it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/conv_frag.h"
#include "../nerf-3dtalker-code_amd/csrc/s3fd_core.h"

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

// a map of the carve: `floats` elements, each counting its stores
struct Map {
    std::vector<unsigned char> count;
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
        return used;
    }
};

// the pack kernel's decode over one matrix, and the reads of the MFMA step
static void walk_pack(int j) {
    const S3Geom g = s3_gemm_geom(j, S3_MIN_HW, S3_MIN_HW);
    const size_t elems = (size_t)g.K * g.np;
    std::vector<unsigned char> written(elems, 0);
    for (size_t e = 0; e < elems; ++e) {
        int k, n;
        cf_pack_decode(e, g.np / 32, &k, &n);
        CHECK(k >= 0 && k < g.K && n >= 0 && n < g.np, "pack %d: element %zu decodes to (%d, %d)", j, e, k, n);
        const size_t back = cf_frag_elem(k / 16, g.np / 32, n / 32, 0, (n % 32) + 32 * ((k % 16) / 8), k % 8);
        CHECK(back == e, "pack %d: element %zu is read back at %zu", j, e, back);
        ++written[e];
    }
    for (int s = 0; s < g.K / 16; ++s)
        for (int t = 0; t < g.np / 32; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int jj = 0; jj < 8; ++jj) {
                    const size_t e = cf_frag_elem(s, g.np / 32, t, 0, lane, jj);
                    CHECK(e < elems && written[e] == 1, "pack %d: read at %zu not written", j, e);
                }
}

// the convolution kernel's grid: loads checked against `in_floats`, stores counted in `out`
static void walk_conv(int j, int n, int Hi, int Wi, size_t in_floats, Map& out) {
    const S3Geom g = s3_gemm_geom(j, Hi, Wi);
    const long long Mq = (long long)n * g.Hq * g.Wq;
    const int NT = cn_wave_ntiles(Mq, g.np);
    CHECK((NT == 1 || NT == 2) && g.np % (32 * NT) == 0, "conv %d: %d tiles a wave do not divide the %d columns", j, NT, g.np);
    const int ntn = g.np / (32 * NT);
    const size_t mtiles = ((size_t)Mq + CN_TILE_M - 1) / CN_TILE_M, tiles = mtiles * ntn;
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    const int pad = g.ihalo - g.ioff;
    CHECK(s3_in_elems(&g, n) <= in_floats, "conv %d: the input map has %zu elements, its region %zu", j, s3_in_elems(&g, n), in_floats);
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
                        const size_t base = s3_field_base(img, y, x, g.stride, g.ioff, g.Hp, g.Wp, g.cinp);
                        int s = 0;
                        for (int tap = 0; tap < g.k * g.k; ++tap) {
                            const size_t toff = cn_tap_offset(tap, g.k, g.Wp, g.cinp) + 8 * h;
                            for (int c0 = 0; c0 < g.cinp; c0 += 16, ++s) {
                                const size_t at = base + toff + c0;
                                CHECK(at + 8 <= in_floats && at % 4 == 0, "conv %d: load at %zu of %zu", j, at, in_floats);
                                // the cell it reads is the convolution's tap (ky, kx) of pixel (y, x), in image img
                                const size_t cell = at / g.cinp;
                                const int xp = (int)(cell % g.Wp), yp = (int)(cell / g.Wp % g.Hp), im = (int)(cell / g.Wp / g.Hp);
                                CHECK(im == img && yp - g.ihalo == y * g.stride - pad + tap / g.k && xp - g.ihalo == x * g.stride - pad + tap % g.k &&
                                          (int)(at % g.cinp) == c0 + 8 * h,
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
                            if (co >= g.cstore) continue;
                            out.store((size_t)m * g.cstore + co, "conv");
                        }
                    }
            }
        }
}

static void walk_pool(int n, int Hi, int Wi, int ihalo, int C, int opad, size_t in_floats, Map& out) {
    const int Ho = Hi / 2, Wo = Wi / 2, Hq = Ho + 2 * opad, Wq = Wo + 2 * opad, C4 = C / 4;
    const size_t total = (size_t)n * Hq * Wq * C4, row = (size_t)(Wi + 2 * ihalo) * C;
    for (size_t e = 0; e < total; ++e) {
        const int c = (int)(e % C4) * 4;
        int img, yq, xq;
        cn_cell(e / C4, Hq, Wq, &img, &yq, &xq);
        if (cn_interior(yq, xq, Ho, Wo, opad)) {
            const size_t p = s3_pool_base(img, yq - opad, xq - opad, Hi, Wi, ihalo, C) + c;
            CHECK(p + row + C + 4 <= in_floats, "pool: load at %zu of %zu", p + row + C, in_floats);
            const size_t cell = p / C;
            const int xp = (int)(cell % (Wi + 2 * ihalo)), yp = (int)(cell / (Wi + 2 * ihalo) % (Hi + 2 * ihalo));
            CHECK(xp - ihalo == 2 * (xq - opad) && yp - ihalo == 2 * (yq - opad) && xp - ihalo + 1 < Wi && yp - ihalo + 1 < Hi,
                  "pool: cell (%d, %d) reads (%d, %d)", yq, xq, yp, xp);
        }
        for (int k = 0; k < 4; ++k) out.store(e * 4 + k, "pool");
    }
}

static void walk_norm(int n, int H, int W, int C, size_t in_floats, Map& out) {
    const int Hq = H + 2, Wq = W + 2;
    const size_t total = (size_t)n * Hq * Wq;
    for (size_t e = 0; e < total; ++e) {
        int img, yq, xq;
        cn_cell(e, Hq, Wq, &img, &yq, &xq);
        if (cn_interior(yq, xq, H, W, 1)) {
            const size_t at = (((size_t)img * H + (yq - 1)) * W + (xq - 1)) * C;
            CHECK(at + C <= in_floats, "norm: load at %zu of %zu", at, in_floats);
        }
        for (int c = 0; c < C; ++c) out.store(e * C + c, "norm");
    }
}

static void line(int n, int H, int W, int block, int Hi, int Wi, int Ho, int Wo, int C, size_t stores) {
    printf("%d %d %d %d %d %d %d %d %d %zu\n", n, H, W, block, Hi, Wi, Ho, Wo, C, stores);
}

// the chain as s3_chain in s3fd.hip launches it
static void walk_chain(int n, int H, int W) {
    const S3Workspace w = s3_workspace(n, H, W);
    const S3Sizes s = s3_sizes(H, W);
    CHECK(s3_hw_ok(H, W) && n >= 1 && n <= s3_max_images(H, W), "%d x %d x %d is outside the limits", n, H, W);
    const size_t map_floats = (w.map[1] - w.map[0]) / sizeof(float), norm_floats = (w.head[0] - w.norm) / sizeof(float);
    Map maps[2] = {Map(map_floats), Map(map_floats)};
    Map norm(norm_floats);
    int in = 0, pool = 0;
    // the prologue writes map 0: every cell of [n, H + 2, W + 2, 16]
    CHECK((size_t)n * (H + 2) * (W + 2) * 16 <= map_floats, "the input map leaves its region");
    for (int c = 0; c < S3_CONVS; ++c) {
        const S3Conv t = S3_TABLE[c];
        const S3Geom g = s3_gemm_geom(c, s.h[c], s.w[c]);
        walk_conv(c, n, s.h[c], s.w[c], map_floats, maps[1 - in]);
        line(n, H, W, c, g.Hi, g.Wi, g.Ho, g.Wo, g.cstore, maps[1 - in].once(s3_out_elems(&g, n), "conv", c));
        in = 1 - in;
        if (t.level) {
            const int l = t.level - 1;
            CHECK(g.Ho == s.lh[l] && g.Wo == s.lw[l], "level %d: %d x %d against %d x %d", l, g.Ho, g.Wo, s.lh[l], s.lw[l]);
            size_t src_floats = map_floats;
            if (l < S3_NORMS) {
                CHECK(g.opad == 0, "a norm's input carries a halo");
                walk_norm(n, s.lh[l], s.lw[l], s3_level_c(l), map_floats, norm);
                line(n, H, W, S3_FIRST_NORM + l, g.Ho, g.Wo, g.Ho, g.Wo, s3_level_c(l),
                     norm.once((size_t)n * s3_norm_elems(s.lh[l], s.lw[l], s3_level_c(l)), "norm", l));
                src_floats = norm_floats;
            } else {
                CHECK(g.opad == 1, "a head's input needs halo 1");
            }
            const S3Geom hg = s3_gemm_geom(S3_CONVS + l, s.lh[l], s.lw[l]);
            const size_t head_floats = ((l + 1 < S3_LEVELS ? w.head[l + 1] : w.score) - w.head[l]) / sizeof(float);
            Map head(head_floats);
            walk_conv(S3_CONVS + l, n, s.lh[l], s.lw[l], src_floats, head);
            line(n, H, W, S3_FIRST_HEAD + l, hg.Hi, hg.Wi, hg.Ho, hg.Wo, hg.cstore, head.once(s3_out_elems(&hg, n), "head", l));
        }
        if (t.pool) {
            const int opad = S3_TABLE[c + 1].pad;
            CHECK(s3_conv_ihalo(c + 1) == opad, "pool %d writes halo %d, its reader expects %d", pool, opad, s3_conv_ihalo(c + 1));
            walk_pool(n, g.Ho, g.Wo, g.opad, t.cout, opad, map_floats, maps[1 - in]);
            line(n, H, W, S3_FIRST_POOL + pool, g.Ho, g.Wo, g.Ho / 2, g.Wo / 2, t.cout,
                 maps[1 - in].once((size_t)n * (g.Ho / 2 + 2 * opad) * (g.Wo / 2 + 2 * opad) * t.cout, "pool", pool));
            CHECK(g.Ho / 2 == s.h[c + 1] && g.Wo / 2 == s.w[c + 1], "pool %d: %d x %d against %d x %d", pool, g.Ho / 2, g.Wo / 2, s.h[c + 1], s.w[c + 1]);
            in = 1 - in;
            ++pool;
        } else if (c + 1 < S3_CONVS) {
            CHECK(s3_conv_ihalo(c + 1) == g.opad && g.Ho == s.h[c + 1] && g.Wo == s.w[c + 1], "conv %d's output is not conv %d's input", c, c + 1);
        }
    }
    // the tail's regions hold n P scores, boxes and flags
    int first[S3_LEVELS + 1];
    const size_t P = (size_t)s3_positions(&s, first);
    CHECK(w.box - w.score >= n * P * 8 && w.sup - w.box >= n * P * 32 && w.total - w.sup >= n * P, "the tail's regions are too small");
    for (int p = 0; p < (int)P; ++p) {
        int l, y, x;
        s3_position(p, first, s.lw, &l, &y, &x);
        CHECK(l >= 0 && l < S3_LEVELS && y >= 0 && y < s.lh[l] && x >= 0 && x < s.lw[l] && first[l] + y * s.lw[l] + x == p, "position %d decodes wrongly", p);
    }
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: %s N H W [N H W ...]\n", argv[0]);
        return 2;
    }
    for (int j = 0; j < S3_GEMMS; ++j) walk_pack(j);
    for (int a = 1; a + 2 < argc; a += 3) walk_chain(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]));
    // the smoothing's windows against a literal slice
    for (int F = 1; F <= 12; ++F)
        for (int T = 1; T <= 8; ++T)
            for (int i = 0; i < F; ++i) {
                int a, b;
                s3_smooth_window(i, F, T, &a, &b);
                CHECK(a >= 0 && a < b && b <= F, "smoothing window [%d, %d) of %d", a, b, F);
            }
    if (failures) fprintf(stderr, "%d failures\n", failures);
    return failures ? 1 : 0;
}
