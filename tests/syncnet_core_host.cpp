// The index arithmetic of csrc/syncnet_core.h walked on the CPU over the grid of csrc/syncnet.hip's convolution kernel, for all 31
// blocks and the window counts given on the command line (default 1 2 3), and the weight pack of every block against the addresses
// the MFMA step reads it at.  The loop nest below is RE-TYPED from syncnet_conv_kernel (block / wave / lane / K step), and so is
// conv_net_pack_kernel's weight lookup: a change there must be made here too.  NOT re-typed, but the very functions the kernels are
// compiled from: syncnet_core.h's, and from csrc/conv_frag.h the epilogue's register -> row map (cf_acc_row), the pack kernel's
// element decode (cf_pack_decode) and the address of the step's weight fragments (cf_frag_group / cf_frag_elem).
// Built by tests/test_syncnet_cpu.py with the host compiler under -fsanitize=address,undefined: the maps are heap blocks of exactly
// the size the library allocates, so a read or a store outside one ends the program through the sanitizer; a read of the wrong
// element, a cell stored twice or never, a K step too many or too few fails the program's own check (exit code 1).
// Prints one line per (n, block): n block Hi Wi Ho Wo Hq Wq C_out tiles-per-wave reads stores.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/conv_frag.h"
#include "../nerf-3dtalker-code_amd/csrc/syncnet_core.h"

static int g_fail = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            fprintf(stderr, __VA_ARGS__);        \
            fprintf(stderr, "\n");               \
            if (++g_fail > 20) exit(1);          \
        }                                        \
    } while (0)

// one launch of syncnet_conv_kernel<NT> over block `b` for n windows
static void walk_conv(int b, int n, int NT, bool print) {
    const SnGeom g = sn_geom(b);
    const size_t in_elems = sn_in_elems(&g, n), out_elems = sn_out_elems(&g, n);
    float* in = new float[in_elems];
    for (size_t i = 0; i < in_elems; ++i) in[i] = (float)(i % 4093);
    unsigned char* stored = new unsigned char[out_elems]();
    const size_t frags = (size_t)(g.K / 16) * (g.cout / 32) * 64;  // 8-element fragments of the packed hi (and lo) matrix
    unsigned long long reads = 0, stores = 0;
    volatile float sink = 0.0f;

    const long long Mq = (long long)n * g.Hq * g.Wq;
    const int ntn = g.cout / (32 * NT);
    CHECK(g.cout % (32 * NT) == 0, "block %d: C_out %d is no multiple of %d", b, g.cout, 32 * NT);
    const size_t mtiles = ((size_t)Mq + CN_TILE_M - 1) / CN_TILE_M;
    const size_t tiles = mtiles * ntn;
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    for (unsigned block = 0; block < grid; ++block)
        for (int wave = 0; wave < 4; ++wave) {
            const long long tile = (long long)block * 4 + wave;
            const long long m0 = tile / ntn * CN_TILE_M;
            if (m0 >= Mq) continue;
            const int nt0 = (int)(tile % ntn) * NT;
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, h = lane >> 5;
                size_t base[2];
                int py[2], px[2], pimg[2];
                for (int mt = 0; mt < 2; ++mt) {
                    int img, yq, xq;
                    cn_row_cell(m0 + mt * 32 + r, Mq, g.Hq, g.Wq, &img, &yq, &xq);
                    const int y = cn_clampi(yq - g.opad, 0, g.Ho - 1), x = cn_clampi(xq - g.opad, 0, g.Wo - 1);
                    CHECK(img >= 0 && img < n && y >= 0 && y < g.Ho && x >= 0 && x < g.Wo, "block %d: row decodes outside the map", b);
                    base[mt] = sn_field_base(img, y, x, g.sh, g.sw, g.Hp, g.Wp, g.cinp);
                    pimg[mt] = img; py[mt] = y; px[mt] = x;
                }
                int s = 0;
                for (int tap = 0; tap < g.kh * g.kw; ++tap) {
                    const size_t toff = cn_tap_offset(tap, g.kw, g.Wp, g.cinp) + 8 * h;
                    for (int c0 = 0; c0 < g.cinp; c0 += 16, ++s) {
                        for (int mt = 0; mt < 2; ++mt) {
                            const float* p = in + base[mt] + toff + c0;
                            // the element this k-step must read: tap (ky, kx) of pixel (y, x), channel c0 + 8 h
                            const int ky = tap / g.kw, kx = tap % g.kw;
                            const size_t want = (((size_t)pimg[mt] * g.Hp + (size_t)(py[mt] * g.sh + ky)) * g.Wp + (size_t)(px[mt] * g.sw + kx)) * g.cinp +
                                                (size_t)(c0 + 8 * h);
                            CHECK((size_t)(p - in) == want, "block %d: k-step %d reads element %zu, not %zu", b, s, (size_t)(p - in), want);
                            CHECK(py[mt] * g.sh + ky < g.Hp && px[mt] * g.sw + kx < g.Wp, "block %d: tap leaves the padded map", b);
                            for (int j = 0; j < 8; ++j) sink = sink + p[j];
                            reads += 8;
                        }
                        for (int nt = 0; nt < NT; ++nt) {
                            const size_t f = cf_frag_group(s, g.cout >> 5, nt0, nt, lane);
                            CHECK(f < frags, "block %d: weight fragment %zu of %zu", b, f, frags);
                        }
                    }
                }
                CHECK(s == g.K / 16, "block %d: %d K steps, expected %d", b, s, g.K / 16);
                for (int mt = 0; mt < 2; ++mt)
                    for (int i = 0; i < 16; ++i) {
                        const long long m = m0 + mt * 32 + cf_acc_row(i, h);
                        if (m >= Mq) continue;
                        int img, yq, xq;
                        cn_row_cell(m, Mq, g.Hq, g.Wq, &img, &yq, &xq);
                        const bool inside = cn_interior(yq, xq, g.Ho, g.Wo, g.opad);
                        const size_t o = (size_t)m * g.cout;
                        CHECK(o == (((size_t)img * g.Hq + yq) * g.Wq + xq) * g.cout, "block %d: row %lld is not its cell", b, m);
                        const float* res = nullptr;
                        if (inside && g.residual) {
                            const size_t at = sn_residual_pixel(img, yq - g.opad, xq - g.opad, g.Hp, g.Wp, g.ipad, g.cinp);
                            CHECK(g.cinp == g.cout && g.Ho == g.Hi && g.Wo == g.Wi, "block %d: residual block changes the shape", b);
                            CHECK(at == (((size_t)img * g.Hp + (yq - g.opad + g.ipad)) * g.Wp + (xq - g.opad + g.ipad)) * g.cinp,
                                  "block %d: residual pixel", b);
                            res = in + at;
                        }
                        for (int nt = 0; nt < NT; ++nt) {
                            const int co = (nt0 + nt) * 32 + r;
                            CHECK(co < g.cout, "block %d: channel %d of %d", b, co, g.cout);
                            if (res) {
                                sink = sink + res[co];
                                ++reads;
                            }
                            stored[o + co] += 1;
                            ++stores;
                        }
                    }
            }
        }
    size_t bad = 0;
    for (size_t i = 0; i < out_elems; ++i) bad += stored[i] != 1;
    CHECK(bad == 0, "block %d, n %d, NT %d: %zu of %zu output elements not stored exactly once", b, n, NT, bad, out_elems);
    if (print)
        printf("%d %d %d %d %d %d %d %d %d %d %llu %llu\n", n, b, g.Hi, g.Wi, g.Ho, g.Wo, g.Hq, g.Wq, g.cout, NT, reads, stores);
    delete[] in;
    delete[] stored;
}

// conv_net_pack_kernel for block b -- one thread per element e of the packed matrix -- and then every weight read of the MFMA step
// over the column tiles of syncnet_conv_kernel<NT>.  packed[e] stands for what the kernel stores at e: 1 + the index of
// w[n][ci][ky][kx], or 0 where it stores zero.  The decode must hit every (k, n) once and use every weight once; the reader must
// stay inside the matrix, take every element once, and find at the address of (K step s, tile, lane, j) the weight of the k its A
// operand holds there and of the column the epilogue stores that tile's lane to: zero for the padded channels ci >= C_in, where
// the layout kernel wrote zero activations.
static void walk_pack(int b, int NT) {
    const SnGeom g = sn_geom(b);
    const int cin = SN_TABLE[b].cin, taps = g.kh * g.kw, ntiles = g.cout / 32, ntn = g.cout / (32 * NT);
    const size_t elems = (size_t)g.K * g.cout, weights = (size_t)g.cout * cin * taps;
    std::vector<size_t> packed(elems, 0);
    std::vector<int> decoded(elems, 0), used(weights, 0), read(elems, 0);
    for (size_t e = 0; e < elems; ++e) {
        int k, n;
        cf_pack_decode(e, ntiles, &k, &n);
        CHECK(k >= 0 && k < g.K && n >= 0 && n < g.cout, "block %d: element %zu decodes to (%d, %d)", b, e, k, n);
        if (k < 0 || k >= g.K || n < 0 || n >= g.cout) continue;
        ++decoded[(size_t)k * g.cout + n];
        const int tap = k / g.cinp, ci = k - tap * g.cinp;
        if (ci < cin) {
            const size_t w = ((size_t)n * cin + ci) * taps + tap;
            CHECK(w < weights, "block %d: element %zu reads weight %zu of %zu", b, e, w, weights);
            if (w >= weights) continue;
            ++used[w];
            packed[e] = 1 + w;
        }
    }
    size_t bad = 0;
    for (size_t i = 0; i < elems; ++i) bad += decoded[i] != 1;
    CHECK(bad == 0, "block %d: %zu of %zu (k, n) not packed exactly once", b, bad, elems);
    bad = 0;
    for (size_t w = 0; w < weights; ++w) bad += used[w] != 1;
    CHECK(bad == 0, "block %d: %zu of %zu weights not packed exactly once", b, bad, weights);
    for (int tn = 0; tn < ntn; ++tn)  // nt0 = (tile % ntn) * NT
        for (int s = 0; s < g.K / 16; ++s)
            for (int nt = 0; nt < NT; ++nt)
                for (int lane = 0; lane < 64; ++lane) {
                    CHECK(cf_frag_elem(s, ntiles, tn * NT, nt, lane, 0) == 8 * cf_frag_group(s, ntiles, tn * NT, nt, lane), "block %d: group", b);
                    for (int j = 0; j < 8; ++j) {  // one 16-byte load of 8 bf16
                        const size_t e = cf_frag_elem(s, ntiles, tn * NT, nt, lane, j);
                        CHECK(e < elems, "block %d: the step reads element %zu of %zu", b, e, elems);
                        if (e >= elems) continue;
                        ++read[e];
                        const int k = 16 * s + 8 * (lane >> 5) + j;           // what the A operand holds in this position
                        const int n = (tn * NT + nt) * 32 + (lane & 31);      // the epilogue's co
                        int dk, dn;
                        cf_pack_decode(e, ntiles, &dk, &dn);
                        CHECK(dk == k && dn == n, "block %d: the step reads (%d, %d) where the pack put (%d, %d)", b, k, n, dk, dn);
                        const int tap = k / g.cinp, ci = k % g.cinp;
                        const size_t want = ci < cin ? 1 + ((size_t)n * cin + ci) * taps + tap : 0;
                        CHECK(packed[e] == want, "block %d: (k, n) = (%d, %d) holds %zu, expected %zu", b, k, n, packed[e], want);
                    }
                }
    bad = 0;
    for (size_t e = 0; e < elems; ++e) bad += read[e] != 1;
    CHECK(bad == 0, "block %d, NT %d: %zu of %zu packed elements not read exactly once", b, NT, bad, elems);
}

// the prologue's addresses: every element of one face window of an H x W frame under `box`
static void walk_faces(int H, int W, int b0, int b1, int b2, int b3) {
    float* frame = new float[(size_t)H * W];
    for (size_t i = 0; i < (size_t)H * W; ++i) frame[i] = 0.5f;
    const int box[4] = {b0, b1, b2, b3};
    int y1, h, x1, w;
    cn_clamp_box(box, H, W, &y1, &h, &x1, &w);
    CHECK(y1 >= 0 && h >= 1 && y1 + h <= H && x1 >= 0 && w >= 1 && x1 + w <= W, "box (%d,%d,%d,%d) clamps outside %dx%d", b0, b1, b2, b3, H, W);
    volatile float sink = 0.0f;
    for (int y = 0; y < SN_FACE_H; ++y)
        for (int x = 0; x < SN_FACE_W; ++x) {
            int ya, yb, xa, xb;
            double wy, wx;
            cn_bilinear(SN_CROP - SN_FACE_H + y, h, SN_CROP, &ya, &yb, &wy);
            cn_bilinear(x, w, SN_CROP, &xa, &xb, &wx);
            CHECK(ya >= 0 && ya <= yb && yb < h && xa >= 0 && xa <= xb && xb < w && wy >= 0.0 && wy <= 1.0 && wx >= 0.0 && wx <= 1.0,
                  "bilinear (%d,%d) of a %dx%d crop", y, x, h, w);
            sink = sink + frame[(size_t)(y1 + ya) * W + (x1 + xa)] + frame[(size_t)(y1 + ya) * W + (x1 + xb)] +
                   frame[(size_t)(y1 + yb) * W + (x1 + xa)] + frame[(size_t)(y1 + yb) * W + (x1 + xb)];
        }
    delete[] frame;
}

int main(int argc, char** argv) {
    std::vector<int> counts;
    for (int i = 1; i < argc; ++i) counts.push_back(atoi(argv[i]));
    if (counts.empty()) counts = {1, 2, 3};
    // the table chains: a block's output map IS the next block's input map, and the encoders end in [n, 1, 1, 512]
    for (int b = 0; b < SN_BLOCKS; ++b) {
        const SnGeom g = sn_geom(b);
        CHECK(g.K % 16 == 0 && g.cinp % 16 == 0 && g.cout % 32 == 0, "block %d: K %d, cinp %d, cout %d", b, g.K, g.cinp, g.cout);
        CHECK(sn_in_elems(&g, 1) <= sn_max_map_elems() && sn_out_elems(&g, 1) <= sn_max_map_elems(), "block %d exceeds the largest map", b);
        walk_pack(b, 1);
        if (g.cout % 64 == 0) walk_pack(b, 2);
        if (b == SN_FACE_BLOCKS - 1 || b == SN_BLOCKS - 1) {
            CHECK(g.Ho == 1 && g.Wo == 1 && g.opad == 0 && g.cout == SN_EMB, "block %d does not end in a 512-vector", b);
        } else {
            const SnGeom nx = sn_geom(b + 1);
            CHECK(nx.Hi == g.Ho && nx.Wi == g.Wo && nx.ipad == g.opad && nx.cinp == g.cout && nx.Hp == g.Hq && nx.Wp == g.Wq,
                  "block %d's output is not block %d's input", b, b + 1);
        }
    }
    for (int n : counts) {
        if (n < 1 || n > SN_MAX_WINDOWS) {
            fprintf(stderr, "window count %d outside 1..%d\n", n, SN_MAX_WINDOWS);
            return 2;
        }
        for (int b = 0; b < SN_BLOCKS; ++b) {
            const SnGeom g = sn_geom(b);
            const int nt = cn_wave_ntiles((long long)n * g.Hq * g.Wq, g.cout);
            CHECK((nt == 1 || nt == 2) && g.cout % (32 * nt) == 0, "block %d: %d tiles a wave do not divide C_out %d", b, nt, g.cout);
            walk_conv(b, n, nt, true);
            if (n == counts[0] && g.cout % 64 == 0) walk_conv(b, n, 3 - nt, false);  // the other instantiation too, once
        }
    }
    walk_faces(160, 160, 7, 138, 20, 137);   // an odd 131 x 117 box
    walk_faces(160, 160, 0, 160, 0, 160);    // the whole frame
    walk_faces(160, 160, 100, 160, 90, 160); // touching the bottom-right corner
    walk_faces(32, 32, 0, 32, 0, 32);        // upsampled 3 x
    walk_faces(2, 2, 0, 1, 1, 2);            // a single pixel
    walk_faces(64, 48, -5, 900, 40, 7);      // a box the kernel must clamp
    return g_fail ? 1 : 0;
}
