// The index arithmetic of csrc/wav2lip_core.h walked on the CPU over the grid of csrc/wav2lip.hip's convolution kernel, for all 51
// blocks and the window counts given on the command line (default 1 3 65), and the weight pack of every block and class against the
// addresses the MFMA step reads it at.  The loop nest below is RE-TYPED from wav2lip_conv_kernel (block / wave / class / lane / K
// step), and so are wav2lip_pack_kernel's weight lookup and the flat decodes of the head and layout kernels: a change there must be
// made here too.  NOT re-typed, but the very functions the kernels are compiled from: wav2lip_core.h's (table, geometry, classes,
// row -> cell, input cell, tap offset), syncnet_core.h's (row decode, clamp, interior, resample, box clamp) and conv_frag.h's.
// Built by tests/test_wav2lip_cpu.py with the host compiler under -fsanitize=address,undefined.  The maps are heap blocks (one
// byte per element: only addresses are walked) in their chain form: a block that reads or writes a concatenation buffer gets a
// block of that buffer's size (w2l_cat_elems, what the workspace carves for it), with its row stride and channel offset; a map of
// its own is a block of exactly the map's size (w2l_in_elems / w2l_out_elems), which main checks against the size of the two
// alternating maps the workspace carves (w2l_max_map_elems) -- for the chain and for the single-block entry point, which lays a
// block's input out where the chain holds it.  So a read or a store outside one ends the program through the sanitizer; a tap
// that is not the convolution's, a cell stored twice or never, a concatenation buffer whose two producers do not cover it exactly
// once fails the program's own check (exit code 1).
// The K loop is walked for the waves of the first column tile only: the A addresses do not depend on the column tile.
// Prints one line per (n, block): n block Hi Wi Ho Wo Hq Wq C_out tiles-per-wave classes reads stores.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/conv_frag.h"
#include "../nerf-3dtalker-code_amd/csrc/wav2lip_core.h"

static int g_fail = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            fprintf(stderr, __VA_ARGS__);        \
            fprintf(stderr, "\n");               \
            if (++g_fail > 20) exit(1);          \
        }                                        \
    } while (0)

typedef std::vector<unsigned char> Bytes;

// one launch of wav2lip_conv_kernel<NT> over block `b` for n windows.  `in` holds in_elems bytes and the block reads cells of
// istride at channel in_off; `stored` counts the stores into the output buffer (cells of ostride, channel out_off)
static void walk_conv(int b, int n, int NT, const unsigned char* in, int in_off, int istride, unsigned char* stored, int out_off, int ostride,
                      unsigned long long* reads_out, unsigned long long* stores_out, int* ncls_out) {
    const W2lGeom g = w2l_geom(b);
    unsigned long long reads = 0, stores = 0;
    volatile unsigned sink = 0;
    W2lClass cls[W2L_MAX_CLASSES];
    long long tiles;
    const int ncls = w2l_classes(&g, n, NT, cls, &tiles);
    CHECK(ncls >= 1 && ncls <= W2L_MAX_CLASSES, "block %d: %d classes", b, ncls);
    CHECK(g.np % (32 * NT) == 0, "block %d: np %d is no multiple of %d", b, g.np, 32 * NT);
    const int ntn = g.np / (32 * NT);
    const size_t block_elems = w2l_packed_elems(b);
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    const unsigned char* inb = in + in_off;
    unsigned char* outb = stored + out_off;
    for (unsigned block = 0; block < grid; ++block)
        for (int wave = 0; wave < 4; ++wave) {
            const long long tile = (long long)block * 4 + wave;
            W2lClass k = cls[0];
            for (int c = 1; c < W2L_MAX_CLASSES; ++c)
                if (c < ncls && tile >= cls[c].tile0) k = cls[c];
            const long long Mc = w2l_class_rows(&k, n);
            const long long lt = tile - k.tile0;
            const long long m0 = lt / ntn * CN_TILE_M;
            if (m0 >= Mc) continue;
            const int nt0 = (int)(lt % ntn) * NT;
            const int taps = k.tkh * k.tkw;
            const size_t class_elems = (size_t)taps * g.cinp * g.np;
            CHECK((size_t)k.woff + 2 * class_elems <= block_elems, "block %d: class matrices leave the block's %zu elements", b, block_elems);
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, h = lane >> 5;
                if (nt0 == 0) {
                    size_t base[2];
                    int py[2], px[2], pin[2];
                    for (int mt = 0; mt < 2; ++mt) {
                        int img, yq, xq;
                        w2l_row_cell(m0 + mt * 32 + r, Mc, k.oy, k.ox, k.Hc, k.Wc, k.step, &img, &yq, &xq);
                        CHECK(img >= 0 && img < n && yq >= 0 && yq < g.Hq && xq >= 0 && xq < g.Wq, "block %d: row decodes outside the map", b);
                        py[mt] = cn_clampi(yq - g.opad, 0, g.Ho - 1);
                        px[mt] = cn_clampi(xq - g.opad, 0, g.Wo - 1);
                        pin[mt] = cn_interior(yq, xq, g.Ho, g.Wo, g.opad);
                        base[mt] = w2l_cell(img, w2l_in_cell(py[mt], g.tr, g.sh, g.ihalo, g.pad), w2l_in_cell(px[mt], g.tr, g.sw, g.ihalo, g.pad), g.Hp,
                                            g.Wp, istride);
                    }
                    int s = 0;
                    for (int tap = 0; tap < taps; ++tap) {
                        const size_t toff = w2l_tap_offset(tap, k.tkw, g.Wp, istride) + 8 * h;
                        const int kid = g.tr ? k.kidx[tap] : tap, ky = kid / g.kw, kx = kid % g.kw;
                        for (int c0 = 0; c0 < g.cinp; c0 += 16, ++s) {
                            for (int mt = 0; mt < 2; ++mt) {
                                const unsigned char* p = inb + base[mt] + toff + c0;
                                if (pin[mt] && c0 == 0) {
                                    // the cell this tap reads must be the one the (transposed) convolution pairs with kernel element
                                    // (ky, kx) at output pixel (y, x): Conv2d i = y s - pad + ky; ConvTranspose2d y = i s - pad + ky
                                    const size_t cell = (size_t)(p - inb - 8 * h) / istride;
                                    const int ix = (int)(cell % g.Wp) - g.ihalo, iy = (int)(cell / g.Wp % g.Hp) - g.ihalo;
                                    if (g.tr)
                                        CHECK(py[mt] == iy * g.sh - g.pad + ky && px[mt] == ix * g.sw - g.pad + kx,
                                              "block %d: pixel (%d, %d) tap (%d, %d) reads input (%d, %d)", b, py[mt], px[mt], ky, kx, iy, ix);
                                    else
                                        CHECK(iy == py[mt] * g.sh - g.pad + ky && ix == px[mt] * g.sw - g.pad + kx,
                                              "block %d: pixel (%d, %d) tap (%d, %d) reads input (%d, %d)", b, py[mt], px[mt], ky, kx, iy, ix);
                                    CHECK(iy >= -g.ihalo && iy < g.Hi + g.ihalo && ix >= -g.ihalo && ix < g.Wi + g.ihalo, "block %d: tap leaves the padded map", b);
                                }
                                unsigned acc = 0;
                                for (int j = 0; j < 8; ++j) acc += p[j];
                                sink = sink + acc;
                                reads += 8;
                            }
                            for (int nt = 0; nt < NT; ++nt) {
                                const size_t f = cf_frag_group(s, g.np >> 5, nt0, nt, lane);
                                CHECK(f * 8 + 8 <= class_elems, "block %d: weight fragment %zu of a class of %zu elements", b, f, class_elems);
                            }
                        }
                    }
                    CHECK(s == taps * g.cinp / 16, "block %d: %d K steps, expected %d", b, s, taps * g.cinp / 16);
                }
                for (int mt = 0; mt < 2; ++mt)
                    for (int i = 0; i < 16; ++i) {
                        const long long m = m0 + mt * 32 + cf_acc_row(i, h);
                        if (m >= Mc) continue;
                        int img, yq, xq;
                        w2l_row_cell(m, Mc, k.oy, k.ox, k.Hc, k.Wc, k.step, &img, &yq, &xq);
                        const bool inside = cn_interior(yq, xq, g.Ho, g.Wo, g.opad);
                        unsigned char* o = outb + w2l_cell(img, yq, xq, g.Hq, g.Wq, ostride);
                        const unsigned char* res = nullptr;
                        if (inside && g.residual) {
                            CHECK(g.cinp == g.cout && g.Ho == g.Hi && g.Wo == g.Wi && !g.tr, "block %d: residual block changes the shape", b);
                            res = inb + w2l_cell(img, yq - g.opad + g.ihalo, xq - g.opad + g.ihalo, g.Hp, g.Wp, istride);
                        }
                        for (int nt = 0; nt < NT; ++nt) {
                            const int co = (nt0 + nt) * 32 + r;
                            if (co >= g.cout) continue;
                            if (res) {
                                sink = sink + res[co];
                                ++reads;
                            }
                            o[co] += 1;
                            ++stores;
                        }
                    }
            }
        }
    *reads_out = reads;
    *stores_out = stores;
    *ncls_out = ncls;
}

// wav2lip_pack_kernel for every class of block b, then every weight read of the MFMA step over the column tiles of
// wav2lip_conv_kernel<NT>.  packed[e] stands for what the kernel stores at e: 1 + the index of the weight, or 0 where it stores zero.
static void walk_pack(int b, int NT) {
    const W2lGeom g = w2l_geom(b);
    W2lClass cls[W2L_MAX_CLASSES];
    long long tiles;
    const int ncls = w2l_classes(&g, 1, NT, cls, &tiles);
    const int taps_full = g.kh * g.kw, ntiles = g.np / 32, ntn = g.np / (32 * NT);
    const size_t weights = (size_t)g.cout * g.cin * taps_full, block_elems = w2l_packed_elems(b);
    std::vector<int> used(weights, 0);
    std::vector<unsigned char> covered(block_elems, 0);
    for (int c = 0; c < ncls; ++c) {
        const int taps = cls[c].tkh * cls[c].tkw, Kc = taps * g.cinp;
        const size_t elems = (size_t)Kc * g.np;
        CHECK(taps >= 1 && taps <= (g.tr ? 4 : taps_full), "block %d class %d: %d taps", b, c, taps);
        std::vector<size_t> packed(elems, 0);
        std::vector<int> decoded(elems, 0), read(elems, 0);
        for (int part = 0; part < 2; ++part)  // hi, then lo
            for (size_t e = 0; e < elems; ++e) {
                const size_t at = (size_t)cls[c].woff + part * elems + e;
                CHECK(at < block_elems, "block %d class %d: element %zu of %zu", b, c, at, block_elems);
                if (at < block_elems) covered[at] += 1;
            }
        for (size_t e = 0; e < elems; ++e) {
            int k, n;
            cf_pack_decode(e, ntiles, &k, &n);
            CHECK(k >= 0 && k < Kc && n >= 0 && n < g.np, "block %d: element %zu decodes to (%d, %d)", b, e, k, n);
            if (k < 0 || k >= Kc || n < 0 || n >= g.np) continue;
            ++decoded[(size_t)k * g.np + n];
            const int tap = k / g.cinp, ci = k - tap * g.cinp;
            const int kid = !g.tr ? tap : cls[c].kidx[tap];
            CHECK(kid >= 0 && kid < taps_full, "block %d class %d: tap %d is kernel element %d", b, c, tap, kid);
            if (ci < g.cin && n < g.cout) {
                const size_t w = g.tr ? ((size_t)ci * g.cout + n) * taps_full + kid : ((size_t)n * g.cin + ci) * taps_full + kid;
                CHECK(w < weights, "block %d: element %zu reads weight %zu of %zu", b, e, w, weights);
                if (w >= weights) continue;
                ++used[w];
                packed[e] = 1 + w;
            }
        }
        size_t bad = 0;
        for (size_t i = 0; i < elems; ++i) bad += decoded[i] != 1;
        CHECK(bad == 0, "block %d class %d: %zu of %zu (k, n) not packed exactly once", b, c, bad, elems);
        for (int tn = 0; tn < ntn; ++tn)
            for (int s = 0; s < Kc / 16; ++s)
                for (int nt = 0; nt < NT; ++nt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const size_t e = cf_frag_elem(s, ntiles, tn * NT, nt, lane, j);
                            CHECK(e < elems, "block %d: the step reads element %zu of %zu", b, e, elems);
                            if (e >= elems) continue;
                            ++read[e];
                            const int k = 16 * s + 8 * (lane >> 5) + j;       // what the A operand holds in this position
                            const int n = (tn * NT + nt) * 32 + (lane & 31);  // the epilogue's co
                            const int tap = k / g.cinp, ci = k % g.cinp;
                            const int kid = !g.tr ? tap : cls[c].kidx[tap];
                            size_t want = 0;
                            if (ci < g.cin && n < g.cout) want = 1 + (g.tr ? ((size_t)ci * g.cout + n) * taps_full + kid : ((size_t)n * g.cin + ci) * taps_full + kid);
                            CHECK(packed[e] == want, "block %d class %d: (k, n) = (%d, %d) holds %zu, expected %zu", b, c, k, n, packed[e], want);
                        }
        bad = 0;
        for (size_t e = 0; e < elems; ++e) bad += read[e] != 1;
        CHECK(bad == 0, "block %d class %d, NT %d: %zu of %zu packed elements not read exactly once", b, c, NT, bad, elems);
    }
    size_t bad = 0;
    for (size_t w = 0; w < weights; ++w) bad += used[w] != 1;
    CHECK(bad == 0, "block %d: %zu of %zu weights not packed exactly once over its classes", b, bad, weights);
    bad = 0;
    for (size_t e = 0; e < block_elems; ++e) bad += covered[e] != 1;
    CHECK(bad == 0, "block %d: %zu of %zu packed elements belong to no class or to two", b, bad, block_elems);
}

// the prologue's and the paste's addresses: every element of one frame of H x W under `box`
static void walk_frames(int H, int W, int b0, int b1, int b2, int b3) {
    Bytes frame((size_t)H * W, 1), face((size_t)W2L_IMG * W2L_IMG, 1);
    const int box[4] = {b0, b1, b2, b3};
    int y1, h, x1, w;
    cn_clamp_box(box, H, W, &y1, &h, &x1, &w);
    CHECK(y1 >= 0 && h >= 1 && y1 + h <= H && x1 >= 0 && w >= 1 && x1 + w <= W, "box (%d,%d,%d,%d) clamps outside %dx%d", b0, b1, b2, b3, H, W);
    volatile unsigned sink = 0;
    const unsigned char* fr = frame.data();
    const unsigned char* fa = face.data();
    for (int y = 0; y < W2L_IMG; ++y)
        for (int x = 0; x < W2L_IMG; ++x) {
            int ya, yb, xa, xb;
            double wy, wx;
            cn_bilinear(y, h, W2L_IMG, &ya, &yb, &wy);
            cn_bilinear(x, w, W2L_IMG, &xa, &xb, &wx);
            CHECK(ya >= 0 && ya <= yb && yb < h && xa >= 0 && xa <= xb && xb < w && wy >= 0.0 && wy <= 1.0 && wx >= 0.0 && wx <= 1.0,
                  "bilinear (%d,%d) of a %dx%d crop", y, x, h, w);
            sink = sink + fr[(size_t)(y1 + ya) * W + (x1 + xa)] + fr[(size_t)(y1 + ya) * W + (x1 + xb)] + fr[(size_t)(y1 + yb) * W + (x1 + xa)] +
                   fr[(size_t)(y1 + yb) * W + (x1 + xb)];
        }
    for (int y = y1; y < y1 + h; ++y)
        for (int x = x1; x < x1 + w; ++x) {
            int ya, yb, xa, xb;
            double wy, wx;
            cn_bilinear(y - y1, W2L_IMG, h, &ya, &yb, &wy);
            cn_bilinear(x - x1, W2L_IMG, w, &xa, &xb, &wx);
            CHECK(ya >= 0 && yb < W2L_IMG && xa >= 0 && xb < W2L_IMG && wy >= 0.0 && wy <= 1.0 && wx >= 0.0 && wx <= 1.0, "paste (%d,%d) of a %dx%d box", y, x, h, w);
            sink = sink + fa[(size_t)ya * W2L_IMG + xa] + fa[(size_t)ya * W2L_IMG + xb] + fa[(size_t)yb * W2L_IMG + xa] + fa[(size_t)yb * W2L_IMG + xb];
        }
}

int main(int argc, char** argv) {
    std::vector<int> counts;
    for (int i = 1; i < argc; ++i) counts.push_back(atoi(argv[i]));
    if (counts.empty()) counts = {1, 3, 65};
    // the table chains: a block's output map IS the next block's input map, a concatenation buffer is its two producers' slices
    for (int b = 0; b < W2L_BLOCKS; ++b) {
        const W2lGeom g = w2l_geom(b);
        CHECK(g.K % 16 == 0 && g.cinp % 16 == 0 && g.np % 32 == 0 && g.istride % 16 == 0 && g.in_off % 16 == 0 && g.out_off % 16 == 0,
              "block %d: K %d, cinp %d, np %d", b, g.K, g.cinp, g.np);
        CHECK(g.ihalo >= g.pad || g.tr, "block %d: halo %d below its padding %d", b, g.ihalo, g.pad);
        CHECK(!g.tr || g.sh == 1 || g.ihalo >= 1, "block %d: a stride-2 transposed block needs the halo cell behind the last row", b);
        if (g.in_cat >= 0) {
            const int j = g.in_cat;
            CHECK(g.Hi == W2L_CAT_HW[j] && g.Wi == W2L_CAT_HW[j] && g.ihalo == W2L_CAT_HALO[j] && g.in_off + g.cinp <= W2L_CAT_C[j] && g.cin == g.cinp,
                  "block %d does not read CAT %d", b, j);
        } else if (b != 0 && b != W2L_FIRST_AUDIO) {
            const W2lGeom p = w2l_geom(b - 1);
            CHECK(p.Ho == g.Hi && p.Wo == g.Wi && p.opad == g.ihalo && p.cout == g.cinp && p.Hq == g.Hp && p.Wq == g.Wp,
                  "block %d's output is not block %d's input", b - 1, b);
            CHECK(w2l_in_elems(&g, 1) <= w2l_max_map_elems(), "block %d's input exceeds the largest map", b);
        }
        if (g.out_cat >= 0) {
            const int j = g.out_cat;
            CHECK(g.Ho == W2L_CAT_HW[j] && g.Wo == W2L_CAT_HW[j] && g.opad == W2L_CAT_HALO[j] && g.out_stride == W2L_CAT_C[j] &&
                      (b < W2L_FIRST_AUDIO ? g.out_off == W2L_CAT_A[j] && g.cout == W2L_CAT_C[j] - W2L_CAT_A[j] : g.out_off == 0 && g.cout == W2L_CAT_A[j]),
                  "block %d does not write its slice of CAT %d", b, j);
        }
        CHECK(w2l_out_elems(&g, 1) <= w2l_max_map_elems(), "block %d's output exceeds the largest map", b);
        // where the single-block entry point lays the input out (n3dt_launch_wav2lip_block): channels in_off .. in_off + cinp - 1 of
        // every cell of the CAT buffer the chain reads it from, or a map; and with a skip feature its output CAT buffer must be free
        if (g.in_cat >= 0)
            CHECK((size_t)(g.Hp * g.Wp - 1) * g.istride + g.in_off + g.cinp <= w2l_cat_elems(g.in_cat) && g.istride == W2L_CAT_C[g.in_cat],
                  "block %d's input laid out in CAT %d leaves the buffer", b, g.in_cat);
        else
            CHECK(w2l_in_elems(&g, 1) <= w2l_max_map_elems() && g.istride == g.cinp, "block %d's input exceeds the largest map", b);
        CHECK(!(b >= W2L_FIRST_DEC && g.out_cat >= 0 && g.in_cat >= 0), "block %d reads a CAT buffer and ends in one", b);
        if (b == W2L_HEAD) continue;
        walk_pack(b, 1);
        if (g.np % 64 == 0) walk_pack(b, 2);
    }
    {
        const W2lGeom last = w2l_geom(W2L_HEAD), out = w2l_geom(W2L_OUT_BLOCK);
        CHECK(last.Hi == W2L_IMG && last.Wi == W2L_IMG && last.ihalo == 0 && last.cin == W2L_HEAD_C && last.cout == W2L_OUT_C && out.cout == W2L_HEAD_C,
              "the head does not read [96, 96, 32]");
    }
    for (int n : counts) {
        if (n < 1 || n > W2L_MAX_WINDOWS) {
            fprintf(stderr, "window count %d outside 1..%d\n", n, W2L_MAX_WINDOWS);
            return 2;
        }
        std::vector<Bytes> cat(W2L_CATS);  // the stores of a whole forward into the concatenation buffers
        for (int j = 0; j < W2L_CATS; ++j) cat[j].assign((size_t)n * w2l_cat_elems(j), 0);
        for (int b = 0; b < W2L_HEAD; ++b) {
            const W2lGeom g = w2l_geom(b);
            const int nt = w2l_wave_ntiles(&g, n);
            CHECK((nt == 1 || nt == 2) && g.np % (32 * nt) == 0, "block %d: %d tiles a wave do not divide the %d columns", b, nt, g.np);
            for (int pass = 0; pass < 2; ++pass) {  // the chain's instantiation, then (once) the other one
                const int NT = pass == 0 ? nt : 3 - nt;
                if (pass == 1 && !(n == counts[0] && g.np % 64 == 0)) continue;
                Bytes own_in, own_out;
                const unsigned char* in;
                if (g.in_cat >= 0) {
                    own_in.assign((size_t)n * w2l_cat_elems(g.in_cat), 1);
                } else {
                    own_in.assign(w2l_in_elems(&g, n), 1);
                }
                in = own_in.data();
                unsigned char* stored;
                if (g.out_cat >= 0 && pass == 0) {
                    stored = cat[g.out_cat].data();
                } else {
                    own_out.assign(g.out_cat >= 0 ? (size_t)n * w2l_cat_elems(g.out_cat) : w2l_out_elems(&g, n), 0);
                    stored = own_out.data();
                }
                unsigned long long reads, stores;
                int ncls;
                walk_conv(b, n, NT, in, g.in_off, g.istride, stored, g.out_off, g.out_stride, &reads, &stores, &ncls);
                if (!own_out.empty()) {  // a map of its own: every element once; a slice of a buffer: the slice once, nothing else
                    size_t bad = 0;
                    for (size_t i = 0; i < own_out.size(); ++i) {
                        const int c = (int)(i % g.out_stride);
                        bad += own_out[i] != ((c >= g.out_off && c < g.out_off + g.cout) ? 1 : 0);
                    }
                    CHECK(bad == 0, "block %d, n %d, NT %d: %zu of %zu output elements not stored exactly once", b, n, NT, bad, own_out.size());
                }
                CHECK(stores == (unsigned long long)n * g.Hq * g.Wq * g.cout, "block %d, n %d: %llu stores", b, n, stores);
                if (pass == 0)
                    printf("%d %d %d %d %d %d %d %d %d %d %d %llu %llu\n", n, b, g.Hi, g.Wi, g.Ho, g.Wo, g.Hq, g.Wq, g.cout, NT, ncls, reads, stores);
            }
        }
        for (int j = 0; j < W2L_CATS; ++j) {
            size_t bad = 0;
            for (size_t i = 0; i < cat[j].size(); ++i) bad += cat[j][i] != 1;
            CHECK(bad == 0, "n %d: %zu of %zu elements of CAT %d not stored exactly once by its two producers", n, bad, cat[j].size(), j);
        }
        {  // the head: one thread per pixel reads 32 channels of [n, 96, 96, 32] and stores three planes of [n, 3, 96, 96]
            const size_t hw = (size_t)W2L_IMG * W2L_IMG, total = (size_t)n * hw;
            Bytes in(total * W2L_HEAD_C, 1), out(total * W2L_OUT_C, 0);
            const W2lGeom g = w2l_geom(W2L_HEAD);
            CHECK(in.size() == w2l_in_elems(&g, n) && out.size() == w2l_out_elems(&g, n), "the head's maps");
            volatile unsigned sink = 0;
            const unsigned char* p = in.data();
            for (size_t e = 0; e < total; ++e) {
                const size_t img = e / hw, px = e - img * hw;
                for (int c = 0; c < W2L_HEAD_C; ++c) sink = sink + p[e * W2L_HEAD_C + c];
                for (int o = 0; o < W2L_OUT_C; ++o) out[(img * W2L_OUT_C + o) * hw + px] += 1;
            }
            size_t bad = 0;
            for (size_t i = 0; i < out.size(); ++i) bad += out[i] != 1;
            CHECK(bad == 0, "head, n %d: %zu output elements not stored exactly once", n, bad);
            printf("%d %d %d %d %d %d %d %d %d %d %d %llu %llu\n", n, W2L_HEAD, g.Hi, g.Wi, g.Ho, g.Wo, g.Hq, g.Wq, g.cout, 0, 1,
                   (unsigned long long)in.size(), (unsigned long long)out.size());
        }
    }
    walk_frames(160, 160, 7, 138, 20, 137);   // an odd 131 x 117 box
    walk_frames(160, 160, 0, 160, 0, 160);    // the whole frame
    walk_frames(160, 160, 100, 160, 90, 160); // touching the bottom-right corner
    walk_frames(32, 32, 0, 32, 0, 32);        // upsampled 3 x
    walk_frames(2, 2, 0, 1, 1, 2);            // a single pixel
    walk_frames(64, 48, -5, 900, 40, 7);      // a box the kernel must clamp
    return g_fail ? 1 : 0;
}
