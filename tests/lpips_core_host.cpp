// csrc/lpips_core.h -- the index arithmetic the LPIPS kernels (csrc/lpips.hip) are compiled from -- walked on the CPU over the
// kernels' full grids: every workgroup, wave, lane and K step of the five implicit-GEMM convolutions (rows past M included), the
// epilogue's stores, both pools, the halo kernel's cells, the prologue's reinterpretation and the weight pack of every layer
// against the addresses the MFMA step reads it at.  Every buffer is a std::vector of
// exactly the size the workspace gives it and holds, per element, the LOGICAL coordinate it stands for, so an index that leaves
// its buffer ends the program through the address sanitizer and an index that stays inside but names the wrong element fails a
// check.
//
// The loop nests below (block / wave / lane / K step, the pool's and the halo kernel's element decodes, the pack kernel's weight
// lookup) are RE-TYPED from lpips_conv_kernel, lpips_pool_kernel, lpips_halo_kernel and lpips_pack_kernel in csrc/lpips.hip.  A
// change to one of those loops there must be made here too, or this program checks a kernel that no longer exists.  NOT re-typed,
// but the very functions the kernels are compiled from: the lp_* functions of lpips_core.h, and from csrc/conv_frag.h the
// epilogue's register -> row map (cf_acc_row), the pack kernel's element decode (cf_pack_decode) and the address the MFMA step
// reads its weight fragments at (cf_frag_group / cf_frag_elem).
// Not walked: the flat element decodes of the prologue's output and of the distance kernel.
//
// usage: lpips_core_host B H W [B H W ...]; prints one line per shape: B H W fh1 fw1 ... fh5 fw5 reads
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/conv_frag.h"
#include "../nerf-3dtalker-code_amd/csrc/lpips_core.h"

struct Cell {
    int img, y, x, c;  // y == -1: halo (must read as zero)
};

static long long g_reads = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "lpips_core_host: " __VA_ARGS__); \
            fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); \
            exit(2);                                      \
        }                                                 \
    } while (0)

// a padded NHWC map [n, H + 2 pad, W + 2 pad, C] labelled with its logical coordinates
static std::vector<Cell> labelled(int n, int H, int W, int pad, int C) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    std::vector<Cell> m((size_t)n * Hp * Wp * C);
    size_t e = 0;
    for (int img = 0; img < n; ++img)
        for (int yp = 0; yp < Hp; ++yp)
            for (int xp = 0; xp < Wp; ++xp)
                for (int c = 0; c < C; ++c) {
                    const bool in = yp >= pad && yp < Hp - pad && xp >= pad && xp < Wp - pad;
                    m[e++] = in ? Cell{img, yp - pad, xp - pad, c} : Cell{img, -1, -1, c};
                }
    return m;
}

static void expect_tap(const Cell& got, int img, int y, int x, int c, int H, int W, int layer, int k) {
    const bool inside = y >= 0 && y < H && x >= 0 && x < W;
    if (inside)
        CHECK(got.img == img && got.y == y && got.x == x && got.c == c, "layer %d k %d: read (%d,%d,%d,%d), expected (%d,%d,%d,%d)", layer, k,
              got.img, got.y, got.x, got.c, img, y, x, c);
    else
        CHECK(got.img == img && got.y == -1, "layer %d k %d: expected the halo of image %d, read (%d,%d,%d,%d)", layer, k, img, got.img, got.y,
              got.x, got.c);
}

// the conv kernel's loads and stores for layer l: in [n, Hi + 2 pad, Wi + 2 pad, cin] -> writes counted in `out`
static void walk_conv(int l, int n, int Hi, int Wi, const std::vector<Cell>& in, size_t in_elems, int Ho, int Wo, std::vector<int>& out) {
    const int cin = lp_cin(l), cout = lp_cout(l), ks = lp_ksize(l), stride = lp_stride(l), pad = lp_pad(l);
    const int Hp = Hi + 2 * pad, Wp = Wi + 2 * pad, K = lp_k(l), kp = lp_kp(l), out_pad = lp_feat_pad(l);
    CHECK(in.size() == in_elems, "layer %d: input has %zu elements, the workspace gives it %zu", l, in.size(), in_elems);
    CHECK(Ho == lp_conv_out(Hi, ks, stride, pad) && Wo == lp_conv_out(Wi, ks, stride, pad), "layer %d: output extent", l);
    CHECK(cout % LP_TILE_N == 0 && (l == 0 || cin % 16 == 0) && kp % 16 == 0 && kp >= K && kp - K < 16, "layer %d: tile divisibility", l);
    const long long M = (long long)n * Ho * Wo;
    const long long blocks = (M + LP_WG_M - 1) / LP_WG_M;
    for (long long blk = 0; blk < blocks; ++blk)
        for (int wave = 0; wave < 4; ++wave) {
            const long long m0 = (blk * 4 + wave) * LP_TILE_M;
            if (m0 >= M) continue;
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, h = lane >> 5;
                for (int mt = 0; mt < 2; ++mt) {
                    int img, y, x;
                    lp_row_pixel(m0 + mt * 32 + r, M, Ho, Wo, &img, &y, &x);
                    CHECK(img >= 0 && img < n && y >= 0 && y < Ho && x >= 0 && x < Wo, "layer %d: row %lld decodes outside the map", l, m0 + mt * 32 + r);
                    if (m0 + mt * 32 + r >= M) CHECK(img == n - 1 && y == Ho - 1 && x == Wo - 1, "layer %d: a row past M is not the last pixel", l);
                    const size_t base = lp_field_base(img, y, x, stride, Hp, Wp, cin);
                    if (l == 0) {
                        for (int s = 0; s < kp / 16; ++s)
                            for (int j = 0; j < 8; ++j) {
                                const int k = 16 * s + 8 * h + j;
                                if (k >= K) continue;  // the kernel feeds 0 and the packed rows are 0
                                const Cell got = in[base + lp_gather_offset(k, ks, Wp, cin)];
                                ++g_reads;
                                const int tap = k / cin;
                                expect_tap(got, img, y * stride + tap / ks - pad, x * stride + tap % ks - pad, k % cin, Hi, Wi, l, k);
                            }
                    } else {
                        int s = 0;
                        for (int tap = 0; tap < ks * ks; ++tap)
                            for (int c0 = 0; c0 < cin; c0 += 16, ++s)
                                for (int j = 0; j < 8; ++j) {  // one 32-byte load of 8 floats
                                    const Cell got = in[base + lp_tap_offset(tap, ks, Wp, cin) + 8 * h + c0 + j];
                                    ++g_reads;
                                    const int k = 16 * s + 8 * h + j;
                                    CHECK(k == tap * cin + c0 + 8 * h + j, "layer %d: K order", l);
                                    expect_tap(got, img, y + tap / ks - pad, x + tap % ks - pad, c0 + 8 * h + j, Hi, Wi, l, k);
                                }
                        CHECK(s * 16 == kp, "layer %d: %d K steps, the pack has %d", l, s, kp / 16);
                    }
                }
                // epilogue: register i of lane (r, h) is row cf_acc_row(i, h)
                for (int mt = 0; mt < 2; ++mt)
                    for (int i = 0; i < 16; ++i) {
                        const long long m = m0 + mt * 32 + cf_acc_row(i, h);
                        if (m >= M) continue;
                        int img, y, x;
                        lp_row_pixel(m, M, Ho, Wo, &img, &y, &x);
                        const size_t o = lp_out_pixel(img, y, x, Ho, Wo, out_pad, cout);
                        for (int nt = 0; nt < cout / 32; ++nt) ++out[o + 32 * nt + r];
                    }
            }
        }
    // every interior element stored exactly once, the halo never
    const std::vector<Cell> lab = labelled(n, Ho, Wo, out_pad, cout);
    CHECK(lab.size() == out.size(), "layer %d: output size", l);
    for (size_t e = 0; e < out.size(); ++e) CHECK(out[e] == (lab[e].y >= 0 ? 1 : 0), "layer %d: element %zu stored %d times", l, e, out[e]);
}

// lpips_pack_kernel for layer l -- one thread per element e of the packed matrix -- and then every weight read of the MFMA step
// over the convolution's grid.y.  packed[e] stands for what the kernel stores at e: 1 + the index of W[n][ci][ky][kx], or 0 where
// it stores zero.  The decode must hit every (k, n) once and use every weight once; the reader must stay inside the matrix, take
// every element once, and find at the address of (K step s, tile, lane, j) the weight of the k its A operand holds there and of
// the column the epilogue stores that tile's lane to: zero for the rows k >= K, which conv1's gather feeds 0.
static void walk_pack(int l) {
    const int cin = lp_cin(l), cout = lp_cout(l), ks = lp_ksize(l), K = lp_k(l), kp = lp_kp(l), ntiles = cout / 32;
    CHECK(kp % 16 == 0 && cout % LP_TILE_N == 0 && kp >= K, "layer %d: pack divisibility", l);
    const size_t elems = (size_t)kp * cout, weights = (size_t)cout * K;
    std::vector<size_t> packed(elems, 0);
    std::vector<int> decoded(elems, 0), used(weights, 0), read(elems, 0);
    for (size_t e = 0; e < elems; ++e) {
        int k, n;
        cf_pack_decode(e, ntiles, &k, &n);
        CHECK(k >= 0 && k < kp && n >= 0 && n < cout, "layer %d: element %zu decodes to (%d, %d)", l, e, k, n);
        ++decoded[(size_t)k * cout + n];
        if (k < ks * ks * cin) {
            const int tap = k / cin, ci = k - tap * cin;
            const size_t w = ((size_t)n * cin + ci) * (ks * ks) + tap;
            CHECK(w < weights, "layer %d: element %zu reads weight %zu of %zu", l, e, w, weights);
            ++used[w];
            packed[e] = 1 + w;
        }
    }
    for (size_t i = 0; i < elems; ++i) CHECK(decoded[i] == 1, "layer %d: (k, n) = (%zu, %zu) packed %d times", l, i / cout, i % cout, decoded[i]);
    for (size_t w = 0; w < weights; ++w) CHECK(used[w] == 1, "layer %d: weight %zu packed %d times", l, w, used[w]);
    for (int by = 0; by < cout / LP_TILE_N; ++by)  // grid.y of the convolution; nt0 = 2 blockIdx.y
        for (int s = 0; s < kp / 16; ++s)
            for (int nt = 0; nt < 2; ++nt)
                for (int lane = 0; lane < 64; ++lane) {
                    CHECK(cf_frag_elem(s, ntiles, by * 2, nt, lane, 0) == 8 * cf_frag_group(s, ntiles, by * 2, nt, lane), "layer %d: group", l);
                    for (int j = 0; j < 8; ++j) {  // one 16-byte load of 8 bf16
                        const size_t e = cf_frag_elem(s, ntiles, by * 2, nt, lane, j);
                        CHECK(e < elems, "layer %d: the step reads element %zu of %zu", l, e, elems);
                        ++read[e];
                        const int k = 16 * s + 8 * (lane >> 5) + j;           // what the A operand holds in this position
                        const int n = (by * 2 + nt) * 32 + (lane & 31);       // the epilogue's co
                        int dk, dn;
                        cf_pack_decode(e, ntiles, &dk, &dn);
                        CHECK(dk == k && dn == n, "layer %d: the step reads (%d, %d) where the pack put (%d, %d)", l, k, n, dk, dn);
                        const size_t want = k < K ? 1 + ((size_t)n * cin + k % cin) * (ks * ks) + k / cin : 0;
                        CHECK(packed[e] == want, "layer %d: (k, n) = (%d, %d) holds %zu, expected %zu", l, k, n, packed[e], want);
                    }
                }
    for (size_t e = 0; e < elems; ++e) CHECK(read[e] == 1, "layer %d: element %zu read %d times", l, e, read[e]);
}

static void walk_pool(int n, int Hi, int Wi, int C, int Ho, int Wo, size_t in_elems, size_t out_elems, int pad) {
    CHECK(Ho == lp_pool_out(Hi) && Wo == lp_pool_out(Wi) && Ho >= 1 && Wo >= 1, "pool extent");
    const std::vector<Cell> in = labelled(n, Hi, Wi, 0, C);
    CHECK(in.size() == in_elems, "pool input size");
    const std::vector<Cell> out = labelled(n, Ho, Wo, pad, C);
    CHECK(out.size() == out_elems, "pool output size");
    const int C4 = C / 4, Hq = Ho + 2 * pad, Wq = Wo + 2 * pad;
    const size_t total = (size_t)n * Hq * Wq * C4;
    for (size_t e = 0; e < total; ++e) {  // the kernel's decode of its element index
        const int c4 = (int)(e % C4);
        size_t t = e / C4;
        const int xq = (int)(t % Wq);
        t /= Wq;
        const int yq = (int)(t % Hq), img = (int)(t / Hq);
        const bool inside = xq >= pad && xq < Wq - pad && yq >= pad && yq < Hq - pad;
        CHECK((out[e * 4].y >= 0) == inside && out[e * 4].c == 4 * c4 && out[e * 4 + 3].c == 4 * c4 + 3, "pool: output decode");
        if (!inside) continue;
        for (int d = 0; d < 9; ++d)
            for (int q = 0; q < 4; ++q) {
                const Cell got = in[lp_pool_src(img, yq - pad, xq - pad, d / 3, d % 3, Hi, Wi, C) + 4 * c4 + q];
                ++g_reads;
                CHECK(got.img == img && got.y == 2 * (yq - pad) + d / 3 && got.x == 2 * (xq - pad) + d % 3 && got.c == 4 * c4 + q, "pool: window");
            }
    }
}

// the halo kernel's cells on a [n, H + 2, W + 2, C] map: every border element zeroed exactly once, no interior element touched
static void walk_halo(int n, int H, int W, int C) {
    const std::vector<Cell> lab = labelled(n, H, W, 1, C);
    std::vector<int> hit(lab.size(), 0);
    const int cells = lp_halo_cells(H, W);
    const size_t total = (size_t)n * cells * C;
    for (size_t e = 0; e < total; ++e) {  // the kernel's decode of its element index
        const int c = (int)(e % C);
        const size_t t = e / C;
        const int cell = (int)(t % cells), img = (int)(t / cells);
        int y, x;
        lp_halo_cell(cell, H, W, &y, &x);
        ++hit[(((size_t)img * (H + 2) + y) * (W + 2) + x) * C + c];
        ++g_reads;
    }
    for (size_t e = 0; e < hit.size(); ++e) CHECK(hit[e] == (lab[e].y < 0 ? 1 : 0), "halo: element %zu zeroed %d times", e, hit[e]);
}

// the reference's reshape(-1, 3, h, w) of the HWC byte image, literally, against lp_reinterpret_src on the planar image
static void walk_reinterpret(int H, int W) {
    const size_t hw = (size_t)H * W;
    std::vector<int> planar(3 * hw), hwc(3 * hw);
    for (size_t i = 0; i < 3 * hw; ++i) planar[i] = (int)((i * 2654435761u) >> 7) & 0xffff;
    for (int c = 0; c < 3; ++c)
        for (size_t p = 0; p < hw; ++p) hwc[p * 3 + c] = planar[c * hw + p];  // the transpose the other metrics' uint8 image is made by
    for (int c = 0; c < 3; ++c)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const long long src = lp_reinterpret_src(c, y, x, H, W);
                CHECK(src >= 0, "reinterpretation: negative offset");
                ++g_reads;
                CHECK(planar[(size_t)src] == hwc[c * hw + (size_t)y * W + x], "reinterpretation at (%d,%d,%d)", c, y, x);
            }
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3) {
        fprintf(stderr, "usage: %s B H W [B H W ...]\n", argv[0]);
        return 1;
    }
    for (int l = 0; l < LP_LAYERS; ++l) walk_pack(l);
    for (int a = 1; a + 2 < argc; a += 3) {
        const int B = atoi(argv[a]), H = atoi(argv[a + 1]), W = atoi(argv[a + 2]);
        CHECK(B >= 1 && B <= LP_MAX_BATCH && H >= LP_MIN_HW && W >= LP_MIN_HW && H <= LP_MAX_HW && W <= LP_MAX_HW, "shape outside the limits");
        g_reads = 0;
        const int n = 2 * B;
        const LpMaps g = lp_maps(n, H, W);
        walk_reinterpret(H, W);
        for (int l = 0; l < LP_LAYERS; ++l) {
            CHECK(g.fh[l] >= 1 && g.fw[l] >= 1, "layer %d has no pixel", l);
            std::vector<int> out(g.relu[l], 0);
            if (l == 0) {
                walk_conv(0, n, H, W, labelled(n, H, W, 2, 3), g.in0, g.fh[0], g.fw[0], out);
            } else if (l <= 2) {  // a pool in front
                walk_pool(n, g.fh[l - 1], g.fw[l - 1], lp_cout(l - 1), g.fh[l], g.fw[l], g.relu[l - 1], g.pool[l - 1], lp_pad(l));
                walk_conv(l, n, g.fh[l], g.fw[l], labelled(n, g.fh[l], g.fw[l], lp_pad(l), lp_cin(l)), g.pool[l - 1], g.fh[l], g.fw[l], out);
            } else {  // relu3 / relu4 carry the halo themselves, zeroed by the halo kernel
                walk_halo(n, g.fh[l - 1], g.fw[l - 1], lp_cout(l - 1));
                CHECK(lp_feat_pad(l - 1) == lp_pad(l), "layer %d: the stored halo is not the convolution's", l);
                walk_conv(l, n, g.fh[l - 1], g.fw[l - 1], labelled(n, g.fh[l - 1], g.fw[l - 1], 1, lp_cin(l)), g.relu[l - 1], g.fh[l], g.fw[l], out);
            }
        }
        printf("%d %d %d", B, H, W);
        for (int l = 0; l < LP_LAYERS; ++l) printf(" %d %d", g.fh[l], g.fw[l]);
        printf(" %lld\n", g_reads);
    }
    return 0;
}
