// The index arithmetic of n3dt_fan (csrc/fan_core.h, csrc/conv_frag.h) walked on the CPU over the kernels' grids: a stand-alone
// program with its own main, built by tests/test_fan_cpu.py with the host compiler under -fsanitize=address,undefined.
//
//   fan_core_host forward M N n      the whole forward's plan
//   fan_core_host block b M N n H W  one block alone
//
// The loop nest of fan_conv_kernel (csrc/fan.hip) is re-typed here -- block / wave / lane for the A fetch, accumulator register /
// half for the epilogue -- over a workspace of one int per float that holds the step that last wrote it:
//   * every A fetch (row, tap) lies inside the map the step was handed, on floats an EARLIER step of this plan wrote (the image
//     and a block's inputs count as written by step -1), and the skip likewise;
//   * every store lies inside the slice the step was given, and after the step every element of that slice -- and of the raw map --
//     has been stored exactly once;
//   * the pack's decode covers every element of the packed matrix once and reads inside the weight tensor;
//   * the decode's index rules stay inside the 4096 cells for every argmax below 4095 under all four flag settings.
// Prints one line per step: op conv H W Ho Wo stores.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/conv_frag.h"
#include "../nerf-3dtalker-code_amd/csrc/fan_core.h"

static int fails = 0;
#define CHECK(c, ...)                      \
    do {                                   \
        if (!(c)) {                        \
            if (fails++ < 20) {            \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");     \
            }                              \
        }                                  \
    } while (0)

struct Walk {
    std::vector<int> writer;      // per float of the workspace: the step that last wrote it, -2 never
    std::vector<unsigned char> n; // stores of the current step
    int images;
    size_t at(size_t off) const { return off * (size_t)images; }
};

static void mark_input(Walk& w, size_t off, size_t elems) {
    for (size_t i = 0; i < elems; ++i) w.writer[w.at(off) + i] = -1;
}

static void read_range(const Walk& w, int step, size_t first, size_t count, size_t lo, size_t hi, const char* what) {
    CHECK(first >= lo && first + count <= hi, "step %d: %s read [%zu, %zu) outside its map [%zu, %zu)", step, what, first, first + count, lo, hi);
    if (first < lo || first + count > hi) return;
    for (size_t i = 0; i < count; ++i) {
        const int by = w.writer[first + i];
        CHECK(by >= -1 && by < step, "step %d: %s reads float %zu written by step %d", step, what, first + i, by);
    }
}

static size_t store(Walk& w, int step, size_t addr, size_t lo, size_t hi) {
    CHECK(addr >= lo && addr < hi, "step %d: store at %zu outside its map [%zu, %zu)", step, addr, lo, hi);
    if (addr < lo || addr >= hi) return 0;
    CHECK(w.n[addr] == 0, "step %d: float %zu stored twice", step, addr);
    w.n[addr]++;
    w.writer[addr] = step;
    return 1;
}

// after a step: the slice [c0, c0 + cw) of every cell of a map cs wide was stored exactly once; the counters are cleared
static void settle(Walk& w, int step, size_t base, size_t cells, int cs, int c0, int cw) {
    for (size_t m = 0; m < cells; ++m)
        for (int c = 0; c < cw; ++c) {
            const size_t a = base + m * cs + c0 + c;
            CHECK(w.n[a] == 1, "step %d: cell %zu channel %d stored %d times", step, m, c0 + c, (int)w.n[a]);
            w.n[a] = 0;
        }
}

static size_t walk_conv(Walk& w, int s, const FanStep& t, int N, int* Ho_, int* Wo_) {
    const FanConv c = fan_conv(t.conv, N);
    const int n = w.images, pad = c.k / 2, Hi = t.H, Wi = t.W;
    const int Ho = cn_conv_out(Hi, c.k, c.stride, pad), Wo = cn_conv_out(Wi, c.k, c.stride, pad);
    *Ho_ = Ho; *Wo_ = Wo;
    const int cin = fan_cinp(&c), np = fan_np(&c), cstore = c.kind == FAN_L ? cn_round16(c.cout) : c.cout;
    const long long M = (long long)n * Ho * Wo;
    const int NT = cn_wave_ntiles(M, np), ntn = np / (32 * NT);
    CHECK((NT == 1 || NT == 2) && np % (32 * NT) == 0, "step %d: %d tiles a wave do not divide the %d columns", s, NT, np);
    CHECK(np % (32 * NT) == 0 && cin % (c.kind == FAN_STEM ? 1 : 16) == 0, "step %d: tile widths", s);
    const size_t in_lo = w.at(t.in), in_hi = in_lo + (size_t)n * Hi * Wi * t.in_cs;
    const size_t out_lo = w.at(t.out), out_hi = out_lo + (size_t)M * t.out_cs;
    CHECK(t.in_c0 + (c.kind == FAN_STEM ? 3 : cin) <= t.in_cs && t.out_c0 + cstore <= t.out_cs, "step %d: slices wider than their maps", s);
    const long long tiles = (M + CN_TILE_M - 1) / CN_TILE_M * ntn;
    const long long grid = (tiles + 3) / 4;
    size_t stores = 0;
    for (long long block = 0; block < grid; ++block)
        for (int wave = 0; wave < 4; ++wave) {
            const long long tile = block * 4 + wave, m0 = tile / ntn * CN_TILE_M;
            if (m0 >= M) continue;
            const int nt0 = (int)(tile % ntn) * NT;
            if (nt0 == 0)  // the A fetch does not depend on the column tile: walk it once per row tile
                for (int mt = 0; mt < 2; ++mt)
                    for (int r = 0; r < 32; ++r) {
                        int img, y, x;
                        cn_row_cell(m0 + mt * 32 + r, M, Ho, Wo, &img, &y, &x);
                        const size_t base = in_lo + (size_t)img * Hi * Wi * t.in_cs + t.in_c0;
                        if (c.kind == FAN_STEM) {
                            for (int k = 0; k < CN_STEM_K; ++k) {
                                int ky, kx, ch;
                                cn_stem_tap(k, &ky, &kx, &ch);
                                const int iy = fan_tap_pixel(y, ky, 2, 3), ix = fan_tap_pixel(x, kx, 2, 3);
                                if (fan_inside(iy, ix, Hi, Wi)) read_range(w, s, base + ((size_t)iy * Wi + ix) * 3 + ch, 1, in_lo, in_hi, "stem");
                            }
                        } else {
                            for (int tap = 0; tap < c.k * c.k; ++tap) {
                                const int ky = tap / c.k, kx = tap - ky * c.k;
                                const int iy = fan_tap_pixel(y, ky, c.stride, pad), ix = fan_tap_pixel(x, kx, c.stride, pad);
                                if (!fan_inside(iy, ix, Hi, Wi)) continue;
                                for (int h = 0; h < 2; ++h)
                                    for (int c0 = 0; c0 < cin; c0 += 16)
                                        read_range(w, s, base + ((size_t)iy * Wi + ix) * t.in_cs + 8 * h + c0, 8, in_lo, in_hi, "A");
                            }
                        }
                    }
            for (int mt = 0; mt < 2; ++mt)
                for (int i = 0; i < 16; ++i)
                    for (int h = 0; h < 2; ++h) {
                        const long long m = m0 + mt * 32 + cf_acc_row(i, h);
                        if (m >= M) continue;
                        for (int nt = 0; nt < NT; ++nt)
                            for (int r = 0; r < 32; ++r) {
                                const int co = (nt0 + nt) * 32 + r;
                                if (co >= cstore) continue;
                                if (t.raw != FAN_NONE) stores += store(w, s, w.at(t.raw) + (size_t)m * t.raw_cs + co, w.at(t.raw), w.at(t.raw) + (size_t)M * t.raw_cs);
                                if (t.skip != FAN_NONE)
                                    read_range(w, s, w.at(t.skip) + (size_t)m * t.skip_cs + t.skip_c0 + co, 1, w.at(t.skip), w.at(t.skip) + (size_t)M * t.skip_cs, "skip");
                                stores += store(w, s, out_lo + (size_t)m * t.out_cs + t.out_c0 + co, out_lo, out_hi);
                            }
                    }
        }
    settle(w, s, out_lo, (size_t)M, t.out_cs, t.out_c0, cstore);
    if (t.raw != FAN_NONE) settle(w, s, w.at(t.raw), (size_t)M, t.raw_cs, 0, c.cout);
    return stores;
}

static size_t walk_small(Walk& w, int s, const FanStep& t, int* Ho_, int* Wo_) {
    const int n = w.images, C = t.C;
    size_t stores = 0;
    if (t.op == FAN_OP_POOL) {
        const int Ho = t.H / 2, Wo = t.W / 2;
        *Ho_ = Ho; *Wo_ = Wo;
        const size_t in_lo = w.at(t.in), in_hi = in_lo + (size_t)n * t.H * t.W * C, out_lo = w.at(t.out), out_hi = out_lo + (size_t)n * Ho * Wo * C;
        for (size_t e = 0; e < (size_t)n * Ho * Wo * (C / 4); ++e) {
            const int c = (int)(e % (C / 4)) * 4;
            size_t q = e / (C / 4);
            const int xo = (int)(q % Wo);
            q /= Wo;
            const int yo = (int)(q % Ho);
            const size_t img = q / Ho, p = in_lo + ((img * t.H + 2 * yo) * t.W + 2 * xo) * C + c;
            read_range(w, s, p, 4, in_lo, in_hi, "pool");
            read_range(w, s, p + C, 4, in_lo, in_hi, "pool");
            read_range(w, s, p + (size_t)t.W * C, 4, in_lo, in_hi, "pool");
            read_range(w, s, p + (size_t)t.W * C + C, 4, in_lo, in_hi, "pool");
            for (int j = 0; j < 4; ++j) stores += store(w, s, out_lo + e * 4 + j, out_lo, out_hi);
        }
        settle(w, s, out_lo, (size_t)n * Ho * Wo, C, 0, C);
    } else {
        const int H = t.H, W = t.W;
        *Ho_ = H; *Wo_ = W;
        const size_t lo_lo = w.at(t.in), lo_hi = lo_lo + (size_t)n * (H / 2) * (W / 2) * C, up_lo = w.at(t.skip), up_hi = up_lo + (size_t)n * H * W * C;
        const size_t out_lo = w.at(t.out), out_hi = out_lo + (size_t)n * H * W * C;
        for (size_t e = 0; e < (size_t)n * H * W * (C / 4); ++e) {
            const int c = (int)(e % (C / 4)) * 4;
            size_t q = e / (C / 4);
            const int x = (int)(q % W);
            q /= W;
            const int y = (int)(q % H);
            const size_t img = q / H;
            read_range(w, s, up_lo + e * 4, 4, up_lo, up_hi, "upper");
            read_range(w, s, lo_lo + ((img * (H / 2) + y / 2) * (W / 2) + x / 2) * C + c, 4, lo_lo, lo_hi, "lower");
            for (int j = 0; j < 4; ++j) stores += store(w, s, out_lo + e * 4 + j, out_lo, out_hi);
        }
        settle(w, s, out_lo, (size_t)n * H * W, C, 0, C);
    }
    return stores;
}

static void walk_plan(FanPlan* p, Walk& w, int N) {
    for (int s = 0; s < p->steps; ++s) {
        const FanStep& t = p->step[s];
        int Ho = 0, Wo = 0;
        const size_t stores = t.op == FAN_OP_CONV ? walk_conv(w, s, t, N, &Ho, &Wo) : walk_small(w, s, t, &Ho, &Wo);
        printf("%d %d %d %d %d %d %zu\n", t.op, t.conv, t.H, t.W, Ho, Wo, stores);
    }
}

static void walk_pack(int modules, int N) {
    for (int j = 0; j < fan_convs(modules); ++j) {
        if (!fan_conv_exists(j, modules)) continue;
        const FanConv c = fan_conv(j, N);
        const int K = fan_K(&c), np = fan_np(&c), cinp = fan_cinp(&c), taps = c.k * c.k;
        const int wc = c.kind == FAN_STEM ? 6 : c.kind == FAN_COORD ? (j < FAN_FRONT_CONVS + FAN_STACK_CONVS ? 259 : 261) : c.cin;
        const size_t wsize = (size_t)c.cout * wc * taps;
        std::vector<unsigned char> seen((size_t)K * np, 0);
        for (size_t e = 0; e < (size_t)K * np; ++e) {
            int k, n;
            cf_pack_decode(e, np / 32, &k, &n);
            CHECK(k >= 0 && k < K && n >= 0 && n < np, "conv %d: pack element %zu decodes to (%d, %d)", j, e, k, n);
            if (k < 0 || k >= K || n < 0 || n >= np) continue;
            CHECK(!seen[(size_t)k * np + n], "conv %d: (%d, %d) packed twice", j, k, n);
            seen[(size_t)k * np + n] = 1;
            if (n >= c.cout) continue;
            size_t src;
            if (c.kind == FAN_STEM) {
                if (k >= CN_STEM_K) continue;
                int ky, kx, ch;
                cn_stem_tap(k, &ky, &kx, &ch);
                src = ((size_t)n * wc + ch) * 49 + ky * 7 + kx;
            } else {
                const int tap = k / cinp, ci = k - tap * cinp;
                if (ci >= c.cin) continue;
                src = ((size_t)n * wc + ci) * taps + tap;
            }
            CHECK(src < wsize, "conv %d: pack reads weight %zu of %zu", j, src, wsize);
        }
    }
}

static void walk_decode() {
    for (int i = 0; i < FAN_CELLS - 1; ++i)
        for (int up = fan_flag_up(i); up < 2; ++up)        // a frame-wide flag is set at least where this landmark sets it
            for (int down = fan_flag_down(i); down < 2; ++down) {
                const int idx[4] = {fan_x_up(i), fan_x_down(i), fan_y_up(i, up), fan_y_down(i, down)};
                for (int q = 0; q < 4; ++q) CHECK(idx[q] >= 0 && idx[q] < FAN_CELLS, "decode: argmax %d (up %d, down %d) reads cell %d", i, up, down, idx[q]);
            }
    CHECK(fan_x_down(0) == FAN_CELLS - 1 && fan_flag_down(64) && !fan_flag_down(65) && fan_flag_up(4032) && !fan_flag_up(4031), "decode: the flag thresholds");
    CHECK(fan_better(1.0f, 5, 1.0f, 9) && !fan_better(1.0f, 9, 1.0f, 5) && fan_better(2.0f, 9, 1.0f, 5), "decode: the first index wins ties");
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    static FanPlan plan;
    Walk w;
    if (!strcmp(argv[1], "forward")) {
        const int M = atoi(argv[2]), N = atoi(argv[3]);
        w.images = atoi(argv[4]);
        fan_plan_forward(&plan, M, N);
        w.writer.assign(plan.peak * (size_t)w.images, -2);
        w.n.assign(plan.peak * (size_t)w.images, 0);
        mark_input(w, plan.image, (size_t)w.images * FAN_IMG * FAN_IMG * 3);
        walk_plan(&plan, w, N);
        // every stack's heat map is still the one its l wrote when the forward ends
        for (int s = 0; s < M; ++s) {
            const int by = w.writer[w.at(plan.heat[s])];
            CHECK(by >= 0 && plan.step[by].conv == fan_stack_conv(s, 44), "heat map %d was last written by step %d", s, by);
        }
        walk_pack(M, N);
        walk_decode();
    } else {
        if (argc < 8) return 2;
        const int b = atoi(argv[2]), M = atoi(argv[3]), N = atoi(argv[4]), H = atoi(argv[6]), W = atoi(argv[7]);
        w.images = atoi(argv[5]);
        CHECK(fan_block_exists(b, M), "no block %d", b);
        const FanBlockMaps m = fan_plan_block(&plan, b, N, H, W);
        w.writer.assign(plan.peak * (size_t)w.images, -2);
        w.n.assign(plan.peak * (size_t)w.images, 0);
        mark_input(w, m.in, (size_t)w.images * H * W * m.in_cs);
        if (m.skip != FAN_NONE) mark_input(w, m.skip, (size_t)w.images * m.Ho * m.Wo * m.out_cs);
        walk_plan(&plan, w, N);
    }
    if (fails) fprintf(stderr, "%d checks failed\n", fails);
    return fails ? 1 : 0;
}
