/*
 * n3dt_oracle.c -- CPU restatement of NeRF-3DTalker's per-frame volumetric head render.
 *
 * TEST INFRASTRUCTURE ONLY.  This file is the parity oracle and the timed CPU baseline
 * ("port") for the HIP path.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load it; the product path (nerf-3dtalker-code_amd/) never does.
 *
 * Parity pin: checked against golden vectors emitted by the reference itself
 * (tools/gen_golden.py imports /root/reference/NetWorks in the build container;
 * tests/test_oracle_golden.py compares every seam).  The only arithmetic not in the
 * reference tree is kornia.filters.filter2d (kornia==0.6.12, un-vendored): restated from
 * its documented semantics, "parity unpinned" for that one call.
 *
 * Plain C99, fp32 everywhere the reference is fp32, compiled with -ffp-contract=off so the
 * geometry keeps the reference's operation order (the positional encoding multiplies point
 * coordinates by up to 512, so one ulp there is visible).  The MLP contraction uses explicit
 * fmaf and is laid out [channel][sample] so the inner loop vectorises without reassociation.
 *
 * Each function cites the reference lines it follows (paths relative to /root/reference).
 * Layouts are the reference's: NCHW-like [B, C, N_r, N_s], weights [out][in].
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define PE_FREQS 10
#define PE_DIM 63

int orc_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

void orc_set_num_threads(int n) {
#ifdef _OPENMP
    omp_set_num_threads(n);
#else
    (void)n;
#endif
}

/* torch.linspace(0,1,steps) on CPU: step=(end-start)/(steps-1); first half start+i*step,
 * second half end-(steps-1-i)*step.  Used at NetWorks/utils.py:140. */
static inline float linspace01(int i, int steps) {
    float step = 1.0f / (float)(steps - 1);
    int half = steps / 2;
    if (i < half) return 0.0f + step * (float)i;
    return 1.0f - step * (float)(steps - 1 - i);
}

/* ---------------------------------------------------------------------------------------
 * a1: GenSamplePoints.forward            NetWorks/utils.py:147-161
 * a2: _calc_sample_points                NetWorks/utils.py:118-145
 *     _calc_sample_points_by_zvals       NetWorks/utils.py:65-116
 * xy [B,2,Nr]; R [B,3,3]; T [B,3]; Kinv [B,3,3]; t_rand nullable [B,Nr,Ns+1]
 * ray_d [B,3,Nr]; ray_l [B,Nr]; pts [B,3,Nr,Ns]; zvals,z_dists [B,Nr,Ns]
 * ------------------------------------------------------------------------------------- */
static void ray_setup(const float* R, const float* T, const float* K, float x, float y, float* d, float* l_out) {
    /* temp_xyz = [x, y, 1]; cam = Kinv @ xyz; d = R @ cam   (utils.py:149-151) */
    float c[3], w[3];
    for (int i = 0; i < 3; ++i) c[i] = K[i * 3 + 0] * x + K[i * 3 + 1] * y + K[i * 3 + 2] * 1.0f;
    for (int i = 0; i < 3; ++i) w[i] = R[i * 3 + 0] * c[0] + R[i * 3 + 1] * c[1] + R[i * 3 + 2] * c[2];
    float n = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]); /* torch.norm dim=1   (utils.py:153) */
    d[0] = w[0] / n; d[1] = w[1] / n; d[2] = w[2] / n;         /* utils.py:154 */
    *l_out = -1.0f / d[2];                                     /* utils.py:155 */
    (void)T;
}

/* edge value j (0..Ns) of the sample planes, jittered when t_rand is given */
static inline float edge_z(float rz1, float rz2, int j, int Ns, const float* tr) {
    float t = linspace01(j, Ns + 1);
    float zv = rz1 * (1.0f - t) + rz2 * t;                      /* utils.py:142 */
    if (!tr) return zv;
    /* utils.py:73-78: mids, upper, lower, lower + (upper-lower)*t_rand */
    float lower, upper;
    if (j == 0) lower = zv;
    else { float tp = linspace01(j - 1, Ns + 1); float zp = rz1 * (1.0f - tp) + rz2 * tp; lower = 0.5f * (zv + zp); }
    if (j == Ns) upper = zv;
    else { float tn = linspace01(j + 1, Ns + 1); float zn = rz1 * (1.0f - tn) + rz2 * tn; upper = 0.5f * (zn + zv); }
    return lower + (upper - lower) * tr[j];
}

void orc_sample(int B, int Nr, int Ns, const float* xy, const float* R, const float* T, const float* Kinv,
                float world_z1, float world_z2, const float* t_rand,
                float* ray_d, float* ray_l, float* pts, float* zvals, float* z_dists) {
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < Nr; ++r) {
            float d[3], l;
            const float* Tb = T + b * 3;
            ray_setup(R + b * 9, Tb, Kinv + b * 9, xy[(b * 2 + 0) * Nr + r], xy[(b * 2 + 1) * Nr + r], d, &l);
            if (ray_d) for (int i = 0; i < 3; ++i) ray_d[(b * 3 + i) * Nr + r] = d[i];
            if (ray_l) ray_l[b * Nr + r] = l;
            float rz1 = Tb[2] - world_z1, rz2 = Tb[2] - world_z2; /* utils.py:125-126 */
            const float* tr = t_rand ? t_rand + ((size_t)b * Nr + r) * (Ns + 1) : NULL;
            float z_lo = edge_z(rz1, rz2, 0, Ns, tr);
            for (int s = 0; s < Ns; ++s) {
                float z_hi = edge_z(rz1, rz2, s + 1, Ns, tr);
                size_t o = ((size_t)b * Nr + r) * Ns + s;
                if (z_dists) z_dists[o] = (z_hi - z_lo) * l;      /* utils.py:80-81 */
                if (zvals) zvals[o] = z_lo;                       /* utils.py:83 */
                if (pts)
                    for (int i = 0; i < 3; ++i)                   /* o + d*l*z   (utils.py:86) */
                        pts[(((size_t)b * 3 + i) * Nr + r) * Ns + s] = Tb[i] + (d[i] * l) * z_lo;
                z_lo = z_hi;
            }
        }
}

/* ---------------------------------------------------------------------------------------
 * f4: FineSample.forward                  NetWorks/utils.py:211-263 (hierarchical sample planes)
 * weight [R][Nc] (coarse compositing weights), zc [R][Nc] (coarse zvals), u [R][Nf+1] or NULL (linspace),
 * out [R][Nc+Nf+1] ascending.
 * ------------------------------------------------------------------------------------- */
static int cmp_float(const void* a, const void* b) {
    float x = *(const float*)a, y = *(const float*)b;
    return (x > y) - (x < y);
}
void orc_fine_sample(long R, int Nc, int Nf, const float* weight, const float* zc, const float* u_in, float* out) {
    const int Nu = Nf + 1, Nt = Nc - 2, Nall = Nc + Nu;     /* utils.py:214,220 */
#pragma omp parallel for schedule(static)
    for (long r = 0; r < R; ++r) {
        const float* w = weight + r * Nc + 1;               /* batch_weight[..., 1:-1]  (:219) */
        const float* z = zc + r * Nc;
        float* cdf = (float*)malloc(sizeof(float) * (Nt + 1));
        float* o = out + r * Nall;
        float total = 0.0f;
        for (int j = 0; j < Nt; ++j) total += w[j] + 1e-5f;  /* x = w + 1e-5; sum(x)      (:223-224) */
        cdf[0] = 0.0f;                                       /* F.pad(cdf, [1,0])         (:226) */
        float run = 0.0f;
        for (int j = 0; j < Nt; ++j) { run += w[j] / total; cdf[j + 1] = run; }   /* pdf, cumsum (:224-225) */
        for (int j = 0; j < Nc; ++j) o[j] = z[j];
        for (int i = 0; i < Nu; ++i) {
            float u = u_in ? u_in[r * Nu + i] : (Nu > 1 ? linspace01(i, Nu) : 0.0f); /* :229-232; linspace(0, 1, 1) = [0] */
            int inds = 0;                                                          /* searchsorted(right=True) (:235) */
            while (inds < Nt + 1 && cdf[inds] <= u) ++inds;
            int below = inds - 1 > 0 ? inds - 1 : 0;                               /* :236 */
            int above = inds < Nt ? inds : Nt;                                     /* :237 */
            float b0 = 0.5f * (z[below + 1] + z[below]), b1 = 0.5f * (z[above + 1] + z[above]);  /* bins (:241) */
            float denom = cdf[above] - cdf[below];                                 /* :246 */
            if (denom < 1e-5f) denom = 1.0f;                                       /* :247 */
            float t = (u - cdf[below]) / denom;                                    /* :248 */
            o[Nc + i] = b0 + t * (b1 - b0);                                        /* :249 */
        }
        qsort(o, (size_t)Nall, sizeof(float), cmp_float);                          /* torch.sort (:251) */
        free(cdf);
    }
}

/* FineSample._calc_sample_points_by_zvals  utils.py:173-208: planes [B][Nr][N+1] -> pts, zvals, z_dists over N samples */
void orc_sample_planes(int B, int Nr, int N, const float* xy, const float* R, const float* T, const float* Kinv,
                       const float* planes, float* pts, float* zvals, float* z_dists) {
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < Nr; ++r) {
            float d[3], l;
            const float* Tb = T + b * 3;
            ray_setup(R + b * 9, Tb, Kinv + b * 9, xy[(b * 2 + 0) * Nr + r], xy[(b * 2 + 1) * Nr + r], d, &l);
            const float* z = planes + ((size_t)b * Nr + r) * (N + 1);
            for (int s = 0; s < N; ++s) {
                size_t o = ((size_t)b * Nr + r) * N + s;
                if (z_dists) z_dists[o] = (z[s + 1] - z[s]) * l;   /* :182-183 */
                if (zvals) zvals[o] = z[s];                        /* :185 */
                if (pts)
                    for (int i = 0; i < 3; ++i) pts[(((size_t)b * 3 + i) * Nr + r) * N + s] = Tb[i] + (d[i] * l) * z[s];  /* :188 */
            }
        }
}

/* ---------------------------------------------------------------------------------------
 * a3: Embedder.forward                    NetWorks/utils.py:20-51  (freqs 2^k, no pi)
 * pts [B,3,M] -> pe [B,63,M]: [p, sin(2^0 p), cos(2^0 p), ..., sin(2^9 p), cos(2^9 p)]
 * ------------------------------------------------------------------------------------- */
static inline void embed_point(const float p[3], float* out, size_t stride) {
    for (int i = 0; i < 3; ++i) out[(size_t)i * stride] = p[i];
    float f = 1.0f;
    for (int k = 0; k < PE_FREQS; ++k) {
        for (int i = 0; i < 3; ++i) {
            float a = p[i] * f;
            out[(size_t)(3 + 6 * k + i) * stride] = sinf(a);
            out[(size_t)(3 + 6 * k + 3 + i) * stride] = cosf(a);
        }
        f *= 2.0f;
    }
}

void orc_embed(int B, long M, const float* pts, float* pe) {
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (long m = 0; m < M; ++m) {
            float p[3] = {pts[((size_t)b * 3 + 0) * M + m], pts[((size_t)b * 3 + 1) * M + m], pts[((size_t)b * 3 + 2) * M + m]};
            embed_point(p, pe + (size_t)b * PE_DIM * M + m, (size_t)M);
        }
}

/* ---------------------------------------------------------------------------------------
 * a4+a5: latent concat + MLPforNeRF.forward   NetWorks/HeadNeRFNet.py:84,89,149-152
 *                                             NetWorks/models.py:62-87
 * One block = up to NB samples laid out [channel][NB]; dense contraction exactly as the
 * reference executes it (306 / 626 / 511-wide inputs, no latent folding).
 * mlp_w: pointers in order W0,b0,...,W7,b7, Wd,bd, Wr0,br0, Wr1,br1, Wr2,br2.
 * ------------------------------------------------------------------------------------- */
#define NB 64

typedef struct {
    int H, C, shape_dim, appea_dim, audio_dim;
    int vd_dim; /* include_vd: 27 view-direction channels between RGB_layer_0's output and the appearance code, else 0
                   (NetWorks/HeadNeRFNet.py:56-63,86; models.py:80) */
} orc_dims;

/* vd_encoder: Embedder(N_freqs=4, include_input=True) of a ray direction (HeadNeRFNet.py:30-31,61,141-142; utils.py:20-51) */
#define VD_FREQS 4
#define VD_DIM (3 + 6 * VD_FREQS)
static inline void embed_dir(const float d[3], float* out, size_t stride) {
    for (int i = 0; i < 3; ++i) out[(size_t)i * stride] = d[i];
    float f = 1.0f;
    for (int k = 0; k < VD_FREQS; ++k) {
        for (int i = 0; i < 3; ++i) {
            float a = d[i] * f;
            out[(size_t)(3 + 6 * k + i) * stride] = sinf(a);
            out[(size_t)(3 + 6 * k + 3 + i) * stride] = cosf(a);
        }
        f *= 2.0f;
    }
}

static void dense(const float* W, const float* bias, int cin, int cout, const float* x, float* y, int relu) {
    for (int o = 0; o < cout; ++o) {
        float acc[NB];
        float b0 = bias[o];
        for (int p = 0; p < NB; ++p) acc[p] = b0;
        const float* w = W + (size_t)o * cin;
        for (int i = 0; i < cin; ++i) {
            float wi = w[i];
            const float* xi = x + (size_t)i * NB;
            for (int p = 0; p < NB; ++p) acc[p] = fmaf(wi, xi[p], acc[p]);
        }
        float* yo = y + (size_t)o * NB;
        if (relu) for (int p = 0; p < NB; ++p) yo[p] = acc[p] > 0.0f ? acc[p] : 0.0f;
        else      for (int p = 0; p < NB; ++p) yo[p] = acc[p];
    }
}

/* pe_blk: [63][NB]; outputs rgb_blk [C][NB], dens_blk [NB].  scratch >= (in5 + 2H + in_rgb1) * NB floats. */
static void mlp_block(const orc_dims* dm, const float* const* w, const float* pe_blk, const float* shape,
                      const float* appea, const float* audio, const float* vd_blk /* [vd_dim][NB] or NULL */, float* rgb_blk,
                      float* dens_blk, float* scratch) {
    int H = dm->H, vp = PE_DIM + dm->shape_dim, in0 = vp + dm->audio_dim, in5 = vp + H, inr = H + dm->vd_dim + dm->appea_dim;
    float* x0 = scratch;                        /* [max(in0,in5)][NB], rows 0..vp-1 = [PE | shape] */
    int xrows = in0 > in5 ? in0 : in5;
    float* ha = x0 + (size_t)xrows * NB;        /* [H][NB] */
    float* hb = ha + (size_t)H * NB;            /* [H][NB] */
    float* xr = hb + (size_t)H * NB;            /* [inr][NB] */
    memcpy(x0, pe_blk, sizeof(float) * PE_DIM * NB);
    for (int i = 0; i < dm->shape_dim; ++i) for (int p = 0; p < NB; ++p) x0[(size_t)(PE_DIM + i) * NB + p] = shape[i];
    for (int i = 0; i < dm->audio_dim; ++i) for (int p = 0; p < NB; ++p) x0[(size_t)(vp + i) * NB + p] = audio[i];
    /* models.py:69-76 */
    dense(w[0], w[1], in0, H, x0, ha, 1);
    float* cur = ha; float* nxt = hb;
    for (int l = 1; l < 8; ++l) {
        if (l == 5) { /* skip: cat([vp, x])  (models.py:75-76) */
            memcpy(x0 + (size_t)vp * NB, cur, sizeof(float) * H * NB);
            dense(w[2 * l], w[2 * l + 1], in5, H, x0, nxt, 1);
        } else {
            dense(w[2 * l], w[2 * l + 1], H, H, cur, nxt, 1);
        }
        float* t = cur; cur = nxt; nxt = t;
    }
    /* density head (models.py:78,84) */
    {
        float tmp[NB];
        dense(w[16], w[17], H, 1, cur, tmp, 1);
        memcpy(dens_blk, tmp, sizeof(tmp));
    }
    /* feature head (models.py:79-82): RGB_layer_0 has no activation; cat appea; relu after RGB_layer_1 */
    dense(w[18], w[19], H, H, cur, xr, 0);
    /* include_vd: cat([x, embed_vds]) with embed_vds = cat([vd_embed, appea]) (HeadNeRFNet.py:86, models.py:80) */
    if (dm->vd_dim) memcpy(xr + (size_t)H * NB, vd_blk, sizeof(float) * (size_t)dm->vd_dim * NB);
    for (int i = 0; i < dm->appea_dim; ++i) for (int p = 0; p < NB; ++p) xr[(size_t)(H + dm->vd_dim + i) * NB + p] = appea[i];
    dense(w[20], w[21], inr, H / 2, xr, nxt, 1);
    dense(w[22], w[23], H / 2, dm->C, nxt, rgb_blk, 0); /* C != 3: no sigmoid (models.py:85-86) */
}

static size_t mlp_scratch_floats(const orc_dims* dm) {
    int H = dm->H, vp = PE_DIM + dm->shape_dim, in0 = vp + dm->audio_dim, in5 = vp + H, inr = H + dm->vd_dim + dm->appea_dim;
    int xrows = in0 > in5 ? in0 : in5;
    return (size_t)(xrows + 2 * H + inr) * NB;
}

/* pe [B,63,M] -> rgb [B,C,M], density [B,M] */
void orc_mlp_vd(int B, long M, int H, int C, int shape_dim, int appea_dim, int audio_dim, int vd_dim, const float* const* w,
                const float* pe, const float* shape, const float* appea, const float* audio, const float* vd /* [B,vd_dim,M] */,
                float* rgb, float* density);
void orc_mlp(int B, long M, int H, int C, int shape_dim, int appea_dim, int audio_dim, const float* const* w,
             const float* pe, const float* shape, const float* appea, const float* audio, float* rgb, float* density) {
    orc_mlp_vd(B, M, H, C, shape_dim, appea_dim, audio_dim, 0, w, pe, shape, appea, audio, NULL, rgb, density);
}
void orc_mlp_vd(int B, long M, int H, int C, int shape_dim, int appea_dim, int audio_dim, int vd_dim, const float* const* w,
                const float* pe, const float* shape, const float* appea, const float* audio, const float* vd, float* rgb,
                float* density) {
    orc_dims dm = {H, C, shape_dim, appea_dim, audio_dim, vd_dim};
    long nblk = (M + NB - 1) / NB;
#pragma omp parallel
    {
        float* scratch = (float*)malloc(sizeof(float) * (mlp_scratch_floats(&dm) + (size_t)(PE_DIM + C + 1 + VD_DIM) * NB));
        float* pe_blk = scratch + mlp_scratch_floats(&dm);
        float* rgb_blk = pe_blk + (size_t)PE_DIM * NB;
        float* dens_blk = rgb_blk + (size_t)C * NB;
        float* vd_blk = dens_blk + NB;
#pragma omp for collapse(2) schedule(dynamic, 4)
        for (int b = 0; b < B; ++b)
            for (long k = 0; k < nblk; ++k) {
                long m0 = k * NB;
                int n = (int)((M - m0) < NB ? (M - m0) : NB);
                for (int c = 0; c < PE_DIM; ++c)
                    for (int p = 0; p < NB; ++p)
                        pe_blk[(size_t)c * NB + p] = p < n ? pe[((size_t)b * PE_DIM + c) * M + m0 + p] : 0.0f;
                for (int c = 0; c < vd_dim; ++c)
                    for (int p = 0; p < NB; ++p)
                        vd_blk[(size_t)c * NB + p] = p < n ? vd[((size_t)b * vd_dim + c) * M + m0 + p] : 0.0f;
                mlp_block(&dm, w, pe_blk, shape + (size_t)b * shape_dim, appea + (size_t)b * appea_dim,
                          audio_dim ? audio + (size_t)b * audio_dim : NULL, vd_dim ? vd_blk : NULL, rgb_blk, dens_blk, scratch);
                for (int c = 0; c < C; ++c)
                    for (int p = 0; p < n; ++p) rgb[((size_t)b * C + c) * M + m0 + p] = rgb_blk[(size_t)c * NB + p];
                for (int p = 0; p < n; ++p) density[(size_t)b * M + m0 + p] = dens_blk[p];
            }
        free(scratch);
    }
}

/* ---------------------------------------------------------------------------------------
 * a6: CalcRayColor.forward                 NetWorks/utils.py:268-309
 * rgb [B,C,Nr,Ns]; density,z_dists,zvals [B,Nr,Ns]
 * -> fg_feat [B,C,Nr]; bg_alpha, depth [B,Nr]; weight [B,Nr,Ns] (nullable)
 * ------------------------------------------------------------------------------------- */
static void ray_weights(int Ns, const float* dens, const float* dist, float* wout) {
    float T = 1.0f;                                            /* pad value 1 (utils.py:284) */
    for (int s = 0; s < Ns; ++s) {
        float alpha = 1.0f - expf(-dens[s] * dist[s]);         /* utils.py:275 */
        wout[s] = alpha * T;                                   /* utils.py:287 */
        float x = 1.0f - alpha + 1e-10f;                       /* utils.py:283 */
        T = T * x;                                             /* cumprod (utils.py:285) */
    }
}

void orc_composite(int B, int Nr, int Ns, int C, const float* rgb, const float* density, const float* z_dists,
                   const float* zvals, float* fg_feat, float* bg_alpha, float* depth, float* weight) {
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < Nr; ++r) {
            float wbuf[1024];
            size_t o = ((size_t)b * Nr + r) * Ns;
            ray_weights(Ns, density + o, z_dists + o, wbuf);
            float acc = 0.0f, dep = 0.0f;
            for (int s = 0; s < Ns; ++s) { acc += wbuf[s]; dep += wbuf[s] * zvals[o + s]; } /* utils.py:303-305 */
            bg_alpha[(size_t)b * Nr + r] = 1.0f - acc;          /* utils.py:306 */
            if (depth) depth[(size_t)b * Nr + r] = dep;
            if (weight) memcpy(weight + o, wbuf, sizeof(float) * Ns);
            for (int c = 0; c < C; ++c) {
                const float* f = rgb + (((size_t)b * C + c) * Nr + r) * Ns;
                float a = 0.0f;
                for (int s = 0; s < Ns; ++s) a += wbuf[s] * f[s]; /* utils.py:302 */
                fg_feat[((size_t)b * C + c) * Nr + r] = a;
            }
        }
}

/* ---------------------------------------------------------------------------------------
 * a8-a10: NeuralRenderer / PixelShuffleUpsample / Blur
 *   NetWorks/neural_renderer.py:49-91, NetWorks/PixelShuffleUpsample.py:8-45
 * All tensors NCHW for one batch element at a time.
 * nr_w pointer order: [to_rgb0.W, to_rgb0.b] then per block i:
 *   [psu.l1.W, psu.l1.b, psu.l2.W, psu.l2.b, feat.W, feat.b, to_rgb(i+1).W, to_rgb(i+1).b]
 * ------------------------------------------------------------------------------------- */
static void conv1x1(const float* W, const float* bias, int cin, int cout, long hw, const float* x, float* y, float slope /* <0: none */) {
#pragma omp parallel for schedule(static)
    for (int o = 0; o < cout; ++o) {
        float* yo = y + (size_t)o * hw;
        float b0 = bias[o];
        for (long p = 0; p < hw; ++p) yo[p] = b0;
        for (int i = 0; i < cin; ++i) {
            float wi = W[(size_t)o * cin + i];
            const float* xi = x + (size_t)i * hw;
            for (long p = 0; p < hw; ++p) yo[p] = fmaf(wi, xi[p], yo[p]);
        }
        if (slope >= 0.0f) for (long p = 0; p < hw; ++p) yo[p] = yo[p] > 0.0f ? yo[p] : yo[p] * slope;
    }
}

static inline int reflect(int i, int n) { /* F.pad(mode='reflect') by 1 */
    if (i < 0) return -i;
    if (i >= n) return 2 * n - 2 - i;
    return i;
}

/* Blur: depthwise [1,2,1]x[1,2,1]/16, reflect border (PixelShuffleUpsample.py:15-18 + kornia filter2d) */
static void blur3(int c, int h, int w, const float* x, float* y) {
    const float k[3] = {1.0f / 4.0f, 2.0f / 4.0f, 1.0f / 4.0f};
#pragma omp parallel for schedule(static)
    for (int ch = 0; ch < c; ++ch)
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) {
                float acc = 0.0f;
                for (int di = -1; di <= 1; ++di)
                    for (int dj = -1; dj <= 1; ++dj)
                        acc += (k[di + 1] * k[dj + 1]) * x[((size_t)ch * h + reflect(i + di, h)) * w + reflect(j + dj, w)];
                y[((size_t)ch * h + i) * w + j] = acc;
            }
}

/* nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False)  (neural_renderer.py:54-55) */
static void bilinear2x(int c, int h, int w, const float* x, float* y) {
    int H2 = 2 * h, W2 = 2 * w;
#pragma omp parallel for schedule(static)
    for (int ch = 0; ch < c; ++ch)
        for (int i = 0; i < H2; ++i) {
            float si = 0.5f * ((float)i + 0.5f) - 0.5f; if (si < 0.0f) si = 0.0f;
            int i0 = (int)si; int i1 = i0 + (i0 < h - 1 ? 1 : 0); float li = si - (float)i0;
            for (int j = 0; j < W2; ++j) {
                float sj = 0.5f * ((float)j + 0.5f) - 0.5f; if (sj < 0.0f) sj = 0.0f;
                int j0 = (int)sj; int j1 = j0 + (j0 < w - 1 ? 1 : 0); float lj = sj - (float)j0;
                const float* xc = x + (size_t)ch * h * w;
                float v = (1.0f - li) * ((1.0f - lj) * xc[(size_t)i0 * w + j0] + lj * xc[(size_t)i0 * w + j1]) +
                          li * ((1.0f - lj) * xc[(size_t)i1 * w + j0] + lj * xc[(size_t)i1 * w + j1]);
                y[((size_t)ch * H2 + i) * W2 + j] = v;
            }
        }
}

/* PixelShuffleUpsample.forward (PixelShuffleUpsample.py:36-45): x [c,h,w] -> out [c,2h,2w] */
static void psu_forward(const float* W1, const float* b1, const float* W2, const float* b2, int c, int h, int w,
                        const float* x, float* out, float* t1, float* t2, float* t3) {
    long hw = (long)h * w;
    conv1x1(W1, b1, c, 2 * c, hw, x, t1, 0.2f);
    conv1x1(W2, b2, 2 * c, 4 * c, hw, t1, t2, 0.2f);
    /* out + x.repeat(1,4,1,1), then pixel_shuffle(2): out[c,2h+i,2w+j] = in[4c+2i+j,h,w] */
#pragma omp parallel for schedule(static)
    for (int ch = 0; ch < c; ++ch)
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j)
                for (int di = 0; di < 2; ++di)
                    for (int dj = 0; dj < 2; ++dj) {
                        int k = ch * 4 + di * 2 + dj;
                        float v = t2[(size_t)k * hw + (size_t)i * w + j] + x[(size_t)(k % c) * hw + (size_t)i * w + j];
                        t3[((size_t)ch * 2 * h + 2 * i + di) * 2 * w + 2 * j + dj] = v;
                    }
    blur3(c, 2 * h, 2 * w, t3, out);
}

static int nr_ch(int C, int i) { int v = C >> i; return v < 32 ? 32 : v; }

/* x [B,C,fs,fs] -> img [B,3,P,P], P = fs << n_blocks.  stage outputs optional (test seams). */
void orc_neural_render(int B, int C, int fs, int n_blocks, const float* const* nr_w, const float* x, float* img,
                       float* dbg_rgb0_up /* [B,3,2fs,2fs] nullable */, float* dbg_psu0 /* [B,C,2fs,2fs] nullable */,
                       float* dbg_net1 /* [B,nr_ch(1),2fs,2fs] nullable */) {
    int P = fs << n_blocks;
    size_t big = (size_t)C * 4 * fs * fs; /* 4C channels at the input resolution == C at 2x; halves each block */
    for (int i = 0; i < n_blocks; ++i) { size_t s = (size_t)nr_ch(C, i) * 4 * (fs << i) * (fs << i); if (s > big) big = s; }
    float* t1 = (float*)malloc(sizeof(float) * big);
    float* t2 = (float*)malloc(sizeof(float) * big);
    float* t3 = (float*)malloc(sizeof(float) * big);
    float* netA = (float*)malloc(sizeof(float) * big);
    float* netB = (float*)malloc(sizeof(float) * big);
    float* rgbA = (float*)malloc(sizeof(float) * 3 * (size_t)P * P);
    float* rgbB = (float*)malloc(sizeof(float) * 3 * (size_t)P * P);
    float* rgbC = (float*)malloc(sizeof(float) * 3 * (size_t)P * P);
    for (int b = 0; b < B; ++b) {
        const float* xb = x + (size_t)b * C * fs * fs;
        int h = fs;
        /* rgb = rgb_upsample(feat_2_rgb_list[0](x))   (neural_renderer.py:75) */
        conv1x1(nr_w[0], nr_w[1], C, 3, (long)h * h, xb, rgbA, -1.0f);
        bilinear2x(3, h, h, rgbA, rgbB);
        blur3(3, 2 * h, 2 * h, rgbB, rgbA);
        if (dbg_rgb0_up) memcpy(dbg_rgb0_up + (size_t)b * 3 * 4 * h * h, rgbA, sizeof(float) * 3 * 4 * h * h);
        const float* net = xb;
        float* cur = netA; float* oth = netB;
        for (int i = 0; i < n_blocks; ++i) {
            const float* const* w = nr_w + 2 + 8 * i;
            int ci = nr_ch(C, i), co = nr_ch(C, i + 1);
            psu_forward(w[0], w[1], w[2], w[3], ci, h, h, net, oth, t1, t2, t3);      /* :79 */
            if (i == 0 && dbg_psu0) memcpy(dbg_psu0 + (size_t)b * ci * 4 * h * h, oth, sizeof(float) * ci * 4 * h * h);
            h *= 2;
            conv1x1(w[4], w[5], ci, co, (long)h * h, oth, cur, 0.2f);                 /* :79-80 */
            if (i == 0 && dbg_net1) memcpy(dbg_net1 + (size_t)b * co * h * h, cur, sizeof(float) * co * h * h);
            conv1x1(w[6], w[7], co, 3, (long)h * h, cur, rgbB, -1.0f);                /* :82 */
            for (size_t k = 0; k < (size_t)3 * h * h; ++k) rgbA[k] = rgbA[k] + rgbB[k];
            if (i < n_blocks - 1) {                                                   /* :83-84 */
                bilinear2x(3, h, h, rgbA, rgbC);
                blur3(3, 2 * h, 2 * h, rgbC, rgbA);
            }
            net = cur;
            float* t = cur; cur = oth; oth = t;
        }
        float* ob = img + (size_t)b * 3 * P * P;
        for (size_t k = 0; k < (size_t)3 * P * P; ++k) ob[k] = 1.0f / (1.0f + expf(-rgbA[k]));   /* :87-88 */
    }
    free(t1); free(t2); free(t3); free(netA); free(netB); free(rgbA); free(rgbB); free(rgbC);
}

void orc_blur(int c, int h, int w, const float* x, float* y) { blur3(c, h, w, x, y); }

/* ---------------------------------------------------------------------------------------
 * a7 + a11: whole forward                 NetWorks/HeadNeRFNet.py:81-120,123-160
 * Streams one ray at a time through a1..a6 (no [B,C,Nr,Ns] intermediates), then a7/a8.
 * outputs: fg_feat [B,C,Nr] (nullable), bg_alpha [B,Nr] (nullable), merge_img [B,3,P,P], bg_img [1,3,P,P]
 * Requires Ns <= NB (64) per block; longer rays are processed in NB-sample blocks.
 * ------------------------------------------------------------------------------------- */
void orc_forward_vd(int B, int Nr, int Ns, int fs, int n_blocks, int H, int C, int shape_dim, int appea_dim, int audio_dim, int vd_dim,
                    const float* const* mlp_w, const float* const* nr_w, const float* bg_featmap, const float* xy, const float* R,
                    const float* T, const float* Kinv, float world_z1, float world_z2, const float* t_rand, const float* shape,
                    const float* appea, const float* audio, float* fg_feat_out, float* bg_alpha_out, float* merge_img, float* bg_img,
                    int skip_neural_render);
void orc_forward(int B, int Nr, int Ns, int fs, int n_blocks, int H, int C, int shape_dim, int appea_dim, int audio_dim,
                 const float* const* mlp_w, const float* const* nr_w, const float* bg_featmap /* [C,fs,fs] */,
                 const float* xy, const float* R, const float* T, const float* Kinv, float world_z1, float world_z2,
                 const float* t_rand, const float* shape, const float* appea, const float* audio,
                 float* fg_feat_out, float* bg_alpha_out, float* merge_img, float* bg_img, int skip_neural_render) {
    orc_forward_vd(B, Nr, Ns, fs, n_blocks, H, C, shape_dim, appea_dim, audio_dim, 0, mlp_w, nr_w, bg_featmap, xy, R, T, Kinv, world_z1,
                   world_z2, t_rand, shape, appea, audio, fg_feat_out, bg_alpha_out, merge_img, bg_img, skip_neural_render);
}
/* vd_dim = 27: include_vd=True (the view direction of the ray, encoded, joins RGB_layer_1's input at every sample:
 * HeadNeRFNet.py:141-142 `vd_encoder(fg_dirs)`, fg_dirs = the ray direction expanded over the samples, utils.py:84) */
void orc_forward_vd(int B, int Nr, int Ns, int fs, int n_blocks, int H, int C, int shape_dim, int appea_dim, int audio_dim, int vd_dim,
                    const float* const* mlp_w, const float* const* nr_w, const float* bg_featmap /* [C,fs,fs] */,
                    const float* xy, const float* R, const float* T, const float* Kinv, float world_z1, float world_z2,
                    const float* t_rand, const float* shape, const float* appea, const float* audio,
                    float* fg_feat_out, float* bg_alpha_out, float* merge_img, float* bg_img, int skip_neural_render) {
    orc_dims dm = {H, C, shape_dim, appea_dim, audio_dim, vd_dim};
    float* fg = fg_feat_out ? fg_feat_out : (float*)malloc(sizeof(float) * (size_t)B * C * Nr);
    float* ba = bg_alpha_out ? bg_alpha_out : (float*)malloc(sizeof(float) * (size_t)B * Nr);
    int nblk = (Ns + NB - 1) / NB;
#pragma omp parallel
    {
        size_t sf = mlp_scratch_floats(&dm);
        float* scratch = (float*)malloc(sizeof(float) * (sf + (size_t)(PE_DIM + C + 1 + VD_DIM) * NB + (size_t)(C + 3) * nblk * NB));
        float* pe_blk = scratch + sf;
        float* rgb_blk = pe_blk + (size_t)PE_DIM * NB;
        float* dens_blk = rgb_blk + (size_t)C * NB;
        float* vd_blk = dens_blk + NB;                        /* [VD_DIM][NB]: the ray's encoded direction at every sample */
        float* ray_rgb = vd_blk + (size_t)VD_DIM * NB;        /* [C][nblk*NB] */
        float* ray_dens = ray_rgb + (size_t)C * nblk * NB;
        float* ray_dist = ray_dens + (size_t)nblk * NB;
        float* ray_w = ray_dist + (size_t)nblk * NB;
#pragma omp for collapse(2) schedule(dynamic, 2)
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < Nr; ++r) {
                float d[3], l;
                const float* Tb = T + b * 3;
                ray_setup(R + b * 9, Tb, Kinv + b * 9, xy[(b * 2 + 0) * Nr + r], xy[(b * 2 + 1) * Nr + r], d, &l);
                float rz1 = Tb[2] - world_z1, rz2 = Tb[2] - world_z2;
                const float* tr = t_rand ? t_rand + ((size_t)b * Nr + r) * (Ns + 1) : NULL;
                int W = nblk * NB;
                if (vd_dim)
                    for (int p = 0; p < NB; ++p) embed_dir(d, vd_blk + p, NB);
                for (int k = 0; k < nblk; ++k) {
                    for (int p = 0; p < NB; ++p) {
                        int s = k * NB + p;
                        float pt[3] = {0.0f, 0.0f, 0.0f};
                        if (s < Ns) {
                            float z_lo = edge_z(rz1, rz2, s, Ns, tr), z_hi = edge_z(rz1, rz2, s + 1, Ns, tr);
                            ray_dist[s] = (z_hi - z_lo) * l;
                            for (int i = 0; i < 3; ++i) pt[i] = Tb[i] + (d[i] * l) * z_lo;
                        }
                        embed_point(pt, pe_blk + p, NB);
                    }
                    mlp_block(&dm, mlp_w, pe_blk, shape + (size_t)b * shape_dim, appea + (size_t)b * appea_dim,
                              audio_dim ? audio + (size_t)b * audio_dim : NULL, vd_dim ? vd_blk : NULL, rgb_blk, dens_blk, scratch);
                    for (int c = 0; c < C; ++c) memcpy(ray_rgb + (size_t)c * W + k * NB, rgb_blk + (size_t)c * NB, sizeof(float) * NB);
                    memcpy(ray_dens + k * NB, dens_blk, sizeof(float) * NB);
                }
                ray_weights(Ns, ray_dens, ray_dist, ray_w);
                float acc = 0.0f;
                for (int s = 0; s < Ns; ++s) acc += ray_w[s];
                ba[(size_t)b * Nr + r] = 1.0f - acc;
                for (int c = 0; c < C; ++c) {
                    float a = 0.0f;
                    const float* f = ray_rgb + (size_t)c * W;
                    for (int s = 0; s < Ns; ++s) a += ray_w[s] * f[s];
                    fg[((size_t)b * C + c) * Nr + r] = a;
                }
            }
        free(scratch);
    }
    if (!skip_neural_render) {
        /* merge = fg + bg_alpha * bg_featmap; render bg alone and merged (HeadNeRFNet.py:103-113) */
        float* merge = (float*)malloc(sizeof(float) * (size_t)B * C * Nr);
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c)
                for (int r = 0; r < Nr; ++r)
                    merge[((size_t)b * C + c) * Nr + r] = fg[((size_t)b * C + c) * Nr + r] + ba[(size_t)b * Nr + r] * bg_featmap[(size_t)c * Nr + r];
        orc_neural_render(1, C, fs, n_blocks, nr_w, bg_featmap, bg_img, NULL, NULL, NULL);
        orc_neural_render(B, C, fs, n_blocks, nr_w, merge, merge_img, NULL, NULL, NULL);
        free(merge);
    }
    if (!fg_feat_out) free(fg);
    if (!bg_alpha_out) free(ba);
}
