// extern "C" entry points of libn3dt.so (declared in include/n3dt.h).
// Host-side only: validates geometry, carves the caller's workspace and enqueues kernels on the
// caller's stream.  No allocation, no synchronisation; the only mutable global state is the opt-in
// measurement hook (n3dt_prof_*, mutex-guarded).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "../../include/n3dt.h"
#include "n3dt_layout.h"
#include "n3dt_launch.h"
#include "eval_metrics_core.h"
#include "lpips_core.h"
#include "mel_core.h"
#include "syncnet_core.h"
#include "wav2lip_core.h"
#include "s3fd_core.h"
#include "face_recon_core.h"
#include "fan_core.h"
#include "head_mask_core.h"

static thread_local char g_err[256] = "";

// the one place a refusal's text is formed: writes the calling thread's n3dt_last_error() string and returns `code`
__attribute__((format(printf, 2, 3))) static int failf(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int fail(int code, const char* msg) { return failf(code, "%s", msg); }

static int check_hip(const char* where) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? N3DT_OK : failf(N3DT_EHIP, "%s: %s", where, hipGetErrorString(e));
}

static int check_geom(const N3dtGeom* g, int precision) {
    if (!g) return fail(N3DT_EINVAL, "geometry is NULL");
    if (precision != N3DT_F32 && precision != N3DT_BF16 && precision != N3DT_F16 && precision != N3DT_BF16X3)
        return fail(N3DT_EINVAL, "unknown precision");
    if (g->batch < 1 || g->n_rays < 1 || g->n_samples < 1) return fail(N3DT_EINVAL, "batch, n_rays and n_samples must be >= 1");
    if (g->n_samples > 1024) return fail(N3DT_EINVAL, "n_samples > 1024 is not supported");
    if (g->hidden != 384) return fail(N3DT_EINVAL, "only mlp_hidden_nchannels == 384 is built");
    if (g->feat_nc != 256) return fail(N3DT_EINVAL, "only featmap_nc == 256 is built");
    if (g->shape_dim < 1 || g->appea_dim < 1 || g->audio_dim < 0) return fail(N3DT_EINVAL, "bad latent widths");
    if (g->shape_dim + g->audio_dim > 512 || g->appea_dim > 512) return fail(N3DT_EINVAL, "latent width > 512");
    if (g->vd_dim != 0 && g->vd_dim != 27) return fail(N3DT_EINVAL, "vd_dim must be 0 or 27 (include_vd: 3 + 6 * 4 channels)");
    return N3DT_OK;
}
// include_vd: the per-ray bias must come with the flag, and only with it
static int check_ray_bias(const N3dtGeom* g, const void* ray_bias, const char* who) {
    if ((g->vd_dim > 0) != (ray_bias != nullptr)) return failf(N3DT_EINVAL, "%s: the per-ray bias must be given iff vd_dim > 0", who);
    return N3DT_OK;
}

static inline int block_samples(int precision) { return precision == N3DT_F32 ? 16 : 32; }
static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct RenderCarve {
    size_t fold, part, wlocal, bghwc, total;  // byte offsets / total bytes
    int bpr, bs;
};

static RenderCarve render_carve(const N3dtGeom* g, int precision) {
    RenderCarve c;
    c.bs = block_samples(precision);
    c.bpr = (g->n_samples + c.bs - 1) / c.bs;
    const size_t blocks = (size_t)g->batch * g->n_rays * c.bpr;
    c.fold = 0;
    c.part = align256(n3dt_fold_region_floats(g->batch, g->n_rays, g->vd_dim) * sizeof(float));  // (+ the per-ray table of include_vd)
    c.wlocal = c.part + align256(blocks * (192 + 4) * sizeof(float));
    c.bghwc = c.wlocal + align256(blocks * c.bs * sizeof(float));  // the background map transposed to [N_r][C] for the merge
    c.total = c.bghwc + align256((size_t)g->n_rays * g->feat_nc * sizeof(float));
    return c;
}

// ---- opt-in measurement hook (see n3dt.h) ---------------------------------------------------
static std::mutex g_prof_mu;
static hipEvent_t* g_prof_ev = nullptr;  // 2 * g_prof_cap events
static int g_prof_cap = 0, g_prof_n = 0;

static void prof_free_locked(int created) {
    for (int i = 0; i < created; ++i) (void)hipEventDestroy(g_prof_ev[i]);
    delete[] g_prof_ev;
    g_prof_ev = nullptr;
    g_prof_cap = g_prof_n = 0;
}

extern "C" int n3dt_prof_enable(int max_records) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    prof_free_locked(2 * g_prof_cap);
    if (max_records <= 0) return N3DT_OK;
    g_prof_ev = new hipEvent_t[2 * (size_t)max_records];
    for (int i = 0; i < 2 * max_records; ++i)
        if (hipEventCreate(&g_prof_ev[i]) != hipSuccess) {
            prof_free_locked(i);  // the events created so far do not leak
            return fail(N3DT_EHIP, "n3dt_prof_enable: hipEventCreate failed");
        }
    g_prof_cap = max_records;
    return N3DT_OK;
}

// A measured span: begin records an event on `s` and returns its slot (or -1: hook off / record list full), end records the
// closing event.  Used by n3dt_render_fwd (the fused MLP kernel) and by the fused training path (forward kernel, dX chain,
// weight-gradient stage: three spans per step, in that order) -- internal, not part of the ABI.
extern "C" int n3dt_prof_span_begin(hipStream_t s) {
    if (g_prof_cap <= 0) return -1;  // the unlocked read is the hook's documented contract: enabled from one thread, while idle
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (g_prof_n >= g_prof_cap) return -1;
    const int slot = g_prof_n++;
    (void)hipEventRecord(g_prof_ev[2 * slot], s);
    return slot;
}
extern "C" void n3dt_prof_span_end(int slot, hipStream_t s) {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (slot < g_prof_cap) (void)hipEventRecord(g_prof_ev[2 * slot + 1], s);
}

extern "C" int n3dt_prof_collect(float* ms_out, int capacity, int* n_out) {
    if (!ms_out || !n_out) return fail(N3DT_EINVAL, "n3dt_prof_collect: NULL argument");
    std::lock_guard<std::mutex> lock(g_prof_mu);
    int n = g_prof_n < capacity ? g_prof_n : capacity;
    for (int i = 0; i < n; ++i) {
        if (hipEventSynchronize(g_prof_ev[2 * i + 1]) != hipSuccess) return fail(N3DT_EHIP, "n3dt_prof_collect: sync failed");
        if (hipEventElapsedTime(&ms_out[i], g_prof_ev[2 * i], g_prof_ev[2 * i + 1]) != hipSuccess)
            return fail(N3DT_EHIP, "n3dt_prof_collect: elapsed failed");
    }
    *n_out = n;
    g_prof_n = 0;
    return N3DT_OK;
}

extern "C" int n3dt_abi_version(void) { return N3DT_ABI_VERSION; }
extern "C" const char* n3dt_last_error(void) { return g_err; }

extern "C" size_t n3dt_mlp_packed_bytes(const N3dtGeom* g, int precision) {
    if (check_geom(g, precision) != N3DT_OK) return 0;
    return n3dt_packed_tail_offset(precision) + n3dt_packed_tail_floats() * sizeof(float);
}

extern "C" int n3dt_mlp_pack(const N3dtGeom* g, int precision, const N3dtMlpParams* p, void* packed, void* stream) {
    int rc = check_geom(g, precision);
    if (rc) return rc;
    if (!p || !packed) return fail(N3DT_EINVAL, "n3dt_mlp_pack: NULL argument");
    for (int l = 0; l < N3DT_MLP_LAYERS; ++l)
        if (!p->weight[l] || !p->bias[l]) return fail(N3DT_EINVAL, "n3dt_mlp_pack: NULL parameter pointer");
    n3dt_launch_pack(g, precision, p, packed, (hipStream_t)stream);
    return check_hip("n3dt_mlp_pack");
}

extern "C" size_t n3dt_render_workspace_bytes(const N3dtGeom* g, int precision) {
    if (check_geom(g, precision) != N3DT_OK) return 0;
    return render_carve(g, precision).total;
}

// n3dt_render_fwd and n3dt_render_fwd16 (the latter with the ray head's 16-bit map / level-0 RGB outputs)
static int render_fwd_common(const N3dtGeom* g, int precision, const void* packed_mlp, const N3dtMlpParams* p, const float* xy,
                             const float* R, const float* T, const float* Kinv, const float* shape, const float* appea,
                             const float* audio, const float* t_rand, const float* bg_featmap, const float* ray_bias, float* fg_feat,
                             float* bg_alpha, float* depth, float* weight, float* merge_feat, void* merge_feat16, float* rgb0,
                             const float* rgb0_w, const float* rgb0_b, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_geom(g, precision);
    if (rc) return rc;
    if ((rc = check_ray_bias(g, ray_bias, "n3dt_render_fwd")) != N3DT_OK) return rc;
    if (!packed_mlp || !p || !xy || !R || !T || !Kinv || !shape || !appea || !workspace)
        return fail(N3DT_EINVAL, "n3dt_render_fwd: NULL argument");
    if (!fg_feat && !merge_feat && !merge_feat16) return fail(N3DT_EINVAL, "n3dt_render_fwd: neither fg_feat nor merge_feat requested");
    if (g->audio_dim > 0 && !audio) return fail(N3DT_EINVAL, "n3dt_render_fwd: audio is NULL but audio_dim > 0");
    if ((merge_feat || merge_feat16 || rgb0) && !bg_featmap) return fail(N3DT_EINVAL, "n3dt_render_fwd: merge_feat needs bg_featmap");
    if ((merge_feat16 || rgb0) && precision == N3DT_F32)
        return fail(N3DT_EINVAL, "n3dt_render_fwd16: the 16-bit map and rgb0 are outputs of the 16-bit precisions");
    if (rgb0 && (!rgb0_w || !rgb0_b)) return fail(N3DT_EINVAL, "n3dt_render_fwd16: rgb0 needs rgb0_w and rgb0_b");
    if (g->z_planes_given && !t_rand) return fail(N3DT_EINVAL, "n3dt_render_fwd: z_planes_given but no planes passed as t_rand");
    const RenderCarve c = render_carve(g, precision);
    if (workspace_bytes < c.total) return fail(N3DT_EWORKSPACE, "n3dt_render_fwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    float* fold = (float*)(ws + c.fold);
    float* part = (float*)(ws + c.part);
    float* wlocal = (float*)(ws + c.wlocal);
    n3dt_launch_fold(g, p, shape, appea, audio, fold, precision != N3DT_F32, s);
    if (ray_bias) n3dt_launch_rayfold(g, fold, ray_bias, s);
    const int span = n3dt_prof_span_begin(s);
    if (precision == N3DT_F32)
        n3dt_launch_nerf_fwd_f32(g, p, packed_mlp, fold, xy, R, T, Kinv, t_rand, part, weight ? wlocal : nullptr, s);
    else if (precision == N3DT_BF16X3)
        n3dt_launch_nerf_fwd_x16s(g, packed_mlp, fold, xy, R, T, Kinv, t_rand, part, weight ? wlocal : nullptr, s);
    else
        n3dt_launch_nerf_fwd_x16(g, precision, packed_mlp, fold, xy, R, T, Kinv, t_rand, part, weight ? wlocal : nullptr, s);
    n3dt_prof_span_end(span, s);
    const float* tail = (const float*)((const unsigned char*)packed_mlp + n3dt_packed_tail_offset(precision));
    const float* bghwc = bg_featmap;
    const bool merged = merge_feat || merge_feat16 || rgb0;
    if (merged && !g->bg_is_hwc) {  // [C][N_r] parameter -> [N_r][C]
        n3dt_launch_chw_to_hwc(g->feat_nc, g->n_rays, bg_featmap, (float*)(ws + c.bghwc), s);
        bghwc = (const float*)(ws + c.bghwc);
    }
    if (precision == N3DT_F32)
        n3dt_launch_ray_head(g, c.bpr, c.bs, part, wlocal, tail, bghwc, 1, fg_feat, bg_alpha, depth, weight, merge_feat, s);
    else if (merge_feat16 || rgb0)  // (the renderer runs the split-precision mode on its f16 path)
        n3dt_launch_ray_head_mfma16(g, c.bpr, c.bs, part, wlocal, tail, bghwc, 1, fg_feat, bg_alpha, depth, weight, merge_feat, merge_feat16,
                                    precision == N3DT_BF16 ? N3DT_BF16 : N3DT_F16, rgb0, rgb0_w, rgb0_b, s);
    else
        n3dt_launch_ray_head_mfma(g, c.bpr, c.bs, part, wlocal, tail, bghwc, 1, fg_feat, bg_alpha, depth, weight, merge_feat, nullptr, s);
    return check_hip("n3dt_render_fwd");
}

extern "C" int n3dt_render_fwd(const N3dtGeom* g, int precision, const void* packed_mlp, const N3dtMlpParams* p, const float* xy,
                               const float* R, const float* T, const float* Kinv, const float* shape, const float* appea,
                               const float* audio, const float* t_rand, const float* bg_featmap, const float* ray_bias, float* fg_feat,
                               float* bg_alpha, float* depth, float* weight, float* merge_feat, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return render_fwd_common(g, precision, packed_mlp, p, xy, R, T, Kinv, shape, appea, audio, t_rand, bg_featmap, ray_bias, fg_feat, bg_alpha,
                             depth, weight, merge_feat, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int n3dt_render_fwd16(const N3dtGeom* g, int precision, const void* packed_mlp, const N3dtMlpParams* p, const float* xy,
                                 const float* R, const float* T, const float* Kinv, const float* shape, const float* appea,
                                 const float* audio, const float* t_rand, const float* bg_featmap, const float* ray_bias, float* fg_feat,
                                 float* bg_alpha, float* depth, float* weight, float* merge_feat, void* merge_feat16, float* rgb0,
                                 const float* rgb0_w, const float* rgb0_b, void* workspace, size_t workspace_bytes, void* stream) {
    return render_fwd_common(g, precision, packed_mlp, p, xy, R, T, Kinv, shape, appea, audio, t_rand, bg_featmap, ray_bias, fg_feat, bg_alpha,
                             depth, weight, merge_feat, merge_feat16, rgb0, rgb0_w, rgb0_b, workspace, workspace_bytes, stream);
}

// ---- stand-alone seams (csrc/seams.hip) ------------------------------------------------------------
extern "C" int n3dt_sample_points(const N3dtGeom* g, const float* xy, const float* R, const float* T, const float* Kinv,
                                  const float* t_rand, float* pts, float* zvals, float* z_dists, float* ray_d, float* ray_l, void* stream) {
    int rc = check_geom(g, N3DT_F32);
    if (rc) return rc;
    if (!xy || !R || !T || !Kinv) return fail(N3DT_EINVAL, "n3dt_sample_points: NULL argument");
    if (g->z_planes_given && !t_rand) return fail(N3DT_EINVAL, "n3dt_sample_points: z_planes_given but no planes passed as t_rand");
    n3dt_launch_sample_points(g, xy, R, T, Kinv, t_rand, pts, zvals, z_dists, ray_d, ray_l, (hipStream_t)stream);
    return check_hip("n3dt_sample_points");
}

extern "C" int n3dt_embed(int batch, size_t m, const float* pts, float* pe, void* stream) {
    if (batch < 1 || m < 1 || !pts || !pe) return fail(N3DT_EINVAL, "n3dt_embed: bad argument");
    n3dt_launch_embed(batch, m, pts, pe, (hipStream_t)stream);
    return check_hip("n3dt_embed");
}

extern "C" int n3dt_embed_freqs(int batch, size_t m, int n_freqs, const float* pts, float* pe, void* stream) {
    if (batch < 1 || m < 1 || n_freqs < 1 || n_freqs > 16 || !pts || !pe) return fail(N3DT_EINVAL, "n3dt_embed_freqs: bad argument");
    n3dt_launch_embed_freqs(batch, m, n_freqs, pts, pe, (hipStream_t)stream);
    return check_hip("n3dt_embed_freqs");
}

extern "C" int n3dt_ray_vd_bias(const N3dtGeom* g, const float* w_vd, int64_t ld_w, const float* xy, const float* R, const float* Kinv,
                                float* ray_bias, void* stream) {
    int rc = check_geom(g, N3DT_F32);
    if (rc) return rc;
    if (g->vd_dim != 27) return fail(N3DT_EINVAL, "n3dt_ray_vd_bias: vd_dim must be 27");
    if (!w_vd || ld_w < 27 || !xy || !R || !Kinv || !ray_bias) return fail(N3DT_EINVAL, "n3dt_ray_vd_bias: bad argument");
    n3dt_launch_ray_vd_bias(g, w_vd, (long)ld_w, xy, R, Kinv, ray_bias, (hipStream_t)stream);
    return check_hip("n3dt_ray_vd_bias");
}

extern "C" size_t n3dt_mlp_points_workspace_bytes(const N3dtGeom* g, size_t m) {
    if (check_geom(g, N3DT_F32) != N3DT_OK || m < 1) return 0;
    return n3dt_seam_mlp_ws_floats(g, m) * sizeof(float);
}

extern "C" int n3dt_mlp_points(const N3dtGeom* g, size_t m, const N3dtMlpParams* p, const float* audio, const float* embed_vps,
                               const float* embed_vds, float* rgb, float* density, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_geom(g, N3DT_F32);
    if (rc) return rc;
    if (m < 1 || !p || !embed_vps || !embed_vds || !rgb || !density || !workspace) return fail(N3DT_EINVAL, "n3dt_mlp_points: NULL argument");
    if (g->audio_dim > 0 && !audio) return fail(N3DT_EINVAL, "n3dt_mlp_points: audio is NULL but audio_dim > 0");
    if ((size_t)g->batch * m > (size_t)1 << 30) return fail(N3DT_EINVAL, "n3dt_mlp_points: more than 2^30 points");
    if (workspace_bytes < n3dt_mlp_points_workspace_bytes(g, m)) return fail(N3DT_EWORKSPACE, "n3dt_mlp_points: workspace too small");
    for (int l = 0; l < N3DT_MLP_LAYERS; ++l)
        if (!p->weight[l] || !p->bias[l]) return fail(N3DT_EINVAL, "n3dt_mlp_points: NULL parameter pointer");
    n3dt_launch_mlp_points(g, m, p, audio, embed_vps, embed_vds, rgb, density, (float*)workspace, (hipStream_t)stream);
    return check_hip("n3dt_mlp_points");
}

extern "C" int n3dt_composite(int batch, int n_rays, int n_samples, int channels, const float* rgb, const float* density,
                              const float* z_dists, const float* zvals, float* feat, float* bg_alpha, float* depth, float* weight,
                              void* stream) {
    if (batch < 1 || n_rays < 1 || n_samples < 1 || channels < 1 || !rgb || !density || !z_dists || !zvals || !feat)
        return fail(N3DT_EINVAL, "n3dt_composite: bad argument");
    if (n_samples > 4096) return fail(N3DT_EINVAL, "n3dt_composite: more than 4096 samples per ray");
    n3dt_launch_composite(batch, n_rays, n_samples, channels, rgb, density, z_dists, zvals, feat, bg_alpha, depth, weight,
                          (hipStream_t)stream);
    return check_hip("n3dt_composite");
}

extern "C" int n3dt_x16_pack_probe(int precision, int form, size_t n, const float* in, uint16_t* out, void* stream) {
    if (precision != N3DT_BF16 && precision != N3DT_F16) return fail(N3DT_EINVAL, "n3dt_x16_pack_probe: precision must be N3DT_BF16 or N3DT_F16");
    if (form != 0 && form != 1) return fail(N3DT_EINVAL, "n3dt_x16_pack_probe: form must be 0 (pack) or 1 (element-wise cast)");
    if (n < 512 || n % 512 != 0 || n / 512 > 0x7fffffffu) return fail(N3DT_EINVAL, "n3dt_x16_pack_probe: n must be a multiple of 512, at most 2^40");
    if (!in || !out) return fail(N3DT_EINVAL, "n3dt_x16_pack_probe: NULL argument");
    n3dt_launch_x16_pack_probe(precision, form, n, in, out, (hipStream_t)stream);
    return check_hip("n3dt_x16_pack_probe");
}

extern "C" int n3dt_x16_pe_probe(int precision, int form, size_t n, const float* points, uint16_t* out, void* stream) {
    if (precision != N3DT_BF16 && precision != N3DT_F16) return fail(N3DT_EINVAL, "n3dt_x16_pe_probe: precision must be N3DT_BF16 or N3DT_F16");
    if (form != 0 && form != 1) return fail(N3DT_EINVAL, "n3dt_x16_pe_probe: form must be 0 (by octave half) or 1 (per channel)");
    if (n < 32 || n % 32 != 0 || n / 32 > 0x7fffffffu) return fail(N3DT_EINVAL, "n3dt_x16_pe_probe: n must be a multiple of 32, at most 2^36");
    if (!points || !out) return fail(N3DT_EINVAL, "n3dt_x16_pe_probe: NULL argument");
    n3dt_launch_x16_pe_probe(precision, form, n, points, out, (hipStream_t)stream);
    return check_hip("n3dt_x16_pe_probe");
}

extern "C" int n3dt_fine_sample(const N3dtGeom* g, int n_fine, const float* weight, const float* T, const float* t_rand, const float* u,
                                float* z_planes, void* stream) {
    int rc = check_geom(g, N3DT_F32);
    if (rc) return rc;
    if (!weight || !T || !z_planes) return fail(N3DT_EINVAL, "n3dt_fine_sample: NULL argument");
    if (g->z_planes_given && !t_rand) return fail(N3DT_EINVAL, "n3dt_fine_sample: z_planes_given but no coarse planes passed as t_rand");
    if (g->n_samples < 3) return fail(N3DT_EINVAL, "n3dt_fine_sample: needs at least 3 coarse samples");
    if (n_fine < 0 || g->n_samples + n_fine + 1 > 2048) return fail(N3DT_EINVAL, "n3dt_fine_sample: more than 2048 planes per ray");
    n3dt_launch_fine_sample(g, n_fine, weight, T, t_rand, u, z_planes, (hipStream_t)stream);
    return check_hip("n3dt_fine_sample");
}

extern "C" size_t n3dt_neural_render_workspace_bytes(const N3dtGeom* g, int nb) {
    if (!g || nb < 1 || g->n_blocks < 1 || g->n_blocks > N3DT_MAX_BLOCKS || g->featmap_size < 2) return 0;
    return n3dt_nr_workspace_floats(g, nb) * sizeof(float);
}

// featmap16 / rgb0 (n3dt_neural_render_fwd16_reuse): the 16-bit input map and its level-0 projection instead of `featmap`
static int neural_render_common(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap, float* img,
                                void* workspace, size_t workspace_bytes, int pack_mode, void* stream, const char* who,
                                const void* featmap16 = nullptr, const float* rgb0 = nullptr) {
    if (!g || !p || !workspace || (pack_mode != 2 && ((!featmap && !featmap16) || !img))) return fail(N3DT_EINVAL, "neural render: NULL argument");
    if (featmap16 && (!rgb0 || precision == N3DT_F32)) return fail(N3DT_EINVAL, "neural render: a 16-bit map needs rgb0 and a 16-bit precision");
    // the split-precision mode renders the 2-D stage on its fp16 path: 2.3e-4 on RGB where bf16 maps reach 1.6e-3 (fixture
    // `contrast`, features O(10)), inside the mode's 1e-3 budget without splitting the renderer's products as well
    if (precision == N3DT_BF16X3) precision = N3DT_F16;
    if (precision != N3DT_F32 && precision != N3DT_BF16 && precision != N3DT_F16) return fail(N3DT_EINVAL, "unknown precision");
    if (nb < 1) return fail(N3DT_EINVAL, "neural render: nb < 1");
    if (g->n_blocks < 1 || g->n_blocks > N3DT_MAX_BLOCKS) return fail(N3DT_EINVAL, "n_blocks must be in 1..8");
    if (g->feat_nc != 256) return fail(N3DT_EINVAL, "only featmap_nc == 256 is built");
    if (g->featmap_size < 2) return fail(N3DT_EINVAL, "featmap_size < 2 (reflect border needs 2 pixels)");
    {
        // the kernels index one map level with 32-bit in-plane offsets: pixels x channels of the largest level below 2^31
        const size_t side = (size_t)g->featmap_size << g->n_blocks, elems = (size_t)nb * side * side * 32;
        if (elems >= ((size_t)1 << 31)) return fail(N3DT_EINVAL, "neural render: nb x output pixels x 32 channels must stay below 2^31 (split the batch)");
    }
    if (workspace_bytes < n3dt_neural_render_workspace_bytes(g, nb)) return fail(N3DT_EWORKSPACE, "neural render workspace too small");
    for (int i = 0; i <= g->n_blocks; ++i)
        if (!p->to_rgb_w[i] || !p->to_rgb_b[i]) return fail(N3DT_EINVAL, "NULL feat_2_rgb parameter");
    for (int i = 0; i < g->n_blocks; ++i)
        if (!p->psu1_w[i] || !p->psu1_b[i] || !p->psu2_w[i] || !p->psu2_b[i] || !p->feat_w[i] || !p->feat_b[i])
            return fail(N3DT_EINVAL, "NULL neural-render block parameter");
    if (featmap16)
        n3dt_launch_neural_render16(g, nb, precision, p, featmap16, rgb0, img, (float*)workspace, (hipStream_t)stream);
    else
        n3dt_launch_neural_render(g, nb, precision, p, featmap, img, (float*)workspace, pack_mode, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_neural_render_fwd(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap,
                                      float* img, void* workspace, size_t workspace_bytes, void* stream) {
    return neural_render_common(g, nb, precision, p, featmap, img, workspace, workspace_bytes, 0, stream, "n3dt_neural_render_fwd");
}

extern "C" int n3dt_neural_render_pack(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return neural_render_common(g, nb, precision, p, nullptr, nullptr, workspace, workspace_bytes, 2, stream, "n3dt_neural_render_pack");
}

extern "C" int n3dt_neural_render_fwd_reuse(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap,
                                            float* img, void* workspace, size_t workspace_bytes, void* stream) {
    return neural_render_common(g, nb, precision, p, featmap, img, workspace, workspace_bytes, 1, stream, "n3dt_neural_render_fwd_reuse");
}

extern "C" int n3dt_feat_to_rgb0(int nb, int n_pix, const float* featmap, const float* w, const float* b, float* rgb0, void* stream) {
    if (nb < 1 || n_pix < 1 || !featmap || !w || !b || !rgb0) return fail(N3DT_EINVAL, "n3dt_feat_to_rgb0: bad argument");
    if ((size_t)nb * n_pix >= ((size_t)1 << 27)) return fail(N3DT_EINVAL, "n3dt_feat_to_rgb0: more than 2^27 pixels");
    n3dt_launch_feat_to_rgb0(nb, n_pix, featmap, w, b, rgb0, (hipStream_t)stream);
    return check_hip("n3dt_feat_to_rgb0");
}

extern "C" int n3dt_neural_render_fwd16_reuse(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const void* featmap16,
                                              const float* rgb0, float* img, void* workspace, size_t workspace_bytes, void* stream) {
    if (!featmap16) return fail(N3DT_EINVAL, "n3dt_neural_render_fwd16_reuse: NULL argument");
    return neural_render_common(g, nb, precision, p, nullptr, img, workspace, workspace_bytes, 1, stream, "n3dt_neural_render_fwd16_reuse",
                                featmap16, rgb0);
}

// ---- VGG16 perceptual term (csrc/vgg_loss.hip) ----
static int check_vgg(const char* who, int batch, int img_size, int precision) {
    if (precision != N3DT_F32 && precision != N3DT_BF16)
        return failf(N3DT_EINVAL, "%s: unsupported precision %d (N3DT_F32 or N3DT_BF16)", who, precision);
    if (batch < 1 || batch > 64) return failf(N3DT_EINVAL, "%s: batch %d outside 1..64", who, batch);
    if (img_size < 16 || img_size > 2048) return failf(N3DT_EINVAL, "%s: img_size %d outside 16..2048", who, img_size);
    return N3DT_OK;
}

extern "C" size_t n3dt_vgg_packed_bytes(int precision) {
    if (check_vgg("n3dt_vgg_packed_bytes", 1, 224, precision)) return 0;
    return n3dt_vgg_packed_layout_bytes(precision);
}

extern "C" size_t n3dt_vgg_saved_bytes(int batch, int precision) {
    if (check_vgg("n3dt_vgg_saved_bytes", batch, 224, precision)) return 0;
    return n3dt_vgg_saved_floats(batch) * sizeof(float);
}

extern "C" size_t n3dt_vgg_workspace_bytes(int batch, int img_size, int precision) {
    if (check_vgg("n3dt_vgg_workspace_bytes", batch, img_size, precision)) return 0;
    return n3dt_vgg_ws_floats(batch) * sizeof(float);
}

extern "C" int n3dt_vgg_pack(int precision, const N3dtVggParams* p, void* packed, void* stream) {
    int rc = check_vgg("n3dt_vgg_pack", 1, 224, precision);
    if (rc) return rc;
    if (!p || !packed) return fail(N3DT_EINVAL, "n3dt_vgg_pack: NULL argument");
    for (int l = 0; l < N3DT_VGG_CONVS; ++l)
        if (!p->weight[l] || !p->bias[l]) return fail(N3DT_EINVAL, "n3dt_vgg_pack: NULL parameter pointer");
    n3dt_launch_vgg_pack(precision, p, packed, (hipStream_t)stream);
    return check_hip("n3dt_vgg_pack");
}

extern "C" int n3dt_vgg_loss_fwd(int batch, int img_size, int precision, const void* packed, const float* merge_img, const float* gt,
                                 const float* mask, float bg_value, float* terms, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                                 void* stream) {
    int rc = check_vgg("n3dt_vgg_loss_fwd", batch, img_size, precision);
    if (rc) return rc;
    if (!packed || !merge_img || !gt || !terms || !saved || !ws) return fail(N3DT_EINVAL, "n3dt_vgg_loss_fwd: NULL argument");
    if (saved_bytes < n3dt_vgg_saved_floats(batch) * sizeof(float)) return fail(N3DT_EWORKSPACE, "n3dt_vgg_loss_fwd: saved buffer too small");
    if (ws_bytes < n3dt_vgg_ws_floats(batch) * sizeof(float)) return fail(N3DT_EWORKSPACE, "n3dt_vgg_loss_fwd: workspace too small");
    n3dt_launch_vgg_fwd(batch, img_size, precision, packed, merge_img, gt, mask, bg_value, terms, saved, ws, (hipStream_t)stream);
    return check_hip("n3dt_vgg_loss_fwd");
}

extern "C" int n3dt_vgg_loss_bwd(int batch, int img_size, int precision, const void* packed, const float* merge_img, const float* g_total,
                                 const void* saved, size_t saved_bytes, float* d_merge, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_vgg("n3dt_vgg_loss_bwd", batch, img_size, precision);
    if (rc) return rc;
    if (!packed || !merge_img || !g_total || !saved || !d_merge || !ws) return fail(N3DT_EINVAL, "n3dt_vgg_loss_bwd: NULL argument");
    if (saved_bytes < n3dt_vgg_saved_floats(batch) * sizeof(float)) return fail(N3DT_EWORKSPACE, "n3dt_vgg_loss_bwd: saved buffer too small");
    if (ws_bytes < n3dt_vgg_ws_floats(batch) * sizeof(float)) return fail(N3DT_EWORKSPACE, "n3dt_vgg_loss_bwd: workspace too small");
    n3dt_launch_vgg_bwd(batch, img_size, precision, packed, merge_img, g_total, saved, d_merge, ws, (hipStream_t)stream);
    return check_hip("n3dt_vgg_loss_bwd");
}

extern "C" int n3dt_vgg_conv_stage(int precision, const void* packed, int layer, int dgrad, int n_img, int H, int W, const float* in,
                                   const float* gate, float* out, int out_pad, void* stream) {
    static const char* who = "n3dt_vgg_conv_stage";
    int rc = check_vgg(who, 1, 224, precision);
    if (rc) return rc;
    const char* what = nullptr;
    if (layer < 0 || layer >= N3DT_VGG_CONVS) what = "layer outside 0..9";
    else if (dgrad != 0 && dgrad != 1) what = "direction must be 0 (forward) or 1 (dgrad)";
    else if (n_img < 1 || n_img > 128) what = "n_img outside 1..128";
    else if (H < 1 || H > 224 || W < 1 || W > 224) what = "H, W outside 1..224";
    else if (out_pad != 0 && out_pad != 1) what = "out_pad must be 0 or 1";
    else if (!packed || !in || !out) what = "NULL pointer";
    else if (gate && !dgrad) what = "a gate goes with dgrad only";
    else if ((((size_t)in) | ((size_t)out) | ((size_t)gate)) & 15) what = "in, gate and out must be 16-byte aligned";
    else if (((size_t)packed) & 255) what = "packed must be 256-byte aligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_vgg_conv_stage(precision, packed, layer, dgrad, n_img, H, W, in, gate, out, out_pad, (hipStream_t)stream);
    return check_hip(who);
}

// ---- Audio2style encoder (csrc/audio_lstm.hip) ----
static int check_a2s_T(const char* who, int T) {
    if (T < 1 || T > N3DT_A2S_MAX_T) return failf(N3DT_EINVAL, "%s: T = %d outside 1..%d", who, T, N3DT_A2S_MAX_T);
    return N3DT_OK;
}

static bool a2s_aligned(const void* q) { return (((size_t)q) & 15) == 0; }

// every parameter pointer non-NULL and 16-byte aligned (the step kernels read W_hh with 16-byte loads)
static int check_a2s_params(const char* who, const N3dtA2sParams* p) {
    if (!p) return failf(N3DT_EINVAL, "%s: params is NULL", who);
    static const char* names[4] = {"w_ih", "w_hh", "b_ih", "b_hh"};
    const float* const* lstm[4] = {p->w_ih, p->w_hh, p->b_ih, p->b_hh};
    for (int a = 0; a < 4; ++a)
        for (int k = 0; k < 4; ++k)
            if (!lstm[a][k] || !a2s_aligned(lstm[a][k]))
                return failf(N3DT_EINVAL, "%s: params->%s[%d] is NULL or not 16-byte aligned", who, names[a], k);
    for (int k = 0; k < 3; ++k) {
        if (!p->lin_w[k] || !a2s_aligned(p->lin_w[k]))
            return failf(N3DT_EINVAL, "%s: params->lin_w[%d] is NULL or not 16-byte aligned", who, k);
        if (!p->lin_b[k] || !a2s_aligned(p->lin_b[k]))
            return failf(N3DT_EINVAL, "%s: params->lin_b[%d] is NULL or not 16-byte aligned", who, k);
    }
    return N3DT_OK;
}

static int check_a2s_buf(const char* who, const char* name, const void* q, size_t have, size_t need) {
    if (!q || !a2s_aligned(q)) return failf(N3DT_EINVAL, "%s: %s is NULL or not 16-byte aligned", who, name);
    if (have < need) return failf(N3DT_EINVAL, "%s: %s_bytes = %zu, %zu needed", who, name, have, need);
    return N3DT_OK;
}

extern "C" size_t n3dt_a2s_saved_bytes(int T) {
    if (check_a2s_T("n3dt_a2s_saved_bytes", T)) return 0;
    return n3dt_a2s_saved_floats(T) * sizeof(float);
}

extern "C" size_t n3dt_a2s_workspace_bytes(int T) {
    if (check_a2s_T("n3dt_a2s_workspace_bytes", T)) return 0;
    return n3dt_a2s_ws_floats(T) * sizeof(float);
}

extern "C" int n3dt_a2s_fwd(int T, const N3dtA2sParams* p, const float* mel, const float* mask1, const float* mask2, const float* mask3,
                            float* out, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "n3dt_a2s_fwd";
    int rc = check_a2s_T(who, T);
    if (!rc) rc = check_a2s_params(who, p);
    if (rc) return rc;
    if (!mel || !a2s_aligned(mel)) return failf(N3DT_EINVAL, "%s: mel is NULL or not 16-byte aligned", who);
    if (!out) return failf(N3DT_EINVAL, "%s: out is NULL", who);
    const float* masks[3] = {mask1, mask2, mask3};
    if ((mask1 != nullptr) != (mask2 != nullptr) || (mask1 != nullptr) != (mask3 != nullptr))
        return failf(N3DT_EINVAL, "%s: mask1, mask2 and mask3 must be all given or all NULL", who);
    if ((rc = check_a2s_buf(who, "saved", saved, saved_bytes, n3dt_a2s_saved_floats(T) * sizeof(float)))) return rc;
    if ((rc = check_a2s_buf(who, "ws", ws, ws_bytes, n3dt_a2s_ws_floats(T) * sizeof(float)))) return rc;
    n3dt_launch_a2s_fwd(T, p, mel, masks, out, saved, ws, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_a2s_bwd(int T, const N3dtA2sParams* p, const float* g_out, const void* saved, size_t saved_bytes, float* grad_arena,
                            void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "n3dt_a2s_bwd";
    int rc = check_a2s_T(who, T);
    if (!rc) rc = check_a2s_params(who, p);
    if (rc) return rc;
    if (!g_out) return failf(N3DT_EINVAL, "%s: g_out is NULL", who);
    if (!grad_arena || !a2s_aligned(grad_arena)) return failf(N3DT_EINVAL, "%s: grad_arena is NULL or not 16-byte aligned", who);
    if ((rc = check_a2s_buf(who, "saved", saved, saved_bytes, n3dt_a2s_saved_floats(T) * sizeof(float)))) return rc;
    if ((rc = check_a2s_buf(who, "ws", ws, ws_bytes, n3dt_a2s_ws_floats(T) * sizeof(float)))) return rc;
    n3dt_launch_a2s_bwd(T, p, g_out, saved, grad_arena, ws, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" size_t n3dt_flat_adam_record_bytes(int which) {
    return which == 0 ? sizeof(N3dtAdamTensor) : which == 1 ? sizeof(N3dtAdamChunk) : which == 2 ? sizeof(N3dtAdamGroup) : 0;
}

extern "C" int n3dt_flat_adam_step(const void* tensor_table, const void* chunk_table, int n_chunks, const void* group_table,
                                   int n_groups, void* step_counter, void* stream) {
    if (!tensor_table || !chunk_table || !group_table || !step_counter) return fail(N3DT_EINVAL, "n3dt_flat_adam_step: NULL table");
    if (n_chunks <= 0) return fail(N3DT_EINVAL, "n3dt_flat_adam_step: n_chunks must be >= 1");
    if (n_groups < 1 || n_groups > N3DT_ADAM_MAX_GROUPS) return fail(N3DT_EINVAL, "n3dt_flat_adam_step: n_groups outside 1..64");
    if ((((size_t)tensor_table) | ((size_t)chunk_table) | ((size_t)group_table)) & 7 || ((size_t)step_counter) & 3)
        return fail(N3DT_EINVAL, "n3dt_flat_adam_step: tables must be 8-byte aligned, the step counter 4-byte aligned");
    n3dt_launch_flat_adam(tensor_table, chunk_table, n_chunks, group_table, n_groups, step_counter, (hipStream_t)stream);
    return check_hip("n3dt_flat_adam_step");
}

extern "C" size_t n3dt_flat_adam_guard_bytes(void) { return sizeof(N3dtAdamGuard); }

extern "C" int n3dt_flat_adam_guarded_step(const void* tensor_table, const void* chunk_table, int n_chunks, const void* group_table,
                                           int n_groups, void* step_counter, void* partials, void* guard, void* stream) {
    static const char* who = "n3dt_flat_adam_guarded_step";
    const char* what = nullptr;
    if (!tensor_table || !chunk_table || !group_table || !step_counter) what = "NULL table";
    else if (!partials || !guard) what = "NULL partials or guard record";
    else if (n_chunks <= 0) what = "n_chunks must be >= 1";
    else if (n_groups < 1 || n_groups > N3DT_ADAM_MAX_GROUPS) what = "n_groups outside 1..64";
    else if ((((size_t)tensor_table) | ((size_t)chunk_table) | ((size_t)group_table)) & 7 || ((size_t)step_counter) & 3)
        what = "tables must be 8-byte aligned, the step counter 4-byte aligned";
    else if (((size_t)partials) & 7 || ((size_t)guard) & 3) what = "partials must be 8-byte aligned, the guard record 4-byte aligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_flat_adam_guarded(tensor_table, chunk_table, n_chunks, group_table, n_groups, step_counter, partials, guard,
                                  (hipStream_t)stream);
    return check_hip(who);
}

// validation metrics (csrc/eval_metrics.hip): the limits of include/n3dt.h, checked before anything is enqueued
static const char* eval_metrics_geometry(int n_images, int height, int width) {
    if (n_images < 1) return "n_images must be >= 1";
    if (height < EVM_WIN || width < EVM_WIN) return "height and width must be >= 7 (one 7x7 window)";
    if ((long long)height * (long long)width >= EVM_MAX_HW) return "height * width must stay below 2^31";
    return nullptr;
}

extern "C" size_t n3dt_eval_metrics_workspace_bytes(int n_images, int height, int width) {
    const char* what = eval_metrics_geometry(n_images, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_eval_metrics_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_eval_metrics_ws_bytes(n_images, height, width);
}

extern "C" int n3dt_eval_metrics(int n_images, int height, int width, const float* pred, const float* gt, double* ssim, double* psnr,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_eval_metrics";
    const char* what = eval_metrics_geometry(n_images, height, width);
    if (!what) {
        if (!pred || !gt || !ssim || !psnr || !workspace) what = "NULL pointer";
        else if ((((size_t)ssim) | ((size_t)psnr) | ((size_t)workspace)) & 7) what = "ssim, psnr and the workspace must be 8-byte aligned";
        else if ((((size_t)pred) | ((size_t)gt)) & 3) what = "pred and gt must be 4-byte aligned";
        else if (workspace_bytes < n3dt_eval_metrics_ws_bytes(n_images, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_eval_metrics(n_images, height, width, pred, gt, ssim, psnr, workspace, (hipStream_t)stream);
    return check_hip(who);
}

// LPIPS (csrc/lpips.hip): the limits of include/n3dt.h, checked before anything is enqueued
static const char* lpips_geometry(int batch, int height, int width) {
    if (batch < 1 || batch > LP_MAX_BATCH) return "batch outside 1..64";
    if (height < LP_MIN_HW || width < LP_MIN_HW) return "height and width must be >= 31 (one pixel of every layer)";
    if (height > LP_MAX_HW || width > LP_MAX_HW) return "height and width must be <= 2048";
    return nullptr;
}

extern "C" size_t n3dt_lpips_packed_bytes(void) { return n3dt_lpips_packed_layout_bytes(); }

extern "C" int n3dt_lpips_pack(const N3dtLpipsParams* p, void* packed, void* stream) {
    if (!p || !packed) return fail(N3DT_EINVAL, "n3dt_lpips_pack: NULL argument");
    if (((size_t)packed) & 255) return fail(N3DT_EINVAL, "n3dt_lpips_pack: packed must be 256-byte aligned");
    for (int l = 0; l < N3DT_LPIPS_LAYERS; ++l)
        if (!p->weight[l] || !p->bias[l] || !p->lin[l]) return fail(N3DT_EINVAL, "n3dt_lpips_pack: NULL parameter pointer");
    n3dt_launch_lpips_pack(p, packed, (hipStream_t)stream);
    return check_hip("n3dt_lpips_pack");
}

extern "C" size_t n3dt_lpips_workspace_bytes(int batch, int height, int width) {
    const char* what = lpips_geometry(batch, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_lpips_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_lpips_ws_bytes(batch, height, width);
}

extern "C" int n3dt_lpips(int batch, int height, int width, int input_mode, const void* packed, const float* pred, const float* gt,
                          double* out, double* layers, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_lpips";
    const char* what = lpips_geometry(batch, height, width);
    if (!what) {
        if (input_mode != N3DT_LPIPS_REFERENCE && input_mode != N3DT_LPIPS_STANDARD) what = "input_mode must be N3DT_LPIPS_REFERENCE or N3DT_LPIPS_STANDARD";
        else if (!packed || !pred || !gt || !out || !workspace) what = "NULL pointer";
        else if ((((size_t)out) | ((size_t)layers)) & 7) what = "out and layers must be 8-byte aligned";
        else if ((((size_t)pred) | ((size_t)gt)) & 3) what = "pred and gt must be 4-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_lpips_ws_bytes(batch, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_lpips(batch, height, width, input_mode, packed, pred, gt, out, layers, workspace, (hipStream_t)stream);
    return check_hip(who);
}

// audio front end (csrc/mel.hip): the limits of include/n3dt.h, checked before anything is enqueued
extern "C" size_t n3dt_mel_workspace_bytes(void) { return n3dt_mel_ws_bytes(); }

extern "C" int n3dt_mel_spectrogram(int64_t n_samples, const float* wav, int64_t wav_offset, const float* prev_sample, int64_t total_samples,
                                    int64_t first_frame, int n_frames, const float* basis, const double* table, void* out, int64_t out_ld,
                                    int out_is_f64, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_mel_spectrogram";
    const char* what = nullptr;
    if (n_samples < MEL_MIN_SAMPLES) what = "n_samples must be >= 401 (the reflect padding of 400 needs 401 samples)";
    else if (n_frames < 1 || n_frames > MEL_MAX_FRAMES) what = "n_frames outside 1..2^24";
    else if (!wav || !basis || !table || !out || !workspace) what = "NULL pointer";
    else if (n_samples > ((int64_t)1 << 40) || wav_offset > ((int64_t)1 << 40) || first_frame > ((int64_t)1 << 32)) what = "signal position out of range";
    else what = mel_run_covers(n_samples, wav_offset, total_samples, prev_sample != nullptr, first_frame, n_frames);
    if (!what) {
        if (out_ld < n_frames) what = "out_ld must be >= n_frames";
        else if (((size_t)table) & 7 || (out_is_f64 && ((size_t)out) & 7)) what = "table and a double out must be 8-byte aligned";
        else if ((((size_t)wav) | ((size_t)prev_sample) | ((size_t)basis) | ((size_t)out) | ((size_t)workspace)) & 3)
            what = "wav, prev_sample, basis, out and the workspace must be 4-byte aligned";
        else if (workspace_bytes < n3dt_mel_ws_bytes()) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    MelSignal sig;
    sig.wav = wav;
    sig.prev = prev_sample;
    sig.n_samples = n_samples;
    sig.offset = wav_offset;
    sig.total = total_samples < 0 ? -1 : total_samples;
    n3dt_launch_mel_spectrogram(&sig, first_frame, n_frames, basis, table, out, out_ld, out_is_f64, workspace, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_mel_windows(int64_t T, const void* mel, int64_t mel_ld, int mel_is_f64, int n_windows, const int32_t* start, float* out,
                                void* stream) {
    static const char* who = "n3dt_mel_windows";
    const char* what = nullptr;
    if (T < 1 || mel_ld < T || mel_ld > ((int64_t)1 << 40)) what = "need 1 <= T <= mel_ld";
    else if (n_windows < 1) what = "n_windows must be >= 1";
    else if (!mel || !start || !out) what = "NULL pointer";
    else if ((((size_t)mel) & (mel_is_f64 ? 7 : 3)) || (((size_t)start) | ((size_t)out)) & 3) what = "mel, start or out misaligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_mel_windows(mel, T, mel_ld, mel_is_f64, start, n_windows, out, (hipStream_t)stream);
    return check_hip(who);
}

// lip-sync expert (csrc/syncnet.hip): the limits of include/n3dt.h, checked before anything is enqueued
static const char* syncnet_windows(int n) { return (n < 1 || n > SN_MAX_WINDOWS) ? "n outside 1..1024" : nullptr; }
static const char* syncnet_frames(int n, int height, int width, const float* frames, const int32_t* boxes, int n_boxes) {
    if (height < 2 || width < 2 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) return "height and width must be in 2..4096";
    if (!frames || !boxes) return "NULL pointer";
    if (n_boxes != 1 && n_boxes != n + SN_FACE_FRAMES - 1) return "n_boxes must be 1 or n + 4 (one box per frame)";
    if ((((size_t)frames) | ((size_t)boxes)) & 3) return "frames and boxes must be 4-byte aligned";
    return nullptr;
}

extern "C" size_t n3dt_syncnet_packed_bytes(void) { return n3dt_syncnet_packed_layout_bytes(); }

extern "C" int n3dt_syncnet_pack(const N3dtSyncnetParams* p, void* packed, void* stream) {
    if (!p || !packed) return fail(N3DT_EINVAL, "n3dt_syncnet_pack: NULL argument");
    if (((size_t)packed) & 255) return fail(N3DT_EINVAL, "n3dt_syncnet_pack: packed must be 256-byte aligned");
    for (int b = 0; b < N3DT_SYNCNET_BLOCKS; ++b)
        if (!p->weight[b] || !p->bias[b] || !p->bn_weight[b] || !p->bn_bias[b] || !p->bn_mean[b] || !p->bn_var[b])
            return fail(N3DT_EINVAL, "n3dt_syncnet_pack: NULL parameter pointer");
    n3dt_launch_syncnet_pack(p, packed, (hipStream_t)stream);
    return check_hip("n3dt_syncnet_pack");
}

extern "C" size_t n3dt_syncnet_workspace_bytes(int n) {
    const char* what = syncnet_windows(n);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_syncnet_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_syncnet_ws_bytes(n);
}

extern "C" int n3dt_syncnet_face_windows(int n, int height, int width, const float* frames, const int32_t* boxes, int n_boxes,
                                         float* face_windows, void* stream) {
    static const char* who = "n3dt_syncnet_face_windows";
    const char* what = syncnet_windows(n);
    if (!what) what = syncnet_frames(n, height, width, frames, boxes, n_boxes);
    if (!what) {
        if (!face_windows) what = "NULL pointer";
        else if (((size_t)face_windows) & 15) what = "face_windows must be 16-byte aligned";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_syncnet_faces(n, height, width, frames, boxes, n_boxes == 1 ? 0 : 4, face_windows, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_syncnet_fwd(int n, const void* packed, const float* mel_windows, const float* face_windows, const float* frames,
                                const int32_t* boxes, int n_boxes, int height, int width, float* audio_emb, float* face_emb, double* cosv,
                                void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_syncnet_fwd";
    const char* what = syncnet_windows(n);
    if (!what) {
        if ((face_windows != nullptr) == (frames != nullptr)) what = "give exactly one of face_windows and frames";
        else if (frames) what = syncnet_frames(n, height, width, frames, boxes, n_boxes);
    }
    if (!what) {
        if (!packed || !mel_windows || !workspace) what = "NULL pointer";
        else if (((size_t)cosv) & 7) what = "cos must be 8-byte aligned";
        else if ((((size_t)mel_windows) | ((size_t)face_windows) | ((size_t)audio_emb) | ((size_t)face_emb)) & 15)
            what = "mel_windows, face_windows, audio_emb and face_emb must be 16-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_syncnet_ws_bytes(n)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    if (frames) {
        float* faces = n3dt_syncnet_ws_faces(n, workspace);
        n3dt_launch_syncnet_faces(n, height, width, frames, boxes, n_boxes == 1 ? 0 : 4, faces, (hipStream_t)stream);
        face_windows = faces;
    }
    n3dt_launch_syncnet_fwd(n, packed, mel_windows, face_windows, audio_emb, face_emb, cosv, workspace, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_syncnet_block(int block, int n, const void* packed, const float* in, float* out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    static const char* who = "n3dt_syncnet_block";
    const char* what = syncnet_windows(n);
    if (!what) {
        if (block < 0 || block >= SN_BLOCKS) what = "block outside 0..30";
        else if (!packed || !in || !out || !workspace) what = "NULL pointer";
        else if ((((size_t)in) | ((size_t)out)) & 15) what = "in and out must be 16-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_syncnet_ws_bytes(n)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_syncnet_block(block, n, packed, in, out, workspace, (hipStream_t)stream);
    return check_hip(who);
}

// Wav2Lip's generator (csrc/wav2lip.hip): the limits of include/n3dt.h, checked before anything is enqueued
static const char* wav2lip_windows(int n) { return (n < 1 || n > W2L_MAX_WINDOWS) ? "n outside 1..128" : nullptr; }
static const char* wav2lip_frames(int n, int height, int width, const float* frames, const int32_t* boxes, int n_boxes, const float* other,
                                  const float* out) {
    if (n < 1 || n > W2L_MAX_FRAMES) return "n outside 1..4096";
    if (height < 2 || width < 2 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) return "height and width must be in 2..4096";
    if (!frames || !boxes || !out) return "NULL pointer";
    if (n_boxes != 1 && n_boxes != n) return "n_boxes must be 1 or n (one box per frame)";
    if ((((size_t)frames) | ((size_t)boxes) | ((size_t)other)) & 3) return "frames and boxes must be 4-byte aligned";
    return nullptr;
}

extern "C" size_t n3dt_wav2lip_packed_bytes(void) { return n3dt_wav2lip_packed_layout_bytes(); }

extern "C" int n3dt_wav2lip_pack(const N3dtWav2lipParams* p, void* packed, void* stream) {
    if (!p || !packed) return fail(N3DT_EINVAL, "n3dt_wav2lip_pack: NULL argument");
    if (((size_t)packed) & 255) return fail(N3DT_EINVAL, "n3dt_wav2lip_pack: packed must be 256-byte aligned");
    for (int b = 0; b < N3DT_WAV2LIP_BLOCKS; ++b) {
        const bool bn = b != W2L_HEAD;
        if (!p->weight[b] || !p->bias[b] || (bn && (!p->bn_weight[b] || !p->bn_bias[b] || !p->bn_mean[b] || !p->bn_var[b])))
            return fail(N3DT_EINVAL, "n3dt_wav2lip_pack: NULL parameter pointer");
    }
    n3dt_launch_wav2lip_pack(p, packed, (hipStream_t)stream);
    return check_hip("n3dt_wav2lip_pack");
}

extern "C" size_t n3dt_wav2lip_workspace_bytes(int n) {
    const char* what = wav2lip_windows(n);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_wav2lip_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_wav2lip_ws_bytes(n);
}

extern "C" int n3dt_wav2lip_fwd(int n, const void* packed, const float* mel_windows, const float* face_inputs, float* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_wav2lip_fwd";
    const char* what = wav2lip_windows(n);
    if (!what) {
        if (!packed || !mel_windows || !face_inputs || !out || !workspace) what = "NULL pointer";
        else if ((((size_t)mel_windows) | ((size_t)face_inputs) | ((size_t)out)) & 15) what = "mel_windows, face_inputs and out must be 16-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_wav2lip_ws_bytes(n)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_wav2lip_fwd(n, packed, mel_windows, face_inputs, out, workspace, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_wav2lip_block(int block, int n, const void* packed, const float* in, const float* skip, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_wav2lip_block";
    const char* what = wav2lip_windows(n);
    if (!what) {
        if (block < 0 || block >= W2L_BLOCKS) what = "block outside 0..50";
        else if (!packed || !in || !out || !workspace) what = "NULL pointer";
        else if ((((size_t)in) | ((size_t)skip) | ((size_t)out)) & 15) what = "in, skip and out must be 16-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_wav2lip_ws_bytes(n)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_wav2lip_block(block, n, packed, in, skip, out, workspace, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_wav2lip_face_inputs(int n, int height, int width, const float* frames, const float* ref_frames, const int32_t* boxes,
                                        int n_boxes, float* out, void* stream) {
    static const char* who = "n3dt_wav2lip_face_inputs";
    const char* what = wav2lip_frames(n, height, width, frames, boxes, n_boxes, ref_frames, out);
    if (!what && (((size_t)out) & 15)) what = "out must be 16-byte aligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_wav2lip_face_inputs(n, height, width, frames, ref_frames, boxes, n_boxes == 1 ? 0 : 4, out, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_wav2lip_paste(int n, int height, int width, const float* faces, const float* frames, const int32_t* boxes, int n_boxes,
                                  float* out, void* stream) {
    static const char* who = "n3dt_wav2lip_paste";
    const char* what = wav2lip_frames(n, height, width, frames, boxes, n_boxes, nullptr, out);
    if (!what) {
        if (!faces) what = "NULL pointer";
        else if (((size_t)faces) & 15) what = "faces must be 16-byte aligned";
        else if (((size_t)out) & 3) what = "out must be 4-byte aligned";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_wav2lip_paste(n, height, width, faces, frames, boxes, n_boxes == 1 ? 0 : 4, out, (hipStream_t)stream);
    return check_hip(who);
}

// The S3FD face detector (csrc/s3fd.hip): the limits of include/n3dt.h, checked before anything is enqueued
static const char* s3fd_size(int n, int height, int width) {
    if (!s3_hw_ok(height, width)) return "height and width must be in 32..4096";
    if (n < 1 || n > s3_max_images(height, width)) return "n outside 1..n3dt_s3fd_max_images (the workspace budget)";
    return nullptr;
}

extern "C" size_t n3dt_s3fd_packed_bytes(void) { return n3dt_s3fd_packed_layout_bytes(); }

extern "C" int n3dt_s3fd_pack(const N3dtS3fdParams* p, void* packed, void* stream) {
    if (!p || !packed) return fail(N3DT_EINVAL, "n3dt_s3fd_pack: NULL argument");
    if (((size_t)packed) & 255) return fail(N3DT_EINVAL, "n3dt_s3fd_pack: packed must be 256-byte aligned");
    for (int b = 0; b < N3DT_S3FD_PARAMS; ++b)
        if (!p->weight[b] || !p->bias[b]) return fail(N3DT_EINVAL, "n3dt_s3fd_pack: NULL parameter pointer");
    for (int l = 0; l < 3; ++l)
        if (!p->norm_weight[l]) return fail(N3DT_EINVAL, "n3dt_s3fd_pack: NULL parameter pointer");
    n3dt_launch_s3fd_pack(p, packed, (hipStream_t)stream);
    return check_hip("n3dt_s3fd_pack");
}

extern "C" int n3dt_s3fd_max_images(int height, int width) {
    if (!s3_hw_ok(height, width)) {
        (void)fail(N3DT_EINVAL, "n3dt_s3fd_max_images: height and width must be in 32..4096");
        return 0;
    }
    return s3_max_images(height, width);
}

extern "C" int n3dt_s3fd_positions(int height, int width) {
    if (!s3_hw_ok(height, width)) {
        (void)fail(N3DT_EINVAL, "n3dt_s3fd_positions: height and width must be in 32..4096");
        return 0;
    }
    const S3Sizes s = s3_sizes(height, width);
    return s3_positions(&s, nullptr);
}

extern "C" size_t n3dt_s3fd_workspace_bytes(int n, int height, int width) {
    const char* what = s3fd_size(n, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_s3fd_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_s3fd_ws_bytes(n, height, width);
}

extern "C" int n3dt_s3fd_heads(int n, int height, int width, const void* packed, const float* x, float* const* out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_s3fd_heads";
    const char* what = s3fd_size(n, height, width);
    if (!what) {
        if (!packed || !x || !out || !workspace) what = "NULL pointer";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_s3fd_ws_bytes(n, height, width)) what = "workspace too small";
        else
            for (int i = 0; i < 12 && !what; ++i)
                if (!out[i] || (((size_t)out[i]) & 3)) what = "out[i] NULL or not 4-byte aligned";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_s3fd_heads(n, height, width, packed, x, out, workspace, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_s3fd_detect(int n, int height, int width, const void* packed, const float* frames, int max_faces, double* scores,
                                double* dets, int32_t* count, int32_t* left, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_s3fd_detect";
    const char* what = s3fd_size(n, height, width);
    if (!what) {
        if (max_faces < 1 || max_faces > S3_MAX_FACES) what = "max_faces outside 1..64";
        else if (!packed || !frames || !dets || !count || !left || !workspace) what = "NULL pointer";
        else if ((((size_t)dets) | ((size_t)scores)) & 7) what = "dets and scores must be 8-byte aligned";
        else if ((((size_t)frames) | ((size_t)count) | ((size_t)left)) & 3) what = "frames, count and left must be 4-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_s3fd_ws_bytes(n, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_s3fd_detect(n, height, width, packed, frames, max_faces, scores, dets, count, left, workspace, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_s3fd_boxes(int n_frames, int height, int width, int max_faces, const double* dets, const int32_t* count, int pady1,
                               int pady2, int padx1, int padx2, int smooth, int32_t* boxes, int32_t* found, int32_t* scratch, void* stream) {
    static const char* who = "n3dt_s3fd_boxes";
    const char* what = nullptr;
    const int lim = 1 << 20;
    if (n_frames < 1 || n_frames > S3_MAX_CLIP) what = "n_frames outside 1..2^20";
    else if (height < 2 || width < 2 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) what = "height and width must be in 2..4096";
    else if (max_faces < 1 || max_faces > S3_MAX_FACES) what = "max_faces outside 1..64";
    else if (smooth < 0 || smooth > S3_MAX_SMOOTH) what = "smooth outside 0..64";
    else if (pady1 < -lim || pady1 > lim || pady2 < -lim || pady2 > lim || padx1 < -lim || padx1 > lim || padx2 < -lim || padx2 > lim)
        what = "pads outside -2^20..2^20";
    else if (!dets || !count || !boxes || !found || !scratch) what = "NULL pointer";
    else if (((size_t)dets) & 7) what = "dets must be 8-byte aligned";
    else if ((((size_t)count) | ((size_t)boxes) | ((size_t)found) | ((size_t)scratch)) & 3) what = "count, boxes, found and scratch must be 4-byte aligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    const int pads[4] = {pady1, pady2, padx1, padx2};
    n3dt_launch_s3fd_boxes(n_frames, height, width, max_faces, dets, count, pads, smooth, boxes, found, scratch, (hipStream_t)stream);
    return check_hip(who);
}

// one block at a caller-given input size: the output must not be empty, and the maps stay inside the workspace budget
static const char* s3fd_block_size(int block, int n, int height, int width) {
    if (block < 0 || block >= S3_BLOCKS) return "block outside 0..32";
    if (n < 1 || n > S3_MAX_IMAGES) return "n outside 1..1024";
    if (height < 1 || width < 1 || height > CN_MAX_FRAME_HW + 4 || width > CN_MAX_FRAME_HW + 4) return "height and width must be in 1..4100";
    const bool pool = block >= S3_FIRST_POOL && block < S3_FIRST_NORM;
    if (pool && (height < 2 || width < 2)) return "a pool needs 2 x 2 pixels";
    if (n3dt_s3fd_block_ws_bytes(block, n, height, width) > S3_WS_BUDGET) return "the block's maps exceed the workspace budget";
    return nullptr;
}

extern "C" size_t n3dt_s3fd_block_workspace_bytes(int block, int n, int height, int width) {
    const char* what = s3fd_block_size(block, n, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_s3fd_block_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_s3fd_block_ws_bytes(block, n, height, width);
}

extern "C" int n3dt_s3fd_block(int block, int n, int height, int width, const void* packed, const float* in, float* out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_s3fd_block";
    const char* what = s3fd_block_size(block, n, height, width);
    if (!what) {
        if (!packed || !in || !out || !workspace) what = "NULL pointer";
        else if ((((size_t)in) | ((size_t)out)) & 3) what = "in and out must be 4-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_s3fd_block_ws_bytes(block, n, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_s3fd_block(block, n, height, width, packed, in, out, workspace, (hipStream_t)stream);
    return check_hip(who);
}

// The 3-D face reconstruction net (csrc/face_recon.hip): the limits of include/n3dt.h, checked before anything is enqueued
static const char* face_recon_size(int n, int height, int width) {
    if (!fr_hw_ok(height, width)) return "height and width must be in 32..4096";
    if (n < 1 || n > fr_max_images(height, width)) return "n outside 1..n3dt_face_recon_max_images (the workspace budget)";
    return nullptr;
}

extern "C" size_t n3dt_face_recon_packed_bytes(void) { return n3dt_face_recon_packed_layout_bytes(); }

extern "C" int n3dt_face_recon_pack(const N3dtFaceReconParams* p, void* packed, void* stream) {
    static const char* who = "n3dt_face_recon_pack";
    if (!p || !packed) return failf(N3DT_EINVAL, "%s: NULL argument", who);
    if (((size_t)packed) & 255) return failf(N3DT_EINVAL, "%s: packed must be 256-byte aligned", who);
    for (int j = 0; j < N3DT_FACE_RECON_CONVS; ++j) {
        if (!p->weight[j] || !p->bn_weight[j] || !p->bn_bias[j] || !p->bn_mean[j] || !p->bn_var[j])
            return failf(N3DT_EINVAL, "%s: NULL parameter pointer", who);
        if (!(p->bn_eps[j] > 0.0) || !(p->bn_eps[j] < 1.0)) return failf(N3DT_EINVAL, "%s: bn_eps outside (0, 1)", who);
    }
    for (int i = 0; i < N3DT_FACE_RECON_HEADS; ++i)
        if (!p->head_weight[i] || !p->head_bias[i]) return failf(N3DT_EINVAL, "%s: NULL parameter pointer", who);
    n3dt_launch_face_recon_pack(p, packed, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_face_recon_max_images(int height, int width) {
    if (!fr_hw_ok(height, width)) {
        (void)fail(N3DT_EINVAL, "n3dt_face_recon_max_images: height and width must be in 32..4096");
        return 0;
    }
    return fr_max_images(height, width);
}

extern "C" size_t n3dt_face_recon_workspace_bytes(int n, int height, int width) {
    const char* what = face_recon_size(n, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_face_recon_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_face_recon_ws_bytes(n, height, width);
}

extern "C" int n3dt_face_recon_fwd(int n, int height, int width, const void* packed, const float* x, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_face_recon_fwd";
    const char* what = face_recon_size(n, height, width);
    if (!what) {
        if (!packed || !x || !out || !workspace) what = "NULL pointer";
        else if ((((size_t)x) | ((size_t)out)) & 3) what = "x and out must be 4-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_face_recon_ws_bytes(n, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_face_recon_fwd(n, height, width, packed, x, out, workspace, (hipStream_t)stream);
    return check_hip(who);
}

// one block at a caller-given input size: the output must not be empty, and the maps stay inside the workspace budget
static const char* face_recon_block_size(int block, int n, int height, int width) {
    if (block < 0 || block >= FR_BLOCKS) return "block outside 0..55";
    if (n < 1 || n > FR_MAX_IMAGES) return "n outside 1..1024";
    if (height < 1 || width < 1 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) return "height and width must be in 1..4096";
    if (block == 0 && (height < 2 || width < 2)) return "the stem needs 2 x 2 pixels";
    if (block == FR_HEAD_BLOCK && (height != 1 || width != 1)) return "the head takes height = width = 1";
    if (n3dt_face_recon_block_ws_bytes(block, n, height, width) > FR_WS_BUDGET) return "the block's maps exceed the workspace budget";
    return nullptr;
}

extern "C" size_t n3dt_face_recon_block_workspace_bytes(int block, int n, int height, int width) {
    const char* what = face_recon_block_size(block, n, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_face_recon_block_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_face_recon_block_ws_bytes(block, n, height, width);
}

extern "C" int n3dt_face_recon_block(int block, int n, int height, int width, const void* packed, const float* in, const float* skip,
                                     float* out, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_face_recon_block";
    const char* what = face_recon_block_size(block, n, height, width);
    if (!what) {
        const bool third = block < FR_CONVS && fr_conv(block).role == FR_CONV3;
        if (!packed || !in || !out || !workspace) what = "NULL pointer";
        else if (third && !skip) what = "a bottleneck's third convolution takes the identity as skip";
        else if (!third && skip) what = "only a bottleneck's third convolution takes a skip";
        else if ((((size_t)in) | ((size_t)out) | ((size_t)skip)) & 3) what = "in, skip and out must be 4-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_face_recon_block_ws_bytes(block, n, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_face_recon_block(block, n, height, width, packed, in, skip, out, workspace, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_face_recon_align(int n, int height, int width, const float* frames, const double* landmarks, int points,
                                     const double* lm3d_std, const double* pinv, int quantize, float* crops, double* trans_params,
                                     int32_t* geom, int32_t* status, void* stream) {
    static const char* who = "n3dt_face_recon_align";
    const char* what = nullptr;
    if (n < 1 || n > (1 << 20)) what = "n outside 1..2^20";
    else if (height < 2 || width < 2 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) what = "height and width must be in 2..4096";
    else if (landmarks && points != 68 && points != 5) what = "points must be 68 or 5";
    else if (!frames || !lm3d_std || !pinv || !crops || !trans_params || !geom || !status) what = "NULL pointer";
    else if ((((size_t)landmarks) | ((size_t)lm3d_std) | ((size_t)pinv) | ((size_t)trans_params)) & 7)
        what = "landmarks, lm3d_std, pinv and trans_params must be 8-byte aligned";
    else if ((((size_t)frames) | ((size_t)crops) | ((size_t)geom) | ((size_t)status)) & 3) what = "frames, crops, geom and status must be 4-byte aligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_face_recon_align(n, height, width, frames, landmarks, points, lm3d_std, pinv, quantize ? 1 : 0, crops, trans_params, geom, status,
                                 (hipStream_t)stream);
    return check_hip(who);
}

// The AWing FAN landmark detector (csrc/fan.hip): the limits of include/n3dt.h, checked before anything is enqueued
static const char* fan_net(int modules, int N) {
    if (modules < 1 || modules > FAN_MAX_MODULES) return "num_modules outside 1..4";
    if (N < 1 || N > FAN_MAX_LANDMARKS) return "num_landmarks outside 1..127";
    return nullptr;
}

static int fan_max_images(int modules, int N) {
    const size_t one = n3dt_fan_ws_bytes(modules, N, 1);
    const size_t n = FAN_WS_BUDGET / one;
    return (int)(n > FAN_MAX_IMAGES ? FAN_MAX_IMAGES : n);
}

extern "C" size_t n3dt_fan_packed_bytes(int num_modules, int num_landmarks) {
    const char* what = fan_net(num_modules, num_landmarks);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_fan_packed_bytes: %s", what);
        return 0;
    }
    return n3dt_fan_packed_layout_bytes(num_modules, num_landmarks);
}

extern "C" int n3dt_fan_pack(const N3dtFanParams* p, void* packed, void* stream) {
    static const char* who = "n3dt_fan_pack";
    if (!p || !packed) return failf(N3DT_EINVAL, "%s: NULL argument", who);
    const char* what = fan_net(p->num_modules, p->num_landmarks);
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    if (((size_t)packed) & 255) return failf(N3DT_EINVAL, "%s: packed must be 256-byte aligned", who);
    if (!p->coords256 || !p->coords64) return failf(N3DT_EINVAL, "%s: NULL parameter pointer", who);
    for (int j = 0; j < fan_convs(p->num_modules); ++j) {
        if (!fan_conv_exists(j, p->num_modules)) continue;
        const FanConv c = fan_conv(j, p->num_landmarks);
        if (!p->weight[j] || (c.bias && !p->bias[j])) return failf(N3DT_EINVAL, "%s: NULL parameter pointer", who);
        if ((c.pre || c.post) && (!p->bn_weight[j] || !p->bn_bias[j] || !p->bn_mean[j] || !p->bn_var[j]))
            return failf(N3DT_EINVAL, "%s: NULL parameter pointer", who);
    }
    n3dt_launch_fan_pack(p, packed, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_fan_max_images(int num_modules, int num_landmarks) {
    const char* what = fan_net(num_modules, num_landmarks);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_fan_max_images: %s", what);
        return 0;
    }
    return fan_max_images(num_modules, num_landmarks);
}

static const char* fan_size(int modules, int N, int n) {
    const char* what = fan_net(modules, N);
    if (what) return what;
    if (n < 1 || n > fan_max_images(modules, N)) return "n outside 1..n3dt_fan_max_images (the workspace budget)";
    return nullptr;
}

extern "C" size_t n3dt_fan_workspace_bytes(int num_modules, int num_landmarks, int n) {
    const char* what = fan_size(num_modules, num_landmarks, n);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_fan_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_fan_ws_bytes(num_modules, num_landmarks, n);
}

extern "C" int n3dt_fan_fwd(int num_modules, int num_landmarks, int end_relu, int n, const void* packed, const float* x, int compute_gates,
                            uint8_t* gates, float* heat, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_fan_fwd";
    const char* what = fan_size(num_modules, num_landmarks, n);
    if (!what) {
        if (!packed || !x || !heat || !workspace || !gates) what = "NULL pointer";
        else if ((((size_t)x) | ((size_t)heat)) & 3) what = "x and heat must be 4-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_fan_ws_bytes(num_modules, num_landmarks, n)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_fan_fwd(num_modules, num_landmarks, end_relu ? 1 : 0, n, packed, x, compute_gates ? 1 : 0, gates, heat, workspace, (hipStream_t)stream);
    return check_hip(who);
}

static const char* fan_block_size(int block, int modules, int N, int n, int height, int width) {
    const char* what = fan_net(modules, N);
    if (what) return what;
    if (!fan_block_exists(block, modules)) return "no such block (the last stack has neither bl nor al)";
    if (n < 1 || n > FAN_MAX_IMAGES) return "n outside 1..1024";
    if (height < 1 || width < 1 || height > 1024 || width > 1024) return "height and width must be in 1..1024";
    const FanBlock k = fan_block(block, N);
    if (k.fixed_hw && (height != k.fixed_hw || width != k.fixed_hw)) return "a CoordConv takes its own geometry only (the stem 256 x 256, a stack's 64 x 64)";
    if (block == FAN_POOL_BLOCK && ((height | width) & 1)) return "the pool takes even sizes";
    if (n3dt_fan_block_ws_bytes(block, N, n, height, width) > FAN_WS_BUDGET) return "the block's maps exceed the workspace budget";
    return nullptr;
}

extern "C" size_t n3dt_fan_block_workspace_bytes(int block, int num_modules, int num_landmarks, int n, int height, int width) {
    const char* what = fan_block_size(block, num_modules, num_landmarks, n, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_fan_block_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_fan_block_ws_bytes(block, num_landmarks, n, height, width);
}

extern "C" int n3dt_fan_block(int block, int num_modules, int num_landmarks, int end_relu, int n, int height, int width, const void* packed,
                              const float* in, const float* skip, const uint8_t* gates, float* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
    static const char* who = "n3dt_fan_block";
    const char* what = fan_block_size(block, num_modules, num_landmarks, n, height, width);
    if (!what) {
        const FanBlock k = fan_block(block, num_landmarks);
        const bool gated = k.fixed_hw == FAN_HEAT && block >= FAN_FRONT_BLOCKS + FAN_STACK_BLOCKS;
        if (!packed || !in || !out || !workspace) what = "NULL pointer";
        else if (k.takes_skip && !skip) what = "this block takes a skip";
        else if (!k.takes_skip && skip) what = "this block takes no skip";
        else if (gated && !gates) what = "a coordconv behind the first stack takes gates";
        else if (!gated && gates) what = "this block takes no gates";
        else if ((((size_t)in) | ((size_t)out) | ((size_t)skip)) & 3) what = "in, skip and out must be 4-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_fan_block_ws_bytes(block, num_landmarks, n, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_fan_block(block, num_modules, num_landmarks, end_relu ? 1 : 0, n, height, width, packed, in, skip, gates, out, workspace,
                          (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_fan_crops(int n, int height, int width, const float* frames, const int32_t* boxes, float* out, void* stream) {
    static const char* who = "n3dt_fan_crops";
    const char* what = nullptr;
    if (n < 1 || n > (1 << 20)) what = "n outside 1..2^20";
    else if (height < 1 || width < 1 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) what = "height and width must be in 1..4096";
    else if (!frames || !boxes || !out) what = "NULL pointer";
    else if ((((size_t)frames) | ((size_t)boxes) | ((size_t)out)) & 3) what = "frames, boxes and out must be 4-byte aligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_fan_crops(n, height, width, frames, boxes, out, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_fan_points(int n, int num_landmarks, const float* heat, int64_t frame_stride, double* pts, int32_t* status, void* stream) {
    static const char* who = "n3dt_fan_points";
    const char* what = nullptr;
    if (n < 1 || n > (1 << 20)) what = "n outside 1..2^20";
    else if (num_landmarks < 1 || num_landmarks > FAN_MAX_LANDMARKS) what = "num_landmarks outside 1..127";
    else if (frame_stride < (int64_t)num_landmarks * FAN_CELLS) what = "frame_stride below num_landmarks * 4096";
    else if (!heat || !pts || !status) what = "NULL pointer";
    else if ((((size_t)heat) | ((size_t)status)) & 3 || ((size_t)pts) & 7) what = "heat and status must be 4-byte, pts 8-byte aligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_fan_points(n, num_landmarks, heat, frame_stride, pts, status, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_fan_tail(int n, int num_landmarks, int points_out, int height, int width, const double* pts, const int32_t* decode_status,
                             const int32_t* boxes, const int32_t* table, int carry, double* out, int32_t* status, void* stream) {
    static const char* who = "n3dt_fan_tail";
    const char* what = nullptr;
    if (n < 1 || n > (1 << 20)) what = "n outside 1..2^20";
    else if (num_landmarks < 1 || num_landmarks > FAN_MAX_LANDMARKS) what = "num_landmarks outside 1..127";
    else if (points_out < 1 || points_out > 1024 || (!table && points_out != num_landmarks)) what = "points_out outside 1..1024, or not num_landmarks without a table";
    else if (height < 1 || width < 1 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) what = "height and width must be in 1..4096";
    else if (!pts || !decode_status || !boxes || !out || !status) what = "NULL pointer";
    else if ((((size_t)pts) | ((size_t)out)) & 7) what = "pts and out must be 8-byte aligned";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_fan_tail(n, num_landmarks, points_out, height, width, pts, decode_status, boxes, table, carry ? 1 : 0, out, status, (hipStream_t)stream);
    return check_hip(who);
}

// The head-mask generator (csrc/head_mask.hip): the limits of include/n3dt.h, checked before anything is enqueued
static const char* head_mask_size(int n, int height, int width) {
    if (!hm_hw_ok(height, width)) return "height and width must be in 32..4096";
    if (n < 1 || n > hm_max_images(height, width)) return "n outside 1..n3dt_head_mask_max_images (the workspace budget)";
    return nullptr;
}

static const char* head_mask_pixels(int n, int height, int width) {
    if (height < 1 || width < 1 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) return "height and width must be in 1..4096";
    if (n < 1 || (size_t)n * height * width > ((size_t)1 << 30)) return "n outside 1..2^30 / (height width)";
    return nullptr;
}

extern "C" size_t n3dt_head_mask_packed_bytes(void) { return n3dt_head_mask_packed_layout_bytes(); }

extern "C" int n3dt_head_mask_pack(const N3dtHeadMaskParams* p, void* packed, void* stream) {
    static const char* who = "n3dt_head_mask_pack";
    if (!p || !packed) return failf(N3DT_EINVAL, "%s: NULL argument", who);
    if (((size_t)packed) & 255) return failf(N3DT_EINVAL, "%s: packed must be 256-byte aligned", who);
    if (p->n_classes < 1 || p->n_classes > HM_MAX_CLASSES) return failf(N3DT_EINVAL, "%s: n_classes outside 1..32", who);
    if (!(p->bn_eps > 0.0) || !(p->bn_eps < 1.0)) return failf(N3DT_EINVAL, "%s: bn_eps outside (0, 1)", who);
    for (int j = 0; j < HM_CONVS; ++j) {
        if (!p->weight[j]) return failf(N3DT_EINVAL, "%s: NULL parameter pointer", who);
        if (HM_TABLE[j].bn && (!p->bn_weight[j] || !p->bn_bias[j] || !p->bn_mean[j] || !p->bn_var[j]))
            return failf(N3DT_EINVAL, "%s: NULL parameter pointer", who);
    }
    n3dt_launch_head_mask_pack(p, packed, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_head_mask_max_images(int height, int width) {
    if (!hm_hw_ok(height, width)) {
        (void)fail(N3DT_EINVAL, "n3dt_head_mask_max_images: height and width must be in 32..4096");
        return 0;
    }
    return hm_max_images(height, width);
}

extern "C" size_t n3dt_head_mask_workspace_bytes(int n, int height, int width) {
    const char* what = head_mask_size(n, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_head_mask_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_head_mask_ws_bytes(n, height, width);
}

extern "C" int n3dt_head_mask_fwd(int n, int height, int width, int n_classes, const void* packed, const float* x, int outputs, int upsample,
                                  float* out, float* out16, float* out32, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_head_mask_fwd";
    const char* what = head_mask_size(n, height, width);
    float* outs[3] = {out, out16, out32};
    if (!what) {
        if (n_classes < 1 || n_classes > HM_MAX_CLASSES) what = "n_classes outside 1..32";
        else if (outputs < 1 || outputs > 7) what = "outputs must be a non-empty set of bits 1, 2, 4";
        else if (!packed || !x || !workspace) what = "NULL pointer";
        else if (((outputs & 1) && !out) || ((outputs & 2) && !out16) || ((outputs & 4) && !out32)) what = "a selected output is NULL";
        else if ((((size_t)x) | ((size_t)out) | ((size_t)out16) | ((size_t)out32)) & 3) what = "x and the outputs must be 4-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_head_mask_ws_bytes(n, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_head_mask_fwd(n, height, width, n_classes, packed, x, outputs, upsample ? 1 : 0, outs, workspace, (hipStream_t)stream);
    return check_hip(who);
}

// one block at a caller-given geometry: the output must not be empty, and the maps stay inside the workspace budget
static const char* head_mask_block_size(int block, int n, int height, int width, int src_height, int src_width) {
    if (block < 0 || block >= HM_BLOCKS) return "block outside 0..36";
    if (n < 1 || n > HM_MAX_IMAGES) return "n outside 1..1024";
    if (height < 1 || width < 1 || height > CN_MAX_FRAME_HW || width > CN_MAX_FRAME_HW) return "height and width must be in 1..4096";
    if (src_height < 1 || src_width < 1 || src_height > height || src_width > width) return "src_height and src_width must be in 1..height, 1..width";
    const bool resamples = block == HM_HEAD32 || block == HM_HEAD16;
    if (!resamples && (src_height != height || src_width != width)) return "only blocks 24 and 25 read through the nearest upsample";
    if (block == 0 && (height < 2 || width < 2)) return "the stem needs 2 x 2 pixels";
    if (n3dt_head_mask_block_ws_bytes(block, n, height, width, src_height, src_width) > HM_WS_BUDGET) return "the block's maps exceed the workspace budget";
    return nullptr;
}

extern "C" size_t n3dt_head_mask_block_workspace_bytes(int block, int n, int height, int width, int src_height, int src_width) {
    const char* what = head_mask_block_size(block, n, height, width, src_height, src_width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_head_mask_block_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_head_mask_block_ws_bytes(block, n, height, width, src_height, src_width);
}

extern "C" int n3dt_head_mask_block(int block, int n, int height, int width, int src_height, int src_width, int n_classes, const void* packed,
                                    const float* in, const float* aux, const float* scale, const float* addvec, float* out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    static const char* who = "n3dt_head_mask_block";
    const char* what = head_mask_block_size(block, n, height, width, src_height, src_width);
    if (!what) {
        const bool conv = block < HM_CONVS;
        const bool needs_aux = conv && (hm_takes_skip(block) || block == HM_FFM_BLK);
        const bool may_aux = needs_aux || (block == HM_HEAD16 && scale);
        const bool may_scale = block == HM_HEAD32 || block == HM_HEAD16 || block == HM_OUT;
        if (n_classes < 1 || n_classes > HM_MAX_CLASSES) what = "n_classes outside 1..32";
        else if (!packed || !in || !out || !workspace) what = "NULL pointer";
        else if (needs_aux && !aux) what = "this block takes aux (a shortcut, or the second half of the channels)";
        else if (!may_aux && aux) what = "this block takes no aux";
        else if (!may_scale && (scale || addvec)) what = "only blocks 24, 25 and 30 take a scale";
        else if (addvec && !scale) what = "addvec needs a scale";
        else if (addvec && (aux || block == HM_OUT)) what = "one added term at most";
        else if ((((size_t)in) | ((size_t)out) | ((size_t)aux)) & 3) what = "in, aux and out must be 4-byte aligned";
        else if ((((size_t)scale) | ((size_t)addvec)) & 15) what = "scale and addvec must be 16-byte aligned";
        else if ((((size_t)packed) | ((size_t)workspace)) & 255) what = "packed and the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_head_mask_block_ws_bytes(block, n, height, width, src_height, src_width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_head_mask_block(block, n, height, width, src_height, src_width, n_classes, packed, in, aux, scale, addvec, out, workspace,
                                (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_head_mask_frames(int n, int height, int width, const void* frames, int frames_are_float, uint8_t* rgb, float* x, void* stream) {
    static const char* who = "n3dt_head_mask_frames";
    const char* what = head_mask_pixels(n, height, width);
    if (!what) {
        if (!frames || !rgb || !x) what = "NULL pointer";
        else if ((((size_t)x) | (frames_are_float ? (size_t)frames : 0)) & 3) what = "x and float frames must be 4-byte aligned";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_head_mask_frames(n, height, width, frames, frames_are_float ? 1 : 0, rgb, x, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_head_mask_resize(int n, int src_height, int src_width, int channels, const uint8_t* src, int height, int width, uint8_t* dst,
                                     void* stream) {
    static const char* who = "n3dt_head_mask_resize";
    const char* what = head_mask_pixels(n, height, width);
    if (!what) what = head_mask_pixels(n, src_height, src_width);
    if (!what) {
        if (channels < 1 || channels > 4) what = "channels outside 1..4";
        else if (!src || !dst) what = "NULL pointer";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_head_mask_resize(n, src_height, src_width, channels, src, height, width, dst, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_head_mask_labels(int n, int n_classes, int h, int w, int height, int width, const float* logits, uint8_t* labels, void* stream) {
    static const char* who = "n3dt_head_mask_labels";
    const char* what = head_mask_pixels(n, height, width);
    if (!what) {
        if (n_classes < 1 || n_classes > 256) what = "n_classes outside 1..256";
        else if (h < 1 || w < 1 || h > CN_MAX_FRAME_HW || w > CN_MAX_FRAME_HW) what = "h and w must be in 1..4096";
        else if (!logits || !labels) what = "NULL pointer";
        else if (((size_t)logits) & 3) what = "logits must be 4-byte aligned";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_head_mask_labels(n, n_classes, h, w, height, width, logits, labels, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_head_mask_green(int n, int height, int width, const uint8_t* rgb, int hue_lo, int hue_hi, uint8_t* cleared, void* stream) {
    static const char* who = "n3dt_head_mask_green";
    const char* what = head_mask_pixels(n, height, width);
    if (!what && (!rgb || !cleared)) what = "NULL pointer";
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_head_mask_green(n, height, width, rgb, hue_lo, hue_hi, cleared, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" size_t n3dt_head_mask_postprocess_workspace_bytes(int n, int height, int width) {
    const char* what = head_mask_pixels(n, height, width);
    if (what) {
        (void)failf(N3DT_EINVAL, "n3dt_head_mask_postprocess_workspace_bytes: %s", what);
        return 0;
    }
    return n3dt_head_mask_post_ws_bytes(n, height, width);
}

extern "C" int n3dt_head_mask_postprocess(int n, int height, int width, const uint8_t* labels, const uint8_t* rgb, const uint8_t* lut,
                                          const uint8_t* element, int elem_h, int elem_w, int anchor_y, int anchor_x, int dilations, int erosions,
                                          int hue_lo, int hue_hi, uint8_t* head, uint8_t* eye, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    static const char* who = "n3dt_head_mask_postprocess";
    const char* what = head_mask_pixels(n, height, width);
    if (!what) {
        if (!labels || !rgb || !lut || !element || !head || !eye || !workspace) what = "NULL pointer";
        else if (elem_h < 1 || elem_w < 1 || elem_h > HM_MAX_ELEMENT || elem_w > HM_MAX_ELEMENT) what = "the element must be 1..64 high and wide";
        else if (anchor_y < 0 || anchor_y >= elem_h || anchor_x < 0 || anchor_x >= elem_w) what = "the anchor lies outside the element";
        else if (dilations < 0 || dilations > 64 || erosions < 0 || erosions > 1024) what = "dilations outside 0..64 or erosions outside 0..1024";
        else if (((size_t)workspace) & 255) what = "the workspace must be 256-byte aligned";
        else if (workspace_bytes < n3dt_head_mask_post_ws_bytes(n, height, width)) what = "workspace too small";
    }
    if (what) return failf(N3DT_EINVAL, "%s: %s", who, what);
    n3dt_launch_head_mask_postprocess(n, height, width, labels, rgb, lut, element, elem_h, elem_w, anchor_y, anchor_x, dilations, erosions, hue_lo, hue_hi,
                                      head, eye, workspace, (hipStream_t)stream);
    return check_hip(who);
}

extern "C" int n3dt_chw_to_hwc(int C, int n, const float* src, float* dst, void* stream) {
    if (C < 1 || n < 1 || !src || !dst) return fail(N3DT_EINVAL, "n3dt_chw_to_hwc: bad argument");
    n3dt_launch_chw_to_hwc(C, n, src, dst, (hipStream_t)stream);
    return check_hip("n3dt_chw_to_hwc");
}

// ---- training path -----------------------------------------------------------------------------
static int check_train_geom(const N3dtGeom* g) {
    int rc = check_geom(g, N3DT_F32);
    if (rc) return rc;
    if ((size_t)g->batch * g->n_rays * g->n_samples > (size_t)1 << 30) return fail(N3DT_EINVAL, "training path: more than 2^30 sample points");
    return N3DT_OK;
}

// one size serves both training precisions (the fp32 layered path and the fused bf16 path lay the buffers out differently)
static inline size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }
extern "C" size_t n3dt_render_train_saved_bytes(const N3dtGeom* g) {
    if (check_train_geom(g) != N3DT_OK) return 0;
    return max_sz(n3dt_train_saved_floats(g) * sizeof(float), n3dt_train16_saved_bytes(g));
}
extern "C" size_t n3dt_render_train_workspace_bytes(const N3dtGeom* g) {
    if (check_train_geom(g) != N3DT_OK) return 0;
    return max_sz(n3dt_train_ws_floats(g) * sizeof(float), n3dt_train16_ws_bytes(g));
}

extern "C" int n3dt_render_train_fwd(const N3dtGeom* g, int precision, const void* packed_mlp, const N3dtMlpParams* p, const float* xy, const float* R,
                                     const float* T, const float* Kinv, const float* shape, const float* appea, const float* audio,
                                     const float* t_rand, const float* bg_featmap, const float* ray_bias, float* fg_feat, float* bg_alpha,
                                     float* depth, float* merge_feat, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    int rc = check_train_geom(g);
    if (rc) return rc;
    if ((rc = check_ray_bias(g, ray_bias, "n3dt_render_train_fwd")) != N3DT_OK) return rc;
    if (precision != N3DT_F32 && precision != N3DT_BF16) return fail(N3DT_EINVAL, "training precision must be N3DT_F32 or N3DT_BF16");
    if (!packed_mlp || !p || !xy || !R || !T || !Kinv || !shape || !appea || !fg_feat || !saved || !workspace)
        return fail(N3DT_EINVAL, "n3dt_render_train_fwd: NULL argument");
    if (g->audio_dim > 0 && !audio) return fail(N3DT_EINVAL, "n3dt_render_train_fwd: audio is NULL but audio_dim > 0");
    if (merge_feat && !bg_featmap) return fail(N3DT_EINVAL, "n3dt_render_train_fwd: merge_feat needs bg_featmap");
    if (saved_bytes < n3dt_render_train_saved_bytes(g)) return fail(N3DT_EWORKSPACE, "n3dt_render_train_fwd: saved buffer too small");
    if (workspace_bytes < n3dt_render_train_workspace_bytes(g)) return fail(N3DT_EWORKSPACE, "n3dt_render_train_fwd: workspace too small");
    // `packed_mlp` is the n3dt_mlp_pack buffer of the SAME precision: the fused bf16 path streams its bf16 matrices,
    // the fp32 path only reads the fp32 tail (W2^T, b2) behind them
    const float* tail = (const float*)((const unsigned char*)packed_mlp + n3dt_packed_tail_offset(precision));
    if (precision == N3DT_BF16) {
        n3dt_launch_train16_fwd(g, p, packed_mlp, tail, xy, R, T, Kinv, shape, appea, audio, t_rand, bg_featmap, fg_feat, bg_alpha, depth,
                                merge_feat, saved, workspace, ray_bias, (hipStream_t)stream);
        return check_hip("n3dt_render_train_fwd");
    }
    n3dt_launch_train_fwd(g, p, tail, xy, R, T, Kinv, shape, appea, audio, t_rand, bg_featmap, fg_feat, bg_alpha, depth, merge_feat,
                          (float*)saved, (float*)workspace, ray_bias, (hipStream_t)stream);
    return check_hip("n3dt_render_train_fwd");
}

extern "C" int n3dt_render_bwd_cam(const N3dtGeom* g, int precision, const N3dtMlpParams* p, const N3dtMlpGrads* grads, const float* shape,
                                   const float* appea, const float* audio, const float* bg_featmap, const float* d_merge_feat,
                                   const float* d_fg_feat, const float* d_bg_alpha, const void* saved, size_t saved_bytes,
                                   float* d_bg_featmap, float* d_shape, float* d_appea, float* d_audio, float* d_ray_bias, const float* xy,
                                   const float* R, const float* T, const float* Kinv, const float* t_rand, float* d_R, float* d_T,
                                   float* d_Kinv, float* d_xy, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_train_geom(g);
    if (rc) return rc;
    if ((rc = check_ray_bias(g, d_ray_bias, "n3dt_render_bwd_cam")) != N3DT_OK) return rc;
    if (precision != N3DT_F32 && precision != N3DT_BF16) return fail(N3DT_EINVAL, "training precision must be N3DT_F32 or N3DT_BF16");
    if (!p || !shape || !appea || !saved || !workspace) return fail(N3DT_EINVAL, "n3dt_render_bwd_cam: NULL argument");
    if (!d_merge_feat && !d_fg_feat && !d_bg_alpha) return fail(N3DT_EINVAL, "n3dt_render_bwd_cam: no incoming gradient");
    if (d_merge_feat && !bg_featmap) return fail(N3DT_EINVAL, "n3dt_render_bwd_cam: d_merge_feat needs bg_featmap");
    if (g->audio_dim > 0 && !audio) return fail(N3DT_EINVAL, "n3dt_render_bwd_cam: audio is NULL but audio_dim > 0");
    // grads == NULL: the network is frozen (single-image fitting) -- no parameter gradient is computed, only d codes / d cameras
    if (grads)
        for (int l = 0; l < N3DT_MLP_LAYERS; ++l)
            if (!grads->weight[l] || !grads->bias[l]) return fail(N3DT_EINVAL, "n3dt_render_bwd_cam: NULL gradient pointer");
    if (!grads && d_bg_featmap) return fail(N3DT_EINVAL, "n3dt_render_bwd_cam: grads == NULL (frozen network) but d_bg_featmap given");
    if (saved_bytes < n3dt_render_train_saved_bytes(g)) return fail(N3DT_EWORKSPACE, "n3dt_render_bwd_cam: saved buffer too small");
    if (workspace_bytes < n3dt_render_train_workspace_bytes(g)) return fail(N3DT_EWORKSPACE, "n3dt_render_bwd_cam: workspace too small");
    if ((d_R || d_T || d_Kinv || d_xy) && (!xy || !R || !T || !Kinv))
        return fail(N3DT_EINVAL, "n3dt_render_bwd_cam: camera gradients need xy, R, T, Kinv");
    if (precision == N3DT_BF16) {
        n3dt_launch_train16_bwd(g, p, grads, shape, appea, audio, bg_featmap, d_merge_feat, d_fg_feat, d_bg_alpha, saved, d_bg_featmap,
                                d_shape, d_appea, d_audio, xy, R, T, Kinv, t_rand, d_R, d_T, d_Kinv, d_xy, workspace, d_ray_bias, (hipStream_t)stream);
        return check_hip("n3dt_render_bwd_cam");
    }
    n3dt_launch_train_bwd(g, p, grads, shape, appea, audio, bg_featmap, d_merge_feat, d_fg_feat, d_bg_alpha, (const float*)saved,
                          d_bg_featmap, d_shape, d_appea, d_audio, xy, R, T, Kinv, t_rand, d_R, d_T, d_Kinv, d_xy, (float*)workspace, d_ray_bias,
                          (hipStream_t)stream);
    return check_hip("n3dt_render_bwd_cam");
}

// the entry point of ABI 5 as it was: no gradient to the intrinsics or the ray coordinates
extern "C" int n3dt_render_bwd(const N3dtGeom* g, int precision, const N3dtMlpParams* p, const N3dtMlpGrads* grads, const float* shape,
                               const float* appea, const float* audio, const float* bg_featmap, const float* d_merge_feat,
                               const float* d_fg_feat, const float* d_bg_alpha, const void* saved, size_t saved_bytes,
                               float* d_bg_featmap, float* d_shape, float* d_appea, float* d_audio, float* d_ray_bias, const float* xy,
                               const float* R, const float* T, const float* Kinv, const float* t_rand, float* d_R, float* d_T, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return n3dt_render_bwd_cam(g, precision, p, grads, shape, appea, audio, bg_featmap, d_merge_feat, d_fg_feat, d_bg_alpha, saved, saved_bytes,
                               d_bg_featmap, d_shape, d_appea, d_audio, d_ray_bias, xy, R, T, Kinv, t_rand, d_R, d_T, nullptr, nullptr,
                               workspace, workspace_bytes, stream);
}

static int check_nr(const N3dtGeom* g, int nb) {
    if (!g) return fail(N3DT_EINVAL, "geometry is NULL");
    if (nb < 1) return fail(N3DT_EINVAL, "nb < 1");
    if (g->n_blocks < 1 || g->n_blocks > N3DT_MAX_BLOCKS) return fail(N3DT_EINVAL, "n_blocks must be in 1..8");
    if (g->feat_nc != 256) return fail(N3DT_EINVAL, "only featmap_nc == 256 is built");
    if (g->featmap_size < 2) return fail(N3DT_EINVAL, "featmap_size < 2 (reflect border needs 2 pixels)");
    return N3DT_OK;
}

extern "C" size_t n3dt_neural_render_train_saved_bytes(const N3dtGeom* g, int nb) {
    if (check_nr(g, nb) != N3DT_OK) return 0;
    return n3dt_nr_train_saved_floats(g, nb) * sizeof(float);
}
extern "C" size_t n3dt_neural_render_train_workspace_bytes(const N3dtGeom* g, int nb) {
    if (check_nr(g, nb) != N3DT_OK) return 0;
    return n3dt_nr_train_ws_floats(g, nb) * sizeof(float);
}

extern "C" int n3dt_neural_render_train_fwd(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap, float* img,
                                            void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_nr(g, nb);
    if (rc) return rc;
    if (!p || !featmap || !img || !saved || !workspace) return fail(N3DT_EINVAL, "n3dt_neural_render_train_fwd: NULL argument");
    if (saved_bytes < n3dt_neural_render_train_saved_bytes(g, nb)) return fail(N3DT_EWORKSPACE, "neural render saved buffer too small");
    if (workspace_bytes < n3dt_neural_render_train_workspace_bytes(g, nb)) return fail(N3DT_EWORKSPACE, "neural render workspace too small");
    n3dt_launch_nr_train_fwd(g, nb, p, featmap, img, (float*)saved, (float*)workspace, precision == N3DT_BF16, (hipStream_t)stream);
    return check_hip("n3dt_neural_render_train_fwd");
}

extern "C" int n3dt_neural_render_bwd(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const N3dtRenderGrads* grads,
                                      const float* featmap, const float* d_img, const void* saved, size_t saved_bytes, float* d_featmap,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_nr(g, nb);
    if (rc) return rc;
    if (!p || !featmap || !d_img || !saved || !d_featmap || !workspace)  // (grads == NULL: frozen renderer, only d_featmap is wanted)
        return fail(N3DT_EINVAL, "n3dt_neural_render_bwd: NULL argument");
    if (saved_bytes < n3dt_neural_render_train_saved_bytes(g, nb)) return fail(N3DT_EWORKSPACE, "neural render saved buffer too small");
    if (workspace_bytes < n3dt_neural_render_train_workspace_bytes(g, nb)) return fail(N3DT_EWORKSPACE, "neural render workspace too small");
    n3dt_launch_nr_bwd(g, nb, p, grads, featmap, d_img, (const float*)saved, d_featmap, (float*)workspace, precision == N3DT_BF16, (hipStream_t)stream);
    return check_hip("n3dt_neural_render_bwd");
}

extern "C" int n3dt_img_to_uint8(int n_images, int pixels, const float* img, unsigned char* out, void* stream) {
    if (n_images < 1 || pixels < 1 || !img || !out) return fail(N3DT_EINVAL, "n3dt_img_to_uint8: bad argument");
    n3dt_launch_img_to_uint8(n_images, pixels, img, out, (hipStream_t)stream);
    return check_hip("n3dt_img_to_uint8");
}

extern "C" int n3dt_loss_fwd(int batch, int pixels, const float* merge_img, const float* bg_img, const float* gt, const float* mask,
                             float bg_value, float* acc, float* terms, void* stream) {
    if (batch < 1 || pixels < 1 || !merge_img || !bg_img || !gt || !mask || !acc || !terms) return fail(N3DT_EINVAL, "n3dt_loss_fwd: bad argument");
    n3dt_launch_loss_fwd(batch, pixels, merge_img, bg_img, gt, mask, bg_value, acc, terms, (hipStream_t)stream);
    return check_hip("n3dt_loss_fwd");
}

extern "C" int n3dt_loss_bwd(int batch, int pixels, const float* merge_img, const float* bg_img, const float* gt, const float* mask,
                             float bg_value, const float* acc, const float* g, const float* g_total, float* d_merge, float* d_bg, void* stream) {
    if (batch < 1 || pixels < 1 || !merge_img || !bg_img || !gt || !mask || !acc || (!g && !g_total) || !d_merge || !d_bg)
        return fail(N3DT_EINVAL, "n3dt_loss_bwd: bad argument");
    n3dt_launch_loss_bwd(batch, pixels, merge_img, bg_img, gt, mask, bg_value, acc, g, g_total, d_merge, d_bg, (hipStream_t)stream);
    return check_hip("n3dt_loss_bwd");
}

// ---- input staging + hipGraph replay (see n3dt.h) -------------------------------------------------------------
extern "C" int n3dt_stage_inputs(const N3dtStageCopy* st, void* stream) {
    if (!st || st->n < 1 || st->n > N3DT_STAGE_MAX) return fail(N3DT_EINVAL, "n3dt_stage_inputs: bad entry count");
    for (int i = 0; i < st->n; ++i)
        if (!st->src[i] || !st->dst[i] || st->count[i] < 1) return fail(N3DT_EINVAL, "n3dt_stage_inputs: NULL pointer or empty entry");
    if (st->view_dims[0] > 0) {
        if (st->view_dims[1] < 1 || st->view_dims[2] < 1 || st->view_dims[0] * st->view_dims[1] * st->view_dims[2] != st->count[0])
            return fail(N3DT_EINVAL, "n3dt_stage_inputs: view_dims do not multiply to count[0]");
        for (int d = 0; d < 3; ++d)
            if (st->view_strides[d] < 0) return fail(N3DT_EINVAL, "n3dt_stage_inputs: negative stride");
    }
    n3dt_launch_stage(st, (hipStream_t)stream);
    return check_hip("n3dt_stage_inputs");
}

struct N3dtGraph {
    hipGraph_t graph;
    hipGraphExec_t exec;
};

extern "C" int n3dt_graph_begin(void* stream) {
    (void)hipGetLastError();
    if (hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        return fail(N3DT_EHIP, "n3dt_graph_begin: hipStreamBeginCapture failed (the legacy NULL stream cannot be captured)");
    }
    return N3DT_OK;
}

extern "C" int n3dt_graph_end(void* stream, void** graph_out) {
    if (!graph_out) return fail(N3DT_EINVAL, "n3dt_graph_end: NULL argument");
    *graph_out = nullptr;
    hipGraph_t graph = nullptr;
    if (hipStreamEndCapture((hipStream_t)stream, &graph) != hipSuccess || !graph) {
        (void)hipGetLastError();
        return fail(N3DT_EHIP, "n3dt_graph_end: hipStreamEndCapture failed (a call inside the capture was not capturable)");
    }
    hipGraphExec_t exec = nullptr;
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipGraphDestroy(graph);
        return fail(N3DT_EHIP, "n3dt_graph_end: hipGraphInstantiate failed");
    }
    *graph_out = new N3dtGraph{graph, exec};
    return N3DT_OK;
}

extern "C" int n3dt_graph_launch(void* graph, void* stream) {
    if (!graph) return fail(N3DT_EINVAL, "n3dt_graph_launch: NULL graph");
    if (hipGraphLaunch(((N3dtGraph*)graph)->exec, (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(N3DT_EHIP, "n3dt_graph_launch: hipGraphLaunch failed");
    }
    return N3DT_OK;
}

extern "C" int n3dt_graph_destroy(void* graph) {
    if (!graph) return N3DT_OK;
    N3dtGraph* g = (N3dtGraph*)graph;
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
    return N3DT_OK;
}
