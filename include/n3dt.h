/*
 * n3dt.h -- C ABI of libn3dt.so: the MI355X (gfx950) head-render hot path of NeRF-3DTalker.
 *
 * The reference has no FFI/operator seam for this path: the boundary is the Python module
 * HeadNeRFNet (reference: NetWorks/HeadNeRFNet.py:10-207).  These entry points are what a
 * binding for that module calls underneath; each one names the reference code it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch/ATen types.
 *   - every data pointer is a DEVICE pointer (hipMalloc'd or torch-owned); all memory is
 *     caller-owned, nothing is allocated or freed inside a call (hipGraph-capturable).
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); calls are
 *     stream-ordered, asynchronous and re-entrant (no global mutable state).
 *   - return 0 on success, a negative N3DT_E* code otherwise; never throws, never exits.
 *     n3dt_last_error() returns a thread-local message for the last failing call.
 *   - tensors are fp32 and contiguous unless a stride is given.  Feature maps cross this ABI
 *     ray-major ("NHWC"): [B, N_r, C]; images are planar [B, 3, P, P] like the reference.
 */
#ifndef N3DT_API_H_
#define N3DT_API_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define N3DT_ABI_VERSION 5

/* arithmetic type of the MLP contraction */
#define N3DT_F32 0  /* v_mfma_f32_16x16x4_f32, exact fp32: the <=1e-3 RGB parity mode */
#define N3DT_BF16 1 /* v_mfma_f32_32x32x16_bf16, fp32 accumulate: the roofline mode  */
#define N3DT_F16 2  /* v_mfma_f32_32x32x16_f16,  fp32 accumulate                      */
/* bf16 MFMA with every operand split hi + lo (x = bf16(x) + bf16(x - bf16(x)), three products per product, ~16 mantissa bits):
 * the parity-grade mode on the matrix pipe -- holds the 1e-3 RGB gate on sharp networks where single bf16 / fp16 operands do
 * not, at a third of the bf16 rate.  Render calls only (n3dt_mlp_pack, n3dt_render_fwd,
 * n3dt_neural_render_fwd, where the 2-D renderer then runs its fp16 path); the training entry points take F32 or BF16. */
#define N3DT_BF16X3 3

#define N3DT_OK 0
#define N3DT_EINVAL (-1)    /* bad geometry / null pointer / unsupported size */
#define N3DT_EWORKSPACE (-2) /* workspace too small */
#define N3DT_EHIP (-3)      /* a HIP runtime call failed */

#define N3DT_PE_DIM 63      /* 3 + 6*10 (reference: NetWorks/HeadNeRFNet.py:27-28,50) */
#define N3DT_MLP_LAYERS 12  /* FeaExt_module_0..7, density_module, RGB_layer_0..2 */

/* Geometry of one call.  Mirrors what HeadNeRFNet reads from `opt` and from the input shapes
 * (reference: NetWorks/HeadNeRFNet.py:22-45,131; HeadNeRFOptions.py:5-34). */
typedef struct N3dtGeom {
    int32_t batch;        /* B frames */
    int32_t n_rays;       /* N_r rays per frame (featmap_size^2 for the reference reading) */
    int32_t n_samples;    /* N_s = opt.num_sample_coarse */
    int32_t hidden;       /* opt.mlp_hidden_nchannels; this build supports 384 */
    int32_t feat_nc;      /* opt.featmap_nc (C); this build supports 256 */
    int32_t shape_dim;    /* iden+expr(+gaze) code width, 179 (+eye_gaze_dim) */
    int32_t appea_dim;    /* text+illu code width, 127 */
    int32_t audio_dim;    /* 64, or 0 for the audio-less *_yuan variant */
    int32_t featmap_size; /* fs; n_rays == fs*fs whenever the neural renderer follows */
    int32_t n_blocks;     /* log2(pred_img_size / featmap_size) */
    float world_z1;       /* opt.world_z1 (2.5)  */
    float world_z2;       /* opt.world_z2 (-3.5) */
    /* element strides of batch_xy [B,2,N_r]; the trainer passes an expand()ed view
     * (reference: talker_trainer.py:768), so stride_b may be 0 */
    int64_t xy_stride_b, xy_stride_c, xy_stride_r;
    /* 0: the N_s+1 sample planes of a ray are the reference's linspace between world_z1 / world_z2 (jittered by
     * `t_rand` in train mode, NetWorks/utils.py:118-145);  1: the `t_rand` argument of the render calls carries the
     * planes themselves, [B,N_r,N_s+1] ascending camera-relative z (the hierarchical pass, utils.py:173-208) */
    int32_t z_planes_given;
    /* 0: `bg_featmap` arguments are the parameter as PyTorch holds it, [C][N_r] (neural_renderer.py:31-46) and the render call
     * transposes it; 1: the caller passes it already ray-major [N_r][C] (e.g. cached per parameter version): no transposition */
    int32_t bg_is_hwc;
    /* include_vd (ABI 5; reference: NetWorks/HeadNeRFNet.py:56-63,86,141-142).  0: RGB_layer_1's input is [RGB_layer_0 out |
     * appea_code], as every caller of the reference builds it.  27 (= 3 + 6 * vd_n_freqs): it is [RGB_layer_0 out | Embedder_4(ray
     * direction) | appea_code].  The direction is constant along a ray, so those 27 columns collapse into a PER-RAY bias of the
     * layer -- the render calls then take it as `ray_bias` [B, N_r, 192] (n3dt_ray_vd_bias computes it) and `weight[10]` is the
     * layer WITHOUT its 27 view-direction columns, [192, 384 + appea_dim] contiguous. */
    int32_t vd_dim;
} N3dtGeom;

/* The MLP's fp32 parameters as PyTorch owns them: weight[l] is [out_l, in_l] row-major
 * (Conv2d 1x1 weight viewed 2-D), bias[l] is [out_l]; order FeaExt_module_0..7, density_module,
 * RGB_layer_0, RGB_layer_1, RGB_layer_2 (reference: NetWorks/models.py:29-59). */
typedef struct N3dtMlpParams {
    const float* weight[N3DT_MLP_LAYERS];
    const float* bias[N3DT_MLP_LAYERS];
} N3dtMlpParams;

/* Neural-renderer parameters (reference: NetWorks/neural_renderer.py:49-69,
 * NetWorks/PixelShuffleUpsample.py:29-33).  Index i = block, 0 <= i < n_blocks (<= 8). */
#define N3DT_MAX_BLOCKS 8
typedef struct N3dtRenderParams {
    const float* to_rgb_w[N3DT_MAX_BLOCKS + 1]; /* feat_2_rgb_list.{0..n}: [3, c_i] */
    const float* to_rgb_b[N3DT_MAX_BLOCKS + 1];
    const float* psu1_w[N3DT_MAX_BLOCKS];       /* feat_upsample_list.i.layer_1: [2c, c]  */
    const float* psu1_b[N3DT_MAX_BLOCKS];
    const float* psu2_w[N3DT_MAX_BLOCKS];       /* feat_upsample_list.i.layer_2: [4c, 2c] */
    const float* psu2_b[N3DT_MAX_BLOCKS];
    const float* feat_w[N3DT_MAX_BLOCKS];       /* feat_layers.i: [c_{i+1}, c_i] */
    const float* feat_b[N3DT_MAX_BLOCKS];
} N3dtRenderParams;

/* Gradient buffers, same shapes and order as the parameters; every training entry point ACCUMULATES (+=)
 * into them, so the caller zeroes them (or passes PyTorch's .grad tensors to accumulate across calls). */
typedef struct N3dtMlpGrads {
    float* weight[N3DT_MLP_LAYERS];
    float* bias[N3DT_MLP_LAYERS];
} N3dtMlpGrads;

typedef struct N3dtRenderGrads {
    float* to_rgb_w[N3DT_MAX_BLOCKS + 1];
    float* to_rgb_b[N3DT_MAX_BLOCKS + 1];
    float* psu1_w[N3DT_MAX_BLOCKS];
    float* psu1_b[N3DT_MAX_BLOCKS];
    float* psu2_w[N3DT_MAX_BLOCKS];
    float* psu2_b[N3DT_MAX_BLOCKS];
    float* feat_w[N3DT_MAX_BLOCKS];
    float* feat_b[N3DT_MAX_BLOCKS];
} N3dtRenderGrads;

int n3dt_abi_version(void);
const char* n3dt_last_error(void);

/* ---- weights ------------------------------------------------------------------------------
 * Re-lay the MLP weights into the MFMA-fragment order (and dtype) the fused kernel streams.
 * PyTorch's optimizer mutates the fp32 parameters in place every step, so the binding
 * re-packs whenever a parameter's version counter changed (SURVEY 8b "Parameters / ownership").
 * Replaces: nothing in the reference (cuDNN consumes the Conv2d weights directly). */
size_t n3dt_mlp_packed_bytes(const N3dtGeom* g, int precision);
int n3dt_mlp_pack(const N3dtGeom* g, int precision, const N3dtMlpParams* p, void* packed, void* stream);

/* ---- volumetric render: a1..a7 of SURVEY 8a in one call --------------------------------------
 * Replaces, fused: GenSamplePoints.forward (NetWorks/utils.py:147-161), Embedder.forward
 * (utils.py:43-51), the latent expand+concat (HeadNeRFNet.py:84,149-152), MLPforNeRF.forward
 * (models.py:62-87), CalcRayColor.forward (utils.py:291-309) and the background merge
 * (HeadNeRFNet.py:103-112).
 *   xy      batch_xy, strides in g                R, Kinv [B,3,3]     T [B,3]
 *   shape [B,shape_dim]  appea [B,appea_dim]  audio [B,audio_dim] (NULL iff audio_dim==0)
 *   t_rand  [B,N_r,N_s+1] uniform noise for mode=="train" (utils.py:73-78), NULL for "test";
 *           with g->z_planes_given: the sample planes themselves (see N3dtGeom)
 *   bg_featmap  neural_render.bg_featmap [C, N_r] (NCHW parameter), NULL to skip the merge
 *   ray_bias    [B, N_r, 192] per-ray addend of RGB_layer_1's pre-activation: required iff g->vd_dim > 0 (include_vd), else NULL
 * outputs (any may be NULL, but one of fg_feat / merge_feat must be given):
 *   fg_feat [B,N_r,C]  bg_alpha [B,N_r]  depth [B,N_r]  weight [B,N_r,N_s]
 *   merge_feat [B,N_r,C] = fg_feat + bg_alpha * bg_featmap
 * `saved` (nullable, n3dt_render_saved_bytes) receives what n3dt_render_bwd needs. */
size_t n3dt_render_workspace_bytes(const N3dtGeom* g, int precision);
int n3dt_render_fwd(const N3dtGeom* g, int precision, const void* packed_mlp, const N3dtMlpParams* p,
                    const float* xy, const float* R, const float* T, const float* Kinv,
                    const float* shape, const float* appea, const float* audio, const float* t_rand,
                    const float* bg_featmap, const float* ray_bias,
                    float* fg_feat, float* bg_alpha, float* depth, float* weight, float* merge_feat,
                    void* workspace, size_t workspace_bytes, void* stream);

/* n3dt_render_fwd for a caller that hands the merged map straight to the 2-D renderer's 16-bit path (precision BF16 / F16 /
 * BF16X3 only).  Two more optional outputs, both written by the ray head from the fp32 values it holds in registers:
 *   merge_feat16 [B,N_r,C] 16-bit: merge_feat rounded (nearest-even) to the renderer's map type -- bf16 for N3DT_BF16, f16
 *                for N3DT_F16 and N3DT_BF16X3 -- exactly what the renderer's first block forms from an fp32 map while staging
 *   rgb0         [B,3,N_r] fp32 planar: feat_2_rgb[0] of the FP32 merged values, rgb0_w [3,C], rgb0_b [3]
 *                (the projection n3dt_neural_render_fwd runs as a pass of its own over an fp32 map)
 * One of fg_feat / merge_feat / merge_feat16 must be given; rgb0 needs rgb0_w and rgb0_b; merge_feat, when NULL, is not
 * written.  Feed both to n3dt_neural_render_fwd16_reuse.  An addition to ABI 5: no existing entry changed. */
int n3dt_render_fwd16(const N3dtGeom* g, int precision, const void* packed_mlp, const N3dtMlpParams* p,
                      const float* xy, const float* R, const float* T, const float* Kinv,
                      const float* shape, const float* appea, const float* audio, const float* t_rand,
                      const float* bg_featmap, const float* ray_bias,
                      float* fg_feat, float* bg_alpha, float* depth, float* weight, float* merge_feat,
                      void* merge_feat16, float* rgb0, const float* rgb0_w, const float* rgb0_b,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- include_vd: the view-direction columns of RGB_layer_1 as a per-ray bias (ABI 5) -------------------------------
 * Replaces, for `include_vd=True`: GenSamplePoints' ray direction (NetWorks/utils.py:149-153), `vd_encoder(fg_dirs)`
 * (HeadNeRFNet.py:141-142: Embedder, 4 frequencies + input = 27 channels, utils.py:20-51), its expand over the samples and the
 * 27 matching columns of RGB_layer_1 (models.py:80; columns 384 .. 410 of its weight):
 *   ray_bias[b, r, o] = sum_j w_vd[o * ld_w + j] * Embedder_4(d(b, r))[j],   o < 192, j < 27
 * w_vd points at RGB_layer_1.weight[0][384] of the FULL parameter ([192, 384 + 27 + appea_dim], ld_w = its row length).
 * Inference helper; the differentiable path forms the same tensor with autograd on the host (a [B*N_r, 27] x [27, 192] product). */
int n3dt_ray_vd_bias(const N3dtGeom* g, const float* w_vd, int64_t ld_w, const float* xy, const float* R, const float* Kinv,
                     float* ray_bias, void* stream);

/* ---- hierarchical (fine) sample planes: SURVEY 8f row 4 ------------------------------------------
 * Replaces FineSample.forward (NetWorks/utils.py:211-263): inverse-CDF resampling of the coarse pass.
 *   g         geometry of the COARSE pass (n_samples = N_c >= 3).  z_planes_given = 0: the coarse planes are recomputed from
 *             T and t_rand; 1: `t_rand` carries them, [B,N_r,N_c+1] (the far edge is not read) -- the fine_samp_func seam,
 *             whose caller holds coarse_sample_dict["zvals"]
 *   n_fine    opt.num_sample_fine (N_f); n_fine + 1 samples are drawn
 *   weight    [B,N_r,N_c] compositing weights of the coarse pass (n3dt_render_fwd's `weight`)
 *   T, t_rand as given to the coarse pass (the coarse planes are recomputed from them)
 *   u         [B*N_r, N_f+1] uniform samples for mode=="train" (torch.rand at utils.py:227), NULL: linspace(0,1)
 *   z_planes  [B,N_r,N_c+N_f+1] out, ascending: the coarse planes merged with the new ones (utils.py:248).
 * The fine pass is then n3dt_render_fwd with n_samples = N_c + N_f, z_planes_given = 1, t_rand = z_planes and the
 * fine network's parameters (the reference's own call site, HeadNeRFNet.py:182-185, omits two arguments and cannot
 * run; this is that call with them supplied). */
int n3dt_fine_sample(const N3dtGeom* g, int n_fine, const float* weight, const float* T, const float* t_rand, const float* u,
                     float* z_planes, void* stream);

/* ---- the reference's inner seams as stand-alone operators ------------------------------------------
 * HeadNeRFNet keeps its sub-modules addressable (sample_func, vp_encoder, fg_CD_predictor, calc_color_func).
 * n3dt_render_fwd never materialises the tensors that cross those seams; these four calls do, in the reference's own
 * layouts, for callers that use the sub-modules directly.  Exact fp32, unfused, inference only.  M = N_r * N_s.
 *   n3dt_sample_points  GenSamplePoints.forward (NetWorks/utils.py:147-161): pts [B,3,N_r,N_s], zvals / z_dists
 *                       [B,1,N_r,N_s], ray_d [B,3,N_r], ray_l [B,1,N_r] (outputs may be NULL); t_rand as in n3dt_render_fwd
 *   n3dt_embed          Embedder.forward (utils.py:43-51): pts [B,3,M] -> pe [B,63,M]
 *   n3dt_mlp_points     MLPforNeRF.forward (NetWorks/models.py:62-87): audio [B,audio_dim,M] (NULL iff audio_dim == 0),
 *                       embed_vps [B,63+shape_dim,M], embed_vds [B,appea_dim,M] -> rgb [B,256,M], density [B,1,M]
 *                       (g supplies batch and the code widths; workspace from n3dt_mlp_points_workspace_bytes)
 *   n3dt_composite      CalcRayColor.forward (utils.py:291-309): rgb [B,C,N_r,N_s], density / z_dists / zvals
 *                       [B,1,N_r,N_s] -> feat [B,C,N_r], bg_alpha / depth [B,1,N_r], weight [B,1,N_r,N_s] (last three nullable) */
int n3dt_sample_points(const N3dtGeom* g, const float* xy, const float* R, const float* T, const float* Kinv, const float* t_rand,
                       float* pts, float* zvals, float* z_dists, float* ray_d, float* ray_l, void* stream);
int n3dt_embed(int batch, size_t m, const float* pts, float* pe, void* stream);
/* the same encoder with n_freqs frequencies (ABI 5): pts [B,3,M] -> pe [B, 3 + 6 n_freqs, M]; n_freqs = 4 is the reference's
 * vd_encoder (HeadNeRFNet.py:30-31,61), 10 equals n3dt_embed */
int n3dt_embed_freqs(int batch, size_t m, int n_freqs, const float* pts, float* pe, void* stream);
size_t n3dt_mlp_points_workspace_bytes(const N3dtGeom* g, size_t m);
int n3dt_mlp_points(const N3dtGeom* g, size_t m, const N3dtMlpParams* p, const float* audio, const float* embed_vps,
                    const float* embed_vds, float* rgb, float* density, void* workspace, size_t workspace_bytes, void* stream);
int n3dt_composite(int batch, int n_rays, int n_samples, int channels, const float* rgb, const float* density, const float* z_dists,
                   const float* zvals, float* feat, float* bg_alpha, float* depth, float* weight, void* stream);
/* The rounding step of the fused 16-bit kernels on its own (an addition: the ABI version stays 5): in [n] floats -> out [n] 16-bit
 * values (bf16 for N3DT_BF16, f16 for N3DT_F16; no other precision), one wave per 512 values, every lane packing eight consecutive
 * values into one MFMA fragment.  form 0: through the kernels' own pack (two values per conversion instruction); form 1: through
 * an element-wise cast kept in this probe only -- the two must agree bit for bit.  n: a multiple of 512. */
int n3dt_x16_pack_probe(int precision, int form, size_t n, const float* in, uint16_t* out, void* stream);
/* The positional encoder of the fused 16-bit kernels on its own (an addition: the ABI version stays 5): points [n][3] floats ->
 * out [n / 32][4][64][8] 16-bit values (bf16 / f16 as above), one wave per 32 points, out = that wave's four MFMA B fragments as
 * the kernels hold them: piece ks, lane (c, h), element j is channel 16 ks + 8 (j >> 2) + 4 h + (j & 3) of point 32 wave + c (channels
 * 0-2 the point, 3 + 6 k + {0, 1, 2} the sines and 3 + 6 k + {3, 4, 5} the cosines of octave k, 63 zero).  form 0: the kernels' own
 * encoder (every octave and axis once, sine and cosine together, through the wave's LDS copy); form 1: the per-channel encoder
 * it replaced, kept in this probe -- the two must agree bit for bit.  n: a multiple of 32. */
int n3dt_x16_pe_probe(int precision, int form, size_t n, const float* points, uint16_t* out, void* stream);

/* ---- 2-D neural renderer: a8..a10 ----------------------------------------------------------------
 * Replaces NeuralRenderer.forward (NetWorks/neural_renderer.py:72-91) including
 * PixelShuffleUpsample.forward (PixelShuffleUpsample.py:36-45) and Blur (…:15-18, kornia filter2d).
 *   featmap [nb, fs, fs, C] ray-major   ->   img [nb, 3, P, P], P = fs << n_blocks
 * `precision` selects the arithmetic of the 1x1-conv GEMMs (N3DT_F32 exact; BF16/F16 inputs with
 * fp32 accumulate); blur, bilinear and the RGB pyramid are always fp32.
 * `nb` is the number of feature maps in this call (the binding renders the B merged maps and the
 * background map together, nb = B+1; reference calls the module twice, HeadNeRFNet.py:109,113).
 * Limit: nb * P * P * 32 < 2^31 (the kernels index one map level with 32-bit offsets: 255 maps at 512^2,
 * 63 at 1024^2); larger batches return N3DT_EINVAL before anything is launched -- split them. */
size_t n3dt_neural_render_workspace_bytes(const N3dtGeom* g, int nb);
int n3dt_neural_render_fwd(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap,
                           float* img, void* workspace, size_t workspace_bytes, void* stream);

/* The 16-bit modes re-lay the upsample blocks' fp32 weights into MFMA order at the start of every n3dt_neural_render_fwd
 * (the renderer takes raw parameters, so it cannot know whether an optimizer touched them): three 6 us launches, 2.5 % of
 * a one-head forward.  A caller that tracks its parameters (version counters) can split the two steps: the packed stream
 * lives in the tail of the caller-owned workspace.
 *   n3dt_neural_render_pack       re-packs the block weights into `workspace` (nothing else is touched);
 *   n3dt_neural_render_fwd_reuse  = n3dt_neural_render_fwd minus the packing: valid when the same workspace was last packed
 *                                   (by _pack or _fwd) for the same geometry, nb, precision and parameter VALUES.
 * fp32 precision reads the raw parameters: _pack is a no-op and _fwd_reuse equals _fwd. */
int n3dt_neural_render_pack(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, void* workspace,
                            size_t workspace_bytes, void* stream);
int n3dt_neural_render_fwd_reuse(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap,
                                 float* img, void* workspace, size_t workspace_bytes, void* stream);
/* n3dt_neural_render_fwd_reuse on the outputs of n3dt_render_fwd16 (16-bit precisions only): featmap16 [nb, fs, fs, C] in the
 * map type of `precision`, rgb0 [nb, 3, fs, fs] the level-0 projection (read only).  The first block then reads 16-bit rows
 * and no projection pass runs; everything behind the first block's staging is the fp32-input form's arithmetic, bit for bit. */
/* The level-0 projection on its own, as n3dt_neural_render_fwd's 16-bit path runs it on an fp32 map: featmap [nb, n_pix, 256]
 * -> rgb0 [nb, 3, n_pix] = feat_2_rgb[0] (w [3,256], b [3]).  A seam for comparing the two producers of rgb0. */
int n3dt_feat_to_rgb0(int nb, int n_pix, const float* featmap, const float* w, const float* b, float* rgb0, void* stream);
int n3dt_neural_render_fwd16_reuse(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const void* featmap16,
                                   const float* rgb0, float* img, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training path (fwd -> loss -> backward) -----------------------------------
 * `precision` = N3DT_F32: exact fp32 (the mode the gradient-parity tests pin); N3DT_BF16: every matrix product
 * on v_mfma_f32_32x32x16_bf16 with operands rounded to bf16 while staging (fp32 storage and accumulation), the
 * rest identical.  The forward keeps the per-layer activations in `saved` (caller-owned, sized by the
 * *_saved_bytes query) for the matching backward call, which must use the same precision; `workspace` is scratch.
 *
 * n3dt_render_train_fwd: same mathematics and outputs as n3dt_render_fwd (fg_feat, bg_alpha, depth?, merge_feat?).
 * n3dt_render_bwd: given dL/d(merge_feat) (and optionally dL/d(fg_feat), dL/d(bg_alpha), both nullable),
 *   accumulates parameter gradients into `grads`, adds dL/d(bg_featmap) [C,N_r] into d_bg_featmap (nullable)
 *   and writes dL/d(shape) [B,shape_dim], dL/d(appea) [B,appea_dim], dL/d(audio) [B,audio_dim] (each nullable).
 *   Differentiates NetWorks/models.py:62-87, NetWorks/utils.py:268-309, NetWorks/HeadNeRFNet.py:84-112,149-152.
 *   Camera gradients (the fitting use-case, FittingSingleImage_new.py:826-859): when d_R [B,3,3] and/or d_T [B,3]
 *   are non-NULL they receive dL/d(batch_Rmats), dL/d(batch_Tvecs); xy, R, T, Kinv (and t_rand if the forward
 *   used it) must then be the forward's inputs.  Pass NULL for all seven to skip that work.
 *   d_ray_bias [B, N_r, 192] (iff g->vd_dim > 0, else NULL) receives dL/d(ray_bias): the per-ray sums of RGB_layer_1's
 *   pre-activation gradient, from which the caller's autograd forms the gradients of the 27 view-direction columns (and, through
 *   the ray direction, of the camera rotation).
 *   `grads` == NULL (both n3dt_render_bwd and n3dt_neural_render_bwd): the network is FROZEN, as in single-image fitting
 *   (FittingSingleImage_new.py:826-859 optimises codes and cameras only) -- no parameter gradient is computed, only the
 *   gradients of the inputs (d_bg_featmap must then be NULL too). */
size_t n3dt_render_train_saved_bytes(const N3dtGeom* g);
size_t n3dt_render_train_workspace_bytes(const N3dtGeom* g);
int n3dt_render_train_fwd(const N3dtGeom* g, int precision, const void* packed_mlp, const N3dtMlpParams* p,
                          const float* xy, const float* R, const float* T, const float* Kinv,
                          const float* shape, const float* appea, const float* audio, const float* t_rand,
                          const float* bg_featmap, const float* ray_bias, float* fg_feat, float* bg_alpha, float* depth, float* merge_feat,
                          void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int n3dt_render_bwd(const N3dtGeom* g, int precision, const N3dtMlpParams* p, const N3dtMlpGrads* grads,
                    const float* shape, const float* appea, const float* audio, const float* bg_featmap,
                    const float* d_merge_feat, const float* d_fg_feat, const float* d_bg_alpha,
                    const void* saved, size_t saved_bytes,
                    float* d_bg_featmap, float* d_shape, float* d_appea, float* d_audio, float* d_ray_bias,
                    const float* xy, const float* R, const float* T, const float* Kinv, const float* t_rand,
                    float* d_R, float* d_T,
                    void* workspace, size_t workspace_bytes, void* stream);
/* n3dt_render_bwd_cam: n3dt_render_bwd plus the gradients of the other two inputs of ray generation (n3dt_render_bwd is this
 * call with both NULL).  With c = Kinv [x, y, 1] and gc = R^T dL/d(R c) per ray:
 *   d_Kinv [B,3,3] (nullable) is ACCUMULATED into (the caller zeroes it): d_Kinv[b][i][j] += sum over rays of gc[i] [x, y, 1][j];
 *   d_xy [B,2,N_r] (nullable, contiguous whatever the strides of xy) is overwritten: d_xy[b][k][ray] = sum_i gc[i] Kinv[b][i][k].
 * Either one needs xy, R, T, Kinv like d_R / d_T; each of the four camera gradients may be NULL on its own.  With include_vd the
 * share that reaches Kinv and xy through ray_bias is the caller's (d_ray_bias), as it is for R. */
int n3dt_render_bwd_cam(const N3dtGeom* g, int precision, const N3dtMlpParams* p, const N3dtMlpGrads* grads,
                        const float* shape, const float* appea, const float* audio, const float* bg_featmap,
                        const float* d_merge_feat, const float* d_fg_feat, const float* d_bg_alpha,
                        const void* saved, size_t saved_bytes,
                        float* d_bg_featmap, float* d_shape, float* d_appea, float* d_audio, float* d_ray_bias,
                        const float* xy, const float* R, const float* T, const float* Kinv, const float* t_rand,
                        float* d_R, float* d_T, float* d_Kinv, float* d_xy,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Neural renderer with saved activations, and its backward (differentiates NetWorks/neural_renderer.py:72-91,
 * NetWorks/PixelShuffleUpsample.py:36-45).  d_featmap [nb,fs,fs,C] is overwritten; parameter gradients accumulate. */
size_t n3dt_neural_render_train_saved_bytes(const N3dtGeom* g, int nb);
size_t n3dt_neural_render_train_workspace_bytes(const N3dtGeom* g, int nb);
int n3dt_neural_render_train_fwd(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap, float* img,
                                 void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int n3dt_neural_render_bwd(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const N3dtRenderGrads* grads,
                           const float* featmap, const float* d_img, const void* saved, size_t saved_bytes,
                           float* d_featmap, void* workspace, size_t workspace_bytes, void* stream);

/* ---- display conversion ----------------------------------------------------------------------------
 * Replaces `(img.permute(1,2,0).numpy() * 255).astype(np.uint8)` (talker_trainer.py:1205, Utils/RenderUtils.py:123-125):
 *   img [n_images,3,pixels] float in (0,1)  ->  out [n_images,pixels,3] uint8 */
int n3dt_img_to_uint8(int n_images, int pixels, const float* img, unsigned char* out, void* stream);

/* ---- validation metrics: SSIM and PSNR of rendered frames (Utils/Eval_utils.py:11-48,54-66,101-106) ---------------------
 * What the reference's validation() scores a frame with, for every image pair of the call:
 *   q      = (unsigned char) min(max(x * 255.0f, 0.0f), 255.0f), NaN -> 0: `(x * 255).astype(np.uint8)` inside [0,1]; outside
 *            it numpy's cast is undefined and the clamp is this library's definition
 *   grey   = (q0 * 3735 + q1 * 19235 + q2 * 9798 + 16384) >> 15: cv2.cvtColor(COLOR_BGR2GRAY) on uint8, channel 0 taken as B
 *            although the image is RGB (the reference's quirk, kept)
 *   ssim   = skimage.metrics.structural_similarity(grey1, grey2), every default on uint8: float64, 7x7 uniform window,
 *            data_range 255, K1 0.01, K2 0.03, sample covariance, the mean over the image cropped by 3 on every side
 *   psnr   = cv2.PSNR(q1, q2) on the colour bytes: 20 log10(255 / (sqrt(SSE / (3 H W)) + DBL_EPSILON)); identical images
 *            give 361.20..., not infinity
 * pred, gt [n_images, 3, height, width] fp32 contiguous -> ssim [n_images], psnr [n_images] doubles.  Two launches whatever
 * n_images is: one workgroup per 32x32 tile forms the window sums and the squared error as exact integers and one
 * (double, uint64) partial; one workgroup per image adds its partials in index order.  No atomics: the result is bitwise
 * reproducible.  workspace: n3dt_eval_metrics_workspace_bytes, contents immaterial between calls.
 * Limits (N3DT_EINVAL before anything is enqueued; the size query returns 0 and sets n3dt_last_error):
 * n_images >= 1, height >= 7, width >= 7, height * width < 2^31; no NULL pointer; ssim, psnr and the workspace 8-byte aligned
 * (they are written as doubles and (double, uint64) records), pred and gt 4-byte aligned; workspace_bytes at least the query's. */
size_t n3dt_eval_metrics_workspace_bytes(int n_images, int height, int width);
int n3dt_eval_metrics(int n_images, int height, int width, const float* pred, const float* gt, double* ssim, double* psnr,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- validation metrics: LPIPS with AlexNet features (Utils/Eval_utils.py:108-115; an addition, the ABI version stays 5) ---
 * lpips.LPIPS(net='alex') (version 0.1, spatial=False, eval mode) of every image pair of the call, as the reference calls it.
 * The lpips package is not a dependency: what is written here about it is from knowledge of lpips 0.1.4, so parity is unpinned
 * to the dependency.
 *   input   N3DT_LPIPS_REFERENCE: the quantiser q above, then the bytes of the [H,W,3] image read as [3,H,W] WITHOUT a transpose
 *           (the reference's reshape(-1,3,h,w): element [c',y',x'] is flat byte c' H W + y' W + x' of the HWC buffer), values
 *           0..255.  N3DT_LPIPS_STANDARD: 2 clamp(x,0,1) - 1, NaN -> -1, channels as given (the metric as its authors define it).
 *   scaling (v - shift) / scale in fp32, shift (-.030,-.088,-.188), scale (.458,.448,.450); the convolution's zero padding follows
 *   relu1..5 torchvision alexnet().features: conv 3->64 k11 s4 p2 | pool 3/2, conv 64->192 k5 p2 | pool 3/2, conv 192->384 k3 p1 |
 *           conv 384->256 k3 p1 | conv 256->256 k3 p1, a ReLU after each; implicit GEMMs on the bf16 MFMA with every operand split
 *           hi + lo and three products per term (the N3DT_F32 mode of the VGG term; the only mode)
 *   layer   mean over pixels of sum_c w_c (n0_c - n1_c)^2, n = f / (sqrt(sum_c f^2) + 1e-10), w = lin[l] [C_out], float64
 *   out     the five layer values added in layer order
 * n3dt_lpips_pack re-lays weight[l] [C_out, C_in, k, k], bias[l] [C_out] and lin[l] [C_out] (device fp32, torchvision order) into
 * `packed` (n3dt_lpips_packed_bytes, 256-byte aligned).  n3dt_lpips: pred, gt [batch,3,height,width] fp32 contiguous ->
 * out [batch] doubles and, unless NULL, layers [5, batch] doubles.  Fixed launch sequence, no atomics, partial sums laid out per
 * image pair: the result is bitwise reproducible, exactly 0 for identical images, symmetric in (pred, gt), and independent of a
 * pair's position in the batch and of the batch size.  workspace: n3dt_lpips_workspace_bytes, contents immaterial between calls.
 * Limits (N3DT_EINVAL before anything is enqueued; the size query returns 0 and sets n3dt_last_error): 1 <= batch <= 64,
 * 31 <= height, width <= 2048 (31 is the smallest size every layer has a pixel of); no NULL pointer but `layers`; out and layers
 * 8-byte, pred and gt 4-byte, packed and workspace 256-byte aligned; workspace_bytes at least the query's. */
#define N3DT_LPIPS_LAYERS 5
#define N3DT_LPIPS_REFERENCE 0
#define N3DT_LPIPS_STANDARD 1
typedef struct N3dtLpipsParams {
    const float* weight[N3DT_LPIPS_LAYERS];
    const float* bias[N3DT_LPIPS_LAYERS];
    const float* lin[N3DT_LPIPS_LAYERS];
} N3dtLpipsParams;
size_t n3dt_lpips_packed_bytes(void);
int n3dt_lpips_pack(const N3dtLpipsParams* p, void* packed, void* stream);
size_t n3dt_lpips_workspace_bytes(int batch, int height, int width);
int n3dt_lpips(int batch, int height, int width, int input_mode, const void* packed, const float* pred, const float* gt, double* out,
               double* layers, void* workspace, size_t workspace_bytes, void* stream);

/* ---- audio front end: waveform -> mel spectrogram -> Audio2style windows -----------------------------------------------
 * The reference computes Audio2style's input on the CPU (wav_audio.melspectrogram with wav_hparams.py, then 16-column windows
 * cut by the data loader, XGaze_utils/data_loader_xgaze.py:256-270).  Here, in float64 on the device (csrc/mel.hip, the
 * arithmetic in csrc/mel_core.h, the formulation in DESIGN section 3.15):
 *   y[0] = x[0], y[n] = x[n] - 0.97 x[n-1]; reflect padding of 400 without the edge sample; frame t = 800 padded samples from
 *   200 t, T = 1 + L / 200 frames; periodic Hann window; |DFT| of 401 bins; basis [80, 401] . |D|; 20 log10(max(1e-5, .)) - 20;
 *   8 (S + 100) / 100 - 4 clipped to [-4, 4].
 * n3dt_mel_spectrogram computes the frames first_frame .. first_frame + n_frames - 1 of a signal from a RUN of it:
 * wav[0 .. n_samples) are the samples wav_offset .. wav_offset + n_samples of the signal, *prev_sample is the sample
 * wav_offset - 1 (device memory; read only when wav_offset > 0, where it carries the pre-emphasis across the cut), and
 * total_samples is the signal's length, or -1 while its end is unknown (no frame may then reach past the run).  The whole
 * signal at once is wav_offset 0, prev_sample NULL, total_samples n_samples, first_frame 0, n_frames 1 + n_samples / 200; a
 * stream computes its interior frames from a buffer that starts mid-signal.  A frame's value depends on the samples it reads,
 * `table` and `basis` alone -- not on the run, the frame's position in the call or n_frames -- and is bitwise reproducible.
 * basis: [80, 401] fp32 (device); table: cos(2 pi n / 800), n = 0 .. 799, doubles (device); both are the caller's.
 * out: [80, out_ld] with frame first_frame + f in column f, doubles when out_is_f64, else floats (one conversion at the store).
 * NaN samples give NaN values.  Two launches.  workspace: n3dt_mel_workspace_bytes (the basis transposed for the kernel).
 * n3dt_mel_windows: mel [80, mel_ld] with T valid columns, start [n_windows] int32 (device) -> out [n_windows, 80, 16] fp32,
 * out[w, i, c] = mel[i, clamp(start[w] + c, 0, T - 1)].  One launch.
 * Limits (N3DT_EINVAL before anything is enqueued): n_samples >= 401; 1 <= n_frames <= 2^24; the run must hold every sample the
 * frames read (the left reflection needs wav_offset 0, the right one total_samples); out_ld >= n_frames, mel_ld >= T >= 1,
 * n_windows >= 1; no NULL pointer; table and a double `out` / `mel` 8-byte aligned, the rest 4-byte aligned; workspace_bytes at
 * least the query's. */
size_t n3dt_mel_workspace_bytes(void);
int n3dt_mel_spectrogram(int64_t n_samples, const float* wav, int64_t wav_offset, const float* prev_sample, int64_t total_samples,
                         int64_t first_frame, int n_frames, const float* basis, const double* table, void* out, int64_t out_ld,
                         int out_is_f64, void* workspace, size_t workspace_bytes, void* stream);
int n3dt_mel_windows(int64_t T, const void* mel, int64_t mel_ld, int mel_is_f64, int n_windows, const int32_t* start, float* out,
                     void* stream);

/* ---- lip-sync metric: Wav2Lip's expert SyncNet_color, frozen, inference only (an addition, the ABI version stays 5) ---------
 * The reference's wav_models/syncnet.py: a 17-block face encoder over windows [15,48,96] (five consecutive lower-half face crops,
 * BGR, channel 3 t + c) and a 14-block audio encoder over mel windows [1,80,16]; each block is Conv2d + BatchNorm2d (eval mode,
 * eps 1e-5), then for residual blocks the block's own input, then ReLU (wav_models/conv.py:15-19); both encoders end in a
 * 512-vector, normalised x / max(||x||_2, 1e-12); the cosine of the two is the sync probability.  csrc/syncnet.hip; the 31-row
 * geometry table and the address arithmetic are csrc/syncnet_core.h; DESIGN section 3.16.
 *   pack    batch norm folded in float64: s = gamma / sqrt(var + 1e-5), w' = fp32(w s), b' = fp32((b - mean) s + beta); w' split
 *           into hi + lo bf16 in MFMA fragment order.  weight[b] [C_out, C_in, kh, kw], the other five [C_out], device fp32, block
 *           b = 0..16 the face encoder's, 17..30 the audio encoder's.  `packed`: n3dt_syncnet_packed_bytes, 256-byte aligned.
 *   blocks  implicit GEMMs on the bf16 MFMA, every operand split hi + lo, three products per term, fp32 accumulation; the only mode
 *   tail    normalisation and cosine in float64, fixed summation order
 * n3dt_syncnet_fwd: mel_windows [n,1,80,16] and EITHER face_windows [n,15,48,96] OR frames [n + 4, 3, height, width] (fp32 RGB in
 * [0,1]; window i is frames i .. i + 4) with boxes [n_boxes, 4] int32 (device) = (y1, y2, x1, x2) per frame, n_boxes = n + 4 or 1
 * (one box for all) -> audio_emb, face_emb [n,512] fp32 and cos [n] doubles (each nullable).  All contiguous.
 * n3dt_syncnet_face_windows is that prologue alone: crop rows y1..y2-1 and columns x1..x2-1, values clamped to [0,1] (NaN -> 0),
 * bilinear resample to 96 x 96 with half-pixel centres (F.interpolate(mode="bilinear", align_corners=False, antialias=False)) in
 * float64, rows 48..95, RGB reversed to BGR -> face_windows [n,15,48,96].  A box reaching outside the frame is clamped into it.
 * n3dt_syncnet_block runs ONE block of the table on in [n, C_in, Hi, Wi] -> out [n, C_out, Ho, Wo] (a debugging aid: the tests
 * judge blocks one at a time with it).
 * A window's results depend on that window's inputs and the packed weights alone -- not on its position in the call or on n -- and
 * are bitwise reproducible.  Everything is enqueued on `stream`, nothing synchronises, no atomics.
 * workspace: n3dt_syncnet_workspace_bytes(n), 256-byte aligned, contents immaterial between calls.
 * Limits (N3DT_EINVAL before anything is enqueued; the size query returns 0 and sets n3dt_last_error): 1 <= n <= 1024;
 * 2 <= height, width <= 4096; 0 <= block <= 30; exactly one of face_windows and frames; n_boxes 1 or n + 4; no NULL pointer but
 * the three outputs of n3dt_syncnet_fwd; cos 8-byte, frames and boxes 4-byte, packed and workspace 256-byte, the rest 16-byte aligned; workspace_bytes at
 * least the query's. */
#define N3DT_SYNCNET_BLOCKS 31
typedef struct N3dtSyncnetParams {
    const float* weight[N3DT_SYNCNET_BLOCKS];
    const float* bias[N3DT_SYNCNET_BLOCKS];
    const float* bn_weight[N3DT_SYNCNET_BLOCKS];
    const float* bn_bias[N3DT_SYNCNET_BLOCKS];
    const float* bn_mean[N3DT_SYNCNET_BLOCKS];
    const float* bn_var[N3DT_SYNCNET_BLOCKS];
} N3dtSyncnetParams;
size_t n3dt_syncnet_packed_bytes(void);
int n3dt_syncnet_pack(const N3dtSyncnetParams* p, void* packed, void* stream);
size_t n3dt_syncnet_workspace_bytes(int n);
int n3dt_syncnet_face_windows(int n, int height, int width, const float* frames, const int32_t* boxes, int n_boxes, float* face_windows,
                              void* stream);
int n3dt_syncnet_fwd(int n, const void* packed, const float* mel_windows, const float* face_windows, const float* frames,
                     const int32_t* boxes, int n_boxes, int height, int width, float* audio_emb, float* face_emb, double* cos,
                     void* workspace, size_t workspace_bytes, void* stream);
int n3dt_syncnet_block(int block, int n, const void* packed, const float* in, float* out, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- Wav2Lip's generator: audio-driven lip-synced faces, frozen, inference only (an addition, the ABI version stays 5) ------
 * The reference's wav_models/wav2lip.py: 51 blocks in state-dict order -- 18 of the face encoder on [6,96,96] (the outputs of its
 * seven groups are skip features), 13 of the audio encoder on [1,80,16], 18 of the decoder (six of them ConvTranspose2d; behind
 * each of its seven groups torch.cat((x, skip), 1)), Conv2d(80,32,3) and the plain nn.Conv2d(32,3,1) with its sigmoid.  Every
 * block but the last is convolution + BatchNorm2d (eval mode, eps 1e-5), then for residual blocks the block's own input, then
 * ReLU.  csrc/wav2lip.hip; the table, the classes of a transposed block's rows and the address arithmetic are
 * csrc/wav2lip_core.h; DESIGN section 3.17.
 *   pack    batch norm folded in float64 as n3dt_syncnet_pack does; weight[b] [C_out, C_in, kh, kw] (ConvTranspose2d:
 *           [C_in, C_out, kh, kw]), the other five [C_out], device fp32; block 50 has weight and bias alone (its bn_* are ignored).
 *   blocks  implicit GEMMs on the bf16 MFMA, every operand split hi + lo, three products per term, fp32 accumulation: the only mode;
 *           block 50 accumulates in float64
 * n3dt_wav2lip_fwd: mel_windows [n,1,80,16], face_inputs [n,6,96,96] (channels 0..2 the masked target, 3..5 the reference, BGR) ->
 *   out [n,3,96,96] fp32 (BGR, in [0,1]).  All contiguous.
 * n3dt_wav2lip_block runs ONE block on in [n, C_in, Hi, Wi] -> out [n, C_out, Ho, Wo]; for the last block of a decoder group
 *   (31, 33, 36, 39, 42, 45, 48) with skip [n, C_skip, Ho, Wo] given, out is the concatenation [n, C_out + C_skip, Ho, Wo]; block 50
 *   gives its logits (no sigmoid).  skip is ignored for every other block.
 * n3dt_wav2lip_face_inputs: frames [n,3,height,width] fp32 RGB in [0,1] (clamped, NaN -> 0), ref_frames the same (NULL: the frames
 *   themselves), boxes [n_boxes,4] int32 (device) = (y1, y2, x1, x2), n_boxes = n or 1 -> out [n,6,96,96]: the crops resampled to
 *   96 x 96 bilinearly with half-pixel centres in float64, BGR, rows 48..95 of channels 0..2 zero.
 * n3dt_wav2lip_paste: faces [n,3,96,96] (BGR) resampled the same way to each box and written over [y1:y2, x1:x2] of a copy of
 *   frames [n,3,height,width], BGR -> RGB -> out [n,3,height,width]; outside the box out is the frame, bit for bit.
 * A window's results depend on that window's inputs and the packed weights alone -- not on its position in the call or on n -- and
 * are bitwise reproducible.  Everything is enqueued on `stream`, nothing synchronises, no atomics.
 * workspace: n3dt_wav2lip_workspace_bytes(n) (about 11.2 MB a window: the seven concatenation buffers and two copies of the largest
 * other map), 256-byte aligned, never cleared, contents immaterial between calls.
 * Limits (N3DT_EINVAL before anything is enqueued; the size query returns 0 and sets n3dt_last_error): 1 <= n <= 128 for fwd, block
 * and the workspace (1.43 GB at 128), 1 <= n <= 4096 for face_inputs and paste; 2 <= height, width <= 4096; 0 <= block <= 50;
 * n_boxes 1 or n; no NULL pointer but skip and ref_frames; frames and boxes 4-byte, packed and workspace 256-byte, the rest
 * 16-byte aligned; workspace_bytes at least the query's. */
#define N3DT_WAV2LIP_BLOCKS 51
typedef struct N3dtWav2lipParams {
    const float* weight[N3DT_WAV2LIP_BLOCKS];
    const float* bias[N3DT_WAV2LIP_BLOCKS];
    const float* bn_weight[N3DT_WAV2LIP_BLOCKS];
    const float* bn_bias[N3DT_WAV2LIP_BLOCKS];
    const float* bn_mean[N3DT_WAV2LIP_BLOCKS];
    const float* bn_var[N3DT_WAV2LIP_BLOCKS];
} N3dtWav2lipParams;
size_t n3dt_wav2lip_packed_bytes(void);
int n3dt_wav2lip_pack(const N3dtWav2lipParams* p, void* packed, void* stream);
size_t n3dt_wav2lip_workspace_bytes(int n);
int n3dt_wav2lip_fwd(int n, const void* packed, const float* mel_windows, const float* face_inputs, float* out, void* workspace,
                     size_t workspace_bytes, void* stream);
int n3dt_wav2lip_block(int block, int n, const void* packed, const float* in, const float* skip, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);
int n3dt_wav2lip_face_inputs(int n, int height, int width, const float* frames, const float* ref_frames, const int32_t* boxes,
                             int n_boxes, float* out, void* stream);
int n3dt_wav2lip_paste(int n, int height, int width, const float* faces, const float* frames, const int32_t* boxes, int n_boxes,
                       float* out, void* stream);

/* ---- S3FD face detector: frames to Wav2Lip crop boxes -----------------------------------
 * The reference's face_detection/detection/sfd (net_s3fd.py under detect.py, bbox.py, sfd_detector.py and api.py), frozen and
 * inference-only, with the caller's weights: 19 backbone convolutions in state-dict order (conv1_1 .. conv7_2), five 2 x 2 max
 * pools, three L2Norms and six levels' conf / loc heads (strides 4 .. 128), then scores, decode and greedy NMS in float64.
 * csrc/s3fd.hip; the table and the run-time geometry are csrc/s3fd_core.h.  Blocks for the single-block entry: 0..18 the
 * convolutions, 19..23 the pools, 24..26 the norms, 27..32 the head pairs (their stored columns: conf, then loc; no max-out).
 * weight / bias [31]: the 19 convolutions, then (conf, loc) of each level; norm_weight [3].
 * heads: x [n,3,height,width] mean-subtracted -> out[12] = cls1, reg1, .. cls6, reg6 (NCHW, cls1 after the max-out).
 * detect: frames [n,3,height,width] fp32 RGB in [0,1] (clamped, NaN -> 0; 255 u - (104, 117, 123) on R, G, B) -> dets
 *   [n,max_faces,5] float64 (x1, y1, x2, y2, score) in descending score, unused rows 0; count [n]; left [n], the positions still
 *   standing where max_faces cut the NMS short; scores [n,P] float64 or NULL.
 * boxes: dets, count of n_frames frames -> boxes [n_frames,4] int32 (y1, y2, x1, x2) from each frame's top detection: clipped at
 *   0, truncated, padded, clamped to the frame, smoothed over `smooth` frames (0: not) as the reference's get_smoothened_boxes
 *   does; found [n_frames]; a frame without a detection enters as the whole frame.  scratch: 8 n_frames int32.
 * An image's results depend on that image and the packed weights alone and are bitwise reproducible.  Everything is enqueued on
 * `stream`, nothing synchronises, no atomics.  workspace: 256-byte aligned, never cleared, contents immaterial between calls.
 * Limits (N3DT_EINVAL before anything is enqueued; the size queries return 0 and set n3dt_last_error): 32 <= height, width <=
 * 4096; 1 <= n <= the result of the max_images query (a 4 GiB workspace budget, at most 1024); 1 <= max_faces <= 64. */
#define N3DT_S3FD_PARAMS 31
#define N3DT_S3FD_BLOCKS 33
typedef struct N3dtS3fdParams {
    const float* weight[N3DT_S3FD_PARAMS];
    const float* bias[N3DT_S3FD_PARAMS];
    const float* norm_weight[3];
} N3dtS3fdParams;
size_t n3dt_s3fd_packed_bytes(void);
int n3dt_s3fd_pack(const N3dtS3fdParams* p, void* packed, void* stream);
int n3dt_s3fd_max_images(int height, int width);
int n3dt_s3fd_positions(int height, int width);
size_t n3dt_s3fd_workspace_bytes(int n, int height, int width);
int n3dt_s3fd_heads(int n, int height, int width, const void* packed, const float* x, float* const* out, void* workspace,
                    size_t workspace_bytes, void* stream);
int n3dt_s3fd_detect(int n, int height, int width, const void* packed, const float* frames, int max_faces, double* scores, double* dets,
                     int32_t* count, int32_t* left, void* workspace, size_t workspace_bytes, void* stream);
int n3dt_s3fd_boxes(int n_frames, int height, int width, int max_faces, const double* dets, const int32_t* count, int pady1, int pady2,
                    int padx1, int padx2, int smooth, int32_t* boxes, int32_t* found, int32_t* scratch, void* stream);
size_t n3dt_s3fd_block_workspace_bytes(int block, int n, int height, int width);
int n3dt_s3fd_block(int block, int n, int height, int width, const void* packed, const float* in, float* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- 3-D face reconstruction net: frames to expression codes -------------------------------------
 * The reference's net_recon (s_face3d/models/networks.py: ReconNetWrapper over resnet50, use_last_fc=False) behind the crop of
 * s_face3d/util/preprocess.py's align_img as CropAndExtract.generate calls it, frozen and inference-only, with the caller's
 * weights.  csrc/face_recon.hip; the table and the run-time geometry are csrc/face_recon_core.h.  Blocks for the single-block
 * entry: 0..52 the convolutions in state-dict order (conv1; per bottleneck conv1, conv2, conv3 and, in a layer's first,
 * downsample.0), each with its BatchNorm folded in and its ReLU (none behind a downsample); 53 the 3 x 3 / 2 max pool; 54 the
 * global average; 55 the 257-column head (the seven final_layers as one matrix: id 80, exp 64, tex 80, angle 3, gamma 27,
 * (tx, ty) 2, tz 1).
 * pack: weight[53] [C_out, C_in, k, k]; bn_weight / bn_bias / bn_mean / bn_var [53] [C_out] and bn_eps[53] (host doubles): eval-mode
 *   BatchNorm2d folded into weight and bias in float64; head_weight[7] [cols, 2048], head_bias[7] [cols].
 * fwd: x [n,3,height,width] fp32 (the reference feeds RGB in [0,1]) -> out [n,257].
 * block: in [n,C_in,height,width] -> out [n,C_out,Ho,Wo]; a bottleneck's third convolution takes the identity as skip
 *   [n,C_out,Ho,Wo] and gives relu(conv + skip), every other block takes skip = NULL; 54 gives [n,2048] and 55 takes [n,2048]
 *   (height = width = 1) and gives [n,257].
 * align: frames [n,3,height,width] fp32 RGB in [0,1] (clamped, NaN -> 0) and landmarks [n,points,2] float64 image pixels, points 68
 *   or 5 (NULL: every frame gets the fallback a frame whose landmarks average exactly -1 gets) -> crops [n,3,224,224] fp32 in
 *   [0,1], the crop align_img cuts from PIL's BICUBIC resize (quantize 1: through bytes as PIL's byte path rounds; 0: nothing
 *   rounded); trans_params [n,5] float64 (w0, h0, s, t0, t1); geom [n,4] int32 (w, h, left, up); status [n] int32, 1 for
 *   non-finite landmarks, w or h < 1 or s outside [1/16, 16] (such a frame's crop is zeros).  lm3d_std [5,3] and pinv [4,5], the
 *   pseudo-inverse of [lm3d_std, 1], float64 on the device.
 * An image's results depend on that image and the packed weights alone and are bitwise reproducible.  Everything is enqueued on
 * `stream`, nothing synchronises, no atomics.  workspace: 256-byte aligned, never cleared, contents immaterial between calls.
 * Limits (N3DT_EINVAL before anything is enqueued; the size queries return 0 and set n3dt_last_error): fwd 32 <= height, width <=
 * 4096; 1 <= n <= the result of the max_images query (a 4 GiB workspace budget, at most 1024); align 2 <= height, width <= 4096,
 * 1 <= n <= 2^20. */
#define N3DT_FACE_RECON_CONVS 53
#define N3DT_FACE_RECON_HEADS 7
#define N3DT_FACE_RECON_BLOCKS 56
#define N3DT_FACE_RECON_COEFFS 257
typedef struct N3dtFaceReconParams {
    const float* weight[N3DT_FACE_RECON_CONVS];
    const float* bn_weight[N3DT_FACE_RECON_CONVS];
    const float* bn_bias[N3DT_FACE_RECON_CONVS];
    const float* bn_mean[N3DT_FACE_RECON_CONVS];
    const float* bn_var[N3DT_FACE_RECON_CONVS];
    double bn_eps[N3DT_FACE_RECON_CONVS];
    const float* head_weight[N3DT_FACE_RECON_HEADS];
    const float* head_bias[N3DT_FACE_RECON_HEADS];
} N3dtFaceReconParams;
size_t n3dt_face_recon_packed_bytes(void);
int n3dt_face_recon_pack(const N3dtFaceReconParams* p, void* packed, void* stream);
int n3dt_face_recon_max_images(int height, int width);
size_t n3dt_face_recon_workspace_bytes(int n, int height, int width);
int n3dt_face_recon_fwd(int n, int height, int width, const void* packed, const float* x, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t n3dt_face_recon_block_workspace_bytes(int block, int n, int height, int width);
int n3dt_face_recon_block(int block, int n, int height, int width, const void* packed, const float* in, const float* skip, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);
int n3dt_face_recon_align(int n, int height, int width, const float* frames, const double* landmarks, int points, const double* lm3d_std,
                          const double* pinv, int quantize, float* crops, double* trans_params, int32_t* geom, int32_t* status,
                          void* stream);

/* ---- AWing FAN landmark detector: frames to 68 landmarks ---------------------------------------------
 * The reference's KeypointExtractor network (s_face3d/util/my_awing_arch.py: FAN over HourGlass / ConvBlock / CoordConvTh, with
 * calculate_points as get_landmarks calls it), frozen and inference-only, with the caller's weights.  csrc/fan.hip; the table, the
 * launch plan and the index rules are csrc/fan_core.h.  num_modules 1..4 stacks, num_landmarks N in 1..127.
 * Convolutions (weight[j] and its companions): 0 the stem CoordConv; 1..4 conv2's conv1, conv2, conv3, downsample.2; 5..7 conv3's;
 *   8..11 conv4's; then 47 per stack: the hourglass coordconv, 14 ConvBlocks of 3 (the hourglass's 13 in state-dict order, then
 *   top_m), conv_last, l, bl, al (the last stack has neither bl nor al: NULL).  bias[j]: the convolution's bias or NULL.  bn_*[j]:
 *   the BatchNorm in FRONT of a ConvBlock's convolution (downsample.0), or the one BEHIND the stem (bn1) and conv_last (bn_end),
 *   else NULL; eps 1e-5.  coords256 [3,256,256] and coords64 [3,64,64]: the xx, yy, rr channels as AddCoordsTh computes them in fp32.
 * Blocks of the single-block entry: 0 the stem (256 x 256 only), 1..3 the ConvBlocks conv2..conv4, 4 the 2 x 2 average pool (256
 *   channels, even sizes), 5 the upsample-add (in: the lower map; skip: the upper, twice as large); then 19 per stack: coordconv (64 x
 *   64 only; from the second stack on it takes gates [n,4096]), the 13 hourglass ConvBlocks, top_m, conv_last (+ bn_end + ReLU), l,
 *   bl (skip: previous), al (skip: previous + bl).
 * fwd: x [n,3,256,256] fp32 BGR in [0,1] -> heat [num_modules][n,N+1,64,64].  gates uint8 [n, max(num_modules-1,1), 4096]:
 *   compute_gates 1 writes clamp(previous heat map's last channel, 0, 1) > 0.05f there, 0 reads what the caller left.
 * crops: frames [n,3,height,width] fp32 RGB + boxes [n,4] int32 (y1, y2, x1, x2) -> [n,3,256,256] BGR, bilinear, half-pixel
 *   centres; a box with a negative start, an empty extent or an end outside the frame gives zeros.
 * points: heat, landmark l of frame f at heat + f * frame_stride + l * 4096, -> pts [n,N,2] float64 (x, y) in heat-map cells and
 *   status [n] (2: a landmark's argmax is cell 4095, where the reference raises IndexError; the frame's points are -1).
 * tail: pts, that status and the boxes -> out [n,P,2] float64 image pixels and status (| 4 for a bad box; such a frame is -1).
 *   table [P][2] int32 NOT NULL: P output points, each the mean of two of the N rounded to fp32, the origin added in fp32; NULL:
 *   P = N, float64 throughout.  carry 1: a failed frame takes the last frame before it that did not fail.
 * An image's results depend on that image, its gates and the packed weights alone and are bitwise reproducible.  Everything is
 * enqueued on `stream`, nothing synchronises, no atomics.  workspace: 256-byte aligned, never cleared. */
#define N3DT_FAN_MAX_CONVS 200
#define N3DT_FAN_MAX_BLOCKS 82
typedef struct N3dtFanParams {
    int32_t num_modules, num_landmarks;
    const float* weight[N3DT_FAN_MAX_CONVS];
    const float* bias[N3DT_FAN_MAX_CONVS];
    const float* bn_weight[N3DT_FAN_MAX_CONVS];
    const float* bn_bias[N3DT_FAN_MAX_CONVS];
    const float* bn_mean[N3DT_FAN_MAX_CONVS];
    const float* bn_var[N3DT_FAN_MAX_CONVS];
    const float* coords256;
    const float* coords64;
} N3dtFanParams;
size_t n3dt_fan_packed_bytes(int num_modules, int num_landmarks);
int n3dt_fan_pack(const N3dtFanParams* p, void* packed, void* stream);
int n3dt_fan_max_images(int num_modules, int num_landmarks);
size_t n3dt_fan_workspace_bytes(int num_modules, int num_landmarks, int n);
int n3dt_fan_fwd(int num_modules, int num_landmarks, int end_relu, int n, const void* packed, const float* x, int compute_gates,
                 uint8_t* gates, float* heat, void* workspace, size_t workspace_bytes, void* stream);
size_t n3dt_fan_block_workspace_bytes(int block, int num_modules, int num_landmarks, int n, int height, int width);
int n3dt_fan_block(int block, int num_modules, int num_landmarks, int end_relu, int n, int height, int width, const void* packed,
                   const float* in, const float* skip, const uint8_t* gates, float* out, void* workspace, size_t workspace_bytes,
                   void* stream);
int n3dt_fan_crops(int n, int height, int width, const float* frames, const int32_t* boxes, float* out, void* stream);
int n3dt_fan_points(int n, int num_landmarks, const float* heat, int64_t frame_stride, double* pts, int32_t* status, void* stream);
int n3dt_fan_tail(int n, int num_landmarks, int points_out, int height, int width, const double* pts, const int32_t* decode_status,
                  const int32_t* boxes, const int32_t* table, int carry, double* out, int32_t* status, void* stream);

/* ---- head-mask generator: BiSeNet parsing to head and eye masks ---------------------------------------
 * The reference's DataProcess/Gen_HeadMask.py: BiSeNet(n_classes) over DataProcess/resnet.py's ResNet-18, frozen and
 * inference-only, with the caller's weights, then argmax, LUT, largest component, hair erosion, largest component, green-screen
 * filter and the dilated eye mask, on byte maps.  csrc/head_mask.hip; the table, the run-time geometry and the index rules are
 * csrc/head_mask_core.h.  n_classes 1..32; any image 32..4096 high and wide.
 * Convolutions (weight[j]; bn_*[j] the BatchNorm behind it or NULL; eps 1e-5 unless bn_eps says otherwise), state-dict order:
 *   0 cp.resnet.conv1; then per BasicBlock conv1, conv2 and (layer2..4, block 0) downsample.0: 1..4 layer1, 5..9 layer2, 10..14
 *   layer3, 15..19 layer4; 20, 21 cp.arm16's conv, conv_atten; 22, 23 cp.arm32's; 24 cp.conv_head32; 25 cp.conv_head16; 26
 *   cp.conv_avg; 27..29 ffm's convblk, conv1, conv2; 30, 31 conv_out's conv, conv_out; 32, 33 conv_out16's; 34, 35 conv_out32's.
 * Blocks of the single-block entry: the 36 convolutions, then 36 the max pool.  A spatial block takes in [n,C_in,src_height,
 *   src_width], read as a height x width map through torch's nearest rule, and gives [n,C_out,Ho,Wo]; aux is the shortcut
 *   [n,C_out,Ho,Wo] of a BasicBlock's conv2 (required there), the second 128 channels of block 27's input (required), or, with
 *   scale on block 25, a map [n,128,src_height,src_width] added behind the scale.  scale, addvec [n,C_in] (blocks 24, 25, 30
 *   only, 16-byte aligned): the fetched value v becomes v * scale + (addvec | aux | v on block 30 | 0).  The five small blocks (21,
 *   23, 26, 28, 29) average in [n,C_in,height,width] and give [n,C_out] through the 1 x 1 convolution in float64.
 * fwd: x [n,3,height,width] fp32, normalised -> for bit o of `outputs` (1 out, 2 out16, 4 out32) the map at out / out16 / out32:
 *   [n,n_classes,h,w] low-resolution logits (h, w: 1/8, 1/8 and 1/16 by the convolutions' floor rules), or with `upsample`
 *   [n,n_classes,height,width], bilinear with align_corners.  Only the convolutions the selected outputs need are run.
 * frames: bytes [n,height,width,3] RGB, or (frames_are_float) fp32 [n,3,height,width] in [0,1] rounded once -> rgb bytes
 *   [n,height,width,3] and x = (byte / 255 - mean) / std with the ImageNet constants, fp32.
 * resize: bytes [n,src_height,src_width,channels] -> [n,height,width,channels], bilinear with half-pixel centres in float64, rounded
 *   to the nearest byte; OpenCV's fixed-point INTER_LINEAR is not reproduced.
 * labels: logits [n,n_classes,h,w] -> uint8 [n,height,width]: argmax of the align_corners interpolation, float64, first maximum.
 * green: rgb -> 255 where OpenCV's 8-bit hue of the bytes taken as (B, G, R) lies in hue_lo..hue_hi, else 0.
 * postprocess: labels, rgb, lut [256], element [elem_h, elem_w] anchored at (anchor_y, anchor_x) -> head, eye [n,height,width]
 *   in {0, 255}.  Integer atomics only; the result does not depend on scheduling.
 * Everything is enqueued on `stream`, nothing synchronises.  Workspaces: 256-byte aligned, caller-owned, never cleared; their
 * contents do not matter. */
#define N3DT_HEAD_MASK_CONVS 36
#define N3DT_HEAD_MASK_BLOCKS 37
#define N3DT_HEAD_MASK_MAX_CLASSES 32
typedef struct N3dtHeadMaskParams {
    int32_t n_classes, reserved;
    const float* weight[N3DT_HEAD_MASK_CONVS];
    const float* bn_weight[N3DT_HEAD_MASK_CONVS];
    const float* bn_bias[N3DT_HEAD_MASK_CONVS];
    const float* bn_mean[N3DT_HEAD_MASK_CONVS];
    const float* bn_var[N3DT_HEAD_MASK_CONVS];
    double bn_eps;
} N3dtHeadMaskParams;
size_t n3dt_head_mask_packed_bytes(void);
int n3dt_head_mask_pack(const N3dtHeadMaskParams* p, void* packed, void* stream);
int n3dt_head_mask_max_images(int height, int width);
size_t n3dt_head_mask_workspace_bytes(int n, int height, int width);
int n3dt_head_mask_fwd(int n, int height, int width, int n_classes, const void* packed, const float* x, int outputs, int upsample,
                       float* out, float* out16, float* out32, void* workspace, size_t workspace_bytes, void* stream);
size_t n3dt_head_mask_block_workspace_bytes(int block, int n, int height, int width, int src_height, int src_width);
int n3dt_head_mask_block(int block, int n, int height, int width, int src_height, int src_width, int n_classes, const void* packed,
                         const float* in, const float* aux, const float* scale, const float* addvec, float* out, void* workspace,
                         size_t workspace_bytes, void* stream);
int n3dt_head_mask_frames(int n, int height, int width, const void* frames, int frames_are_float, uint8_t* rgb, float* x,
                          void* stream);
int n3dt_head_mask_resize(int n, int src_height, int src_width, int channels, const uint8_t* src, int height, int width, uint8_t* dst,
                          void* stream);
int n3dt_head_mask_labels(int n, int n_classes, int h, int w, int height, int width, const float* logits, uint8_t* labels,
                          void* stream);
int n3dt_head_mask_green(int n, int height, int width, const uint8_t* rgb, int hue_lo, int hue_hi, uint8_t* cleared, void* stream);
size_t n3dt_head_mask_postprocess_workspace_bytes(int n, int height, int width);
int n3dt_head_mask_postprocess(int n, int height, int width, const uint8_t* labels, const uint8_t* rgb, const uint8_t* lut,
                               const uint8_t* element, int elem_h, int elem_w, int anchor_y, int anchor_x, int dilations, int erosions,
                               int hue_lo, int hue_hi, uint8_t* head, uint8_t* eye, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---- fused loss tail -----------------------------------------------------------------
 * The three MSE data terms of the reference's loss (Utils/HeadNeRFLossUtils.py:125-146: bg_loss, head_loss,
 * nonhead_loss, including its nan_to_num) in one pass, and their gradient in one more; replaces three boolean-mask
 * gathers.  merge_img, gt [B,3,P,P]; bg_img [1,3,P,P]; mask [B,1,P,P] (head where >= 0.5); pixels = P*P.
 * n3dt_loss_fwd writes terms[4] = {bg, head, nonhead, (bg + head) + nonhead -- the reference's total, :228-231} and keeps
 * its sums/counts in acc[8] for n3dt_loss_bwd, which takes the upstream gradients g[3] of the three terms and / or g_total[1]
 * of their sum (each nullable, not both) and writes d_merge [B,3,P,P] and d_bg [1,3,P,P].  (ABI 4: acc grew from 6 to 8
 * floats, terms from 3 to 4, g_total is new.) */
int n3dt_loss_fwd(int batch, int pixels, const float* merge_img, const float* bg_img, const float* gt, const float* mask,
                  float bg_value, float* acc, float* terms, void* stream);
int n3dt_loss_bwd(int batch, int pixels, const float* merge_img, const float* bg_img, const float* gt, const float* mask,
                  float bg_value, const float* acc, const float* g, const float* g_total, float* d_merge, float* d_bg, void* stream);

/* ---- VGG16 perceptual loss term (Utils/HeadNeRFLossUtils.py:23-64, 140-154) --------------------------------------------
 * The fourth data term of the reference's objective: input = nan_to_num(merge_img), target = gt with bg_value wherever
 * mask < 0.5, both ImageNet-normalised and resized to 224^2 (bilinear, align_corners=False), through torchvision
 * vgg16().features[:23] in four blocks [:4] [4:9] [9:16] [16:23]; the term is the sum over blocks of mean |f_b(x) - f_b(y)|.
 * The VGG weights are frozen: the backward produces d_merge only.
 *   n3dt_vgg_pack      re-lays the ten convs' fp32 weights (weight[l] [C_out, C_in, 3, 3], bias[l] [C_out], torchvision order)
 *                      into MFMA fragment order, forward and transposed-flipped (input gradient); once per weight set
 *   n3dt_vgg_loss_fwd  merge_img, gt [B,3,P,P], mask [B,1,P,P] (NULL: gt is used as given) -> terms[5] = the four block
 *                      terms and their sum ((t0 + t1) + t2) + t3; keeps the activations in `saved` for the backward
 *   n3dt_vgg_loss_bwd  g_total [1] (device) = dL/d(sum) -> d_merge [B,3,P,P] (overwritten; 0 where merge_img is not finite);
 *                      `saved` from the forward with the same batch, img_size, precision and packed weights
 * precision N3DT_F32 (split-bf16 operands, three products: ~16 mantissa bits) or N3DT_BF16; 1 <= batch <= 64,
 * 16 <= img_size <= 2048.
 * n3dt_vgg_conv_stage runs ONE conv of the table (layer 0..9) on the caller's buffers at the geometry the caller names, through the
 * launch path of the two calls above and the pack of n3dt_vgg_pack (a debugging aid: the tests judge the conv kernel one layer at
 * a time with it).  All maps are NHWC fp32.
 *   dgrad 0  in [n_img, H+2, W+2, C_in] with a zero halo -- for the layers that follow a 2x2 max-pool (2, 4, 7) the UN-pooled
 *            [n_img, 2H+2, 2W+2, C_in] -- -> out = ReLU(conv + bias) [n_img, H, W, C_out]; gate must be NULL
 *   dgrad 1  in [n_img, H+2, W+2, C_out] with a zero halo (the gradient of the layer's output) -> out [n_img, H, W, C_in], the
 *            gradient of its input; gate (or NULL) has out's layout, out is kept where gate > 0 and is 0 elsewhere
 *   out_pad 1: out is [n_img, H+2, W+2, C] and only its interior is written (the caller owns the halo); 0: no halo.
 * Image i's result depends on image i and the pack alone, not on n_img; bit-reproducible.  1 <= n_img <= 128, 1 <= H, W <= 224; in,
 * gate and out 16-byte, packed 256-byte aligned. */
#define N3DT_VGG_CONVS 10   /* torchvision vgg16().features indices 0,2,5,7,10,12,14,17,19,21 */
typedef struct N3dtVggParams {
    const float* weight[N3DT_VGG_CONVS];
    const float* bias[N3DT_VGG_CONVS];
} N3dtVggParams;
size_t n3dt_vgg_packed_bytes(int precision);
int n3dt_vgg_pack(int precision, const N3dtVggParams* p, void* packed, void* stream);
size_t n3dt_vgg_saved_bytes(int batch, int precision);
size_t n3dt_vgg_workspace_bytes(int batch, int img_size, int precision);
int n3dt_vgg_loss_fwd(int batch, int img_size, int precision, const void* packed, const float* merge_img, const float* gt,
                      const float* mask, float bg_value, float* terms, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                      void* stream);
int n3dt_vgg_loss_bwd(int batch, int img_size, int precision, const void* packed, const float* merge_img, const float* g_total,
                      const void* saved, size_t saved_bytes, float* d_merge, void* ws, size_t ws_bytes, void* stream);
int n3dt_vgg_conv_stage(int precision, const void* packed, int layer, int dgrad, int n_img, int H, int W, const float* in,
                        const float* gate, float* out, int out_pad, void* stream);

/* ---- Audio2style encoder (talker_trainer.py:407-461) ------------------------------------------------------------------
 * mel [T, 1280] (each frame's 80x16 window, row-major) is ONE sequence of T frames through
 * nn.LSTM(1280, 640, num_layers=2, bidirectional=True) (h0 = c0 = 0, gate order i, f, g, o), then
 * out = drop(lrelu(drop(lrelu(drop(lrelu(H W1^T + b1)) W2^T + b2)) W3^T + b3)) -> [T, 64], lrelu slope 0.2.
 * Dropout (p = 0.5): masks[k] are keep masks of 0 / 1 ([T,640], [T,320], [T,64]); a kept value is scaled by 2.  masks NULL:
 * no dropout (eval).  fp32 throughout.  1 <= T <= 256.
 *   n3dt_a2s_fwd  -> out [T, 64]; keeps what the backward needs in `saved` (mel included)
 *   n3dt_a2s_bwd  g_out [T, 64] -> every parameter gradient, OVERWRITTEN, into grad_arena (layout below); no input gradient.
 *                 No atomics, no split-K: the result is bitwise reproducible.
 * Parameter index k = 2 * layer + direction (weight_ih_l0, _l0_reverse, _l1, _l1_reverse).  The grad arena holds, each
 * contiguous and in this order (the state-dict order without RNNModel.fc1, which forward never reads):
 *   for k in 0..3: dW_ih[k] [2560, 1280], dW_hh[k] [2560, 640], db_ih[k] [2560], db_hh[k] [2560];
 *   then dW1 [640, 1280], db1 [640], dW2 [320, 640], db2 [320], dW3 [64, 320], db3 [64]. */
#define N3DT_A2S_IN 1280
#define N3DT_A2S_HIDDEN 640
#define N3DT_A2S_OUT 64
#define N3DT_A2S_MAX_T 256
#define N3DT_A2S_GRAD_FLOATS 20726784
typedef struct N3dtA2sParams {
    const float* w_ih[4];  /* [2560, 1280] */
    const float* w_hh[4];  /* [2560, 640] */
    const float* b_ih[4];  /* [2560] */
    const float* b_hh[4];  /* [2560] */
    const float* lin_w[3]; /* linear1.0 [640, 1280], linear2.0 [320, 640], linear3.0 [64, 320] */
    const float* lin_b[3];
} N3dtA2sParams;
size_t n3dt_a2s_saved_bytes(int T);
size_t n3dt_a2s_workspace_bytes(int T);
int n3dt_a2s_fwd(int T, const N3dtA2sParams* p, const float* mel, const float* mask1, const float* mask2, const float* mask3,
                 float* out, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, void* stream);
int n3dt_a2s_bwd(int T, const N3dtA2sParams* p, const float* g_out, const void* saved, size_t saved_bytes, float* grad_arena,
                 void* ws, size_t ws_bytes, void* stream);

/* ---- FlatAdam: torch.optim.Adam's step (amsgrad = False) for any number of tensors in ONE launch ------------------
 * The reference ends its step with two torch.optim.Adam steps (talker_trainer.py:722-727, 1063-1067).  The caller lays the
 * work out once per layout in device memory:
 *   tensor table  N3dtAdamTensor[n]: the four fp32 pointers of a tensor (any 4-byte alignment), numel, its group and an
 *                 "active" flag (0: the parameter has no gradient this step -- value and state stay as they are);
 *   chunk table   N3dtAdamChunk[n_chunks]: (tensor, start element, length); the chunks tile every tensor exactly once and
 *                 none crosses a tensor;
 *   group table   N3dtAdamGroup[n_groups <= N3DT_ADAM_MAX_GROUPS]: hyper-parameters as doubles, read from device memory at
 *                 every launch (a replayed graph follows a copy into it);
 *   step counter  int32[N3DT_ADAM_COUNTER_INTS], zeroed once by the caller: [0] = steps taken (the kernel uses t = [0] + 1
 *                 and adds 1 once per launch, after every read), [1] = the kernel's own completion counter.
 * n3dt_flat_adam_record_bytes(which): sizeof of the tensor (0), chunk (1) and group (2) record, 0 for anything else. */
#define N3DT_ADAM_MAX_GROUPS 64
#define N3DT_ADAM_MAX_GRID 1024
#define N3DT_ADAM_COUNTER_INTS 4
typedef struct N3dtAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    int32_t group;
    int32_t active;
} N3dtAdamTensor;
typedef struct N3dtAdamChunk {
    int64_t start;
    int32_t tensor;
    int32_t length;
} N3dtAdamChunk;
typedef struct N3dtAdamGroup {
    double lr, beta1, beta2, eps, weight_decay;
    int32_t maximize;
    int32_t reserved;
} N3dtAdamGroup;
size_t n3dt_flat_adam_record_bytes(int which);
int n3dt_flat_adam_step(const void* tensor_table, const void* chunk_table, int n_chunks, const void* group_table, int n_groups,
                        void* step_counter, void* stream);
/* the guarded step (global-norm clipping, non-finite step skipping, both decided on the device): N3dtAdamGuard and its two
 * entry points, on the same tables */
#include "n3dt_flat_adam_guard.h"

/* [C, N_r] (NCHW parameter) -> [N_r, C]; used to feed bg_featmap to the renderer */
int n3dt_chw_to_hwc(int C, int n, const float* src, float* dst, void* stream);

/* ---- per-call host overhead: input staging + hipGraph replay ----------------------------------------
 * The reference's call shapes are small batches (validation B=1 talker_trainer.py:1119, fitting B=1 x 300 iterations
 * FittingSingleImage_new.py:887): a forward is ~17 short kernels and launch gaps are a quarter of the step.  Every entry
 * point above allocates nothing and only enqueues on `stream`, so a whole forward can be recorded once into a hipGraph
 * and replayed with ONE launch.  A replay reads the addresses recorded at capture time: the caller keeps static
 * buffers and refreshes them with n3dt_stage_inputs (one small kernel instead of one copy per tensor).
 *
 * n3dt_stage_inputs: n <= N3DT_STAGE_MAX copies src[i] -> dst[i] of count[i] floats in one launch.  Entry 0 may be a
 * strided 3-D view (batch_xy [B,2,N_r] with the strides the caller holds it in, e.g. an expand()ed grid): set
 * view_dims / view_strides (elements) and count[0] = product of view_dims; leave view_dims[0] = 0 for a flat copy. */
#define N3DT_STAGE_MAX 12
typedef struct N3dtStageCopy {
    const float* src[N3DT_STAGE_MAX];
    float* dst[N3DT_STAGE_MAX];
    int64_t count[N3DT_STAGE_MAX];
    int64_t view_dims[3], view_strides[3];
    int32_t n;
} N3dtStageCopy;
int n3dt_stage_inputs(const N3dtStageCopy* st, void* stream);

/* hipStreamBeginCapture (relaxed mode: other threads / streams are unaffected) ... hipStreamEndCapture +
 * hipGraphInstantiate.  Between begin and end, enqueue the n3dt_* calls of one forward on `stream`; nothing runs until
 * n3dt_graph_launch.  *graph_out is an opaque handle owned by the library until n3dt_graph_destroy. */
int n3dt_graph_begin(void* stream);
int n3dt_graph_end(void* stream, void** graph_out);
int n3dt_graph_launch(void* graph, void* stream);
int n3dt_graph_destroy(void* graph);

/* ---- measurement hook (bench.py only) ---------------------------------------------------------
 * While enabled, every n3dt_render_fwd brackets its fused MLP kernel launch (the roofline kernel,
 * not the fold / head kernels around it) with a hipEvent pair on the caller's stream.
 * n3dt_prof_collect synchronises those events and returns each launch's duration in ms.
 * Process-global and opt-in: the only mutable global state in the library; not for use while
 * other threads are rendering. */
int n3dt_prof_enable(int max_records);  /* 0 disables and frees the events */
int n3dt_prof_collect(float* ms_out, int capacity, int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* N3DT_API_H_ */
