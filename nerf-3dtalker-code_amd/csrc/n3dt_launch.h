// The one declaration of every function that crosses a translation unit inside libn3dt.so: the kernel launchers, the layout /
// size helpers the entry points of n3dt_api.hip call, and the measurement spans.  Internal: not installed, not part of the ABI.
// All of them are extern "C", whose names carry no types: a prototype that disagrees with its definition would link and pass
// its arguments in the wrong registers.  So every .hip / .inc that defines or calls one includes this header, and the compiler
// holds each definition to it ("conflicting types").  A new launcher is declared here and nowhere else.
// (The row-major weight-gradient front end keeps its own header, dw_rowmajor.h; n3dt_gemm32 / n3dt_gemm are C++, in gemm32.h.)
#pragma once
#include <stddef.h>
#include <hip/hip_runtime.h>

#include "../../include/n3dt.h"

struct MelSignal;  // mel_core.h

extern "C" {
// ---- n3dt_api.hip: the opt-in measurement hook's spans
int n3dt_prof_span_begin(hipStream_t s);
void n3dt_prof_span_end(int slot, hipStream_t s);

// ---- nerf_aux.hip
void n3dt_launch_small_gemm(int M, int N, int K, const float* A, long sam, long sak, const float* B, long sbn, long sbk, float* C, long ldc,
                            int accumulate, hipStream_t s);
void n3dt_launch_pack(const N3dtGeom* g, int precision, const N3dtMlpParams* p, void* packed, hipStream_t stream);
void n3dt_launch_fold(const N3dtGeom* g, const N3dtMlpParams* p, const float* shape, const float* appea, const float* audio, float* fold,
                      int merged_rgb, hipStream_t stream);
void n3dt_launch_rayfold(const N3dtGeom* g, const float* fold, const float* ray_bias, hipStream_t s);
void n3dt_launch_ray_vd_bias(const N3dtGeom* g, const float* w_vd, long ld_w, const float* xy, const float* R, const float* Kinv,
                             float* ray_bias, hipStream_t s);
void n3dt_launch_ray_head(const N3dtGeom* g, int bpr, int bs, const float* part, const float* wlocal, const float* tail,
                          const float* bg_featmap, int bg_hwc, float* fg_feat, float* bg_alpha, float* depth, float* weight,
                          float* merge_feat, hipStream_t stream);
void n3dt_launch_ray_head_mfma(const N3dtGeom* g, int bpr, int bs, const float* part, const float* wlocal, const float* tail,
                               const float* bg_featmap, int bg_hwc, float* fg_feat, float* bg_alpha, float* depth, float* weight,
                               float* merge_feat, float* rayrec, hipStream_t stream);
void n3dt_launch_ray_head_mfma16(const N3dtGeom* g, int bpr, int bs, const float* part, const float* wlocal, const float* tail,
                                 const float* bg_featmap, int bg_hwc, float* fg_feat, float* bg_alpha, float* depth, float* weight,
                                 float* merge_feat, void* merge16, int prec16, float* rgb0, const float* rgb_w, const float* rgb_b,
                                 hipStream_t stream);
void n3dt_launch_ray_head_rec(const N3dtGeom* g, int bpr, int bs, const float* part, const float* wlocal, const float* tail,
                              const float* bg_featmap, float* fg_feat, float* bg_alpha, float* depth, float* weight, float* merge_feat,
                              float* rayrec, hipStream_t stream);
void n3dt_launch_chw_to_hwc(int C, int n, const float* src, float* dst, hipStream_t stream);
void n3dt_launch_fine_sample(const N3dtGeom* g, int n_fine, const float* weight, const float* T, const float* t_rand, const float* u,
                             float* z_planes, hipStream_t stream);
void n3dt_launch_stage(const N3dtStageCopy* st, hipStream_t stream);

// ---- nerf_fwd_f32.hip, nerf_fwd_x16.hip, nerf_fwd_x16s.hip: the fused MLP kernel
void n3dt_launch_nerf_fwd_f32(const N3dtGeom* g, const N3dtMlpParams* prm, const void* packed, const float* fold, const float* xy,
                              const float* R, const float* T, const float* Kinv, const float* t_rand, float* part, float* wlocal,
                              hipStream_t stream);
void n3dt_launch_nerf_fwd_x16(const N3dtGeom* g, int precision, const void* packed, const float* fold, const float* xy, const float* R,
                              const float* T, const float* Kinv, const float* t_rand, float* part, float* wlocal, hipStream_t stream);
void n3dt_launch_nerf_fwd_x16_train(const N3dtGeom* g, const void* packed, const float* fold, const float* xy, const float* R,
                                    const float* T, const float* Kinv, const float* t_rand, float* part, float* wlocal, void* xT, void* gS,
                                    float* geo, void* gates, hipStream_t stream);
void n3dt_launch_nerf_fwd_x16s(const N3dtGeom* g, const void* packed, const float* fold, const float* xy, const float* R, const float* T,
                               const float* Kinv, const float* t_rand, float* part, float* wlocal, hipStream_t stream);

// ---- seams.hip
void n3dt_launch_sample_points(const N3dtGeom* g, const float* xy, const float* R, const float* T, const float* Kinv, const float* t_rand,
                               float* pts, float* zvals, float* z_dists, float* ray_d, float* ray_l, hipStream_t s);
void n3dt_launch_embed(int B, size_t M, const float* pts, float* pe, hipStream_t s);
void n3dt_launch_embed_freqs(int B, size_t M, int n_freqs, const float* pts, float* pe, hipStream_t s);
size_t n3dt_seam_mlp_ws_floats(const N3dtGeom* g, size_t M);
void n3dt_launch_mlp_points(const N3dtGeom* g, size_t M, const N3dtMlpParams* p, const float* audio, const float* vps, const float* vds,
                            float* rgb, float* density, float* ws, hipStream_t s);
void n3dt_launch_composite(int B, int Nr, int Ns, int C, const float* rgb, const float* density, const float* z_dists, const float* zvals,
                           float* feat, float* bg_alpha, float* depth, float* weight, hipStream_t s);
void n3dt_launch_x16_pe_probe(int precision, int form, size_t n, const float* points, unsigned short* out, hipStream_t s);
void n3dt_launch_x16_pack_probe(int precision, int form, size_t n, const float* in, unsigned short* out, hipStream_t s);

// ---- neural_render.hip, neural_render_x16.inc
size_t n3dt_nr_workspace_floats(const N3dtGeom* g, int nb);
void n3dt_launch_feat_to_rgb0(int nb, int n_pix, const float* featmap, const float* w, const float* b, float* rgb0, hipStream_t s);
void n3dt_launch_neural_render16(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const void* featmap16,
                                 const float* rgb0, float* img, float* ws, hipStream_t s);
void n3dt_launch_neural_render(const N3dtGeom* g, int nb, int precision, const N3dtRenderParams* p, const float* featmap, float* img,
                               float* ws, int pack_mode, hipStream_t s);
void n3dt_launch_nr_train16_fwd(const N3dtGeom* g, int nb, const N3dtRenderParams* p, const float* featmap, float* img,
                                unsigned char* saved, unsigned char* ws, hipStream_t s);
void n3dt_launch_gemm_regions_bf16(int M, int N, int K, int n_regions, const void* const* base, const int* width, const int* ld,
                                   const float* Wt, const void* gate, void* y, hipStream_t s);
void n3dt_launch_conv1x1_bwd_bf16(int M, int N, int K, const void* dy, const float* Wt, int mode, const void* res, void* y, hipStream_t s);
void n3dt_launch_conv1x1_bf16(int M, int N, int K, const void* x, int x_is_16, const float* Wt, const float* bias, float slope, void* y,
                              hipStream_t s);

// ---- train_mlp.hip, train_x16.inc: the volumetric training path
size_t n3dt_train_saved_floats(const N3dtGeom* g);
size_t n3dt_train_ws_floats(const N3dtGeom* g);
void n3dt_launch_train_fwd(const N3dtGeom* g, const N3dtMlpParams* p, const float* tail, const float* xy, const float* R, const float* T,
                           const float* Kinv, const float* shape, const float* appea, const float* audio, const float* t_rand,
                           const float* bg_featmap, float* fg_feat, float* bg_alpha, float* depth, float* merge_feat, float* saved, float* ws,
                           const float* ray_bias, hipStream_t s);
void n3dt_launch_train_bwd(const N3dtGeom* g, const N3dtMlpParams* p, const N3dtMlpGrads* gp, const float* shape, const float* appea,
                           const float* audio, const float* bg_featmap, const float* d_merge, const float* d_fg, const float* d_ba,
                           const float* saved, float* d_bg_featmap, float* d_shape, float* d_appea, float* d_audio, const float* xy,
                           const float* Rm, const float* Tv, const float* Kinv, const float* t_rand, float* d_R, float* d_T, float* d_Kinv,
                           float* d_xy, float* ws, float* d_ray_bias, hipStream_t s);
size_t n3dt_train16_saved_bytes(const N3dtGeom* g);
size_t n3dt_train16_ws_bytes(const N3dtGeom* g);
void n3dt_launch_train16_fwd(const N3dtGeom* g, const N3dtMlpParams* p, const void* packed_bf16, const float* tail, const float* xy,
                             const float* R, const float* T, const float* Kinv, const float* shape, const float* appea, const float* audio,
                             const float* t_rand, const float* bg_featmap, float* fg_feat, float* bg_alpha, float* depth, float* merge_feat,
                             void* saved, void* wsv, const float* ray_bias, hipStream_t s);
void n3dt_launch_train16_bwd(const N3dtGeom* g, const N3dtMlpParams* p, const N3dtMlpGrads* gp, const float* shape, const float* appea,
                             const float* audio, const float* bg_featmap, const float* d_merge, const float* d_fg, const float* d_ba,
                             const void* saved, float* d_bg_featmap, float* d_shape, float* d_appea, float* d_audio, const float* xy,
                             const float* Rm, const float* Tv, const float* Kinv, const float* t_rand, float* d_R, float* d_T,
                             float* d_Kinv, float* d_xy, void* wsv, float* d_ray_bias, hipStream_t s);

// ---- train_nr.hip: the 2-D renderer's training path
size_t n3dt_nr_train_saved_floats(const N3dtGeom* g, int nb);
size_t n3dt_nr_train_ws_floats(const N3dtGeom* g, int nb);
size_t n3dt_nr_train16_saved_bytes(const N3dtGeom* g, int nb);
size_t n3dt_nr_train16_ws_bytes(const N3dtGeom* g, int nb);
void n3dt_launch_nr_train_fwd(const N3dtGeom* g, int nb, const N3dtRenderParams* p, const float* featmap, float* img, float* saved,
                              float* ws, int bf16, hipStream_t s);
void n3dt_launch_nr_bwd(const N3dtGeom* g, int nb, const N3dtRenderParams* p, const N3dtRenderGrads* gp, const float* featmap,
                        const float* d_img, const float* saved, float* d_featmap, float* ws, int bf16, hipStream_t s);

// ---- loss_tail.hip
void n3dt_launch_img_to_uint8(int V, int HW, const float* img, unsigned char* out, hipStream_t s);
void n3dt_launch_loss_fwd(int B, int HW, const float* merge, const float* bg, const float* gt, const float* mask, float v, float* acc,
                          float* terms, hipStream_t s);
void n3dt_launch_loss_bwd(int B, int HW, const float* merge, const float* bg, const float* gt, const float* mask, float v, const float* acc,
                          const float* g, const float* g_total, float* d_merge, float* d_bg, hipStream_t s);

// ---- vgg_loss.hip
size_t n3dt_vgg_packed_layout_bytes(int precision);
size_t n3dt_vgg_saved_floats(int batch);
size_t n3dt_vgg_ws_floats(int batch);
void n3dt_launch_vgg_pack(int precision, const N3dtVggParams* p, void* packed, hipStream_t st);
void n3dt_launch_vgg_fwd(int batch, int P, int precision, const void* packed, const float* merge, const float* gt, const float* mask,
                         float bg, float* terms, void* saved, void* ws, hipStream_t st);
void n3dt_launch_vgg_bwd(int batch, int P, int precision, const void* packed, const float* merge, const float* g_total, const void* saved,
                         float* d_merge, void* ws, hipStream_t st);
void n3dt_launch_vgg_conv_stage(int precision, const void* packed, int l, int dgrad, int n_img, int H, int W, const float* in,
                                const float* gate, float* out, int out_pad, hipStream_t st);

// ---- audio_lstm.hip
size_t n3dt_a2s_saved_floats(int T);
size_t n3dt_a2s_ws_floats(int T);
void n3dt_launch_a2s_fwd(int T, const N3dtA2sParams* p, const float* mel, const float* const masks[3], float* out, void* saved, void* ws,
                         hipStream_t st);
void n3dt_launch_a2s_bwd(int T, const N3dtA2sParams* p, const float* g_out, const void* saved, float* arena, void* ws, hipStream_t st);

// ---- flat_adam.hip
void n3dt_launch_flat_adam(const void* tensors, const void* chunks, int n_chunks, const void* groups, int n_groups, void* counter,
                           hipStream_t stream);
void n3dt_launch_flat_adam_guarded(const void* tensors, const void* chunks, int n_chunks, const void* groups, int n_groups, void* counter,
                                   void* partials, void* guard, hipStream_t stream);

// ---- eval_metrics.hip, lpips.hip
size_t n3dt_eval_metrics_ws_bytes(int n_images, int height, int width);
void n3dt_launch_eval_metrics(int n_images, int height, int width, const float* pred, const float* gt, double* ssim, double* psnr,
                              void* workspace, hipStream_t stream);
size_t n3dt_lpips_packed_layout_bytes(void);
size_t n3dt_lpips_ws_bytes(int batch, int height, int width);
void n3dt_launch_lpips_pack(const N3dtLpipsParams* p, void* packed, hipStream_t st);
void n3dt_launch_lpips(int batch, int height, int width, int input_mode, const void* packed, const float* pred, const float* gt,
                       double* out, double* layers, void* workspace, hipStream_t st);

// ---- mel.hip
size_t n3dt_mel_ws_bytes(void);
void n3dt_launch_mel_spectrogram(const MelSignal* sig, long long first_frame, int n_frames, const float* basis, const double* table,
                                 void* out, long long out_ld, int out_is_f64, void* workspace, hipStream_t stream);
void n3dt_launch_mel_windows(const void* mel, long long T, long long mel_ld, int mel_is_f64, const int* start, int n_windows, float* out,
                             hipStream_t stream);

// ---- syncnet.hip
size_t n3dt_syncnet_packed_layout_bytes(void);
size_t n3dt_syncnet_ws_bytes(int n);
float* n3dt_syncnet_ws_faces(int n, void* workspace);
void n3dt_launch_syncnet_pack(const N3dtSyncnetParams* p, void* packed, hipStream_t st);
void n3dt_launch_syncnet_faces(int n, int height, int width, const float* frames, const int* boxes, int box_stride, float* faces,
                               hipStream_t st);
void n3dt_launch_syncnet_fwd(int n, const void* packed, const float* mel, const float* faces, float* audio_emb, float* face_emb,
                             double* cosv, void* workspace, hipStream_t st);
void n3dt_launch_syncnet_block(int block, int n, const void* packed, const float* in, float* out, void* workspace, hipStream_t st);

// ---- wav2lip.hip
size_t n3dt_wav2lip_packed_layout_bytes(void);
size_t n3dt_wav2lip_ws_bytes(int n);
void n3dt_launch_wav2lip_pack(const N3dtWav2lipParams* p, void* packed, hipStream_t st);
void n3dt_launch_wav2lip_face_inputs(int n, int height, int width, const float* frames, const float* ref_frames, const int* boxes,
                                     int box_stride, float* out, hipStream_t st);
void n3dt_launch_wav2lip_paste(int n, int height, int width, const float* faces, const float* frames, const int* boxes, int box_stride,
                               float* out, hipStream_t st);
void n3dt_launch_wav2lip_fwd(int n, const void* packed, const float* mel, const float* faces, float* out, void* workspace, hipStream_t st);
void n3dt_launch_wav2lip_block(int block, int n, const void* packed, const float* in, const float* skip, float* out, void* workspace,
                               hipStream_t st);

// ---- s3fd.hip
size_t n3dt_s3fd_packed_layout_bytes(void);
size_t n3dt_s3fd_ws_bytes(int n, int H, int W);
size_t n3dt_s3fd_block_ws_bytes(int block, int n, int Hi, int Wi);
void n3dt_launch_s3fd_pack(const N3dtS3fdParams* p, void* packed, hipStream_t st);
void n3dt_launch_s3fd_heads(int n, int H, int W, const void* packed, const float* x, float* const* out, void* workspace, hipStream_t st);
void n3dt_launch_s3fd_detect(int n, int H, int W, const void* packed, const float* frames, int max_faces, double* scores, double* dets,
                             int* count, int* left, void* workspace, hipStream_t st);
void n3dt_launch_s3fd_boxes(int F, int H, int W, int max_faces, const double* dets, const int* count, const int* pads, int T, int* boxes,
                            int* found, int* scratch, hipStream_t st);
void n3dt_launch_s3fd_block(int block, int n, int Hi, int Wi, const void* packed, const float* in, float* out, void* workspace,
                            hipStream_t st);

// ---- face_recon.hip
size_t n3dt_face_recon_packed_layout_bytes(void);
size_t n3dt_face_recon_ws_bytes(int n, int H, int W);
size_t n3dt_face_recon_block_ws_bytes(int block, int n, int Hi, int Wi);
void n3dt_launch_face_recon_pack(const N3dtFaceReconParams* p, void* packed, hipStream_t st);
void n3dt_launch_face_recon_fwd(int n, int H, int W, const void* packed, const float* x, float* out, void* workspace, hipStream_t st);
void n3dt_launch_face_recon_block(int block, int n, int Hi, int Wi, const void* packed, const float* in, const float* skip, float* out,
                                  void* workspace, hipStream_t st);
void n3dt_launch_face_recon_align(int n, int H, int W, const float* frames, const double* landmarks, int points, const double* lm3d_std,
                                  const double* pinv, int quantize, float* crops, double* trans_params, int* geom, int* status,
                                  hipStream_t st);

// ---- fan.hip
size_t n3dt_fan_packed_layout_bytes(int modules, int N);
size_t n3dt_fan_ws_bytes(int modules, int N, int n);
size_t n3dt_fan_block_ws_bytes(int block, int N, int n, int H, int W);
void n3dt_launch_fan_pack(const N3dtFanParams* q, void* packed, hipStream_t st);
void n3dt_launch_fan_fwd(int modules, int N, int end_relu, int n, const void* packed, const float* x, int compute_gates, uint8_t* gates,
                         float* heat, void* workspace, hipStream_t st);
void n3dt_launch_fan_block(int block, int modules, int N, int end_relu, int n, int H, int W, const void* packed, const float* in,
                           const float* skip, const uint8_t* gates, float* out, void* workspace, hipStream_t st);
void n3dt_launch_fan_crops(int n, int H, int W, const float* frames, const int* boxes, float* out, hipStream_t st);
void n3dt_launch_fan_points(int n, int N, const float* heat, long long frame_stride, double* pts, int* status, hipStream_t st);
void n3dt_launch_fan_tail(int n, int N, int P, int H, int W, const double* pts, const int* dstatus, const int* boxes, const int* table,
                          int carry, double* out, int* status, hipStream_t st);

// ---- head_mask.hip
size_t n3dt_head_mask_packed_layout_bytes(void);
size_t n3dt_head_mask_ws_bytes(int n, int H, int W);
size_t n3dt_head_mask_block_ws_bytes(int block, int n, int Hi, int Wi, int Hs, int Ws);
size_t n3dt_head_mask_post_ws_bytes(int n, int H, int W);
void n3dt_launch_head_mask_pack(const N3dtHeadMaskParams* p, void* packed, hipStream_t st);
void n3dt_launch_head_mask_fwd(int n, int H, int W, int n_classes, const void* packed, const float* x, int outputs, int upsample,
                               float* const* out, void* workspace, hipStream_t st);
void n3dt_launch_head_mask_block(int block, int n, int Hi, int Wi, int Hs, int Ws, int n_classes, const void* packed, const float* in,
                                 const float* aux, const float* scale, const float* addvec, float* out, void* workspace, hipStream_t st);
void n3dt_launch_head_mask_frames(int n, int H, int W, const void* frames, int is_float, uint8_t* rgb, float* x, hipStream_t st);
void n3dt_launch_head_mask_resize(int n, int Hs, int Ws, int C, const uint8_t* src, int Hd, int Wd, uint8_t* dst, hipStream_t st);
void n3dt_launch_head_mask_labels(int n, int nc, int h, int w, int H, int W, const float* logits, uint8_t* labels, hipStream_t st);
void n3dt_launch_head_mask_green(int n, int H, int W, const uint8_t* rgb, int hue_lo, int hue_hi, uint8_t* cleared, hipStream_t st);
void n3dt_launch_head_mask_postprocess(int n, int H, int W, const uint8_t* labels, const uint8_t* rgb, const uint8_t* lut, const uint8_t* element,
                                       int eh, int ew, int ay, int ax, int dilations, int erosions, int hue_lo, int hue_hi, uint8_t* head,
                                       uint8_t* eye, void* workspace, hipStream_t st);
}
