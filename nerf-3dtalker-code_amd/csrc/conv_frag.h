/*
 * conv_frag.h -- the fragment arithmetic of the split-operand implicit-GEMM convolutions (vgg_loss.hip, lpips.hip, syncnet.hip,
 * wav2lip.hip, s3fd.hip, face_recon.hip, fan.hip, head_mask.hip; DESIGN sections 3.10, 3.14, 3.16 - 3.22): where an element of a
 * packed B matrix lies, and which output row an accumulator register is.
 *
 * Included by csrc/conv_mfma.h, whose MFMA step reads its B fragments at cf_frag_group, by the pack kernels (vgg's, lpips's,
 * wav2lip's, s3fd's and conv_net.hip's shared one), which decode their element index with cf_pack_decode, by the eight
 * epilogues, which take their rows from cf_acc_row, and by tests/lpips_core_host.cpp and the six networks' host walks
 * (tests/syncnet_core_host.cpp and its siblings), which call the very same functions on the CPU.  Compiles as host C++ on its own;
 * the __host__ __device__ qualifiers exist only under hipcc.
 *
 * A packed matrix B [kp][np] (kp a multiple of 16, np of 32) is kp / 16 x np / 32 fragments, the column tile fastest; a fragment
 * is 64 lanes x 8 bf16, one contiguous KiB: lane (r = lane & 31, h = lane >> 5) element j holds B[16 s + 8 h + j][32 t + r],
 * which is what v_mfma_f32_32x32x16_bf16 wants in lane `lane` as its B operand.
 */
#ifndef N3DT_CONV_FRAG_H
#define N3DT_CONV_FRAG_H

#include <stddef.h>

#ifdef __HIPCC__
#define CF_HD __host__ __device__ static inline
#else
#define CF_HD static inline
#endif

#define CF_FRAG_ELEMS 512 /* 64 lanes x 8 bf16 */

/* accumulator register i (0..15) of a lane in half h = lane >> 5 is row cf_acc_row(i, h) of the 32 x 32 tile; its column is lane & 31 */
CF_HD int cf_acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

/* the reader: lane `lane` takes 8 consecutive elements, the group cf_frag_group, from fragment (K step s, column tile t0 + dt) of a
 * matrix ntiles = np / 32 wide (a wave's first tile and the tile's number within the wave); element j of them is cf_frag_elem */
CF_HD size_t cf_frag_group(int s, int ntiles, int t0, int dt, int lane) { return ((size_t)s * ntiles + t0 + dt) * 64 + lane; }
CF_HD size_t cf_frag_elem(int s, int ntiles, int t0, int dt, int lane, int j) { return cf_frag_group(s, ntiles, t0, dt, lane) * 8 + j; }

/* the packer: flat element e of [0, kp * np) -> the (k, n) of B it holds; the inverse of cf_frag_elem */
CF_HD void cf_pack_decode(size_t e, int ntiles, int* k, int* n) {
    const int frag = (int)(e / CF_FRAG_ELEMS), within = (int)(e % CF_FRAG_ELEMS);
    const int lane = within >> 3, j = within & 7;
    const int s = frag / ntiles, t = frag % ntiles;
    *k = 16 * s + 8 * (lane >> 5) + j;
    *n = 32 * t + (lane & 31);
}

#endif
