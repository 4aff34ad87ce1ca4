"""Stage-by-stage float64 restatement of the 2-D neural renderer's training step, for the tests that pin
csrc/train_nr.hip, the save epilogue of neural_render_x16.inc / nr_fused_x16.inc and nr_train16.h
(test_nr_restatement_cpu.py, test_gpu_nr_stagewise.py).  A helper module, not a test file: CPU only, numpy.
The last section restates the 16-bit INFERENCE renderer (run_x16), forward only, in bf16 and IEEE half, for
test_gpu_nr_infer_stagewise.py.

What is restated (reference: NetWorks/neural_renderer.py:72-91, PixelShuffleUpsample.py:36-45, Blur with the filter2d
semantics of DESIGN section 4: cross-correlation with [1 2 1]^2 / 16 on a reflect border):

    rgb = rgb_upsample(to_rgb_0(x))                      rgb_upsample = bilinear x2 (align_corners=False), then the blur
    per block i:  t1 = lrelu(layer_1 x)   tv = lrelu(layer_2 t1)   ps = pixel_shuffle(tv + x.repeat(1, 4, 1, 1))
                  bl = blur(ps)   net = lrelu(feat_layers bl)   rgb = rgb + to_rgb_{i+1}(net);  rgb_upsample between blocks
    img = sigmoid(rgb)

Maps are [nb, h, w, C] arrays (the kernels' pixel-major layout).  `forward` returns every intermediate.  `backward` is written
by hand, one function per adjoint, and takes a `Tape`: every gate (lrelu') and every GEMM operand is an argument, so it runs
"free" on the tape of its own forward or "teacher-forced" on activations read back from a kernel's `saved` buffer.

Storage points.  `store` (identity, or bf16_rne) is applied exactly where the mixed-precision backwards write a map or a map
gradient to HBM as bf16, `wq` where a bf16 MFMA reads an fp32 weight (gemm_h_kernel converts its B operand, neural_render_x16.inc:179).
Read off the host code of train_nr.hip:

  path "fused"   nr_bwd16 (:1045-1162)
    d_pre   = store(lrelu'(net) (to_rgb^T d_rgb + d x of the next block))                nr16_dpre_kernel (:936-962)
    d_hid   = store(Blur^T d_pre), as four sub-pixel planes                              nr16_blur_adj_q_kernel (:967-1024)
    d Wf    = d_hid^T store(y + x.repeat)   (the loader rounds the rebuilt ps, :694-695)  nrt_dw16_kernel<DwPs>
    d_tv    = store(lrelu'(y) store(d_hid . wq(Wf)))                                     gemm_h, gate epilogue (:1120-1124)
    d_t1    = store(lrelu'(t1) store(d_tv . wq(W2)))                                     (:1130-1134)
              TWO roundings each: gemm_h_kernel stages its accumulators through LDS as 16-bit values and applies the gate to the
              staged value (neural_render_x16.inc:223, :241-242), so an entry behind a closed gate is bf16(0.2f bf16(acc))
    d W1    = d_t1^T store(x)   (block 0: the fp32 feature map, rounded by the loader)
    d_x     = store(d_t1 . wq(W1) + sum_q d_hid_q . wq(R_q))                             the dx ping-pong (:1140-1144); R_q: the fp32
              sum of four entries of Wf in the forward's order (nr16_pack_wt_kernel, :917-930), rounded once
    d_featmap = d_x + to_rgb_0^T d_rgb in fp32                                           nr16_final_kernel (:1026-1043)
  path "exact"   nr_bwd<float> (:1187-1267): the same adjoints in the reference's operator order (feat_layers^T, Blur^T, the
    un-shuffle with the residual's sum over the four repeats, layer_2^T, layer_1^T); nothing is rounded.
  The layered bf16 backward nr_bwd<nrt_bf16> is NOT restated: the library builds featmap_nc == 256 only (n3dt_api.hip: check_nr), every
  such geometry takes the fused path (nr16_supported), and the switch that forces the layered one (N3DT_NR_TRAIN_FUSED) is
  latched per process.
  In both paths d_rgb (the RGB pyramid's gradient), the sigmoid factor and every parameter gradient stay fp32.

`scale` runs the same backward with every weight, operand and cotangent replaced by its absolute value (gate factors stay
1 / 0.2, the sigmoid factor y (1 - y) is non-negative already): S, the per-entry sum of |terms| of every output.  Every
comparison is per entry and relative to S; a tensor's maximum is never the scale.

The floors come from the CPU alone, never from a kernel (test_nr_restatement_cpu.py re-measures them and fails if one moved up):

    NR_F32_FLOOR   largest |g32 - g64| / S per GPU case and output family of the free restatement run in float32 in two
                   accumulation orders (torch.matmul; 16-wide k-steps in sequence) against float64 (on the float32 run's gates:
                   they may differ inside the gate band only)
    NR_BF16_FLOOR  largest |g32 - g64| / S of the teacher-forced backward with store = wq = bf16_rne: float32 in three accumulation
                   orders (one k at a time; 16-wide k-steps; 16-wide over a seeded permutation of k; the stencils' rows or
                   columns first) against float64, on the tape of a bf16 forward emulation, over four seeds of the geometry.
                   That is the spread a correct implementation with bf16 storage has: a few flipped roundings of stored map
                   gradients, each 2^-8 of its entry, which an entry of a later product that one term dominates inherits.
                   The float32 orders are elementwise numpy only, so the figure does not depend on a BLAS.
    GPU bounds are 4 x the floor.
"""
import numpy as np
import torch

import x16_stagewise as xs
from x16_stagewise import bf16_bits, bf16_round, bf16_to_f64

SLOPE = 0.2
FAMILIES = ("d_featmap", "conv_w", "conv_b", "rgb_w", "rgb_b")

# (featmap side, channels, blocks, maps) -> seed of weights and inputs.  ONE table for both test files: the CPU test asserts the
# gate condition, the floors and the check_bf16 caps for every entry, the GPU test runs them.
GPU_CASES = {
    (4, 256, 1, 1): 52,
    (4, 256, 3, 2): 0,
    (8, 256, 2, 3): 0,
    (5, 256, 2, 3): 0,
    (4, 256, 4, 1): 0,      # the fourth block is 32 -> 32: the channel clamp, inside what the library builds
}
# Geometries the library refuses ("only featmap_nc == 256 is built", n3dt_api.hip: check_nr): the restatement is pinned at them on the CPU
# (AUTOGRAD_CASES, FIXTURE_CASES), the GPU test asserts the refusal.
UNBUILT_CASES = ((6, 64, 3, 2), (5, 32, 1, 1))
AUTOGRAD_CASES = {(4, 32, 1, 1): 0, (5, 32, 2, 3): 0, (6, 64, 3, 2): 0, (4, 256, 3, 2): 0}
FIXTURE_CASES = ((4, 32, 2, 2), (5, 32, 1, 1))

MARGIN = 4.0                  # a GPU bound is 4 x the floor
GATE_MARGIN = 1e-5            # the gate band: lrelu pre-activations of the float64 forward within GATE_MARGIN (|b| + sum |w x|) of zero
STRICT_GATE_CASES = ((4, 256, 1, 1),)   # cases whose seed leaves NO pre-activation inside the band (test_gate_condition)
BAND_SHARE_CAP = 1e-3         # |z| / (|b| + sum |w x|) of a sum of K <= 1024 terms is no narrower than ~1 / sqrt(K): a density of
#                               at most ~50 at zero, so at most 100 GATE_MARGIN of a case's entries lie inside the band
# ---- the measured floors (see the module docstring), per case and output family: S grows with the depth of a case (three GEMMs of
# absolute values per block), so a figure pooled over the cases would be the shallowest case's and bind nothing in the deep ones
NR_F32_FLOOR = {
    (4, 256, 1, 1): {"d_featmap": 1.5e-09, "conv_w": 1.9e-07, "conv_b": 5.0e-08, "rgb_w": 3.6e-07, "rgb_b": 3.0e-08},
    (4, 256, 3, 2): {"d_featmap": 4.3e-13, "conv_w": 3.8e-08, "conv_b": 2.0e-08, "rgb_w": 5.9e-08, "rgb_b": 1.7e-08},
    (8, 256, 2, 3): {"d_featmap": 2.2e-11, "conv_w": 3.9e-08, "conv_b": 3.3e-08, "rgb_w": 7.3e-08, "rgb_b": 1.4e-08},
    (4, 256, 4, 1): {"d_featmap": 1.7e-14, "conv_w": 4.9e-08, "conv_b": 2.0e-08, "rgb_w": 3.1e-08, "rgb_b": 2.2e-08},
    (5, 256, 2, 3): {"d_featmap": 2.0e-11, "conv_w": 7.5e-08, "conv_b": 4.0e-08, "rgb_w": 7.1e-08, "rgb_b": 3.0e-08},
}
NR_F32_IMAGE_FLOOR = 1.3e-7      # |img32 - img64| of the free float32 forward (absolute: a sigmoid output)
NR_F32_STAGE_FLOOR = 3.1e-7      # lrelu stages of the free float32 forward: |a32 - a64| / (|b| + sum |w x|), every stage of every case
# the fp32 stages of the 16-bit INFERENCE renderer (the last section of this module): the float32 emulation in two accumulation
# orders (16-wide k-steps in sequence, rows of the stencils first; torch.matmul, columns first) against float64 over every INFER_CASES entry in both formats.  The CPU test
# re-measures them and fails unless measured <= floor < 2 x measured.  GPU bounds are MARGIN x the floor.
NR_X16_RGB0_FLOOR = 3.7e-7          # |rgb0_32 - rgb0_64| / (|b| + sum |w x|); measured 2.67e-7
NR_X16_RGB_FLOOR = 3.1e-7           # pre-sigmoid pyramid value of a level from FIXED 16-bit activations: / (|b| + sum |w net| + up |lo|); measured 2.22e-7
NR_X16_SIGMOID_FLOOR = 1.3e-7       # |sigmoid32(z) - sigmoid64(z)| at the same float32 z (absolute: a value in (0, 1)); measured 9.43e-8
BF16_FLOOR_ORDERS, BF16_FLOOR_SEEDS = 3, 4   # the bf16 floor of a geometry is the maximum over 3 float32 orders x 4 seeds (the case's and
#                               the next three): the figure is the size of the few rounding flips an order causes, a handful of events whose
#                               largest varies several-fold from one draw of the inputs to the next (and hardly between orders on one draw)
NR_BF16_FLOOR = {
    (4, 256, 1, 1): {"d_featmap": 6.8e-06, "conv_w": 2.9e-04, "conv_b": 4.9e-05, "rgb_w": 1.7e-07, "rgb_b": 3.1e-08},
    (4, 256, 3, 2): {"d_featmap": 3.2e-09, "conv_w": 4.9e-06, "conv_b": 2.5e-06, "rgb_w": 1.4e-07, "rgb_b": 6.3e-08},
    (8, 256, 2, 3): {"d_featmap": 2.3e-07, "conv_w": 3.6e-06, "conv_b": 1.2e-06, "rgb_w": 2.2e-07, "rgb_b": 3.6e-08},
    (5, 256, 2, 3): {"d_featmap": 1.1e-07, "conv_w": 2.6e-05, "conv_b": 5.5e-06, "rgb_w": 1.8e-07, "rgb_b": 6.8e-08},
    (4, 256, 4, 1): {"d_featmap": 2.3e-10, "conv_w": 2.2e-06, "conv_b": 2.3e-06, "rgb_w": 8.3e-08, "rgb_b": 3.1e-08},
}


def nr_ch(C, i):  # train_nr.hip:12-15 (nr_ch), nr_train16.h:15-18 (nr16_ch)
    return max(C >> i, 32)


def ident(v):
    return v


def bf16_rne(v):
    v = np.asarray(v)
    return bf16_round(v).astype(v.dtype)


def family(name):
    if name == "d_featmap":
        return name
    if name.startswith("rgb_w"):
        return "rgb_w"
    if name.startswith("rgb_b"):
        return "rgb_b"
    return "conv_w" if name[0] == "w" else "conv_b"


# ---------------------------------------------------------------------------------------------
# parameters
# ---------------------------------------------------------------------------------------------
class Params:
    """rgb_w[i] [3, C_i] / rgb_b[i] (i = 0 .. n), w1[i] [2C, C], w2[i] [4C, 2C], wf[i] [CO, C] and their biases"""
    FIELDS = ("rgb_w", "rgb_b", "w1", "b1", "w2", "b2", "wf", "bf")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, list(kw[f]))
        self.n = len(self.w1)

    def map(self, fn):
        return Params(**{f: [fn(a) for a in getattr(self, f)] for f in self.FIELDS})

    def flat(self):
        """[w, b] pairs flattened in NeuralRenderer._flat_modules() order: to_rgb[0..n], layer_1[..], layer_2[..], feat[..]"""
        out = []
        for wn, bn in (("rgb_w", "rgb_b"), ("w1", "b1"), ("w2", "b2"), ("wf", "bf")):
            for w, b in zip(getattr(self, wn), getattr(self, bn)):
                out += [w, b]
        return out

    def names(self):
        """the gradient names of `backward` in flat() order"""
        out = []
        for wn, bn in (("rgb_w%d", "rgb_b%d"), ("w1_%d", "b1_%d"), ("w2_%d", "b2_%d"), ("wf%d", "bf%d")):
            for i in range(self.n + 1 if wn.startswith("rgb") else self.n):
                out += [wn % i, bn % i]
        return out


def params_from_state_dict(sd, n_blocks, prefix="neural_render."):
    g = lambda k: sd[prefix + k].detach().double().numpy()  # noqa: E731
    w2d = lambda k: g(k).reshape(g(k).shape[0], -1)  # noqa: E731
    return Params(rgb_w=[w2d("feat_2_rgb_list.%d.weight" % i) for i in range(n_blocks + 1)],
                  rgb_b=[g("feat_2_rgb_list.%d.bias" % i) for i in range(n_blocks + 1)],
                  w1=[w2d("feat_upsample_list.%d.layer_1.weight" % i) for i in range(n_blocks)],
                  b1=[g("feat_upsample_list.%d.layer_1.bias" % i) for i in range(n_blocks)],
                  w2=[w2d("feat_upsample_list.%d.layer_2.weight" % i) for i in range(n_blocks)],
                  b2=[g("feat_upsample_list.%d.layer_2.bias" % i) for i in range(n_blocks)],
                  wf=[w2d("feat_layers.%d.weight" % i) for i in range(n_blocks)],
                  bf=[g("feat_layers.%d.bias" % i) for i in range(n_blocks)])


def case_options(case):
    from n3dt import BaseOptions
    fs, C, n, _ = case
    return BaseOptions({"featmap_size": fs, "featmap_nc": C, "pred_img_size": fs << n, "num_sample_coarse": 8})


def case_inputs(case, seed):
    """(Params float64 of fp32 values, x [nb, fs, fs, C] = 0.5 randn, d_img [nb, P, P, 3] = randn per pixel); everything seeded"""
    from n3dt import synthetic as syn
    fs, C, n, nb = case
    sd = syn.make_state_dict(case_options(case), seed=seed, bg_noise=0.1)
    gen = torch.Generator().manual_seed(1000 + seed)
    x = (0.5 * torch.randn(nb, fs, fs, C, generator=gen)).double().numpy()
    P = fs << n
    d_img = torch.randn(nb, P, P, 3, generator=gen).double().numpy()
    return params_from_state_dict(sd, n), x, d_img


# ---------------------------------------------------------------------------------------------
# the spatial operators as matrices over one axis (every one is separable), and their adjoints in closed form
# ---------------------------------------------------------------------------------------------
def reflect1(i, n):
    return -i if i < 0 else (2 * n - 2 - i if i >= n else i)


def blur_matrix(n):
    """out[i] = 0.25 x[reflect(i - 1)] + 0.5 x[i] + 0.25 x[reflect(i + 1)]"""
    B = np.zeros((n, n))
    for i in range(n):
        for d, k in ((-1, 0.25), (0, 0.5), (1, 0.25)):
            B[i, reflect1(i + d, n)] += k
    return B


def blur_adj_matrix(n, doubled=True):
    """Adjoint in closed form, not a transpose: input j is read by outputs j - 1, j, j + 1; the reflected reads of outputs 0 and
    n - 1 land on j = 1 and j = n - 2 and double that tap.  doubled=False is the fault the mutant test injects."""
    A = np.zeros((n, n))
    edge = 0.5 if doubled else 0.25
    for j in range(n):
        if j >= 1:
            A[j, j - 1] = edge if j == 1 else 0.25
        A[j, j] = 0.5
        if j + 1 < n:
            A[j, j + 1] = edge if j == n - 2 else 0.25
    return A


def bilinear_matrix(n):
    """x2, align_corners=False: source coordinate max(0.5 (i + 0.5) - 0.5, 0), the upper neighbour clamped at n - 1"""
    U = np.zeros((2 * n, n))
    for i in range(2 * n):
        s = max(0.5 * (i + 0.5) - 0.5, 0.0)
        i0 = int(s)
        i1 = min(i0 + 1, n - 1)
        l = s - i0
        U[i, i0] += 1.0 - l
        U[i, i1] += l
    return U


def bilinear_adj_matrix(n, edge=1.0):
    """Adjoint in closed form: input m receives 0.75 from outputs 2m and 2m + 1 (all of them, 1, at a clamped edge) and 0.25 from
    outputs 2m - 1 and 2m + 2.  edge=0.75 is the fault the mutant test injects."""
    A = np.zeros((n, 2 * n))
    for m in range(n):
        A[m, 2 * m] = edge if m == 0 else 0.75
        A[m, 2 * m + 1] = edge if m == n - 1 else 0.75
        if m + 1 < n:
            A[m, 2 * m + 2] = 0.25
        if m >= 1:
            A[m, 2 * m - 1] = 0.25
    return A


def sep(A, x, rows_first=True):
    """the separable operator A (x) A on the two spatial axes of x [nb, h, w, C]; rows_first: which axis is summed first (the same
    in exact arithmetic; in float32 another accumulation order)"""
    A = A.astype(x.dtype)
    if rows_first:
        return np.einsum("jw,niwc->nijc", A, np.einsum("ih,nhwc->niwc", A, x))
    return np.einsum("ih,nhjc->nijc", A, np.einsum("jw,nhwc->nhjc", A, x))


def blur_taps(x):
    """the blur by its three taps per axis on a reflect border: the same operator without the dense matrices, for large maps"""
    def along(a, axis):
        a = np.moveaxis(a, axis, 0)
        p = np.concatenate([a[1:2], a, a[-2:-1]])
        return np.moveaxis(0.25 * p[:-2] + 0.5 * p[1:-1] + 0.25 * p[2:], 0, axis)
    return along(along(x, 1), 2)


def blur(x):
    return blur_taps(x) if x.shape[1] > 64 else sep(blur_matrix(x.shape[1]), x)


def blur_adj(d, fault=None, rows_first=True):
    return sep(blur_adj_matrix(d.shape[1], doubled=fault != "blur_border"), d, rows_first)


def rgb_upsample(r):
    n = r.shape[1]
    return sep(blur_matrix(2 * n) @ bilinear_matrix(n), r)


def rgb_upsample_adj(d, fault=None, rows_first=True):
    n = d.shape[1] // 2
    return sep(bilinear_adj_matrix(n, edge=0.75 if fault == "bilinear_edge" else 1.0), blur_adj(d, fault, rows_first), rows_first)


def shuffle(t):
    """pixel_shuffle(2) of [nb, h, w, 4C]: out[2h + di, 2w + dj, c] = t[h, w, 4c + 2 di + dj]"""
    nb, h, w, C4 = t.shape
    C = C4 // 4
    return t.reshape(nb, h, w, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(nb, 2 * h, 2 * w, C)


def unshuffle(p):
    nb, H, W, C = p.shape
    return p.reshape(nb, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(nb, H // 2, W // 2, 4 * C)


def repeat4(x):
    """x.repeat(1, 4, 1, 1): channel o of the result is x[o % C]"""
    return np.tile(x, (1, 1, 1, 4))


def repeat4_adj(d, fault=None):
    nb, h, w, C4 = d.shape
    r = d.reshape(nb, h, w, 4, C4 // 4)
    return (r[:, :, :, :3] if fault == "residual_three" else r).sum(axis=3)


def planes(m):
    """raster [nb, 2h, 2w, K] -> the four sub-pixel planes [4, nb, h, w, K], q = 2 di + dj (nr_train16.h:5-8)"""
    return np.stack([m[:, di::2, dj::2] for di in (0, 1) for dj in (0, 1)])


def lrelu(z):
    return np.where(z > 0, z, z.dtype.type(SLOPE) * z)


def gate_factor(g, dtype):
    return np.where(g, dtype.type(1.0), dtype.type(SLOPE))


def gated(v, g, store):
    """lrelu'(.) v as a GEMM's gate epilogue stores it: exact without a store; with one, the product is staged as a 16-bit value
    first and the closed gates' 0.2f a (an fp32 product) is rounded again (see the module docstring)"""
    if store is ident:
        return gate_factor(g, v.dtype) * v
    a = store(v)
    return store(np.where(g, a, (np.float32(SLOPE) * a.astype(np.float32)).astype(a.dtype)))


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


# ---------------------------------------------------------------------------------------------
# forward, one function per stage
# ---------------------------------------------------------------------------------------------
def conv(x, W, b, mm):
    """1x1 conv on a pixel-major map: [.., K] -> [.., N]; also returns the magnitude |b| + sum |w x| when mm is None"""
    z = mm(x.reshape(-1, x.shape[-1]), np.ascontiguousarray(W.T)) + b
    return z.reshape(x.shape[:-1] + (W.shape[0],))


def conv_mag(x, W, b):
    return (np.abs(x).reshape(-1, x.shape[-1]) @ np.abs(W).T + np.abs(b)).reshape(x.shape[:-1] + (W.shape[0],))


def to_rgb0(x, P, mm):
    return conv(x, P.rgb_w[0], P.rgb_b[0], mm)


def layer_1(x, P, i, mm):
    return conv(x, P.w1[i], P.b1[i], mm)


def layer_2(t1, P, i, mm):
    return conv(t1, P.w2[i], P.b2[i], mm)


def shuffle_residual(tv, x):
    return shuffle(tv + repeat4(x))


def feat_layer(bl, P, i, mm):
    return conv(bl, P.wf[i], P.bf[i], mm)


def feat_2_rgb(net, P, i, mm):
    return conv(net, P.rgb_w[i + 1], P.rgb_b[i + 1], mm)


def forward(x, P, mm=np.matmul):
    """Every intermediate of the renderer, in the reference's operator order (the exact path's).  Lists are per block; *_pre are the lrelu pre-activations, *_mag their |b| + sum |w x|."""
    f = {k: [] for k in ("x", "t1_pre", "t1", "tv_pre", "tv", "ps", "bl", "net_pre", "net", "t1_mag", "tv_mag", "net_mag", "rgb")}
    rgb = rgb_upsample(to_rgb0(x, P, mm))
    f["rgb"].append(rgb)
    net = x
    for i in range(P.n):
        f["x"].append(net)
        t1_pre = layer_1(net, P, i, mm)
        t1 = lrelu(t1_pre)
        tv_pre = layer_2(t1, P, i, mm)
        tv = lrelu(tv_pre)
        ps = shuffle_residual(tv, net)
        bl = blur(ps)
        net_pre = feat_layer(bl, P, i, mm)
        f["t1_mag"].append(conv_mag(net, P.w1[i], P.b1[i]))
        f["tv_mag"].append(conv_mag(t1, P.w2[i], P.b2[i]))
        f["net_mag"].append(conv_mag(bl, P.wf[i], P.bf[i]))
        net = lrelu(net_pre)
        rgb = rgb + feat_2_rgb(net, P, i, mm)
        if i < P.n - 1:
            rgb = rgb_upsample(rgb)
        for k, v in (("t1_pre", t1_pre), ("t1", t1), ("tv_pre", tv_pre), ("tv", tv), ("ps", ps), ("bl", bl), ("net_pre", net_pre), ("net", net),
                     ("rgb", rgb)):
            f[k].append(v)
    f["rgb_pre"] = rgb
    f["img"] = sigmoid(rgb)
    return f


def gate_band(f, k, i):
    """bool: the pre-activations of stage k ("t1", "tv", "net") of block i within GATE_MARGIN (|b| + sum |w x|) of zero"""
    return np.abs(f[k + "_pre"][i]) < GATE_MARGIN * f[k + "_mag"][i]


def gate_distance(f):
    """smallest |pre-activation| / (|b| + sum |w x|) over every lrelu of a forward"""
    return min(float((np.abs(f[k + "_pre"][i]) / f[k + "_mag"][i]).min()) for k in ("t1", "tv", "net") for i in range(len(f["t1"])))


# ---------------------------------------------------------------------------------------------
# backward, by hand
# ---------------------------------------------------------------------------------------------
class Tape:
    """What the backward reads: img [nb, P, P, 3]; per block the GEMM operands x (block input), t1, ps (operand of d Wf on the
    fused path) or bl (on the others), net, and the gates g_t1, g_tv, g_net (bool: pre-activation > 0)."""
    FIELDS = ("x", "t1", "ps", "bl", "net", "g_t1", "g_tv", "g_net")

    def __init__(self, img, **kw):
        self.img = img
        for k in self.FIELDS:
            setattr(self, k, list(kw[k]))

    def map(self, fn):
        """fn on every operand (not the gates)"""
        kw = {k: [None if a is None else fn(a) for a in getattr(self, k)] if not k.startswith("g_") else getattr(self, k) for k in self.FIELDS}
        return Tape(self.img, **kw)


def tape_from_forward(f):
    return Tape(f["img"], x=f["x"], t1=f["t1"], ps=f["ps"], bl=f["bl"], net=f["net"], g_t1=[a > 0 for a in f["t1"]],
                g_tv=[a > 0 for a in f["tv"]], g_net=[a > 0 for a in f["net"]])


def sigmoid_adj(d_img, img):
    return d_img * img * (1.0 - img)


def conv_adj_w(dy, x, mm, fault=None):
    """dW [N, K] = dy^T x over the pixels, db = column sums of dy"""
    a, b = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
    if fault == "dw_slice" and a.shape[0] > 32:
        a, b = a[32:], b[32:]          # one 32-row slice of pixels left out
    return mm(np.ascontiguousarray(a.T), b), dy.reshape(-1, dy.shape[-1]).sum(axis=0)


def conv_adj_x(dy, W, mm):
    return mm(dy.reshape(-1, dy.shape[-1]), W).reshape(dy.shape[:-1] + (W.shape[1],))


def residual_matrix(Wf, q, f32=False, three=False):
    """R_q [CO, C] of the fused path (nr_train16.h:40-45): R_q[o][k] = sum of Wf[o][c] over the four c with (4c + q) % C == k, in the
    forward's summation order (train_nr.hip:925-929); zero unless k % 4 == q.  f32: summed in float32, as the pack kernel does
    before the GEMM rounds it to bf16."""
    if f32:
        return residual_matrix(Wf.astype(np.float32), q, three=three).astype(Wf.dtype)
    CO, C = Wf.shape
    R = np.zeros_like(Wf)
    k = np.arange(q, C, 4)
    c0 = (k - q) >> 2
    last = 0.0 if three else Wf[:, c0 + 3 * (C // 4)]          # three: the fault "residual summed over three repeats"
    R[:, k] = (Wf[:, c0] + Wf[:, c0 + C // 4]) + (Wf[:, c0 + C // 2] + last)
    return R


def backward(d_img, P, tape, mm=np.matmul, store=ident, wq=ident, path="exact", fault=None, frozen=False, rows_first=True):
    """Gradients of sum(img * d_img): {"d_featmap", "rgb_w0".., "rgb_b0".., "w1_0".., "b1_0".., "w2_*", "b2_*", "wf_*", "bf_*"}.
    path: "exact" or "fused" (see the module docstring); store / wq are meant for "fused".
    fault: one deliberate error (test_nr_restatement_cpu.py's mutants); frozen: no parameter gradient (rgrads = None);
    mm / rows_first: the accumulation order of the products / of the separable stencils (the floors' float32 orders)."""
    assert path in ("exact", "fused")
    dt = d_img.dtype
    n, out = P.n, {}
    d_rgb = sigmoid_adj(d_img, tape.img)
    d_next = None
    for i in range(n - 1, -1, -1):
        net, t1, x = tape.net[i], tape.t1[i], tape.x[i]
        # rgb = rgb_up + feat_2_rgb[i + 1](net)
        if not frozen:
            out["rgb_w%d" % (i + 1)], out["rgb_b%d" % (i + 1)] = conv_adj_w(d_rgb, net, mm)
        v = conv_adj_x(d_rgb, P.rgb_w[i + 1], mm)
        if d_next is not None:
            v = v + d_next
        d_pre = store(gate_factor(tape.g_net[i], dt) * v)
        if path == "fused":
            d_hid = store(blur_adj(d_pre, fault, rows_first))
            if not frozen:
                out["wf%d" % i], out["bf%d" % i] = conv_adj_w(d_hid, store(tape.ps[i]), mm, fault if i == n - 1 else None)
            d_tv_pre = unshuffle(conv_adj_x(d_hid, wq(P.wf[i]), mm))
            dq = planes(d_hid)
            d_xres = sum(conv_adj_x(dq[q], wq(residual_matrix(P.wf[i], q, f32=wq is not ident, three=fault == "residual_three")), mm)
                         for q in range(4))
        else:
            if not frozen:
                out["wf%d" % i], out["bf%d" % i] = conv_adj_w(d_pre, tape.bl[i], mm, fault if i == n - 1 else None)
            d_bl = store(conv_adj_x(d_pre, wq(P.wf[i]), mm))
            d_ps = store(blur_adj(d_bl, fault, rows_first))
            d_tv_pre = unshuffle(d_ps)
            d_xres = store(repeat4_adj(d_tv_pre, fault))
        d_tv = gated(d_tv_pre, tape.g_tv[i], store)
        if not frozen:
            out["w2_%d" % i], db2 = conv_adj_w(d_tv, t1, mm)
            if fault == "db2_plane":
                db2 = np.where(np.arange(db2.size) % 4 == 3, 0.0, db2)   # sub-pixel plane 3 (rows 4c + 3) never summed
            out["b2_%d" % i] = db2
        d_t1 = gated(conv_adj_x(d_tv, wq(P.w2[i]), mm), tape.g_t1[i], store)
        if not frozen:
            out["w1_%d" % i], out["b1_%d" % i] = conv_adj_w(d_t1, store(x), mm)
        d_next = store(conv_adj_x(d_t1, wq(P.w1[i]), mm) + d_xres)
        d_rgb = rgb_upsample_adj(d_rgb, fault, rows_first)
    if not frozen:
        out["rgb_w0"], out["rgb_b0"] = conv_adj_w(d_rgb, tape.x[0], mm)
    branch = conv_adj_x(d_rgb, P.rgb_w[0], mm)
    if fault == "rgb0_branch":
        branch = np.zeros_like(branch)
    out["d_featmap"] = d_next + branch
    return out


def scale(d_img, P, tape, path="exact", frozen=False):
    """S: the backward of absolute values -- per entry the sum of |terms| of every output (gate factors 1 / 0.2 as they are)"""
    return backward(np.abs(d_img), P.map(np.abs), tape.map(np.abs), path=path, frozen=frozen)


# ---------------------------------------------------------------------------------------------
# accumulation orders
# ---------------------------------------------------------------------------------------------
def mm32_torch(a, b):
    return torch.matmul(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32))).numpy()


def mm32_seq16(a, b):
    """16-wide k-steps in sequence (the MFMA streams' order)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k0 in range(0, a.shape[1], 16):
        acc = acc + a[:, k0:k0 + 16] @ b[k0:k0 + 16]
    return acc


def _mm32_elementwise(step):
    def mm(a, b):
        a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
        acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
        for k0 in range(0, a.shape[1], step):
            part = np.zeros_like(acc)
            for k in range(k0, min(k0 + step, a.shape[1])):
                part += a[:, k:k + 1] * b[k:k + 1, :]
            acc += part
        return acc
    return mm


def mm32_permuted(seed):
    """16-wide partial sums over a seeded permutation of k: further legal fp32 orders, elementwise numpy only"""
    inner = _mm32_elementwise(16)

    def mm(a, b):
        perm = np.random.RandomState(seed).permutation(a.shape[1])
        return inner(np.asarray(a)[:, perm], np.asarray(b)[perm])
    return mm


mm32_seq1 = _mm32_elementwise(1 << 30)   # one k at a time, elementwise numpy only (no BLAS: the same bits on every machine)
mm32_seq16e = _mm32_elementwise(16)      # 16-wide partial sums added in sequence, elementwise numpy only


def to32(P, *arrays):
    return (P.map(lambda a: a.astype(np.float32)),) + tuple(a.astype(np.float32) for a in arrays)


def compare(got, want, S, bound, tag="", coords=None):
    """The comparison rule of every gradient test: per entry |got - want| <= bound[family] * S; an entry with S == 0 must be equal.
    Returns (per-family maxima of |got - want| / S, failure report lines: tensor, index, got, expected, S)."""
    maxima, lines = {}, []
    for name in want:
        g, w, s = (np.asarray(a, dtype=np.float64) for a in (got[name], want[name], S[name]))
        assert g.shape == w.shape == s.shape, (name, g.shape, w.shape, s.shape)
        fam = family(name)
        err = np.abs(g - w)
        rel = np.where(s > 0, err / np.where(s > 0, s, 1.0), np.where(err > 0, np.inf, 0.0))
        maxima[fam] = max(maxima.get(fam, 0.0), float(rel.max()))
        bad = np.flatnonzero(rel.reshape(-1) > bound[fam])
        for j in bad[np.argsort(-rel.reshape(-1)[bad])][:4]:
            idx = tuple(int(v) for v in np.unravel_index(j, g.shape))
            where = ""
            if name == "d_featmap":
                h = g.shape[1]
                where = " (map %d, pixel (%d, %d)%s)" % (idx[0], idx[1], idx[2], ", border" if min(idx[1], idx[2]) == 0 or max(idx[1], idx[2]) == h - 1 else "")
            lines.append("%s %s%s%s: got %.9g expected %.9g S %.3g  (%.3g of S, bound %.3g)" %
                         (tag, name, list(idx), where, g.reshape(-1)[j], w.reshape(-1)[j], s.reshape(-1)[j], rel.reshape(-1)[j], bound[fam]))
    return maxima, lines


def bound_of(floor):
    return {k: MARGIN * v for k, v in floor.items()}


# ---------------------------------------------------------------------------------------------
# readers of the saved buffers
# ---------------------------------------------------------------------------------------------
def al64(n):   # train_nr.hip:16
    return (n + 63) & ~63


def al256(n):  # nr_train16.h:19 (nr16_al)
    return (n + 255) & ~255


def saved_layout_f32(case):
    """NrSaved (train_nr.hip:18-38): offsets in FLOATS, every region 64-float aligned"""
    fs, C, n, nb = case
    L, o = {"t1": [], "tv": [], "bl": [], "net": []}, 0
    for i in range(n):
        h = fs << i
        M, ci, co = nb * h * h, nr_ch(C, i), nr_ch(C, i + 1)
        for k, sz in (("t1", M * 2 * ci), ("tv", M * 4 * ci), ("bl", 4 * M * ci), ("net", 4 * M * co)):
            L[k].append(o)
            o += al64(sz)
    P = fs << n
    L["img"] = o
    L["total"] = o + al64(nb * 3 * P * P)
    return L


def saved_layout_16(case):
    """Nr16Saved (nr_train16.h:21-38): BYTE offsets, every region 256-byte aligned"""
    fs, C, n, nb = case
    L, o = {"t1": [], "y": [], "net": []}, 0
    for i in range(n):
        h = fs << i
        M, ci, co = nb * h * h, nr_ch(C, i), nr_ch(C, i + 1)
        for k, sz in (("t1", M * 2 * ci * 2), ("y", 4 * M * ci * 2), ("net", 4 * M * co * 2)):
            L[k].append(o)
            o += al256(sz)
    P = fs << n
    L["img"] = o
    L["total"] = o + al256(nb * 3 * P * P * 4)
    return L


class SavedMaps:
    """Decoded `saved` of one forward, kind "exact" (fp32, NrSaved) or "fused" (bf16, Nr16Saved): per block t1, tv, net (and bl on
    the exact path) as float64 arrays [nb, h, w, ch], the 16-bit patterns of the fused path (`bits`), and img [nb, P, P, 3].
    hid / hid_bits: feat_layers' output before the blur, which the fused forward leaves in the workspace -- filled by the caller."""

    def __init__(self, buf, case, kind):
        assert kind in ("exact", "fused")
        fs, C, n, nb = case
        buf = np.ascontiguousarray(np.asarray(buf, dtype=np.uint8))
        self.kind, self.case = kind, case
        self.t1, self.tv, self.bl, self.net, self.bits = [], [], [], [], {"t1": [], "tv": [], "net": []}
        self.hid, self.hid_bits = [None] * n, [None] * n
        P = fs << n
        if kind == "fused":
            L = saved_layout_16(case)
            assert buf.size >= L["total"]
            region = lambda off, cnt: buf[off:off + 2 * cnt].view(np.uint16)  # noqa: E731
            img = buf[L["img"]:L["img"] + 4 * nb * 3 * P * P].view(np.float32)
        else:
            L = saved_layout_f32(case)
            assert buf.size >= 4 * L["total"]
            region = lambda off, cnt: buf[4 * off:4 * (off + cnt)].view(np.float32)  # noqa: E731
            img = buf[4 * L["img"]:4 * (L["img"] + nb * 3 * P * P)].view(np.float32)
        self.img = np.ascontiguousarray(img.reshape(nb, 3, P, P).transpose(0, 2, 3, 1)).astype(np.float64)   # planar -> [nb, P, P, 3]
        dec = (lambda a: a.astype(np.float64)) if kind == "exact" else bf16_to_f64
        for i in range(n):
            h = fs << i
            M, ci, co = nb * h * h, nr_ch(C, i), nr_ch(C, i + 1)
            raw = {"t1": region(L["t1"][i], M * 2 * ci).reshape(nb, h, h, 2 * ci)}
            if kind == "fused":
                # y: four sub-pixel planes [4][M][C] BEFORE the residual (nr_train16.h:7): y_q[m][c] = tv[m][4c + q]
                y = region(L["y"][i], 4 * M * ci).reshape(4, M, ci)
                raw["tv"] = np.ascontiguousarray(y.transpose(1, 2, 0)).reshape(nb, h, h, 4 * ci)
            else:
                raw["tv"] = region(L["tv"][i], M * 4 * ci).reshape(nb, h, h, 4 * ci)
                raw["bl"] = region(L["bl"][i], 4 * M * ci).reshape(nb, 2 * h, 2 * h, ci)
            raw["net"] = region(L["net"][i], 4 * M * co).reshape(nb, 2 * h, 2 * h, co)
            for k, a in raw.items():
                getattr(self, k).append(dec(a))
                if kind == "fused":
                    self.bits[k].append(a.copy())

    def tape(self, x):
        """the teacher-forced tape of the fused path: operands and gates exactly as nr_bwd16's kernels read them.  x: the fp32 feature map."""
        assert self.kind == "fused"
        n = len(self.t1)
        xs_ = [np.asarray(x, dtype=np.float64)] + self.net[:-1]
        # (the d Wf loader adds y and x in fp32 before it rounds the sum to bf16, train_nr.hip:624, :694-695)
        ps = [shuffle_residual(self.tv[i], xs_[i]).astype(np.float32).astype(np.float64) for i in range(n)]
        return Tape(self.img, x=xs_, t1=self.t1, ps=ps, bl=[None] * n, net=self.net,
                    g_t1=[a > 0 for a in self.t1], g_tv=[a > 0 for a in self.tv], g_net=[a > 0 for a in self.net])


# ---------------------------------------------------------------------------------------------
# the fused bf16 forward, stage by stage from the stored maps (check_bf16 with the lrelu)
# ---------------------------------------------------------------------------------------------
def lrelu64(v):
    return np.where(v > 0, v, SLOPE * v)


def hi_lo(b):
    hi, lo = xs.split_hi_lo(b)
    return hi + lo


def fused_stage_t1(x, P, i):
    """t1 = bf16(lrelu(b1' + bf16(W1) bf16(x))), b1' = the hi + lo halves the block kernel's bias MFMA feeds (nr_fused_x16.inc:203-204)"""
    xq, Wq = bf16_round(x), bf16_round(P.w1[i])
    return conv(xq, Wq, hi_lo(P.b1[i]), np.matmul), conv_mag(xq, Wq, P.b1[i])


def fused_stage_y(t1, P, i):
    """y_q = bf16(lrelu(b2' + bf16(W2) t1)), stored before the residual"""
    Wq = bf16_round(P.w2[i])
    return conv(t1, Wq, hi_lo(P.b2[i]), np.matmul), conv_mag(t1, Wq, P.b2[i])


def unplanes(a, nb, h, w):
    """four sub-pixel planes (list or [4, ...], q = 2 di + dj) of [nb, h, w, K] maps -> raster [nb, 2h, 2w, K]"""
    return np.stack(list(a)).reshape(2, 2, nb, h, w, -1).transpose(2, 3, 0, 4, 1, 5).reshape(nb, 2 * h, 2 * w, -1)


def fused_stage_hid(tv, x, P, i):
    """hid_q = bf16(bf16(Wf) y_q + bf16(R_q) bf16(x)): feat_layers BEFORE the blur, no bias, the residual through R_q
    (nr_fused_x16.inc:14-18); returned in raster order [nb, 2h, 2w, CO]"""
    Wq, xq, zero = bf16_round(P.wf[i]), bf16_round(x), np.zeros(P.wf[i].shape[0])
    nb, h, w, _ = x.shape
    Rq = [bf16_round(residual_matrix(P.wf[i], q, f32=True)) for q in range(4)]
    z = conv(shuffle(tv), Wq, 0.0, np.matmul) + unplanes([conv(xq, R, 0.0, np.matmul) for R in Rq], nb, h, w)
    mag = conv_mag(shuffle(tv), Wq, zero) + unplanes([conv_mag(xq, R, zero) for R in Rq], nb, h, w)
    return z, mag


def fused_stage_net(hid, P, i):
    """net = bf16(lrelu(Blur(hid) + bf)) (blur_act_rgb_q_kernel, neural_render_x16.inc:492-494)"""
    return blur(hid) + P.bf[i], blur(np.abs(hid)) + np.abs(P.bf[i])


def fused_stages(sm, x, P):
    """(tag, z64, magnitude, lrelu?, stored bits) of every teacher-forced stage of the fused bf16 forward, each from the STORED
    input of that stage: t1 from the block input, the y planes from t1, hid (where the caller has read it, `sm.hid`) from y and x,
    net from hid"""
    xin = np.asarray(x, dtype=np.float64)
    for i in range(P.n):
        z, mag = fused_stage_t1(xin, P, i)
        yield "t1[%d]" % i, z, mag, True, sm.bits["t1"][i]
        z, mag = fused_stage_y(sm.t1[i], P, i)
        yield "y[%d]" % i, z, mag, True, sm.bits["tv"][i]
        if sm.hid[i] is not None:
            z, mag = fused_stage_hid(sm.tv[i], xin, P, i)
            yield "hid[%d]" % i, z, mag, False, sm.hid_bits[i]
            z, mag = fused_stage_net(sm.hid[i], P, i)
            yield "net[%d]" % i, z, mag, True, sm.bits["net"][i]
        xin = sm.net[i]


def check_stage(stored_bits, z64, mag, act):
    return xs.check_bf16(stored_bits, z64, xs.U * mag, act=lrelu64 if act else None)


def image_from_nets(x, nets, P, absolute=False):
    """the image from the STORED activation maps: the RGB pyramid in float64 (it is fp32 in every path).  absolute: the sum of
    |terms| of the pre-sigmoid rgb instead (the scale of the bf16 image tolerance)."""
    if absolute:
        x, nets, P = np.abs(x), [np.abs(a) for a in nets], P.map(np.abs)
    rgb = rgb_upsample(to_rgb0(x, P, np.matmul))
    for i, net in enumerate(nets):
        rgb = rgb + feat_2_rgb(net, P, i, np.matmul)
        if i < len(nets) - 1:
            rgb = rgb_upsample(rgb)
    return rgb if absolute else sigmoid(rgb)


def emulate_fused(x, P, mm=mm32_seq16):
    """Free-running float32-ordered CPU emulation of the fused bf16 training forward, as a SavedMaps: every stage rounds where the
    kernels do (see fused_stages), so saved-format data of realistic values exists without a GPU."""
    sm = SavedMaps.__new__(SavedMaps)
    sm.kind, sm.t1, sm.tv, sm.bl, sm.net, sm.hid, sm.hid_bits = "fused", [], [], [], [], [], []
    sm.bits = {"t1": [], "tv": [], "net": []}
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    rnd = lambda z32: bf16_round(np.asarray(z32, dtype=np.float32).astype(np.float64))  # noqa: E731
    lin = lambda a, W: mm(f32(a).reshape(-1, a.shape[-1]), np.ascontiguousarray(f32(W).T)).reshape(a.shape[:-1] + (W.shape[0],))  # noqa: E731
    xin = np.asarray(x, dtype=np.float64)
    for i in range(P.n):
        W1q, W2q, Wfq, xq = bf16_round(P.w1[i]), bf16_round(P.w2[i]), bf16_round(P.wf[i]), bf16_round(xin)
        t1 = rnd(lrelu(lin(xq, W1q) + f32(hi_lo(P.b1[i]))))
        tv = rnd(lrelu(lin(t1, W2q) + f32(hi_lo(P.b2[i]))))
        nb, h, w, _ = xin.shape
        hid = rnd(lin(shuffle(tv), Wfq) + unplanes([lin(xq, bf16_round(residual_matrix(P.wf[i], q, f32=True))) for q in range(4)], nb, h, w))
        net = rnd(lrelu(blur(f32(hid)) + f32(P.bf[i])))
        sm.hid.append(hid)
        sm.hid_bits.append(bf16_bits(hid))
        for k, a in (("t1", t1), ("tv", tv), ("net", net)):
            getattr(sm, k).append(a)
            sm.bits[k].append(bf16_bits(a))
        xin = net
    sm.img = image_from_nets(np.asarray(x, dtype=np.float64), sm.net, P).astype(np.float32).astype(np.float64)
    return sm


# =============================================================================================
# The 16-bit INFERENCE renderer (run_x16, neural_render_x16.inc:562-670), forward only, in both map types ("bf16", "fp16" = IEEE
# half): test_gpu_nr_infer_stagewise.py pins it stage by stage from what a call leaves in a caller-owned workspace, the CPU
# test holds the rules to a float32-ordered emulation and to five deliberate faults.
#
# A call over the first k blocks (geometry (fs, C, k, nb)) leaves, in the workspace: hid of block k - 1 as four sub-pixel planes,
# the stored input map of block k - 1 (net[k - 2]; the caller's feature map for k = 1), net[k - 3] in the other ping-pong
# buffer, the fp32 pyramid planes levels k - 1 and k - 2 read, and returns img.  The last level's net is never stored
# (launch_blur_q gets net == nullptr, :650); t1 and y never leave registers (nr_fused_x16.inc:10-11).  So block k - 1 is pinned
# from the k-block run; net[i] (stored by the (i + 2)-block run) is checked from hid[i] as read after the (i + 1)-block run.
#
#   rgb0          fp32, to_rgb16_kernel on the fp32 map with the fp32 weights (neural_render.hip:146-181): per entry within
#                 MARGIN x NR_X16_RGB0_FLOOR x (|b| + sum |w x|)
#   hid[k - 1]    a chain of three roundings from the block's stored input (x16_hid_chain): the interval rule of check16 with
#                 delta_hid, a per-entry tolerance; the median of delta_hid / magnitude over a stage must stay <= HID_MEDIAN_CAP
#   net[i]        one stage from the stored hid[i]: the bit rule (check16, delta = U (Blur |hid| + |b|), the LeakyReLU) with the
#                 caps of the format (xs.CAPS)
#   pyramid plane / img   fp32, from the stored hid, the stored plane the level read, feat_b and to_rgb_{i + 1} (x16_rgb_stage)
# =============================================================================================
INFER_CASES = dict(GPU_CASES)       # every entry runs the latency form of the block kernel (M <= 768 pixels, nr_fused_x16.inc:397)
INFER_CASES.update({
    (64, 256, 1, 5): 0,             # M = 20 480: the throughput kernel at C = 256 with fp32 input; last level K = 128: blur_mfma_q_kernel<., false>
    (48, 256, 3, 2): 0,             # M = 4 608 (latency form), 18 432, 73 728: the throughput kernel at C = 128 and 64 on 16-bit input;
    #                                 blur_mfma_last_kernel at H = 192; blur_mfma_q_kernel<., true> at K = 128 and 64
    (65, 256, 1, 4): 0,             # M = 16 900 = 528 x 32 + 4: a ragged last tile and a partial workgroup; the odd side: blur_act_rgb_q_kernel
})
LARGE_INFER_CASES = ((64, 256, 1, 5), (48, 256, 3, 2), (65, 256, 1, 4))
TRAIN_TWIN_CASES = ((64, 256, 1, 5), (48, 256, 3, 2))      # the SAVE throughput kernels: the training forward's one-stage bit rule
FORM_CASES = ((4, 256, 4, 1), (48, 256, 3, 2))             # the last level (K = 32, H = 32 / 192) in all three blur forms
IN16_CASE = (64, 256, 1, 5)
FORMATS16 = ("bf16", "fp16")
HID_MEDIAN_CAP = 5e-4               # median of delta_hid / magnitude over a stage, either format (measured on the CPU emulation: <= 2.2e-4
#                                     in bf16, <= 1.8e-4 in IEEE half)
# (the floors of this section's fp32 stages -- NR_X16_RGB0_FLOOR, NR_X16_RGB_FLOOR, NR_X16_SIGMOID_FLOOR -- stand with the other floors at the top)


def al128(n):  # neural_render_x16.inc:576
    return (n + 127) & ~127


def nrf_packed_bytes(C, CO):
    """nrf_dims / nrf_packed_bytes (nr_fused_x16.inc:31-49): the piece stream of a block padded to whole chunks of 24 pieces of
    1 KiB (x16_core.h:19-20), then its 6 C fp32 biases"""
    kxq = C // 64 if C >= 128 else C // 16
    s1, s2, s3 = (2 * C // 32) * (C // 16), (C // 32) * (C // 8), (CO // 32) * (C // 16 + kxq)
    total = s1 + 4 * (s2 + s3)
    return (total + 23) // 24 * 24 * 1024 + 6 * C * 4


def infer_ws_layout(case):
    """The workspace of a 16-bit render over case = (fs, C, blocks, maps), BYTE offsets.  run_x16 (neural_render_x16.inc:567-586)
    carves t1 | ps | hid | netA | netB in 16-bit elements, each rounded up to 128 elements, then planar fp32 rgbA | rgbB; the packed
    block weights sit at the tail of what n3dt_neural_render_workspace_bytes returns, which is the fp32 renderer's carve (nr_carve,
    neural_render.hip:236-251: t1 + ps + bl + 2 net + 2 rgb FLOATS) plus nrf_pack_floats (neural_render_x16.inc:545-552: every
    block's stream rounded up to 256 bytes).  "pack": (offset, bytes) of each block's stream."""
    fs, C, n, nb = case
    e_t1 = e_ps = e_hid = 0
    for i in range(n):
        h = fs << i
        M, ci, co = nb * h * h, nr_ch(C, i), nr_ch(C, i + 1)
        e_t1, e_ps, e_hid = max(e_t1, M * 2 * ci), max(e_ps, 4 * M * ci), max(e_hid, 4 * M * co)
    L, o = {}, 0
    for name, e in (("t1", e_t1), ("ps", e_ps), ("hid", e_hid), ("netA", e_hid), ("netB", e_hid)):
        L[name] = 2 * o
        o += al128(e)
    P = fs << n
    plane = nb * 3 * P * P
    L["rgbA"], L["rgbB"], L["end"] = 2 * o, 2 * o + 4 * plane, 2 * o + 8 * plane
    sizes = [nrf_packed_bytes(nr_ch(C, i), nr_ch(C, i + 1)) for i in range(n)]
    pack = sum(al256(s) for s in sizes)
    L["total"] = 4 * (e_t1 + 2 * e_ps + 2 * e_hid + 2 * plane) + pack
    L["packw"] = L["total"] - pack
    L["pack"], o = [], L["packw"]
    for s in sizes:
        L["pack"].append((o, s))
        o += al256(s)
    return L


def infer_written(case, in16=False):
    """[(offset, bytes)] of everything a call over case's blocks writes into its workspace (the fused path: every block of a
    256-channel renderer is nrf_supported): hid by every block; net[i] of a non-last level into netA (i even) / netB (i odd) (:615-616,
    :650, :664-668); the level-0 projection into rgbB unless the caller brings rgb0 (:598-607); level i < n - 1 writes its pyramid
    plane into rgbA (i even) / rgbB (i odd) (:611-612, :651-654); the packed streams.  t1 and ps are the layered fallback's."""
    fs, C, n, nb = case
    L = infer_ws_layout(case)
    size = {"hid": 0, "netA": 0, "netB": 0, "rgbA": 0, "rgbB": 0 if in16 else 4 * nb * 3 * fs * fs}
    for i in range(n):
        h = fs << i
        M, co = nb * h * h, nr_ch(C, i + 1)
        size["hid"] = max(size["hid"], 2 * 4 * M * co)
        if i < n - 1:
            k = "netA" if i % 2 == 0 else "netB"
            size[k] = max(size[k], 2 * 4 * M * co)
            k = "rgbA" if i % 2 == 0 else "rgbB"
            size[k] = max(size[k], 4 * nb * 3 * 4 * h * h)
    return [(L[k], s) for k, s in size.items() if s] + list(L["pack"])


class InferWs:
    """What a call over case = (fs, C, k, nb) left in its workspace (see the section header), decoded: hid_bits [nb, 2h, 2h, co]
    (raster, h = fs << (k - 1)); lo [nb, h, h, 3] float64, the fp32 plane level k - 1 read; for k >= 2 net_bits (the stored input
    of block k - 1, net[k - 2]) and lo_prev (the plane level k - 2 read); for k >= 3 net_prev_bits (net[k - 3]).
    buf: the workspace as uint8; rgb0: the caller's plane [nb, 3, fs * fs] of the 16-bit-input form (it is never copied)."""

    def __init__(self, buf, case, rgb0=None):
        fs, C, k, nb = case
        L = infer_ws_layout(case)
        u16 = lambda off, cnt: buf[off:off + 2 * cnt].view(np.uint16)  # noqa: E731

        def plane(level):   # the plane level `level` reads: rgbB / rgbA alternate (:611-612, :652-654); level 0 may read the caller's
            h = fs << level
            if level == 0 and rgb0 is not None:
                a = np.asarray(rgb0, dtype=np.float32).reshape(-1)
            else:
                off = L["rgbB"] if level % 2 == 0 else L["rgbA"]
                a = buf[off:off + 4 * nb * 3 * h * h].view(np.float32)
            return np.ascontiguousarray(a.reshape(nb, 3, h, h).transpose(0, 2, 3, 1)).astype(np.float64)

        def net(i):
            h = fs << (i + 1)
            return u16(L["netA"] if i % 2 == 0 else L["netB"], nb * h * h * nr_ch(C, i + 1)).reshape(nb, h, h, nr_ch(C, i + 1)).copy()
        h, co = fs << (k - 1), nr_ch(C, k)
        raw = u16(L["hid"], 4 * nb * h * h * co).reshape(2, 2, nb, h, h, co)
        self.hid_bits = np.ascontiguousarray(raw.transpose(2, 3, 0, 4, 1, 5)).reshape(nb, 2 * h, 2 * h, co)   # planes -> raster
        self.lo = plane(k - 1)
        self.net_bits = net(k - 2) if k >= 2 else None
        self.lo_prev = plane(k - 2) if k >= 2 else None
        self.net_prev_bits = net(k - 3) if k >= 3 else None


def rne(fmt):
    return lambda a: xs.round16(a, fmt)


def trunc16(z, fmt):
    """round toward zero: the fault "net rounded by truncation" """
    p, emin = xs.FORMATS[fmt]
    z = np.asarray(z, dtype=np.float64)
    _, e = np.frexp(np.abs(z))
    ulp = np.ldexp(1.0, np.maximum(e, emin + 1) - p)
    return np.copysign(np.floor(np.abs(z) / ulp) * ulp, z)


def hi_lo16(b, fmt):
    hi, lo = xs.split_hi_lo(b, fmt)
    return hi + lo


class X16Block:
    """The parameters of block i as the fused block kernel sees them: the pack kernel rounds W1, W2, Wf and the fp32 sums R_q to the
    map type, one conversion each (nr_fused_x16.inc:77-104); b1 and b2 enter through one MFMA as hi + lo halves (:203-206,
    x16_core.h:67-69, :100-102)."""

    def __init__(self, P, i, fmt):
        r = rne(fmt)
        self.W1, self.W2, self.Wf = r(P.w1[i]), r(P.w2[i]), r(P.wf[i])
        self.R = [r(residual_matrix(P.wf[i], q, f32=True)) for q in range(4)]
        self.b1, self.b2 = hi_lo16(P.b1[i], fmt), hi_lo16(P.b2[i], fmt)


def lin(a, W):
    return (a.reshape(-1, a.shape[-1]) @ np.ascontiguousarray(W.T)).reshape(a.shape[:-1] + (W.shape[0],))


def round_slack(z, delta, nominal, fmt):
    """per entry: the distance from `nominal` = rne16(lrelu(z)) to the farther of rne16(lrelu(z -+ delta))"""
    r = rne(fmt)
    return np.maximum(np.abs(r(lrelu64(z - delta)) - nominal), np.abs(r(lrelu64(z + delta)) - nominal))


def x16_hid_chain(xin, P, i, fmt):
    """hid of block i from the block's STORED input: t1 and y stay in registers, so this is a chain of three roundings.
    Nominal t1 = rne16(lrelu(z1)); its per-entry slack s1 is the distance to the farther of rne16(lrelu(z1 -+ delta1)), delta1 = U mag1;
    delta_y = U mag_y + s1 |W2q|^T; in the same way delta_hid = U mag_hid + shuffle(s_y) |Wfq|^T.  Returns (z_hid, mag_hid, delta_hid) in
    raster order [nb, 2h, 2w, CO]."""
    w, r, U = X16Block(P, i, fmt), rne(fmt), xs.U
    xq = r(np.asarray(xin, dtype=np.float64))    # the fp32-input kernel rounds the map once (:307-314); a 16-bit map is unchanged
    ax = np.abs(xq)
    z1 = lin(xq, w.W1) + w.b1
    d1 = U * (lin(ax, np.abs(w.W1)) + np.abs(w.b1))
    t1 = r(lrelu64(z1))
    s1 = round_slack(z1, d1, t1, fmt)
    z2 = lin(t1, w.W2) + w.b2
    d2 = lin(U * np.abs(t1) + s1, np.abs(w.W2)) + U * np.abs(w.b2)
    y = r(lrelu64(z2))
    sy = round_slack(z2, d2, y, fmt)
    nb, h, wd, _ = xq.shape
    ys = shuffle(y)
    z3 = lin(ys, w.Wf) + unplanes([lin(xq, R) for R in w.R], nb, h, wd)
    mag3 = lin(np.abs(ys), np.abs(w.Wf)) + unplanes([lin(ax, np.abs(R)) for R in w.R], nb, h, wd)
    return z3, mag3, U * mag3 + lin(shuffle(sy), np.abs(w.Wf))


def x16_check_hid(hid_bits, xin, P, i, fmt):
    """the interval rule with delta_hid; "median" / "max": delta_hid / magnitude over the stage"""
    z, mag, d = x16_hid_chain(xin, P, i, fmt)
    st = xs.check16(hid_bits, z, d, fmt)
    ratio = d[mag > 0] / mag[mag > 0]
    st["median"], st["max"] = float(np.median(ratio)), float(ratio.max())
    return st


def x16_check_net(net_bits, hid, P, i, fmt):
    """net[i] = rne16(lrelu(Blur(hid) / 16 + bf)) with the fp32 bias (nr_blur_mfma.inc:289-292, neural_render_x16.inc:492-494): one stage"""
    z, mag = fused_stage_net(hid, P, i)
    return xs.check16(net_bits, z, xs.U * mag, fmt, act=lrelu64)


def blur_form(nb, H, W, K, env=None):
    """which kernel launch_blur_q picks for a level of INPUT resolution H x W (nr_blur_mfma.inc:654-711): "mfma" (blur_mfma_q_kernel,
    blur_mfma_last_kernel: feat_2_rgb's weights enter as hi + lo halves, :12-14, :64-76, :388-401) or "scalar" (blur_act_rgb_q_kernel:
    the fp32 weights themselves, neural_render_x16.inc:496-498)"""
    env = env or {}
    if env.get("N3DT_NR_BLUR_MFMA") == "0" or H < 2 or W < 4 or (H & 1) or (W & 3) or (K & 31) or K > 256:
        return "scalar"
    return "mfma" if 4 * nb * H * W * K * 2 < (1 << 31) else "scalar"


def up_matrix(n, fault=None):
    """rgb_upsample along one axis: the blur of the bilinear x2.  fault "bilinear_swap": the two outer taps (0.3125 / 0.0625) of every
    interior output swapped between even and odd outputs."""
    U = blur_matrix(2 * n) @ bilinear_matrix(n)
    if fault == "bilinear_swap":
        for o in range(2, 2 * n - 2):
            b = o >> 1
            U[o, b - 1], U[o, b + 1] = U[o, b + 1], U[o, b - 1]
    return U


def x16_rgb_stage(hid, net, lo, P, i, fmt, form):
    """The fp32 output of level i before the sigmoid, from the STORED hid [nb, 2h, 2h, CO], the stored plane `lo` [nb, h, h, 3] the level
    read, feat_b and to_rgb_{i + 1}: pre = Wrgb' net + brgb + rgb_upsample(lo), net the 16-bit activation (the kernels round it before
    feat_2_rgb, nr_blur_mfma.inc:25-27, :292, neural_render_x16.inc:494-495) and Wrgb' = hi + lo in the matrix-pipe forms.  net: the
    stored map of a non-last level; None on the last level, whose net is never stored: the nominal rne16(lrelu(z)) then, and its
    rounding slack s_net (round_slack under delta = U mag) enters the bound as sum |Wrgb| s_net.
    Returns (pre, S = |brgb| + sum |w net| + rgb_upsample |lo|, slack)."""
    W = hi_lo16(P.rgb_w[i + 1], fmt) if form == "mfma" else np.asarray(P.rgb_w[i + 1], dtype=np.float64)
    slack = 0.0
    if net is None:
        z, mag = fused_stage_net(hid, P, i)
        net = rne(fmt)(lrelu64(z))
        slack = lin(round_slack(z, xs.U * mag, net, fmt), np.abs(W))
    pre = lin(net, W) + P.rgb_b[i + 1] + rgb_upsample(lo)
    S = lin(np.abs(net), np.abs(W)) + np.abs(P.rgb_b[i + 1]) + rgb_upsample(np.abs(lo))
    return pre, S, slack


def x16_rgb_bounds(pre, S, slack):
    """(bound of the pre-sigmoid plane, bound of img): MARGIN x NR_X16_RGB_FLOOR x S + slack, and through the sigmoid
    sigma'(pre) x that + MARGIN x NR_X16_SIGMOID_FLOOR"""
    b = MARGIN * NR_X16_RGB_FLOOR * S + slack
    s = sigmoid(pre)
    return b, s * (1.0 - s) * b + MARGIN * NR_X16_SIGMOID_FLOOR


def worst_ratio(got, want, bound):
    """(largest |got - want| / bound, its index)"""
    r = np.abs(np.asarray(got, dtype=np.float64) - want) / bound
    j = int(np.argmax(r))
    return float(r.reshape(-1)[j]), tuple(int(v) for v in np.unravel_index(j, r.shape))


def rgb0_stage(x, P):
    """(rgb0, S) of the level-0 projection of the fp32 map: fp32 weights, nothing is rounded"""
    return conv(x, P.rgb_w[0], P.rgb_b[0], np.matmul), conv_mag(x, P.rgb_w[0], P.rgb_b[0])


# ---- float32-ordered emulations -------------------------------------------------------------
RGB_ORDERS = (("16-wide sequential, rows first", mm32_seq16, True), ("torch.matmul, columns first", mm32_torch, False))


def sep32(A, x, rows_first):
    return sep(A.astype(np.float32), np.asarray(x, dtype=np.float32), rows_first)


def rgb_pre32(net, lo, W, b, mm, rows_first, fault=None):
    """the pre-sigmoid value of a level in float32 from fixed activations"""
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    z = mm(f32(net).reshape(-1, net.shape[-1]), np.ascontiguousarray(f32(W).T)).reshape(net.shape[:-1] + (3,))
    return z + f32(b) + sep32(up_matrix(lo.shape[1], fault), lo, rows_first)


def sigmoid32(z, use_torch=False):
    z = np.asarray(z, dtype=np.float32)
    if use_torch:
        return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(z))).numpy()
    return (np.float32(1) / (np.float32(1) + np.exp(-z))).astype(np.float32)


INFER_FAULTS = ("k_block", "residual_plane", "reflect", "bilinear_swap", "net_trunc")


def emulate_infer(x, P, fmt, mm=mm32_seq16, fault=None):
    """Free-running float32-ordered CPU emulation of the 16-bit inference renderer in map type fmt: every stage rounds where the kernels
    do, so workspace-format data of realistic values exists without a GPU.  Per block i: the 16-bit patterns t1_bits, y_bits (in
    registers on the GPU), hid_bits, net_bits (the last level's too; emu_map decodes one); lo[i] the fp32 plane level i reads
    (lo[0] = rgb0), pre[i] what it writes (= lo[i + 1]), img[i] = the image of the call over the first i + 1 blocks.
    fault: one of INFER_FAULTS --
      k_block         one 32-wide k-block (32 .. 63) of the layer_2 product dropped in the first 32-pixel tile of block 0
      residual_plane  R_q taken from the next sub-pixel plane
      reflect         the blur's reflected row above the first row read off by one (row 0 instead of row 1)
      bilinear_swap   rgb_upsample's two outer taps swapped (up_matrix)
      net_trunc       net rounded toward zero"""
    assert fault is None or fault in INFER_FAULTS
    r = rne(fmt)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    rnd = lambda z32: r(f32(z32).astype(np.float64))  # noqa: E731
    lin32 = lambda a, W: mm(f32(a).reshape(-1, a.shape[-1]), np.ascontiguousarray(f32(W).T)).reshape(a.shape[:-1] + (W.shape[0],))  # noqa: E731
    x = np.asarray(x, dtype=np.float64)
    e = {k: [] for k in ("t1_bits", "y_bits", "hid_bits", "net_bits", "pre", "img")}
    e["fmt"] = fmt
    e["lo"] = [(lin32(x, P.rgb_w[0]) + f32(P.rgb_b[0])).astype(np.float64)]
    xin = x
    for i in range(P.n):
        w = X16Block(P, i, fmt)
        nb, h, wd, _ = xin.shape
        xq = r(xin)
        t1 = rnd(lrelu(lin32(xq, w.W1) + f32(w.b1)))
        z2 = lin32(t1, w.W2) + f32(w.b2)
        if fault == "k_block" and i == 0:
            cut = t1.copy().reshape(-1, t1.shape[-1])
            cut[:, 32:64] = 0.0
            rows = min(32, cut.shape[0])
            z2.reshape(-1, z2.shape[-1])[:rows] = (lin32(cut[:rows], w.W2) + f32(w.b2))
        y = rnd(lrelu(z2))
        Rs = w.R[1:] + w.R[:1] if fault == "residual_plane" else w.R
        hid = rnd(lin32(shuffle(y), w.Wf) + unplanes([lin32(xq, R) for R in Rs], nb, h, wd))
        bl = blur(f32(hid))
        if fault == "reflect":
            B = blur_matrix(2 * h)
            Bc = B.copy()
            B[0] = 0.0
            B[0, 0], B[0, 1] = 0.75, 0.25
            bl = np.einsum("jw,niwc->nijc", Bc.astype(np.float32), np.einsum("ih,nhwc->niwc", B.astype(np.float32), f32(hid)))
        zn = lrelu(bl + f32(P.bf[i])).astype(np.float64)
        net = trunc16(zn, fmt) if fault == "net_trunc" else r(zn)
        pre = rgb_pre32(net, e["lo"][i], hi_lo16(P.rgb_w[i + 1], fmt), P.rgb_b[i + 1], mm, True, fault)
        for k, a in (("t1", t1), ("y", y), ("hid", hid), ("net", net)):
            e[k + "_bits"].append(xs.bits16(a, fmt))      # (only the patterns are kept: the large cases' maps are hundreds of MB in float64)
        e["pre"].append(pre.astype(np.float64))
        e["lo"].append(pre.astype(np.float64))
        e["img"].append(sigmoid32(pre).astype(np.float64))
        xin = net
    return e


def emu_map(e, k, i):
    """map k ("t1", "y", "hid", "net") of block i of an emulation as float64"""
    return xs.bits16_to_f64(e[k + "_bits"][i], e["fmt"])


def x16_one_stage(e, x, P, fmt):
    """(tag, z64, magnitude, lrelu?, bits) of the ONE-stage rule on every rounding of an emulation, each from the stage's own stored
    input (t1 and y are observable on the CPU only; on the GPU the training twin stores them)"""
    xin = np.asarray(x, dtype=np.float64)
    for i in range(P.n):
        w = X16Block(P, i, fmt)
        nb, h, wd, _ = xin.shape
        xq = rne(fmt)(xin)
        yield "t1[%d]" % i, lin(xq, w.W1) + w.b1, lin(np.abs(xq), np.abs(w.W1)) + np.abs(w.b1), True, e["t1_bits"][i]
        t1 = emu_map(e, "t1", i)
        yield "y[%d]" % i, lin(t1, w.W2) + w.b2, lin(np.abs(t1), np.abs(w.W2)) + np.abs(w.b2), True, e["y_bits"][i]
        ys = shuffle(emu_map(e, "y", i))
        z = lin(ys, w.Wf) + unplanes([lin(xq, R) for R in w.R], nb, h, wd)
        mag = lin(np.abs(ys), np.abs(w.Wf)) + unplanes([lin(np.abs(xq), np.abs(R)) for R in w.R], nb, h, wd)
        yield "hid[%d]" % i, z, mag, False, e["hid_bits"][i]
        z, mag = fused_stage_net(emu_map(e, "hid", i), P, i)
        yield "net[%d]" % i, z, mag, True, e["net_bits"][i]
        xin = emu_map(e, "net", i)
