"""Stage-by-stage float64 restatement of the Audio2style encoder's forward and BPTT (n3dt_launch_a2s_fwd / _bwd of
csrc/audio_lstm.hip: the recurrent step kernels, the dropout and column-sum kernels, and the fp32 kernel of csrc/gemm32.hip they
call), for the tests that pin it (test_a2s_stagewise_cpu.py, test_gpu_a2s_stagewise.py).  A helper module, not a test file: CPU
only, numpy.

The forward keeps X0, H[2], G[2], C[2], A[3], S[3], Y[2] in `saved` and the input projections XP[l] in its workspace; the backward
leaves the pre-activation gradients DG[l] (over XP[l]), the cell gradients DC[l], DH1, DH0, DZ3, DY2, DY1 in its workspace and
every parameter gradient in the arena.  Every stage is recomputed in float64 from the kernel's own stored inputs ("teacher-forced")
and compared per entry:

    |got - z64| <= u_family * S          S = float64 sum of the absolute terms of that entry

S follows the formulas as the kernels write them: a product is |b| + sum |w x|; `1 - tc * tc` and `g * (1 - g)` contribute |1| and
the square (1 + tc^2, g (1 + g)), so their cancellation is inside S and not excused; an activation is act'(pre64) S_pre + |act|.
LeakyReLU gates of the backward are read from the stored A[k] > 0.  No entry is left out of any comparison and there is no
ambiguity band: LeakyReLU is continuous, and the backward's gates are stored.

Weights.  "seed": n3dt.Audio2style() under torch.manual_seed(5 + seed).  "sharp": the same with the four LSTM tensors (weight_ih,
weight_hh, bias_ih, bias_hh, both directions) of layer l multiplied by SHARP[l].  With the seeded weights every layer-1 gate sits
at 0.5 +- 0.05, so sigma' and tanh' are nearly constant and a wrong derivative factor hides; SHARP was chosen on the CPU so that
in every layer and direction of every sharp case between 10 % and 50 % of the pre-activations have |pre| > 6, at least 10 % have
|pre| < 1, and max |c| >= 3 (test_a2s_stagewise_cpu.py asserts it; at T = 2 a cell state cannot pass 2, since |c_t| <= |c_tp| + 1,
so case t2 is held to max |c| >= 1.5 instead).

Bounds.  Every u_family is FACTOR = 4 times a floor measured on the CPU alone (FLOOR below, re-measured by
test_a2s_stagewise_cpu.py, which fails if a recorded floor is below the measured one or more than twice it): the largest
|z32 - z64| / S of a float32 emulation of the kernels' arithmetic -- products in 16-wide k blocks for the free-running emulation
and the single-fmaf chain of v_mfma_f32_32x32x2_f32 on sampled rows and columns, the ten-element lane partials and xor butterfly
of a2s_step_fwd, the strided rows, butterfly and ordered four-wave sum of a2s_step_bwd, the sequential column sums, numpy's
float32 exp / tanh for expf / tanhf -- over all cases and three seeds.  No bound comes from a GPU run.
"""

import numpy as np
import torch

IN, H, G = 1280, 640, 2560
LIN = ((1280, 640), (640, 320), (320, 64))
GRAD_FLOATS = 20726784            # include/n3dt.h: N3DT_A2S_GRAD_FLOATS
K_STRIDE = G * IN + G * H + 2 * G
FACTOR = 4.0
SHARP = (3.0, 16.0)               # per layer; the shares they give are printed by test_a2s_stagewise_cpu.py::test_the_cases_reach...

# measured floors: largest |z32 - z64| / S of the float32 emulation per family (test_a2s_stagewise_cpu.py::test_floors)
FLOOR = {
    "xp": 4.3e-07,   # measured 3.04e-07
    "gate": 2.0e-07,   # measured 1.42e-07
    "cell": 1.6e-07,   # measured 1.17e-07
    "hidden": 2.3e-07,   # measured 1.63e-07
    "lin": 4.5e-07,   # measured 3.18e-07
    "dx": 2.9e-07,   # measured 2.07e-07
    "dh0": 4.8e-07,   # measured 3.44e-07
    "dc": 1.6e-07,   # measured 1.14e-07
    "dgate": 1.6e-07,   # measured 1.13e-07
    "dw": 1.1e-06,   # measured 7.62e-07
    "colsum": 1.2e-06,   # measured 8.32e-07
}

CASES = {
    "t1": dict(T=1, weights="seed", masks=True),
    "t2": dict(T=2, weights="sharp", masks=True),
    "t5": dict(T=5, weights="seed", masks=False),
    "t17": dict(T=17, weights="sharp", masks=True),
    "t33": dict(T=33, weights="seed", masks=True),
    "t130": dict(T=130, weights="sharp", masks=True),
}

FAULTS = {   # fault -> the stages (tag prefixes) that own it
    "fgrad_c": ("DG",),          # the forget-gate gradient uses c[t] for c_prev
    "carry_f": ("DC", "DG"),     # the dc carry uses f[t] for f[tn] (the DG stage recomputes dc from the stored inputs, so it sees it too)
    "whh_rev_pair": ("dW_hh",),  # the reverse direction's dW_hh pairs with h[t-1]
    "bhh_s0": ("G",),            # b_hh dropped at s = 0
    "dh0_fwd_only": ("DH0",),    # DH0 without the reverse direction's product
    "o_for_i": ("DG",),          # the o-gate derivative used for the i gate
    "bias_twice": ("XP",),       # b_ih added twice in XP
}


def bound(family):
    return FACTOR * FLOOR[family]


def f64(a):
    return np.asarray(a).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# layouts (audio_lstm.hip: a2s_saved, a2s_ws; include/n3dt.h: the grad arena), float offsets
# ---------------------------------------------------------------------------------------------------------------------
def _offsets(sizes):
    out, o = {}, 0
    for name, n in sizes:
        out[name] = (o, n)
        o += n
    out["total"] = o
    return out


def saved_layout(T):
    sizes = [("X0", IN * T), ("H0", 2 * H * T), ("H1", 2 * H * T), ("G0", 2 * G * T), ("G1", 2 * G * T), ("C0", 2 * H * T), ("C1", 2 * H * T)]
    sizes += [("A%d" % k, LIN[k][1] * T) for k in range(3)] + [("S%d" % k, LIN[k][1] * T) for k in range(3)] + [("Y%d" % k, LIN[k][1] * T) for k in range(2)]
    return _offsets(sizes)


def ws_layout(T):
    return _offsets([("XP0", 2 * G * T), ("XP1", 2 * G * T), ("DC0", 2 * H * T), ("DC1", 2 * H * T), ("DH1", 2 * H * T), ("DH0", 2 * H * T),
                     ("DZ3", 64 * T), ("DY2", 320 * T), ("DY1", 640 * T)])


def arena_layout():
    sizes = []
    for k in range(4):
        sizes += [("W_ih%d" % k, G * IN), ("W_hh%d" % k, G * H), ("b_ih%d" % k, G), ("b_hh%d" % k, G)]
    for k in range(3):
        sizes += [("W%d" % k, LIN[k][0] * LIN[k][1]), ("b%d" % k, LIN[k][1])]
    return _offsets(sizes)


def library_totals(T):
    """(n3dt_a2s_saved_bytes, n3dt_a2s_workspace_bytes) of the built library"""
    from n3dt import _lib
    L = _lib.lib()
    return int(L.n3dt_a2s_saved_bytes(T)), int(L.n3dt_a2s_workspace_bytes(T))


class _View:
    def _v(self, buf, L, k, shape):
        o, n = L[k]
        return buf[o:o + n].reshape(shape)


class Saved(_View):
    def __init__(self, buf, T):
        buf, L = np.asarray(buf).reshape(-1), saved_layout(T)
        assert buf.size == L["total"]
        self.buf = buf
        self.X0 = self._v(buf, L, "X0", (T, IN))
        self.H = [self._v(buf, L, "H%d" % l, (T, 2 * H)) for l in range(2)]
        self.G = [self._v(buf, L, "G%d" % l, (2, T, G)) for l in range(2)]
        self.C = [self._v(buf, L, "C%d" % l, (2, T, H)) for l in range(2)]
        self.A = [self._v(buf, L, "A%d" % k, (T, LIN[k][1])) for k in range(3)]
        self.S = [self._v(buf, L, "S%d" % k, (T, LIN[k][1])) for k in range(3)]
        self.Y = [self._v(buf, L, "Y%d" % k, (T, LIN[k][1])) for k in range(2)]


class Workspace(_View):
    """XP[l] is what the forward leaves there, DG[l] (the same floats) what the backward does"""
    def __init__(self, buf, T):
        buf, L = np.asarray(buf).reshape(-1), ws_layout(T)
        assert buf.size == L["total"]
        self.buf = buf
        self.XP = [self._v(buf, L, "XP%d" % l, (2, T, G)) for l in range(2)]
        self.DG = self.XP
        self.DC = [self._v(buf, L, "DC%d" % l, (2, T, H)) for l in range(2)]
        self.DH1, self.DH0 = self._v(buf, L, "DH1", (T, 2 * H)), self._v(buf, L, "DH0", (T, 2 * H))
        self.DZ3, self.DY2, self.DY1 = self._v(buf, L, "DZ3", (T, 64)), self._v(buf, L, "DY2", (T, 320)), self._v(buf, L, "DY1", (T, 640))


class Arena(_View):
    def __init__(self, buf):
        buf, L = np.asarray(buf).reshape(-1), arena_layout()
        assert buf.size == L["total"] == GRAD_FLOATS
        self.buf = buf
        self.W_ih = [self._v(buf, L, "W_ih%d" % k, (G, IN)) for k in range(4)]
        self.W_hh = [self._v(buf, L, "W_hh%d" % k, (G, H)) for k in range(4)]
        self.b_ih = [self._v(buf, L, "b_ih%d" % k, (G,)) for k in range(4)]
        self.b_hh = [self._v(buf, L, "b_hh%d" % k, (G,)) for k in range(4)]
        self.W = [self._v(buf, L, "W%d" % k, (LIN[k][1], LIN[k][0])) for k in range(3)]
        self.b = [self._v(buf, L, "b%d" % k, (LIN[k][1],)) for k in range(3)]

    def by_name(self):
        """{state-dict name: gradient} of the 22 trained tensors"""
        out = {}
        for k in range(4):
            sfx = "_l%d%s" % (k // 2, "_reverse" if k % 2 else "")
            for n, v in (("weight_ih", self.W_ih), ("weight_hh", self.W_hh), ("bias_ih", self.b_ih), ("bias_hh", self.b_hh)):
                out["rnn.rnn." + n + sfx] = v[k]
        for k in range(3):
            out["linear%d.0.weight" % (k + 1)], out["linear%d.0.bias" % (k + 1)] = self.W[k], self.b[k]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
_SD = {}


def state_dict(weights, seed=0):
    """the seeded module's state dict (torch, float32); "sharp": the LSTM tensors of layer l times SHARP[l]"""
    if (weights, seed) not in _SD:
        if ("seed", seed) not in _SD:
            from n3dt import Audio2style
            rng = torch.get_rng_state()
            torch.manual_seed(5 + seed)
            _SD[("seed", seed)] = {k: v.detach().clone() for k, v in Audio2style().state_dict().items()}
            torch.set_rng_state(rng)
        sd = dict(_SD[("seed", seed)])
        if weights == "sharp":
            for k in list(sd):
                if k.startswith("rnn.rnn."):
                    sd[k] = sd[k] * SHARP[1 if "_l1" in k else 0]
        else:
            assert weights == "seed"
        _SD[(weights, seed)] = sd
    return _SD[(weights, seed)]


def case_inputs(name, seed=0, sharp=None, weights=None):
    """Everything a run of a case takes, seeded: T, the 22 parameter arrays (float32 numpy), mel [T, 1280], the three keep masks (or
    None: eval), the cotangent [T, 64].  weights: in place of the case's own kind."""
    from n3dt import synthetic as syn
    c = CASES[name]
    T = c["T"]
    sd = state_dict(weights or c["weights"], seed)
    if sharp is not None:   # another pair of factors (the search that chose SHARP)
        base = state_dict("seed", seed)
        sd = {k: (v * sharp[1 if "_l1" in k else 0] if k.startswith("rnn.rnn.") else v) for k, v in base.items()}
    n = lambda k: sd[k].numpy()  # noqa: E731
    sfx = ["_l%d%s" % (k // 2, "_reverse" if k % 2 else "") for k in range(4)]
    gen = torch.Generator().manual_seed(1000 * seed + T)
    masks = [(torch.rand(T, o, generator=gen) < 0.5).float() for _, o in LIN] if c["masks"] else None
    cot = torch.randn(T, 64, generator=gen)
    return dict(name=name, T=T, sd=sd, mel_t=syn.mel_batch(T, seed=1000 * seed + T), masks_t=masks, cot_t=cot,
                w_ih=[n("rnn.rnn.weight_ih" + s) for s in sfx], w_hh=[n("rnn.rnn.weight_hh" + s) for s in sfx],
                b_ih=[n("rnn.rnn.bias_ih" + s) for s in sfx], b_hh=[n("rnn.rnn.bias_hh" + s) for s in sfx],
                lin_w=[n("linear%d.0.weight" % (k + 1)) for k in range(3)], lin_b=[n("linear%d.0.bias" % (k + 1)) for k in range(3)],
                mel=syn.mel_batch(T, seed=1000 * seed + T).reshape(T, IN).numpy(), masks=None if masks is None else [m.numpy() for m in masks],
                cot=cot.numpy())


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32 order / float64
# ---------------------------------------------------------------------------------------------------------------------
def mm(dt, A, B):
    """A [M, K] B[N, K]^T: float64 exactly, float32 as 16-wide k blocks in sequence (the staging steps of gemm32_kernel)"""
    if dt is np.float64:
        return A @ B.T
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for k0 in range(0, A.shape[1], 16):
        acc = acc + A[:, k0:k0 + 16] @ B[:, k0:k0 + 16].T
    return acc


def mm_fma_chain(A, B, acc=None):
    """the single-fmaf chain of v_mfma_f32_32x32x2_f32: one product at a time in ascending k, each step rounded once to float32
    (the product of two float32 values is exact in float64)"""
    A, B = np.asarray(A, dtype=np.float32).astype(np.float64), np.asarray(B, dtype=np.float32).astype(np.float64)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32) if acc is None else acc
    for k in range(A.shape[1]):
        acc = (acc.astype(np.float64) + A[:, k:k + 1] * B[None, :, k]).astype(np.float32)
    return acc


def butterfly_sum(v):
    """__shfl_xor butterfly over the last axis (64 lanes), offsets 32 .. 1: every lane ends with the same sum"""
    lanes = np.arange(v.shape[-1])
    off = v.shape[-1] // 2
    while off > 0:
        v = v + v[..., lanes ^ off]
        off >>= 1
    return v


def rec_fwd(dt, W64, h):
    """a2s_step_fwd's W_hh h_prev: W64 [2560, 640] (float64 copy of the float32 weights), h [640] -> [2560].  Lane L holds elements
    2 L + 128 i + j (i < 5, j < 2) and chains ten fmaf over them in that order; a butterfly adds the 64 lanes."""
    if dt is np.float64:
        return W64 @ h
    Wr, hr = W64.reshape(G, 5, 64, 2), h.astype(np.float64).reshape(5, 64, 2)
    acc = np.zeros((G, 64), dtype=np.float32)
    for i in range(5):
        for j in range(2):
            acc = (acc.astype(np.float64) + Wr[:, i, :, j] * hr[i, :, j]).astype(np.float32)
    return butterfly_sum(acc)[:, 0]


def rec_bwd(dt, W64, dgn):
    """a2s_step_bwd's W_hh^T dgates_next: thread tid chains rows r = tid + 256 i (i < 10) with fmaf, a butterfly adds the 64 lanes of
    a wave, the four waves are added in order"""
    if dt is np.float64:
        return W64.T @ dgn
    Wr, dr = W64.reshape(10, 4, 64, H), dgn.astype(np.float64).reshape(10, 4, 64)
    acc = np.zeros((4, 64, H), dtype=np.float32)
    for i in range(10):
        acc = (acc.astype(np.float64) + Wr[i] * dr[i][:, :, None]).astype(np.float32)
    p = butterfly_sum(np.ascontiguousarray(acc.transpose(0, 2, 1)))[..., 0]
    return ((p[0] + p[1]) + p[2]) + p[3]


def colsum(dt, X):
    """a2s_colsum: the rows added in order"""
    if dt is np.float64:
        return X.sum(axis=0)
    acc = np.zeros(X.shape[1], dtype=dt)
    for t in range(X.shape[0]):
        acc = acc + X[t]
    return acc


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))   # in x's dtype: a2s_sigmoid


def lrelu(v):
    return np.where(v > 0, v, v.dtype.type(0.2) * v)


def prev_of(T, d, t):
    """(has_prev, tp): the step before t in direction d's forward order"""
    return (t < T - 1, t + 1) if d else (t > 0, t - 1)


def next_of(T, d, t):
    """(has_next, tn): the step whose gradients the backward formed just before t's"""
    return (t > 0, t - 1) if d else (t < T - 1, t + 1)


# ---------------------------------------------------------------------------------------------------------------------
# the whole path in one dtype: float32 = the free-running CPU emulation, float64 = the restatement run end to end
# ---------------------------------------------------------------------------------------------------------------------
def run_path(inp, dt=np.float32, fault=None):
    """-> record dict(saved=Saved, wsf=Workspace after the forward, wsb=Workspace after the backward, arena=Arena, out [T, 64]): what
    a synchronised n3dt_a2s_fwd + n3dt_a2s_bwd on separate workspaces leaves behind, computed in `dt`.  fault: a key of FAULTS."""
    assert fault is None or fault in FAULTS
    T = inp["T"]
    one = dt(1)
    c = lambda a: np.asarray(a).astype(dt)  # noqa: E731
    w_ih, w_hh, b_ih, b_hh = ([c(a) for a in inp[k]] for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
    lin_w, lin_b = [c(a) for a in inp["lin_w"]], [c(a) for a in inp["lin_b"]]
    w_hh64 = [f64(a) for a in w_hh] if dt is np.float32 else w_hh
    sv = Saved(np.zeros(saved_layout(T)["total"], dtype=dt), T)
    wf, wb = Workspace(np.zeros(ws_layout(T)["total"], dtype=dt), T), Workspace(np.zeros(ws_layout(T)["total"], dtype=dt), T)
    ar = Arena(np.zeros(GRAD_FLOATS, dtype=dt))
    # ---- forward
    sv.X0[:] = c(inp["mel"])
    for l in range(2):
        X = sv.X0 if l == 0 else sv.H[0]
        for d in range(2):
            k = 2 * l + d
            wf.XP[l][d] = mm(dt, X, w_ih[k]) + b_ih[k]
            if fault == "bias_twice" and k == 3:
                wf.XP[l][d] += b_ih[k]
        for s in range(T):
            for d in range(2):
                k = 2 * l + d
                t = T - 1 - s if d else s
                has_prev, tp = prev_of(T, d, t)
                if has_prev:
                    acc = rec_fwd(dt, w_hh64[k], sv.H[l][tp, d * H:(d + 1) * H])
                    pre = wf.XP[l][d, t] + (acc + b_hh[k])
                elif fault == "bhh_s0":
                    pre = wf.XP[l][d, t].copy()
                else:
                    pre = wf.XP[l][d, t] + (dt(0) + b_hh[k])
                ig, fg, gg, og = sigmoid(pre[:H]), sigmoid(pre[H:2 * H]), np.tanh(pre[2 * H:3 * H]), sigmoid(pre[3 * H:])
                cp = sv.C[l][d, tp] if has_prev else np.zeros(H, dtype=dt)
                cc = fg * cp + ig * gg
                sv.G[l][d, t] = np.concatenate([ig, fg, gg, og])
                sv.C[l][d, t] = cc
                sv.H[l][t, d * H:(d + 1) * H] = og * np.tanh(cc)
    X = sv.H[1]
    out = None
    for k in range(3):
        sv.A[k][:] = lrelu(mm(dt, X, lin_w[k]) + lin_b[k])
        sv.S[k][:] = c(inp["masks"][k]) * dt(2) if inp["masks"] is not None else one
        Y = sv.A[k] * sv.S[k]
        if k < 2:
            sv.Y[k][:] = Y
        else:
            out = Y
        X = Y
    # ---- backward: the head, last layer first
    dz = [wb.DY1, wb.DY2, wb.DZ3]
    xin = [sv.H[1], sv.Y[0], sv.Y[1]]
    dx_out = [wb.DH1, wb.DY1, wb.DY2]
    dy = c(inp["cot"])
    for k in (2, 1, 0):
        v = dy * sv.S[k]
        dz[k][:] = np.where(sv.A[k] > 0, v, v * dt(0.2))
        ar.W[k][:] = mm(dt, np.ascontiguousarray(dz[k].T), np.ascontiguousarray(xin[k].T))
        ar.b[k][:] = colsum(dt, dz[k])
        dx_out[k][:] = mm(dt, dz[k], np.ascontiguousarray(lin_w[k].T))
        dy = dx_out[k]
    # ---- BPTT
    for l in (1, 0):
        dHout = wb.DH1 if l else wb.DH0
        DG, DC, Gs, Cs = wb.DG[l], wb.DC[l], sv.G[l], sv.C[l]
        for s in range(T):
            for d in range(2):
                k = 2 * l + d
                t = s if d else T - 1 - s
                has_next, tn = next_of(T, d, t)
                rec = rec_bwd(dt, w_hh64[k], DG[d, tn]) if has_next else np.zeros(H, dtype=dt)
                g = Gs[d, t]
                ig, fg, gg, og = g[:H], g[H:2 * H], g[2 * H:3 * H], g[3 * H:]
                tc = np.tanh(Cs[d, t])
                dh = dHout[t, d * H:(d + 1) * H] + rec
                dc = (dh * og) * (one - tc * tc)
                if has_next:
                    dc = dc + DC[d, tn] * (fg if fault == "carry_f" else Gs[d, tn, H:2 * H])
                has_prev, tp = prev_of(T, d, t)
                cp = Cs[d, tp] if has_prev else np.zeros(H, dtype=dt)
                if fault == "fgrad_c":
                    cp = Cs[d, t]
                di = ig * (one - ig) if fault != "o_for_i" else og * (one - og)
                DG[d, t] = np.concatenate([(dc * gg) * di, (dc * cp) * (fg * (one - fg)), (dc * ig) * (one - gg * gg), (dh * tc) * (og * (one - og))])
                DC[d, t] = dc
        X = sv.H[0] if l else sv.X0
        for d in range(2):
            k = 2 * l + d
            ar.W_ih[k][:] = mm(dt, np.ascontiguousarray(DG[d].T), np.ascontiguousarray(X.T))
            if T > 1:
                if d == 0:
                    a, hb = DG[0, 1:], sv.H[l][:-1, :H]
                elif fault == "whh_rev_pair":
                    a, hb = DG[1, 1:], sv.H[l][:-1, H:]
                else:
                    a, hb = DG[1, :-1], sv.H[l][1:, H:]
                ar.W_hh[k][:] = mm(dt, np.ascontiguousarray(a.T), np.ascontiguousarray(hb.T))
            ar.b_ih[k][:] = colsum(dt, DG[d])
            ar.b_hh[k][:] = ar.b_ih[k]
        if l == 1:
            wb.DH0[:] = mm(dt, DG[0], np.ascontiguousarray(w_ih[2].T))
            if fault != "dh0_fwd_only":
                wb.DH0[:] = wb.DH0 + mm(dt, DG[1], np.ascontiguousarray(w_ih[3].T))
    return {"saved": sv, "wsf": wf, "wsb": wb, "arena": ar, "out": out}


# ---------------------------------------------------------------------------------------------------------------------
# the teacher-forced stage checks
# ---------------------------------------------------------------------------------------------------------------------
def prod64(X, Wm, bias=None):
    """z = X Wm^T (+ bias) and S = |bias| + |X| |Wm|^T"""
    X, Wm = f64(X), f64(Wm)
    z, S = X @ Wm.T, np.abs(X) @ np.abs(Wm).T
    if bias is not None:
        z, S = z + f64(bias), S + np.abs(f64(bias))
    return z, S


def chk(tag, family, buf, got, z, S=0.0, exact=False):
    """buf: which buffer `got` lives in (saved, wsf, wsb, arena, out), for the count of compared floats"""
    got = np.asarray(got)
    if exact:
        z = np.asarray(z)
    else:
        z = np.asarray(z, dtype=np.float64)
    assert got.shape == z.shape, (tag, got.shape, z.shape)
    return dict(tag=tag, family=family, buf=buf, got=got, z=z, S=np.broadcast_to(np.asarray(S, dtype=np.float64), z.shape), exact=exact)


def preacts(inp, rec, l, d):
    """float64 pre-activations [T, 2560] of layer l, direction d from the stored XP and H, and their S"""
    T, k = inp["T"], 2 * l + d
    Hs = f64(rec["saved"].H[l])[:, d * H:(d + 1) * H]
    Hp = np.zeros((T, H))
    for t in range(T):
        has_prev, tp = prev_of(T, d, t)
        if has_prev:
            Hp[t] = Hs[tp]
    xp = f64(rec["wsf"].XP[l][d])
    r, S_r = prod64(Hp, inp["w_hh"][k], inp["b_hh"][k])
    return xp + r, np.abs(xp) + S_r


def shifted(a, T, d, which):
    """rows a[tp] (which = prev_of) or a[tn] (next_of) per t, zero where there is none; and the mask of rows that have one"""
    out, has = np.zeros_like(a), np.zeros(T, dtype=bool)
    for t in range(T):
        h, o = which(T, d, t)
        if h:
            out[t], has[t] = a[o], True
    return out, has


def stages(inp, rec):
    """Every check of a run, as dicts of chk().  inp: case_inputs(); rec: a record as run_path() / the GPU run leaves it."""
    T = inp["T"]
    sv, wf, wb, ar = rec["saved"], rec["wsf"], rec["wsb"], rec["arena"]
    rdt = np.asarray(sv.X0).dtype   # single operations are restated in the record's own type: exact for the fp32 kernels
    out = []
    # ---- forward
    out.append(chk("X0", "copy", "saved", sv.X0, inp["mel"].astype(rdt), exact=True))
    for l in range(2):
        X = sv.X0 if l == 0 else sv.H[0]
        for d in range(2):
            k = 2 * l + d
            z, S = prod64(X, inp["w_ih"][k], inp["b_ih"][k])
            out.append(chk("XP[%d][%d]" % (l, d), "xp", "wsf", wf.XP[l][d], z, S))
            pre, S_pre = preacts(inp, rec, l, d)
            sg = sigmoid(pre)
            th = np.tanh(pre[:, 2 * H:3 * H])
            gate = sg.copy()
            gate[:, 2 * H:3 * H] = th
            dact = sg * (1.0 - sg)
            dact[:, 2 * H:3 * H] = 1.0 - th * th
            out.append(chk("G[%d][%d]" % (l, d), "gate", "saved", sv.G[l][d], gate, dact * S_pre + np.abs(gate)))
            g, Cs = f64(sv.G[l][d]), f64(sv.C[l][d])
            ig, fg, gg, og = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
            cp, _ = shifted(Cs, T, d, prev_of)
            out.append(chk("C[%d][%d]" % (l, d), "cell", "saved", sv.C[l][d], fg * cp + ig * gg, np.abs(fg * cp) + np.abs(ig * gg)))
            h = og * np.tanh(Cs)
            out.append(chk("H[%d][%d]" % (l, d), "hidden", "saved", sv.H[l][:, d * H:(d + 1) * H], h, np.abs(h)))
    X = sv.H[1]
    for k in range(3):
        z, S = prod64(X, inp["lin_w"][k], inp["lin_b"][k])
        out.append(chk("A[%d]" % k, "lin", "saved", sv.A[k], np.where(z > 0, z, 0.2 * z), S))
        s32 = inp["masks"][k].astype(rdt) * rdt.type(2) if inp["masks"] is not None else np.ones((T, LIN[k][1]), dtype=rdt)
        out.append(chk("S[%d]" % k, "copy", "saved", sv.S[k], s32, exact=True))
        Y = sv.Y[k] if k < 2 else rec["out"]
        out.append(chk("Y[%d]" % k if k < 2 else "out", "copy", "saved" if k < 2 else "out", Y, np.asarray(sv.A[k]) * np.asarray(sv.S[k]), exact=True))
        X = Y
    # ---- head backward
    v = inp["cot"].astype(rdt) * np.asarray(sv.S[2])
    out.append(chk("DZ3", "copy", "wsb", wb.DZ3, np.where(np.asarray(sv.A[2]) > 0, v, v * rdt.type(0.2)), exact=True))
    dz = [wb.DY1, wb.DY2, wb.DZ3]
    xin = [sv.H[1], sv.Y[0], sv.Y[1]]
    for k, tag, dst in ((2, "DY2", wb.DY2), (1, "DY1", wb.DY1)):   # dY_{k-1} = dZ_k W_k, then (in place) the dropout and LeakyReLU gate of layer k-1
        z, S = prod64(dz[k], inp["lin_w"][k].T)
        gate = f64(sv.S[k - 1]) * np.where(np.asarray(sv.A[k - 1]) > 0, 1.0, 0.2)
        out.append(chk(tag, "dx", "wsb", dst, z * gate, S * gate))
    z, S = prod64(wb.DY1, inp["lin_w"][0].T)
    out.append(chk("DH1", "dx", "wsb", wb.DH1, z, S))
    for k in range(3):
        a, b = f64(dz[k]), f64(xin[k])
        out.append(chk("dW%d" % (k + 1), "dw", "arena", ar.W[k], a.T @ b, np.abs(a).T @ np.abs(b)))
        out.append(chk("db%d" % (k + 1), "colsum", "arena", ar.b[k], a.sum(axis=0), np.abs(a).sum(axis=0)))
    # ---- BPTT
    for l in (1, 0):
        dHout = f64(wb.DH1 if l else wb.DH0)
        X = f64(sv.H[0] if l else sv.X0)
        for d in range(2):
            k = 2 * l + d
            DG, DC, g, Cs = f64(wb.DG[l][d]), f64(wb.DC[l][d]), f64(sv.G[l][d]), f64(sv.C[l][d])
            ig, fg, gg, og = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
            DGn, _ = shifted(DG, T, d, next_of)
            DCn, _ = shifted(DC, T, d, next_of)
            fn, _ = shifted(fg, T, d, next_of)
            cp, _ = shifted(Cs, T, d, prev_of)
            W = f64(inp["w_hh"][k])
            dh = dHout[:, d * H:(d + 1) * H] + DGn @ W
            S_dh = np.abs(dHout[:, d * H:(d + 1) * H]) + np.abs(DGn) @ np.abs(W)
            tc = np.tanh(Cs)
            dc = (dh * og) * (1.0 - tc * tc) + DCn * fn
            S_dc = S_dh * og * (1.0 - tc * tc) + np.abs(dh * og) * (1.0 + tc * tc) + np.abs(DCn * fn)
            out.append(chk("DC[%d][%d]" % (l, d), "dc", "wsb", wb.DC[l][d], dc, S_dc))
            z = np.concatenate([(dc * gg) * (ig * (1.0 - ig)), (dc * cp) * (fg * (1.0 - fg)), (dc * ig) * (1.0 - gg * gg), (dh * tc) * (og * (1.0 - og))], axis=1)
            S = np.concatenate([S_dc * np.abs(gg) * ig * (1.0 - ig) + np.abs(dc * gg) * ig * (1.0 + ig),
                                S_dc * np.abs(cp) * fg * (1.0 - fg) + np.abs(dc * cp) * fg * (1.0 + fg),
                                S_dc * ig * (1.0 - gg * gg) + np.abs(dc * ig) * (1.0 + gg * gg),
                                S_dh * np.abs(tc) * og * (1.0 - og) + np.abs(dh * tc) * og * (1.0 + og)], axis=1)
            out.append(chk("DG[%d][%d]" % (l, d), "dgate", "wsb", wb.DG[l][d], z, S))
            out.append(chk("dW_ih[%d]" % k, "dw", "arena", ar.W_ih[k], DG.T @ X, np.abs(DG).T @ np.abs(X)))
            Hs = f64(sv.H[l])[:, d * H:(d + 1) * H]
            hp, has = shifted(Hs, T, d, prev_of)
            if T > 1:
                out.append(chk("dW_hh[%d]" % k, "dw", "arena", ar.W_hh[k], DG[has].T @ hp[has], np.abs(DG[has]).T @ np.abs(hp[has])))
            else:
                out.append(chk("dW_hh[%d]" % k, "copy", "arena", ar.W_hh[k], np.zeros((G, H), dtype=rdt), exact=True))
            out.append(chk("db_ih[%d]" % k, "colsum", "arena", ar.b_ih[k], DG.sum(axis=0), np.abs(DG).sum(axis=0)))
            out.append(chk("db_hh[%d]" % k, "copy", "arena", ar.b_hh[k], np.asarray(ar.b_ih[k]), exact=True))
        if l == 1:
            z0, S0 = prod64(wb.DG[1][0], inp["w_ih"][2].T)
            z1, S1 = prod64(wb.DG[1][1], inp["w_ih"][3].T)
            out.append(chk("DH0", "dh0", "wsb", wb.DH0, z0 + z1, S0 + S1))
    return out


E_CAP = 1e200   # a carried magnitude beyond this says nothing any more (and must not reach inf: inf * 0)


def chained_S(inp, rec):
    """{tag: magnitude} of `out` and every arena entry, CARRIED from buffer to buffer through the forward and the backward (the S of
    stages() restarts at every stored buffer), for comparing two free-running evaluations of the whole path: E_x below is buffer
    x's own sum of absolute terms plus what its input BUFFERS hand on through |d x / d input| (an entry of DH0 that is small
    against its own sum of absolute terms hands on an error that is not small against it).  The carry runs across buffers (layer
    to layer, DZ3 -> DY2 -> DY1 -> DH1 -> DG[1] -> DH0 -> DG[0] -> gradients), not along the time steps inside one buffer:
    there the stored neighbour's own magnitude is used, since sums of absolute terms carried along a recurrence grow by a
    constant factor per step whatever the weights and say nothing after ten steps.  What the recurrence itself amplifies is
    left to the four decades between the 1e-12 of the comparison and the rounding unit."""
    T = inp["T"]
    sv, wb = rec["saved"], rec["wsb"]
    cap = lambda a: np.minimum(a, E_CAP)  # noqa: E731
    aw = lambda a: np.abs(f64(a))  # noqa: E731
    E_H, E_G, E_C = [None, None], [None, None], [None, None]
    E_X = np.zeros((T, IN))
    for l in range(2):
        X = aw(sv.X0 if l == 0 else sv.H[0])
        E_H[l], E_G[l], E_C[l] = np.zeros((T, 2 * H)), np.zeros((2, T, G)), np.zeros((2, T, H))
        for d in range(2):
            k = 2 * l + d
            W, Whh = aw(inp["w_ih"][k]), aw(inp["w_hh"][k])
            E_XP = X @ W.T + aw(inp["b_ih"][k]) + E_X @ W.T
            g, Cs, Hs = f64(sv.G[l][d]), f64(sv.C[l][d]), f64(sv.H[l])[:, d * H:(d + 1) * H]
            dact = g * (1.0 - g)
            dact[:, 2 * H:3 * H] = 1.0 - g[:, 2 * H:3 * H] ** 2
            for s in range(T):
                t = T - 1 - s if d else s
                has_prev, tp = prev_of(T, d, t)
                E_pre = E_XP[t] + aw(inp["b_hh"][k]) + (np.abs(Hs[tp]) @ Whh.T if has_prev else 0.0)
                Eg = cap(dact[t] * E_pre + np.abs(g[t]))
                ig, fg, gg, og = g[t, :H], g[t, H:2 * H], g[t, 2 * H:3 * H], g[t, 3 * H:]
                cp = np.abs(Cs[tp]) if has_prev else 0.0
                Ec = cap(cp * Eg[H:2 * H] + np.abs(gg) * Eg[:H] + ig * Eg[2 * H:3 * H] + fg * cp + np.abs(ig * gg))
                tc = np.tanh(Cs[t])
                E_G[l][d, t], E_C[l][d, t] = Eg, Ec
                E_H[l][t, d * H:(d + 1) * H] = cap(np.abs(tc) * Eg[3 * H:] + og * (1.0 - tc * tc) * Ec + np.abs(og * tc))
        E_X = E_H[l]
    lin_w = [aw(w) for w in inp["lin_w"]]
    slope = [f64(sv.S[k]) * np.where(np.asarray(sv.A[k]) > 0, 1.0, 0.2) for k in range(3)]
    X, E_Y = aw(sv.H[1]), [None, None, None]
    for k in range(3):
        E_Y[k] = cap((X @ lin_w[k].T + aw(inp["lin_b"][k]) + E_X @ lin_w[k].T) * slope[k])
        X, E_X = aw(sv.Y[k] if k < 2 else rec["out"]), E_Y[k]
    out = {"out": E_Y[2]}
    # ---- backward
    dz = [aw(wb.DY1), aw(wb.DY2), aw(wb.DZ3)]
    E_dz = {2: dz[2]}
    E_dz[1] = cap(((E_dz[2] + dz[2]) @ lin_w[2]) * slope[1])
    E_dz[0] = cap(((E_dz[1] + dz[1]) @ lin_w[1]) * slope[0])
    xin, E_xin = [aw(sv.H[1]), aw(sv.Y[0]), aw(sv.Y[1])], [E_H[1], E_Y[0], E_Y[1]]
    for k in range(3):
        out["dW%d" % (k + 1)] = cap(E_dz[k].T @ xin[k] + dz[k].T @ E_xin[k] + dz[k].T @ xin[k])
        out["db%d" % (k + 1)] = cap(E_dz[k].sum(axis=0) + dz[k].sum(axis=0))
    dHout, E_dHout = f64(wb.DH1), cap((E_dz[0] + dz[0]) @ lin_w[0])
    for l in (1, 0):
        X, E_X = aw(sv.H[0] if l else sv.X0), (E_H[0] if l else np.zeros((T, IN)))
        E_DG = np.zeros((2, T, G))
        for d in range(2):
            k = 2 * l + d
            g, Cs, W = f64(sv.G[l][d]), f64(sv.C[l][d]), aw(inp["w_hh"][k])
            DG, DC = f64(wb.DG[l][d]), f64(wb.DC[l][d])
            E_DC = np.zeros((T, H))
            for s in range(T):
                t = s if d else T - 1 - s
                has_next, tn = next_of(T, d, t)
                has_prev, tp = prev_of(T, d, t)
                ig, fg, gg, og = g[t, :H], g[t, H:2 * H], g[t, 2 * H:3 * H], g[t, 3 * H:]
                Ei, Ef, Egg, Eo = E_G[l][d, t, :H], E_G[l][d, t, H:2 * H], E_G[l][d, t, 2 * H:3 * H], E_G[l][d, t, 3 * H:]
                tc, dtc = np.tanh(Cs[t]), 1.0 - np.tanh(Cs[t]) ** 2
                Ec = E_C[l][d, t]
                rec_ = DG[tn] @ f64(inp["w_hh"][k]) if has_next else 0.0
                dh = np.abs(dHout[t, d * H:(d + 1) * H] + rec_)
                E_dh = cap(E_dHout[t, d * H:(d + 1) * H] + np.abs(dHout[t, d * H:(d + 1) * H]) + (np.abs(DG[tn]) @ W if has_next else 0.0))
                dc = np.abs(DC[t])
                E_dc = E_dh * og * dtc + dh * dtc * Eo + dh * og * 2.0 * np.abs(tc) * dtc * Ec + dh * og * (1.0 + tc * tc)
                if has_next:
                    E_dc = E_dc + np.abs(DC[tn]) * (E_G[l][d, tn, H:2 * H] + g[tn, H:2 * H])
                E_dc = cap(E_dc)
                cp, E_cp = (np.abs(Cs[tp]), E_C[l][d, tp]) if has_prev else (np.zeros(H), np.zeros(H))
                E_DG[d, t] = cap(np.concatenate([
                    E_dc * np.abs(gg) * ig * (1.0 - ig) + dc * ig * (1.0 - ig) * Egg + dc * np.abs(gg) * (np.abs(1.0 - 2.0 * ig) * Ei + ig * (1.0 + ig)),
                    E_dc * cp * fg * (1.0 - fg) + dc * fg * (1.0 - fg) * E_cp + dc * cp * (np.abs(1.0 - 2.0 * fg) * Ef + fg * (1.0 + fg)),
                    E_dc * ig * (1.0 - gg * gg) + dc * (1.0 - gg * gg) * Ei + dc * ig * (2.0 * np.abs(gg) * Egg + 1.0 + gg * gg),
                    E_dh * np.abs(tc) * og * (1.0 - og) + dh * dtc * Ec * og * (1.0 - og) + dh * np.abs(tc) * (np.abs(1.0 - 2.0 * og) * Eo + og * (1.0 + og))]))
                E_DC[t] = E_dc
            aDG = np.abs(DG)
            out["dW_ih[%d]" % k] = cap(E_DG[d].T @ X + aDG.T @ E_X + aDG.T @ X)
            out["db_ih[%d]" % k] = cap(E_DG[d].sum(axis=0) + aDG.sum(axis=0))
            hp, has = shifted(aw(sv.H[l])[:, d * H:(d + 1) * H], T, d, prev_of)
            E_hp, _ = shifted(E_H[l][:, d * H:(d + 1) * H], T, d, prev_of)
            out["dW_hh[%d]" % k] = cap(E_DG[d][has].T @ hp[has] + aDG[has].T @ E_hp[has] + aDG[has].T @ hp[has])
        if l == 1:
            dHout = f64(wb.DH0)
            E_dHout = cap(sum((E_DG[d] + aw(wb.DG[1][d])) @ aw(inp["w_ih"][2 + d]) for d in range(2)))
    return out


def evaluate(c, u=None):
    """-> dict(tag, family, buf, n, ratio = largest |got - z64| / S, bad): `bad` counts entries beyond u S (u: the family's bound
    unless given; exact checks: any difference, or a non-finite value).  Entries with S = 0 must be equal."""
    got, z, S = c["got"].reshape(-1), c["z"].reshape(-1), c["S"].reshape(-1)
    if c["exact"]:
        bad = int(np.sum(~((got == z) & np.isfinite(got))))
        return dict(tag=c["tag"], family=c["family"], buf=c["buf"], n=z.size, ratio=0.0, bad=bad, exact=True)
    u = bound(c["family"]) if u is None else u
    got = f64(got)
    err = np.where(np.isfinite(got), np.abs(got - z), np.inf)
    zero = S == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, np.where(err == 0, 0.0, np.inf), err / np.where(zero, 1.0, S))
    return dict(tag=c["tag"], family=c["family"], buf=c["buf"], n=z.size, ratio=float(ratio.max()), bad=int((ratio > u).sum()), exact=False,
                worst_at=int(ratio.argmax()))


def report(prefix, e):
    if e["exact"]:
        print("%-22s entries %9d  exact, differing %d" % (prefix + " " + e["tag"], e["n"], e["bad"]))
    else:
        print("%-22s entries %9d  worst %.3e of S = %.3f of the bound (%s: floor %.1e x %g) at flat index %d  beyond %d" %
              (prefix + " " + e["tag"], e["n"], e["ratio"], e["ratio"] / bound(e["family"]), e["family"], FLOOR[e["family"]], FACTOR, e["worst_at"], e["bad"]))


def failures(inp, rec, prefix="", quiet=False, only=None):
    """run every check (only: those whose tag starts with one of these) at the GPU bounds;
    -> (list of failing tags, {family: worst ratio}, evaluations)"""
    bad, worst, evs = [], {}, []
    for c in stages(inp, rec):
        if only is not None and not c["tag"].startswith(tuple(only)):
            continue
        e = evaluate(c)
        evs.append(e)
        if not quiet:
            report(prefix, e)
        if not e["exact"]:
            worst[e["family"]] = max(worst.get(e["family"], 0.0), e["ratio"])
        if e["bad"]:
            bad.append(e["tag"])
    return bad, worst, evs


def compared_floats(evs):
    """{buffer: floats compared}; every tag is a different region of its buffer"""
    out = {}
    for e in evs:
        out[e["buf"]] = out.get(e["buf"], 0) + e["n"]
    return out


def sharpness(inp, rec):
    """{(layer, direction): (share of |pre| > 6, share of |pre| < 1, max |c|)} of a float64 record"""
    out = {}
    for l in range(2):
        for d in range(2):
            pre, _ = preacts(inp, rec, l, d)
            out[(l, d)] = (float((np.abs(pre) > 6).mean()), float((np.abs(pre) < 1).mean()), float(np.abs(f64(rec["saved"].C[l][d])).max()))
    return out
