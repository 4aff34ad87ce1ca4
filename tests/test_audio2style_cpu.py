"""CPU checks of the Audio2style encoder (n3dt.Audio2style, n3dt_a2s_* of include/n3dt.h): the reference's state-dict inventory and
initial values, argument refusal before any launch, the grad arena's layout, the module's refusals, the checkpoint keys, and the
fixture the reference's own class emitted (tests/golden/audio2style, tools/gen_golden_a2s.py).  Also home of the tests' float64
restatement on torch.nn.LSTM / nn.Linear that the GPU tests compare against."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

PARAM_NAMES = (["rnn.rnn.%s_l%d%s" % (n, l, s) for l in range(2) for s in ("", "_reverse")
                for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] +
               ["rnn.fc1.weight", "rnn.fc1.bias"] +
               ["linear%d.0.%s" % (i, n) for i in (1, 2, 3) for n in ("weight", "bias")])


# ---- the tests' oracle: the reference's forward restated on torch.nn.LSTM / nn.Linear ------------------------------------------
def restate(sd, mel, masks, w, dtype):
    """out [T, 64] and (w given) the gradients of sum(w * out) by parameter name (fc1: None), in `dtype` on the CPU.
    talker_trainer.py:452-458: flatten, one sequence through the 2-layer bidirectional LSTM, three Linear + LeakyReLU(0.2) +
    Dropout(0.5) with the given keep masks (None: no dropout)."""
    lstm = torch.nn.LSTM(1280, 640, 2, batch_first=True, bidirectional=True).to(dtype)
    lstm.load_state_dict({k[len("rnn.rnn."):]: v.to(dtype) for k, v in sd.items() if k.startswith("rnn.rnn.")})
    lins = [torch.nn.Linear(i, o).to(dtype) for i, o in ((1280, 640), (640, 320), (320, 64))]
    for i, lin in enumerate(lins):
        lin.load_state_dict({"weight": sd["linear%d.0.weight" % (i + 1)].to(dtype), "bias": sd["linear%d.0.bias" % (i + 1)].to(dtype)})
    T = mel.shape[0]
    h = lstm(mel.reshape(T, 1280).to(dtype).unsqueeze(0))[0][0]
    for i, lin in enumerate(lins):
        h = F.leaky_relu(lin(h), 0.2)
        if masks is not None:
            h = h * (masks[i].to(dtype) * 2.0)
    if w is None:
        return h.detach(), None
    (h * w.to(dtype)).sum().backward()
    grads = {"rnn.rnn." + n: p.grad.detach().double() for n, p in lstm.named_parameters()}
    for i, lin in enumerate(lins):
        grads["linear%d.0.weight" % (i + 1)] = lin.weight.grad.detach().double()
        grads["linear%d.0.bias" % (i + 1)] = lin.bias.grad.detach().double()
    grads["rnn.fc1.weight"] = grads["rnn.fc1.bias"] = None
    return h.detach().double(), grads


def fixture_module(m):
    """n3dt.Audio2style built under the fixture's seed, its weights checked against the reference's checksum."""
    from n3dt import Audio2style, synthetic as syn
    torch.manual_seed(m["weights_seed"])
    mod = Audio2style()
    assert np.allclose(syn.state_dict_checksum(mod.state_dict()), m["weights_checksum"], rtol=1e-12, atol=0), "init drifted"
    return mod


def fixture_case(g, T, mode):
    """(mel [T,80,16] float32, keep masks or None, w [T,64] float64) of one fixture case."""
    k = "T%d." % T
    mel = torch.from_numpy(g[k + "mel_u8"]).float() / 32.0 - 4.0
    w = torch.from_numpy(g[k + "w"])
    masks = None
    if mode == "train":
        masks = []
        for i, n in enumerate((640, 320, 64)):
            bits = np.unpackbits(g[k + "train.mask%d" % i], count=T * n)
            masks.append(torch.from_numpy(bits.astype(np.float32)).view(T, n))
    return mel, masks, w


# ---- the module ------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_shapes_and_count_are_the_references(golden):
    from n3dt import Audio2style
    _, m = golden("audio2style")
    sd = Audio2style().state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == m["state_dict"]
    assert sum(v.numel() for v in sd.values()) == 21_546_624 == m["n_params"]
    from n3dt.parallel import FlatBucket
    assert FlatBucket.AUDIO2STYLE_PARAMS == 21_546_624
    assert list(sd.keys()) == PARAM_NAMES


def test_seeded_initial_values_are_the_references(golden):
    _, m = golden("audio2style")
    fixture_module(m)  # asserts the checksum


def test_fixture_masks_and_restatement_agree_with_the_reference(golden):
    """The float64 restatement the GPU tests use reproduces the reference's own outputs on the fixture (so it is a fair oracle)."""
    g, m = golden("audio2style")
    sd = fixture_module(m).state_dict()
    for T in (2, 5):
        for mode in ("train", "eval"):
            mel, masks, w = fixture_case(g, T, mode)
            out, grads = restate(sd, mel, masks, w, torch.float64)
            assert np.abs(out.numpy() - g["T%d.%s.out" % (T, mode)]).max() <= 1e-12
            for j, n in enumerate(m["grad_names"]):
                d = grads[n].reshape(-1).numpy()
                assert np.abs(d[g["T%d.%s.gidx" % (T, mode)][j]] - g["T%d.%s.gval" % (T, mode)][j]).max() <= 1e-12 * max(1.0, g["T%d.%s.gnorm" % (T, mode)][j][1])


def test_grad_arena_is_the_c_layout_without_fc1():
    from n3dt import Audio2style, _lib
    a = Audio2style()
    ar = a.grad_arena()
    assert ar.numel == ar.flat.numel() == _lib.A2S_GRAD_FLOATS
    off = 0
    for i, p in enumerate(a.trained_parameters()):
        assert ar.offsets[i] == off
        off += p.numel()
    assert all(p is not a.rnn.fc1.weight and p is not a.rnn.fc1.bias for p in ar.params)
    assert len(ar.params) == 22


def test_module_refuses_bad_input_without_a_gpu():
    from n3dt import Audio2style
    a = Audio2style()
    for bad in (torch.zeros(0, 80, 16), torch.zeros(257, 80, 16), torch.zeros(4, 80, 15), torch.zeros(1280), "mel"):
        with pytest.raises(ValueError):
            a(bad)
    with pytest.raises(ValueError, match="GPU"):
        a(torch.zeros(4, 80, 16))


def test_mel_batch_is_seeded_and_exact():
    from n3dt import synthetic as syn
    a, b = syn.mel_batch(3, seed=5), syn.mel_batch(3, seed=5)
    assert a.shape == (3, 80, 16) and a.dtype == torch.float32 and torch.equal(a, b)
    assert not torch.equal(a, syn.mel_batch(3, seed=6))
    assert float(a.min()) >= -4.0 and float(a.max()) < 4.0 and torch.equal(a * 32, (a * 32).round())


def test_checkpoint_keys_and_loader(tmp_path):
    from n3dt import Audio2style, checkpoint
    torch.manual_seed(0)
    a = Audio2style()
    opt = torch.optim.Adam(a.parameters(), lr=1e-7, betas=(0.5, 0.999))
    for p in a.trained_parameters():
        p.grad = torch.ones_like(p)
    opt.step()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(2))

    class Opt:
        featmap_size, featmap_nc, pred_img_size = 8, 256, 32
    path = str(tmp_path / "ck.pth")
    checkpoint.save_checkpoint(path, Net(), Opt(), audio2style=a, audio2style_optimizer=opt)
    ck = torch.load(path, map_location="cpu")
    assert "audio2style" in ck and "optim_style" in ck
    b = Audio2style()
    opt_b = torch.optim.Adam(b.parameters(), lr=1e-7, betas=(0.5, 0.999))
    checkpoint.load_audio2style(path, b, optimizer=opt_b)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    sa, sb = opt.state_dict(), opt_b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and len(sb["state"]) == 22  # fc1 took no step
    for i, st in sa["state"].items():
        assert torch.equal(st["exp_avg"], sb["state"][i]["exp_avg"])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_size_queries_refuse_bad_lengths():
    from n3dt import _lib
    L = _lib.lib()
    assert L.n3dt_a2s_saved_bytes(2) > L.n3dt_a2s_saved_bytes(1) > 0
    assert L.n3dt_a2s_workspace_bytes(256) > L.n3dt_a2s_workspace_bytes(1) > 0
    for T in (0, -1, 257):
        assert L.n3dt_a2s_saved_bytes(T) == 0 and b"T = " in L.n3dt_last_error()
        assert L.n3dt_a2s_workspace_bytes(T) == 0 and b"T = " in L.n3dt_last_error()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every refusal returns N3DT_EINVAL with a message naming the call and the argument, before the first HIP call (the pointers
    below are never dereferenced)."""
    from n3dt import _lib
    L = _lib.lib()
    P = 4096
    T = 4
    sv, ws = L.n3dt_a2s_saved_bytes(T), L.n3dt_a2s_workspace_bytes(T)

    def params(**nulls):
        p = _lib.A2sParams()
        for f in ("w_ih", "w_hh", "b_ih", "b_hh"):
            for k in range(4):
                getattr(p, f)[k] = P
        for f in ("lin_w", "lin_b"):
            for k in range(3):
                getattr(p, f)[k] = P
        for f, k in nulls.items():
            getattr(p, f)[k] = None
        return p

    def fwd(t=T, p=None, mel=P, m1=P, m2=P, m3=P, out=P, saved=P, sv_b=sv, w=P, ws_b=ws):
        p = params() if p is None else p
        return L.n3dt_a2s_fwd(t, ctypes.byref(p), mel, m1, m2, m3, out, saved, sv_b, w, ws_b, None)

    def bwd(t=T, p=None, g=P, saved=P, sv_b=sv, arena=P, w=P, ws_b=ws):
        p = params() if p is None else p
        return L.n3dt_a2s_bwd(t, ctypes.byref(p), g, saved, sv_b, arena, w, ws_b, None)

    def refused(rc, *words):
        msg = L.n3dt_last_error()
        assert rc == EINVAL, (rc, msg)
        for wd in words:
            assert wd in msg, (wd, msg)

    for call, who in ((fwd, b"n3dt_a2s_fwd"), (bwd, b"n3dt_a2s_bwd")):
        for t in (0, 257):
            refused(call(t=t), who, b"T = %d" % t)
        refused(call(p=params(w_hh=2)), who, b"w_hh[2]")
        refused(call(p=params(lin_b=1)), who, b"lin_b[1]")
        refused(call(saved=None), who, b"saved")
        refused(call(sv_b=sv - 1), who, b"saved_bytes")
        refused(call(w=None), who, b"ws")
        refused(call(ws_b=ws - 4), who, b"ws_bytes")
        refused(call(t=T + 1), who, b"saved_bytes")  # a buffer sized for T is too small for T + 1
    assert L.n3dt_a2s_fwd(T, None, P, P, P, P, P, P, sv, P, ws, None) == EINVAL and b"params" in L.n3dt_last_error()
    refused(fwd(mel=None), b"mel")
    refused(fwd(mel=P + 4), b"mel")  # misaligned
    refused(fwd(out=None), b"out")
    refused(fwd(m2=None), b"mask")
    refused(bwd(g=None), b"g_out")
    refused(bwd(arena=None), b"grad_arena")


# ---- the fixture is what the reference emits today ------------------------------------------------------------------------------
def test_committed_fixture_is_what_the_reference_emits_today(tmp_path, golden):
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gen_golden_a2s
    if not os.path.exists(os.path.join(gen_golden_a2s.REF, "talker_trainer.py")):
        pytest.skip("the reference is not checked out here")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "gen_golden_a2s.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    g, m = golden("audio2style")
    g2 = np.load(str(tmp_path / "audio2style.npz"))
    assert sorted(g.files) == sorted(g2.files)
    for n in g.files:
        assert np.array_equal(g[n], g2[n]), n
    with open(str(tmp_path / "audio2style.json")) as f:
        assert f.read() == open(os.path.join(REPO, "tests", "golden", "audio2style.json")).read()
