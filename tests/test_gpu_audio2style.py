"""The Audio2style encoder on the MI355X (csrc/audio_lstm.hip through n3dt.Audio2style): against the fixture the reference's own
class emitted in float64 (tests/golden/audio2style, tools/gen_golden_a2s.py), against the tests' float64 restatement on
torch.nn.LSTM / nn.Linear at other lengths, dropout, determinism, streams, fc1, a training step with the renderer, its hipGraph
replay and a checkpoint round trip.

Fixture bounds are the ones the generator recorded: twice the error of the reference's class run in plain float32 on the CPU
(tools/gen_golden_a2s.py, `band` in the manifest).  Restatement bounds at the other lengths are the same kind: twice the float32
restatement's own error against the float64 one, on the case's inputs.
"""
import numpy as np
import pytest
import torch

from test_audio2style_cpu import restate, fixture_module, fixture_case, PARAM_NAMES

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _rel_max(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _grads(mod):
    return {n: (None if p.grad is None else p.grad.detach().cpu().double()) for n, p in mod.named_parameters()}


def _run(mod, mel, masks, w):
    """out and the gradients of sum(w * out) on the GPU (fresh .grad)."""
    for p in mod.parameters():
        p.grad = None
    out = mod(mel.to(dev()), dropout_masks=None if masks is None else [m.to(dev()) for m in masks])
    (out * w.to(dev()).float()).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu().double(), _grads(mod)


def _band_check(mod, mel, masks, seed):
    """GPU vs the float64 restatement, bounded by twice the float32 restatement's own error (floored at 1e-5 of scale)."""
    T = mel.shape[0]
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    w = torch.randn(T, 64, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    out64, g64 = restate(sd, mel, masks, w, torch.float64)
    out32, g32 = restate(sd, mel, masks, w, torch.float32)
    out, g = _run(mod, mel, masks, w)
    band = max(2.0 * _rel_max(out32, out64), 1e-5)
    assert _rel_max(out, out64) <= band, ("out", _rel_max(out, out64), band)
    for n in PARAM_NAMES:
        if g64[n] is None:
            assert g[n] is None, n
            continue
        b = max(2.0 * _rel_max(g32[n], g64[n]), 1e-5)
        e = _rel_max(g[n], g64[n])
        assert e <= b, (n, e, b)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("T", [1, 2, 5, 16])
def test_forward_and_gradients_match_the_reference_fixture(golden, T, mode):
    g, m = golden("audio2style")
    band = m["band"]
    mod = fixture_module(m).to(dev())
    mod.train(mode == "train")
    mod.keep_layer_outputs = True
    mel, masks, w = fixture_case(g, T, mode)
    out, grads = _run(mod, mel, masks, w)
    k = "T%d." % T
    assert _rel_max(out, g[k + mode + ".out"]) <= band["out"]
    for i in range(2):
        got = mod.last_layer_outputs[i].detach().cpu().double().numpy()
        assert _rel_max(got, g[k + "layer%d" % i]) <= band["layer"], i
    norms, idx, vals = g[k + mode + ".gnorm"], g[k + mode + ".gidx"], g[k + mode + ".gval"]
    for j, n in enumerate(m["grad_names"]):
        d = grads[n].reshape(-1).numpy()
        nrm, mx = norms[j]
        assert abs(np.linalg.norm(d) - nrm) <= band["g_norm"] * nrm, (n, np.linalg.norm(d), nrm)
        assert abs(np.abs(d).max() - mx) <= band["g_max"] * mx, (n, np.abs(d).max(), mx)
        assert np.abs(d[idx[j]] - vals[j]).max() <= band["g_entry"] * mx, n
    for n in m["no_grad"]:
        assert grads[n] is None, n


# ---- other lengths against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [33, 64, 256])
def test_other_lengths_match_the_float64_restatement(T):
    from n3dt import Audio2style, synthetic as syn
    torch.manual_seed(5)
    mod = Audio2style().to(dev())
    mel = syn.mel_batch(T, seed=T)
    masks = [(torch.rand(T, n, generator=torch.Generator().manual_seed(T + i)) < 0.5).float() for i, n in enumerate((640, 320, 64))]
    _band_check(mod, mel, masks, seed=T)


def test_two_backward_calls_give_identical_bits():
    from n3dt import Audio2style, synthetic as syn
    torch.manual_seed(1)
    mod = Audio2style().to(dev())
    mel = syn.mel_batch(16, seed=3).to(dev())
    masks = mod.draw_masks(16, dev())
    arenas = []
    for _ in range(2):
        for p in mod.parameters():
            p.grad = None
        mod(mel, dropout_masks=masks).sum().backward()
        arenas.append(mod.grad_arena().flat.clone())
        assert all(p.grad is not None and mod.grad_arena().is_view(i, p.grad) for i, p in enumerate(mod.trained_parameters()))
    torch.cuda.synchronize()
    assert torch.equal(arenas[0], arenas[1])
    assert float(arenas[0].abs().max()) > 0.0


def test_fc1_takes_no_gradient_and_adam_leaves_it_alone():
    from n3dt import Audio2style, synthetic as syn
    torch.manual_seed(2)
    mod = Audio2style().to(dev())
    fc1 = {n: p.detach().clone() for n, p in mod.rnn.fc1.named_parameters()}
    w0 = mod.linear1[0].weight.detach().clone()
    opt = torch.optim.Adam(mod.parameters(), lr=1e-3, betas=(0.5, 0.999))
    mod(syn.mel_batch(4, seed=1).to(dev())).sum().backward()
    assert mod.rnn.fc1.weight.grad is None and mod.rnn.fc1.bias.grad is None
    opt.step()
    torch.cuda.synchronize()
    for n, p in mod.rnn.fc1.named_parameters():
        assert torch.equal(p.detach(), fc1[n]), n
    assert not torch.equal(mod.linear1[0].weight.detach(), w0)


def test_dropout_eval_train_and_reported_masks():
    from n3dt import Audio2style, synthetic as syn
    torch.manual_seed(3)
    T = 64
    mod = Audio2style().to(dev())
    mel = syn.mel_batch(T, seed=9)
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    mod.eval()
    with torch.no_grad():
        y_eval = mod(mel.to(dev())).cpu().double()
    assert mod.last_masks is None
    ref, _ = restate(sd, mel, None, None, torch.float64)
    assert _rel_max(y_eval, ref) <= 1e-4
    mod.train()
    with torch.no_grad():
        y1 = mod(mel.to(dev())).cpu().double()
        m1 = [m.cpu() for m in mod.last_masks]
        y2 = mod(mel.to(dev())).cpu().double()
        m2 = [m.cpu() for m in mod.last_masks]
    for a, b in zip(m1, m2):
        assert set(torch.unique(a).tolist()) <= {0.0, 1.0}
        assert 0.45 <= float(a.mean()) <= 0.55, float(a.mean())
        assert not torch.equal(a, b)
    for y, ms in ((y1, m1), (y2, m2)):
        ref, _ = restate(sd, mel, ms, None, torch.float64)
        assert _rel_max(y, ref) <= 1e-4


def test_a_side_stream_gives_the_default_stream_result():
    from n3dt import Audio2style, synthetic as syn
    torch.manual_seed(4)
    mod = Audio2style().to(dev()).eval()
    mel = syn.mel_batch(8, seed=4).to(dev())
    with torch.no_grad():
        a = mod(mel).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            b = mod(mel).clone()
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_refusals_on_the_device():
    from n3dt import Audio2style
    mod = Audio2style().to(dev())
    with pytest.raises(ValueError):
        mod(torch.zeros(257, 80, 16, device=dev()))
    with pytest.raises(ValueError):
        mod(torch.zeros(0, 80, 16, device=dev()))
    with pytest.raises(ValueError):
        mod(torch.zeros(4, 80, 15, device=dev()))
    with pytest.raises(ValueError):
        mod(torch.zeros(4, 80, 16))


# ---- with the renderer -----------------------------------------------------------------------------------------------------------
def _render_setup(B, graph=False):
    from n3dt import BaseOptions, HeadNeRFNet, Audio2style, synthetic as syn
    from n3dt.train import disk_mask
    opt = BaseOptions({"featmap_size": 8, "featmap_nc": 256, "pred_img_size": 32, "num_sample_coarse": 16})
    sd = syn.make_state_dict(opt, seed=0, bg_noise=0.1)
    d = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in syn.frame_inputs(opt, B).items()}
    d["mel_batch"] = syn.mel_batch(B, seed=11).to(dev())
    net = HeadNeRFNet(opt, False, False, train_precision="bf16").to(dev())
    net.load_state_dict(sd, strict=True)
    torch.manual_seed(6)
    a2s = Audio2style().to(dev())
    gt = torch.full((B, 3, 32, 32), 0.5, device=dev())
    mask = disk_mask(B, 32).to(dev())
    t_rand = syn.stratified_noise(B, 64, 16, seed=3).to(dev())
    return net, a2s, d, gt, mask, t_rand


def test_train_step_drives_the_encoder_with_the_renderers_gradient():
    from n3dt.train import train_step
    net, a2s, d, gt, mask, t_rand = _render_setup(2)
    a2s.eval()  # no dropout: the restatement below sees the same function
    rec = {}
    fwd = a2s.forward

    def keep(gr):
        rec["d"] = gr.detach().cpu().double()

    def tapped(mel, dropout_masks=None):
        y = fwd(mel, dropout_masks)
        y.register_hook(keep)
        return y
    a2s.forward = tapped
    sgd = torch.optim.SGD(net.parameters(), lr=0.0)
    sgd2 = torch.optim.SGD(a2s.parameters(), lr=0.0)
    train_step(net, sgd, d, gt, mask, t_rand=t_rand, extra_optimizers=(sgd2,), audio2style=a2s)
    torch.cuda.synchronize()
    assert "d" in rec and float(rec["d"].abs().max()) > 0.0
    sd = {k: v.detach().cpu() for k, v in a2s.state_dict().items()}
    mel = d["mel_batch"].cpu()
    _, g64 = restate(sd, mel, None, rec["d"], torch.float64)
    _, g32 = restate(sd, mel, None, rec["d"], torch.float32)
    got = _grads(a2s)
    for n in PARAM_NAMES:
        if g64[n] is None:
            assert got[n] is None, n
            continue
        b = max(2.0 * _rel_max(g32[n], g64[n]), 1e-5)
        assert _rel_max(got[n], g64[n]) <= b, (n, _rel_max(got[n], g64[n]), b)


def test_graphed_step_with_both_optimizers_replays_like_eager_steps():
    from n3dt import Audio2style
    from n3dt.train import fused_data_losses, GraphedTrainStep
    n_steps, warm = 6, 2
    runs = []
    for graph in (False, True):
        net, a2s, d, gt, mask, t_rand = _render_setup(2)
        masks = [m.clone() for m in a2s.draw_masks(2, dev())] if not runs else runs[0][2]
        capt = dict(capturable=True) if graph else {}
        o1 = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True, **capt)
        o2 = torch.optim.Adam(a2s.parameters(), lr=1e-5, betas=(0.5, 0.999), fused=True, **capt)

        def step():
            style = a2s(d["mel_batch"], dropout_masks=masks)
            out = net("train", d["batch_xy"], d["batch_uv"], style, None, d["shape_code"], d["appea_code"], d["batch_Rmats"],
                      d["batch_Tvecs"], d["batch_inv_inmats"], t_rand=t_rand)
            t = fused_data_losses(out["coarse_dict"], gt, mask)
            o1.zero_grad()
            o2.zero_grad()
            t["total_loss"].backward()
            o1.step()
            o2.step()
            return t["total_loss"].detach()
        if graph:
            g = GraphedTrainStep(step, warmup=warm)
            for _ in range(n_steps - warm):
                g()
        else:
            for _ in range(n_steps):
                step()
        torch.cuda.synchronize()
        runs.append((net, a2s, masks, d))
    (net_e, a2s_e, _, _), (net_g, a2s_g, _, d) = runs
    for (n, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert float((a - b).abs().max()) <= 6e-4, n  # test_gpu_round4's graphed-step bound
    for (n, a), (_, b) in zip(a2s_e.named_parameters(), a2s_g.named_parameters()):
        assert float((a - b).abs().max()) <= 6e-5, n  # a tenth of it: lr 1e-5 here against 1e-4 there
    # the encoder's optimizer ran inside the graph: its weights moved from their (seeded) start, fc1 excepted
    torch.manual_seed(6)
    start = Audio2style().to(dev())
    assert float((a2s_g.linear3[0].weight - start.linear3[0].weight).abs().max()) > 1e-5
    assert torch.equal(a2s_g.rnn.fc1.weight, start.rnn.fc1.weight)
    # after the replays the graphed module computes what a fresh module loaded from its state dict computes
    fresh = Audio2style().to(dev())
    fresh.load_state_dict(a2s_g.state_dict(), strict=True)
    a2s_g.eval()
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(a2s_g(d["mel_batch"]), fresh(d["mel_batch"]))


def test_checkpoint_round_trip_restores_both_modules_and_optimizers(tmp_path):
    from n3dt import Audio2style, checkpoint
    net, a2s, d, gt, mask, t_rand = _render_setup(2)
    from n3dt.train import train_step
    o1 = torch.optim.Adam(net.parameters(), lr=1e-4)
    o2 = torch.optim.Adam(a2s.parameters(), lr=1e-7, betas=(0.5, 0.999))
    train_step(net, o1, d, gt, mask, t_rand=t_rand, extra_optimizers=(o2,), audio2style=a2s)
    path = str(tmp_path / "ck.pth")
    checkpoint.save_checkpoint(path, net, _opt(), optimizer=o1, audio2style=a2s, audio2style_optimizer=o2)
    ck = torch.load(path, map_location="cpu")
    assert "audio2style" in ck and "optim_style" in ck and "net" in ck and "optim_state" in ck
    net2, _ = checkpoint.build_from_checkpoint(path, train_precision="bf16")
    a2s2 = Audio2style()
    o2b = torch.optim.Adam(a2s2.parameters(), lr=1e-7, betas=(0.5, 0.999))
    checkpoint.load_audio2style(path, a2s2, optimizer=o2b)
    for (n, a), (_, b) in zip(a2s.state_dict().items(), a2s2.state_dict().items()):
        assert torch.equal(a.cpu(), b), n
    for (n, a), (_, b) in zip(net.state_dict().items(), net2.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), n
    s1, s2 = o2.state_dict(), o2b.state_dict()
    assert s1["param_groups"] == s2["param_groups"] and len(s1["state"]) == len(s2["state"]) == 22
    o1b = torch.optim.Adam(net2.parameters(), lr=1e-4)
    o1b.load_state_dict(ck["optim_state"])
    assert len(o1b.state_dict()["state"]) == len(o1.state_dict()["state"])


def _opt():
    from n3dt import BaseOptions
    return BaseOptions({"featmap_size": 8, "featmap_nc": 256, "pred_img_size": 32, "num_sample_coarse": 16})
