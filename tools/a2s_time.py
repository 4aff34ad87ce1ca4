#!/usr/bin/env python3
"""Time the Audio2style encoder, forward + backward, on the GPU: libn3dt's kernels (n3dt.Audio2style) against the same module built
from torch.nn.LSTM / nn.Linear on the same GPU (MIOpen) and on the CPU with 16 threads (where the reference builds it,
talker_trainer.py:631).  Then one config-3 training step (B = 2, bf16 renderer, two Adams) with the real encoder against the same
step with the FlatBucket stand-in.  hipEvents (CPU: wall clock) over `--iters` after `--warmup`; prints one JSON object.

Run each invocation under a time limit, e.g.  timeout -k 10 600 python tools/a2s_time.py
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

from n3dt import Audio2style, BaseOptions, HeadNeRFNet, parallel, synthetic as syn  # noqa: E402
from n3dt.train import fused_data_losses, disk_mask  # noqa: E402


class TorchA2s(torch.nn.Module):
    """The reference's computation on torch.nn modules (the comparator)."""

    def __init__(self, sd):
        super().__init__()
        self.lstm = torch.nn.LSTM(1280, 640, 2, batch_first=True, bidirectional=True)
        self.lstm.load_state_dict({k[len("rnn.rnn."):]: v for k, v in sd.items() if k.startswith("rnn.rnn.")})
        self.lins = torch.nn.ModuleList([torch.nn.Linear(i, o) for i, o in ((1280, 640), (640, 320), (320, 64))])
        for i, lin in enumerate(self.lins):
            lin.load_state_dict({"weight": sd["linear%d.0.weight" % (i + 1)], "bias": sd["linear%d.0.bias" % (i + 1)]})

    def forward(self, mel):
        h = self.lstm(mel.reshape(mel.shape[0], -1).unsqueeze(0))[0][0]
        for lin in self.lins:
            h = F.dropout(F.leaky_relu(lin(h), 0.2), 0.5, True)
        return h


def time_gpu(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def time_cpu(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) * 1e3 / iters


def fwd_bwd(mod):
    def step(mel):
        for p in mod.parameters():
            p.grad = None
        mod(mel).sum().backward()
    return step


def train_step_ms(dev, real, warmup, iters):
    opt = BaseOptions({"featmap_size": 64, "featmap_nc": 256, "pred_img_size": 512, "num_sample_coarse": 64})  # config 3
    B = 2
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in syn.frame_inputs(opt, B).items()}
    mel = syn.mel_batch(B, seed=1).to(dev)
    net = HeadNeRFNet(opt, False, False, train_precision="bf16").to(dev)
    net.load_state_dict(syn.make_state_dict(opt, seed=0, bg_noise=0.1), strict=True)
    o1 = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True)
    enc = Audio2style().to(dev) if real else parallel.FlatBucket().to(dev)
    o2 = torch.optim.Adam(enc.parameters(), lr=1e-7, betas=(0.5, 0.999), fused=True)
    gt = torch.full((B, 3, 512, 512), 0.5, device=dev)
    mask = disk_mask(B, 512).to(dev)

    def step():
        style = enc(mel) if real else d["audiostyle"]
        out = net("train", d["batch_xy"], d["batch_uv"], style, None, d["shape_code"], d["appea_code"], d["batch_Rmats"],
                  d["batch_Tvecs"], d["batch_inv_inmats"])
        t = fused_data_losses(out["coarse_dict"], gt, mask)
        o1.zero_grad()
        o2.zero_grad()
        t["total_loss"].backward()
        if not real:
            enc.fill_grad(1e-3)
        o1.step()
        o2.step()
    return time_gpu(step, warmup, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lengths", default="2,4,16,64")
    ap.add_argument("--cpu-threads", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mod = Audio2style().to(dev)
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    tgpu, tcpu = TorchA2s(sd).to(dev), TorchA2s(sd)
    torch.set_num_threads(args.cpu_threads)
    out = {"iters": args.iters, "cpu_threads": args.cpu_threads, "fwd_bwd_ms": {}}
    for T in (int(t) for t in args.lengths.split(",")):
        mel = syn.mel_batch(T, seed=T)
        melg = mel.to(dev)
        r = {"n3dt": time_gpu(lambda: fwd_bwd(mod)(melg), args.warmup, args.iters),
             "torch_gpu": time_gpu(lambda: fwd_bwd(tgpu)(melg), args.warmup, args.iters),
             "torch_cpu": time_cpu(lambda: fwd_bwd(tcpu)(mel), 1, max(2, args.iters // 5))}
        out["fwd_bwd_ms"]["T%d" % T] = r
    out["config3_train_step_ms"] = {"with_audio2style": train_step_ms(dev, True, args.warmup, args.iters),
                                    "with_flatbucket_standin": train_step_ms(dev, False, args.warmup, args.iters)}
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
