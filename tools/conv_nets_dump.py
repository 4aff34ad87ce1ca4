#!/usr/bin/env python3
"""Dump what the six frozen convolutional networks compute, for a byte-for-byte comparison of two builds of libn3dt.

    python tools/conv_nets_dump.py --out DIR             every network, each in a fresh child process with its own time limit;
                                                         stops at the first child that fails
    python tools/conv_nets_dump.py --compare DIR_A DIR_B the list of files and the verdict, as one JSON object (exit 1: unequal)

Run it once with N3DT_LIB pointing at one library and once at the other.  Weights and inputs are seeded (n3dt.synthetic, CPU
generators), so two runs see the same bits.  Per network the PACKED WEIGHT BUFFER, the forward's outputs and one single-block
entry are written as raw little-endian arrays: SyncNet (embeddings, cosines), Wav2Lip (faces), S3FD (the twelve head maps),
FaceRecon (coefficients), FAN (heat maps, gates), HeadMask (logits, upsampled outputs, head and eye masks).  Sizes: the smallest
frame a network accepts and one odd, non-square size above it where it takes a size, n = 1 and 3, and one larger batch (16; 32
windows for SyncNet, whose maps are small) at which the two-tiles-per-wave instantiations of the convolution kernels run.  The
child prints, per convolution, the column tiles per wave (NT) that csrc/conv_net_core.h's cn_wave_ntiles chooses, restated here;
Wav2Lip sums its tiles over classes with a rule of its own, which is not restated.
"""
import argparse
import filecmp
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nerf-3dtalker-code_amd"))

NETS = ("syncnet", "wav2lip", "s3fd", "face_recon", "fan", "head_mask")
SIZES = ((1, 32, 32), (3, 32, 32), (1, 45, 39), (3, 45, 39))  # n, H, W where a network takes a size


def wave_ntiles(M, np_):
    mtiles = (M + 63) // 64
    return 1 if (np_ % 64 != 0 or mtiles * (np_ // 64) < 1024) else 2


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


class Dump(object):
    def __init__(self, out, net):
        self.out, self.net, self.files = out, net, 0

    def save(self, name, t):
        import torch
        assert torch.is_tensor(t)
        t.detach().contiguous().cpu().numpy().tofile(os.path.join(self.out, "%s_%s.bin" % (self.net, name)))
        self.files += 1

    def nt(self, case, rows):
        """rows: (convolution, M, np)"""
        text = " ".join("%s:%d" % (name, wave_ntiles(M, np_)) for name, M, np_ in rows)
        print("%s %s NT %s" % (self.net, case, text))


def rand(shape, seed, lo=0.0, hi=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=g)).cuda()


def run_syncnet(d):
    from n3dt import SyncNet, synthetic as syn
    from n3dt import syncnet as m
    net = SyncNet(syn.syncnet_state_dict(11))
    import torch
    d.save("packed", net._packed_for(torch.device("cuda:0")))
    for n in (1, 3, 32):
        mel, faces = rand((n,) + m.MEL_SHAPE, 100 + n, -4.0, 4.0), rand((n,) + m.FACE_SHAPE, 200 + n)
        a, f, c = net._run(mel, faces)
        for name, t in (("audio", a), ("face", f), ("cos", c)):
            d.save("n%d_%s" % (n, name), t)
        rows = []
        for enc, blocks, shape in (("f", m.FACE_BLOCKS, m.FACE_SHAPE), ("a", m.AUDIO_BLOCKS, m.MEL_SHAPE)):
            h, w = shape[1:]
            for i, (_, cout, (kh, kw), (sh, sw), pad, _) in enumerate(blocks):
                h, w = conv_out(h, kh, sh, pad), conv_out(w, kw, sw, pad)
                opad = blocks[i + 1][4] if i + 1 < len(blocks) else 0
                rows.append(("%s%d" % (enc, i), n * (h + 2 * opad) * (w + 2 * opad), cout))
        d.nt("n%d" % n, rows)
    shape_in, _ = m.block_shapes()[2]  # a residual 3 x 3 block: haloed input and output
    d.save("block2", net.block(2, rand((3,) + shape_in, 7, -1.0, 1.0)))


def run_wav2lip(d):
    import torch
    from n3dt import Wav2Lip, synthetic as syn
    from n3dt import wav2lip as m
    net = Wav2Lip(syn.wav2lip_state_dict(12))
    d.save("packed", net._packed_for(torch.device("cuda:0")))
    for n in (1, 3, 16):
        d.save("n%d_out" % n, net(rand((n,) + m.MEL_SHAPE, 300 + n, -4.0, 4.0), rand((n,) + m.FACE_SHAPE, 400 + n)))
    shapes = m.block_shapes()
    d.save("block2", net.block(2, rand((3,) + shapes[2][0], 8, -1.0, 1.0)))       # a residual block between two haloed maps
    up = [b for b, blk in enumerate(m.BLOCKS) if blk[0] and blk[4] == (2, 2)][0]  # a stride-2 transposed block: four classes
    d.save("block%d" % up, net.block(up, rand((3,) + shapes[up][0], 9, -1.0, 1.0)))


def run_s3fd(d):
    import torch
    from n3dt import S3FD, synthetic as syn
    from n3dt import s3fd as m
    net = S3FD(syn.s3fd_state_dict(13))
    d.save("packed", net._packed_for(torch.device("cuda:0")))
    for n, H, W in SIZES + ((16, 64, 64),):
        case = "n%d_%dx%d" % (n, H, W)
        for i, t in enumerate(net.forward(rand((n, 3, H, W), 500 + n + H, -120.0, 150.0))):
            d.save("%s_head%d" % (case, i), t)
        rows, h, w = [], H, W
        for c, (name, _, cout, k, s, p, pool, level) in enumerate(m.CONVS):
            h, w = conv_out(h, k, s, p), conv_out(w, k, s, p)
            opad = 0
            if not pool:
                opad = max(1 if level else 0, m.CONVS[c + 1][5] if c + 1 < len(m.CONVS) else 0)
            rows.append((name, n * (h + 2 * opad) * (w + 2 * opad), cout))
            if pool:
                h, w = h // 2, w // 2
        d.nt(case, rows)  # the head pairs are 32 columns wide: one tile
    d.save("block1", net.block(1, rand((3, 64, 13, 11), 10, 0.0, 2.0)))  # conv1_2: a haloed input


def run_face_recon(d):
    import torch
    from n3dt import FaceRecon, synthetic as syn
    from n3dt import face_recon as m
    net = FaceRecon(syn.face_recon_state_dict(14), syn.face_recon_lm3d())
    d.save("packed", net._packed_for(torch.device("cuda:0")))
    for n, H, W in SIZES + ((16, 128, 128),):
        case = "n%d_%dx%d" % (n, H, W)
        d.save("%s_coeffs" % case, net.forward(rand((n, 3, H, W), 600 + n + H)))
        rows = []
        h, w = conv_out(conv_out(H, 7, 2, 3), 3, 2, 1), conv_out(conv_out(W, 7, 2, 3), 3, 2, 1)
        h2, w2 = h, w
        for name, _, _, cout, k, s, p, role, _ in m.CONVS:
            if role == 0:
                rows.append((name, n * conv_out(H, 7, 2, 3) * conv_out(W, 7, 2, 3), cout))
            elif role == 1:
                h, w = h2, w2  # the bottleneck's input: the previous one's output
                rows.append((name, n * (h + 2) * (w + 2), cout))
            elif role == 2:
                h2, w2 = conv_out(h, k, s, p), conv_out(w, k, s, p)
                rows.append((name, n * h2 * w2, cout))
            else:
                rows.append((name, n * h2 * w2, cout))
        d.nt(case, [(r[0].replace("backbone.", ""), r[1], r[2]) for r in rows])
    d.save("block2", net.block(2, rand((3, 64, 9, 7), 11, 0.0, 2.0)))  # a bottleneck's 3 x 3: a haloed input


def run_fan(d):
    import torch
    from n3dt import FAN, synthetic as syn
    M, N = 2, 98
    net = FAN(syn.fan_state_dict(15, num_modules=M, num_landmarks=N), num_modules=M, num_landmarks=N)
    d.save("packed", net._packed_for(torch.device("cuda:0")))
    for n in (1, 3, 16):
        for s, heat in enumerate(net.forward(rand((n, 3, 256, 256), 700 + n))):
            d.save("n%d_heat%d" % (n, s), heat)
        d.save("n%d_gates" % n, net.last_gates)
        # the rule sees only (rows, columns): the stem at 128 x 128, the ConvBlocks' 64 / 128 / 256 columns on maps of side 128 .. 4
        rows = [("%dx%d/np%d" % (side, side, np_), n * side * side, np_) for side in (128, 64, 32, 16, 8, 4) for np_ in (32, 64, 128, 256)]
        d.nt("n%d" % n, rows)
    d.save("block_conv2", net.block("conv2", rand((3, 64, 13, 11), 12, -1.0, 1.0)))  # a ConvBlock; FAN's maps carry no halo
    d.save("block_conv1", net.block("conv1", rand((2, 3, 256, 256), 13)))            # the stem


def run_head_mask(d):
    import torch
    from n3dt import HeadMask, synthetic as syn
    from n3dt import head_mask as m
    net = HeadMask(syn.head_mask_state_dict(16, 19), size=None)
    d.save("packed", net._packed_for(torch.device("cuda:0")))
    level = {0: 0}  # convolution -> the feature size its output has (feature_sizes)
    level.update({b: 1 for b in range(1, 5)})
    level.update({b: 2 for b in list(range(5, 10)) + [m.HEAD16, m.FFM_BLK, m.OUT, m.OUT + 1, m.OUT16, m.OUT16 + 1]})
    level.update({b: 3 for b in list(range(10, 15)) + [m.ARM16, m.HEAD32, m.OUT32, m.OUT32 + 1]})
    level.update({b: 4 for b in list(range(15, 20)) + [m.ARM32]})
    for n, H, W in SIZES + ((16, 256, 256),):
        case = "n%d_%dx%d" % (n, H, W)
        x = rand((n, 3, H, W), 800 + n + H, -2.0, 2.0)
        for o in range(3):
            d.save("%s_logits%d" % (case, o), net.logits(x, o))
        if n < 16:
            for o, t in enumerate(net.forward(x)):
                d.save("%s_out%d" % (case, o), t)
        g = torch.Generator().manual_seed(900 + n + H)
        head, eye = net.masks(torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).cuda())
        d.save("%s_head" % case, head)
        d.save("%s_eye" % case, eye)
        z = m.feature_sizes(H, W)
        d.nt(case, [(m.CONVS[b][0], n * z[lv][0] * z[lv][1], m.CONVS[b][3] or 32) for b, lv in sorted(level.items())])
    d.save("block0", net.block(0, rand((3, 3, 45, 39), 14, -2.0, 2.0)))  # the stem: the one haloed map


def child(net, out):
    import torch
    assert torch.cuda.is_available(), "conv_nets_dump needs a GPU"
    d = Dump(out, net)
    with torch.no_grad():
        globals()["run_" + net](d)
    torch.cuda.synchronize()
    print("%s: %d files" % (net, d.files))


def compare(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    unequal = [n for n in names if not (os.path.isfile(os.path.join(a, n)) and os.path.isfile(os.path.join(b, n))
                                       and filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False))]
    sizes = {n: os.path.getsize(os.path.join(a, n)) for n in names if os.path.isfile(os.path.join(a, n))}
    print(json.dumps({"files": len(names), "bytes": sizes, "unequal": unequal, "verdict": "equal byte for byte" if names and not unequal else "NOT equal"},
                     sort_keys=True))
    return 0 if names and not unequal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--nets", nargs="+", default=list(NETS), choices=NETS)
    ap.add_argument("--timeout", type=int, default=150, help="seconds a network's child process may take")
    ap.add_argument("--child", default=None, choices=NETS)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    assert args.out, "--out DIR"
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out)
        return 0
    for net in args.nets:  # the parent never touches the GPU; each network gets a fresh process
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", net, "--out", args.out], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("conv_nets_dump: %s ended with status %d; stopping" % (net, rc))
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
