"""Host side of the Wav2Lip generator (n3dt.Wav2Lip / n3dt.Wav2LipClip, n3dt_wav2lip_*), no GPU: the exports and their documented
refusals, the sizes against the table, the float64 restatement against the fixture recorded from the reference's class, its
transposed convolution against torch's, the 5-D form, the state-dict loader, the mel windows against literal loops, the fixture's
own conditions, and the kernels' index arithmetic (csrc/wav2lip_core.h) walked over the convolution kernel's grid on the CPU under
the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wav2lip_restatement as wr
from test_eval_metrics_cpu import _host_compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"n3dt_wav2lip_packed_bytes", "n3dt_wav2lip_pack", "n3dt_wav2lip_workspace_bytes", "n3dt_wav2lip_fwd", "n3dt_wav2lip_block",
       "n3dt_wav2lip_face_inputs", "n3dt_wav2lip_paste"}


@pytest.fixture(scope="module")
def fixture(golden):
    data, manifest = golden("wav2lip")
    samples, _ = golden("wav2lip_blocks")
    return data, manifest, samples


@pytest.fixture(scope="module")
def weights():
    from n3dt import synthetic as syn
    return syn.wav2lip_state_dict(wr.WEIGHTS_SEED)


@pytest.fixture(scope="module")
def restated(fixture, weights):
    data = fixture[0]
    faces, mel = wr.faces_from_u8(data["faces_u8"]), wr.mel_from_u8(data["mel_u8"])
    acts, image = wr.chain64(weights, faces, mel)
    return faces, mel, acts, image


def test_new_symbols_are_declared_and_exported():
    from n3dt import _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "n3dt.h")).read()
    declared = set(re.findall(r"\b(n3dt_wav2lip[a-z0-9_]*)\s*\(", header))
    assert declared == NEW
    for name in declared:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        for claimed in ("n3dt_syncnet", "n3dt_lpips", "n3dt_mel", "n3dt_eval_metrics", "n3dt_flat_adam"):
            assert not name.startswith(claimed)
    assert L.n3dt_abi_version() == 5
    assert ctypes.sizeof(_lib.Wav2lipParams) == 6 * 51 * ctypes.sizeof(ctypes.c_void_p)
    import n3dt
    assert n3dt.Wav2Lip is n3dt.wav2lip.Wav2Lip and n3dt.Wav2LipClip is n3dt.wav2lip.Wav2LipClip and n3dt.load_wav2lip is n3dt.wav2lip.load_wav2lip


def test_sizes_follow_the_table():
    from n3dt import _lib
    from n3dt.wav2lip import BLOCKS, DECODER_ENDS, FACE_ENDS, HEAD, SKIP_OF, block_names, block_shapes, state_dict_keys
    L = _lib.lib()
    for n in (0, 129, -1):
        assert L.n3dt_wav2lip_workspace_bytes(n) == 0 and b"n outside 1..128" in L.n3dt_last_error()
    assert len(BLOCKS) == len(block_names()) == 51 and len(set(block_names())) == 51
    assert sum(1 for b in BLOCKS if b[0]) == 6
    shapes = block_shapes()
    assert shapes[0] == ((6, 96, 96), (16, 96, 96)) and shapes[17][1] == (512, 1, 1) and shapes[18][0] == (1, 80, 16)
    assert shapes[21][1] == (64, 27, 16) and shapes[24][1] == (128, 9, 6) and shapes[27][1] == (256, 3, 3) and shapes[30][1] == (512, 1, 1)
    assert shapes[31] == ((512, 1, 1), (512, 1, 1)) and shapes[32] == ((1024, 1, 1), (512, 3, 3)) and shapes[34] == ((1024, 3, 3), (512, 6, 6))
    assert shapes[46] == ((160, 48, 48), (64, 96, 96)) and shapes[49] == ((80, 96, 96), (32, 96, 96)) and shapes[50][1] == (3, 96, 96)
    # the concatenations: the decoder group's output first, the encoder feature behind it; what follows takes both
    cats = []
    for d in DECODER_ENDS:
        (cd, hd, wd), (cf, hf, wf) = shapes[d][1], shapes[SKIP_OF[d]][1]
        assert (hd, wd) == (hf, wf) and shapes[d + 1][0] == (cd + cf, hd, wd)
        cats.append((cd + cf, hd))
    assert [c for c, _ in cats] == [1024, 1024, 768, 512, 320, 160, 80] and sorted(SKIP_OF.values()) == FACE_ENDS
    # packed: hi + lo bf16 matrices with C_in padded to 16 and C_out to 32, the head's 3 x 32 fp32, then the biases, each to 256 bytes
    rup = lambda v: (v + 255) // 256 * 256  # noqa: E731
    mats = [rup(3 * 32 * 4) if b == HEAD else kh * kw * ((cin + 15) // 16 * 16) * ((cout + 31) // 32 * 32) * 4
            for b, (_, cin, cout, (kh, kw), _, _, _, _) in enumerate(BLOCKS)]
    assert all(m % 256 == 0 for m in mats)
    assert L.n3dt_wav2lip_packed_bytes() == sum(mats) + sum(rup(b[2] * 4) for b in BLOCKS)
    n_params = sum(int(np.prod(s)) for k, s in state_dict_keys().items() if "running" not in k)
    assert n_params == 36298035
    # workspace per window: the seven concatenation buffers with their halo (none on the 1 x 1 map), and two copies of the largest
    # other map: a decoder block's [64, 96 + 2, 96 + 2]
    halo = [0, 1, 1, 1, 1, 1, 1]
    per_window = sum(c * (h + 2 * p) ** 2 for (c, h), p in zip(cats, halo)) + 2 * 64 * 98 * 98
    for n in (1, 3, 65, 128):
        assert L.n3dt_wav2lip_workspace_bytes(n) == 4 * n * per_window
    assert 11.1e6 < 4 * per_window < 11.3e6


def test_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    from n3dt import _lib
    L = _lib.lib()
    d, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    need = L.n3dt_wav2lip_workspace_bytes(3)
    good = [3, d, d, d, d, d, need, None]  # n, packed, mel, faces, out, ws, ws_bytes, stream
    for i in (1, 2, 3, 4, 5):
        args = list(good)
        args[i] = None
        assert L.n3dt_wav2lip_fwd(*args) == -1 and b"NULL" in L.n3dt_last_error(), i
    for i, what in ((2, b"16-byte"), (3, b"16-byte"), (4, b"16-byte"), (1, b"256-byte"), (5, b"256-byte")):
        args = list(good)
        args[i] = odd
        assert L.n3dt_wav2lip_fwd(*args) == -1 and what in L.n3dt_last_error(), i
    args = list(good)
    args[6] = need - 1
    assert L.n3dt_wav2lip_fwd(*args) == -1 and b"workspace too small" in L.n3dt_last_error()
    for n in (0, 129):
        assert L.n3dt_wav2lip_fwd(n, *good[1:]) == -1 and b"n outside 1..128" in L.n3dt_last_error()
    big = 1 << 40
    for block in (-1, 51):
        assert L.n3dt_wav2lip_block(block, 1, d, d, None, d, d, big, None) == -1 and b"block outside 0..50" in L.n3dt_last_error()
    for n in (0, 129):
        assert L.n3dt_wav2lip_block(0, n, d, d, None, d, d, big, None) == -1 and b"n outside" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_block(0, 1, d, None, None, d, d, big, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_block(0, 1, d, d, None, None, d, big, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_block(31, 1, d, d, odd, d, d, big, None) == -1 and b"16-byte" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_block(0, 1, odd, d, None, d, d, big, None) == -1 and b"256-byte" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_block(0, 1, d, d, None, d, d, 16, None) == -1 and b"workspace too small" in L.n3dt_last_error()
    # n, H, W, frames, ref, boxes, n_boxes, out, stream
    assert L.n3dt_wav2lip_face_inputs(3, 64, 64, d, None, d, 2, d, None) == -1 and b"n_boxes" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_face_inputs(3, 1, 64, d, None, d, 1, d, None) == -1 and b"2..4096" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_face_inputs(3, 64, 64, None, None, d, 3, d, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_face_inputs(3, 64, 64, d, None, d, 3, None, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_face_inputs(3, 64, 64, d, None, d, 3, odd, None) == -1 and b"16-byte" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_face_inputs(3, 64, 64, ctypes.c_void_p(4097), None, d, 3, d, None) == -1 and b"4-byte" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_face_inputs(0, 64, 64, d, None, d, 1, d, None) == -1 and b"n outside 1..4096" in L.n3dt_last_error()
    # n, H, W, faces, frames, boxes, n_boxes, out, stream
    assert L.n3dt_wav2lip_paste(3, 64, 64, None, d, d, 3, d, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_paste(3, 64, 64, d, d, None, 3, d, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_paste(3, 64, 64, d, d, d, 4, d, None) == -1 and b"n_boxes" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_paste(3, 64, 5000, d, d, d, 3, d, None) == -1 and b"2..4096" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_paste(3, 64, 64, odd, d, d, 3, d, None) == -1 and b"16-byte" in L.n3dt_last_error()
    p = _lib.Wav2lipParams()
    assert L.n3dt_wav2lip_pack(ctypes.byref(p), d, None) == -1 and b"NULL parameter" in L.n3dt_last_error()
    assert L.n3dt_wav2lip_pack(None, d, None) == -1 and L.n3dt_wav2lip_pack(ctypes.byref(p), None, None) == -1
    assert L.n3dt_wav2lip_pack(ctypes.byref(p), ctypes.c_void_p(4100), None) == -1 and b"256-byte" in L.n3dt_last_error()


def test_cpu_tensors_raise(weights):
    from n3dt import Wav2Lip, Wav2LipClip
    from n3dt.wav2lip import face_inputs, paste
    net = Wav2Lip(weights)
    mel, faces = torch.zeros(1, 1, 80, 16), torch.zeros(1, 6, 96, 96)
    frames = torch.zeros(2, 3, 32, 32)
    for call in (lambda: net(mel, faces), lambda: net(mel[None], faces.permute(1, 0, 2, 3)[None]), lambda: net.layers(mel, faces),
                 lambda: net.block(0, faces), lambda: face_inputs(frames, (0, 32, 0, 32)), lambda: paste(torch.zeros(2, 3, 96, 96), frames, (0, 32, 0, 32)),
                 lambda: Wav2LipClip(net).generate(frames, (0, 32, 0, 32), torch.zeros(80, 100), 25.0)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(TypeError, match="Wav2Lip"):
        Wav2LipClip(object())


def test_stand_in_weights_are_seeded_and_have_the_stated_statistics(weights):
    from n3dt import synthetic as syn
    from n3dt.wav2lip import BLOCKS, HEAD, block_names
    again = syn.wav2lip_state_dict(wr.WEIGHTS_SEED)
    assert sorted(weights) == sorted(again) and all(torch.equal(weights[k], again[k]) for k in weights)
    other = syn.wav2lip_state_dict(wr.WEIGHTS_SEED + 1)
    assert not torch.equal(weights["audio_encoder.0.conv_block.0.weight"], other["audio_encoder.0.conv_block.0.weight"])
    assert len(weights) == 50 * 7 + 2
    for b, (name, (tr, cin, cout, (kh, kw), _, _, _, _)) in enumerate(zip(block_names(), BLOCKS)):
        bound = (cin * kh * kw) ** -0.5 * (1.0 + 2.0 ** -22)
        if b == HEAD:
            w, bias = weights[name + ".weight"], weights[name + ".bias"]
            assert float(w.abs().max()) <= bound * syn.WAV2LIP_HEAD_WEIGHT_SCALE and float(bias.abs().max()) <= bound * syn.WAV2LIP_HEAD_BIAS_SCALE
            continue
        w, bias = weights[name + ".conv_block.0.weight"], weights[name + ".conv_block.0.bias"]
        assert tuple(w.shape) == ((cin, cout, kh, kw) if tr else (cout, cin, kh, kw))  # ConvTranspose2d: C_in on axis 0
        assert 0.9 * bound < float(w.abs().max()) <= bound and float(bias.abs().max()) <= bound
        var, gamma = weights[name + ".conv_block.1.running_var"], weights[name + ".conv_block.1.weight"]
        assert 0.5 <= float(var.min()) and float(var.max()) <= 1.5 and 0.5 <= float(gamma.min()) and float(gamma.max()) <= 1.5


def test_loader_takes_the_three_forms_and_is_strict(weights, tmp_path):
    from n3dt.wav2lip import Wav2Lip, load_wav2lip
    plain = load_wav2lip(weights)
    assert len(plain) == 51 and all(len(b) == 6 for b in plain[:50]) and len(plain[50]) == 2
    checkpoint = {"state_dict": {"module." + k: v for k, v in weights.items()}, "optimizer": None, "global_step": 7, "global_epoch": 1}
    path = tmp_path / "wav2lip_stand_in.pth"
    torch.save(checkpoint, str(path))
    for form in (checkpoint, str(path), path):
        for a, b in zip(plain, load_wav2lip(form)):
            assert all(torch.equal(s, t) for s, t in zip(a, b))
    without = {k: v for k, v in weights.items() if "num_batches_tracked" not in k}
    assert len(Wav2Lip(without).weights) == 51
    for key in ("face_encoder_blocks.0.0.conv_block.0.weight", "audio_encoder.12.conv_block.1.running_var", "face_decoder_blocks.1.0.conv_block.0.bias",
                "output_block.0.conv_block.1.bias", "output_block.1.weight", "output_block.1.bias"):
        sd = {k: v for k, v in weights.items() if k != key}
        with pytest.raises(KeyError, match=re.escape(key)):
            Wav2Lip(sd)
    sd = dict(weights)
    sd["face_decoder_blocks.1.0.conv_block.0.weight"] = torch.zeros(512, 1024, 3, 3)  # a ConvTranspose2d weight is [C_in, C_out, kh, kw]
    with pytest.raises(ValueError, match=r"face_decoder_blocks\.1\.0\.conv_block\.0\.weight"):
        Wav2Lip(sd)
    sd = dict(weights)
    sd["output_block.1.bias"] = torch.zeros(32)
    with pytest.raises(ValueError, match=r"output_block\.1\.bias"):
        Wav2Lip(sd)
    sd = dict(weights)
    sd["face_decoder_blocks.7.0.conv_block.0.weight"] = torch.zeros(3)
    with pytest.raises(KeyError, match="unexpected"):
        Wav2Lip(sd)
    with pytest.raises(TypeError):
        Wav2Lip([1, 2, 3])


def test_restatement_reproduces_every_fixture_value(fixture, weights, restated, golden):
    data, manifest, samples = fixture
    assert manifest["weights_seed"] == wr.WEIGHTS_SEED and manifest["input_seed"] == wr.INPUT_SEED and manifest["n_windows"] == wr.N_WINDOWS == 3
    assert sorted(manifest["parity_unpinned"]) == ["opencv_resize", "weights"] and manifest["n_params"] == 36298035
    checksum = float(sum(float(v.double().abs().sum()) for v in weights.values()))
    assert abs(checksum - manifest["weights_checksum"]) <= 1e-9 * checksum, "the seeded weight generator drifted from the fixture"
    faces_u8, mel_u8 = wr.fixture_inputs()
    assert np.array_equal(faces_u8, data["faces_u8"]) and np.array_equal(mel_u8, data["mel_u8"])
    assert not faces_u8[:, :3, 48:].any() and faces_u8[:, 3:, 48:].any()
    _, _, acts, image = restated
    assert len(acts) == 51 and [list(x.shape[1:]) for x in acts] == manifest["block_shapes"]
    for b, act in enumerate(acts):
        s, sa, sample = wr.summary(act)
        want_s, want_sa = data["block_sums"][b]
        assert abs(sa / want_sa - 1.0) <= 1e-12 and abs(s - want_s) <= 1e-12 * want_sa, b
        want = samples["block%02d/sample" % b]
        assert sample.shape == want.shape and np.abs(sample - want).max() <= 1e-12 * np.abs(want).max(), b
        assert abs(float(act.abs().max()) / manifest["block_max_abs"][b] - 1.0) < 1e-12
    assert np.abs(image.numpy() - data["image"]).max() <= 1e-12
    logits = golden("wav2lip_logits")[0]["logits"]  # the pre-sigmoid logits in full, a file of their own for the size limit
    assert logits.shape == (3, 3, 96, 96) and logits.dtype == np.float64
    assert np.abs(acts[-1].numpy() - logits).max() <= 1e-12 * np.abs(logits).max()
    assert np.abs(1.0 / (1.0 + np.exp(-logits)) - data["image"]).max() <= 1e-15


def test_fixture_conditions_hold_for_the_reference_alone(fixture, restated):
    data, manifest, _ = fixture
    image = data["image"]
    assert image.shape == (3, 3, 96, 96) and image.dtype == np.float64
    assert image.min() <= 0.2 and image.max() >= 0.8
    assert float(((image <= 0.02) | (image >= 0.98)).mean()) <= 0.01
    assert len(manifest["block_zero_share"]) == 51 and max(manifest["block_zero_share"]) <= 0.6
    assert 0.5 <= max(manifest["block_max_abs"]) <= 8.0 and min(manifest["block_max_abs"][:50]) >= 0.5  # O(1) through all blocks
    for b, act in enumerate(restated[2]):  # and of the values the restatement pins them with
        assert abs(float((act == 0).double().mean()) - manifest["block_zero_share"][b]) <= 1e-9, b


def test_bounds_are_measured_from_the_emulation_alone(fixture, weights, restated):
    """The manifest's bounds are the emulation's error on the machine that generated the fixture.  Another CPU sums the fp32
    convolutions in another order; what this machine measures must sit within the same 4 x the GPU gets (figures printed)."""
    _, manifest, _ = fixture
    bounds = manifest["bounds"]
    assert bounds["gpu_factor"] == 4.0 and len(bounds["block"]) == 51
    assert all(1e-7 < v < 1e-4 for v in bounds["block"]) and 1e-7 < bounds["image"] < bounds["logits"] < 1e-3
    faces, mel, acts, image = restated
    here = wr.measured_bounds(weights, faces, mel, acts, image)
    for b in range(51):
        print("block %2d: emulation error here %.3e, recorded %.3e" % (b, here["block"][b], bounds["block"][b]))
        assert here["block"][b] <= 4.0 * bounds["block"][b], b
    print("logits %.3e (recorded %.3e), image %.3e (recorded %.3e)" % (here["logits"], bounds["logits"], here["image"], bounds["image"]))
    assert here["logits"] <= 4.0 * bounds["logits"] and here["image"] <= 4.0 * bounds["image"]


@pytest.mark.parametrize("cin,cout,hw,stride", [(1024, 512, (1, 1), 1), (1024, 512, (3, 3), 2), (768, 384, (6, 6), 2), (512, 256, (12, 12), 2),
                                                 (320, 128, (24, 24), 2), (160, 64, (48, 48), 2), (16, 32, (5, 7), 2)])
def test_parity_gather_is_torchs_transposed_convolution(cin, cout, hw, stride):
    """the six transposed blocks' shapes and a 5 x 7 map with odd extents, in float64"""
    g = torch.Generator().manual_seed(cin + hw[0])
    x = torch.randn(2, cin, *hw, generator=g, dtype=torch.float64)
    w = torch.randn(cin, cout, 3, 3, generator=g, dtype=torch.float64) / (3.0 * cin ** 0.5)
    want = F.conv_transpose2d(x, w, None, stride=stride, padding=0 if stride == 1 else 1, output_padding=0 if stride == 1 else 1)
    got = wr.conv_transpose_gather(x, w, stride)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_folded_batch_norm_is_the_formula(weights, restated):
    from n3dt.wav2lip import BLOCKS
    faces, mel, acts, _ = restated
    ins = wr.block_inputs(acts, faces, mel)
    for b in (0, 17, 21, 32, 34, 46, 49):
        tr, _, _, _, stride, pad, op, residual = BLOCKS[b]
        w, bias, gamma, beta, mean, var = wr.block_params(weights, b)
        s = gamma / torch.sqrt(var + 1e-5)
        if tr:
            y = F.conv_transpose2d(ins[b], w * s[None, :, None, None], (bias - mean) * s + beta, stride=stride, padding=pad, output_padding=op)
        else:
            y = F.conv2d(ins[b], w * s[:, None, None, None], (bias - mean) * s + beta, stride=stride, padding=pad)
        y = torch.relu(y + ins[b] if residual else y)
        assert float((y - acts[b]).abs().max()) <= 1e-13 * float(acts[b].abs().max()), b
        w32, _ = wr.fold(weights, b)
        hi, lo = wr.split(w32)
        assert w32.dtype == torch.float32 and float((w32 - hi - lo).abs().max()) <= 2.0 ** -16 * float(w32.abs().max())


def test_five_d_call_is_the_stacked_four_d_call(fixture, weights, restated):
    from n3dt.wav2lip import flatten_sequences, unflatten_sequences
    data = fixture[0]
    faces, mel, _, image = restated
    out5 = wr.forward64(weights, mel[None], faces.permute(1, 0, 2, 3)[None])  # [1,3,1,80,16], [1,6,3,96,96]
    assert tuple(out5.shape) == (1, 3, 3, 96, 96) and torch.equal(out5[0].permute(1, 0, 2, 3), image)
    s, sa, sample = wr.summary(out5)
    assert abs(s - data["image5/sums"][0]) <= 1e-12 * sa and abs(sa / data["image5/sums"][1] - 1.0) <= 1e-12
    assert np.abs(sample - data["image5/sample"]).max() <= 1e-12
    # the package's flattening and re-stacking against the reference's own lines, B = 2, T = 3
    g = torch.Generator().manual_seed(3)
    a, f = torch.rand(2, 3, 1, 80, 16, generator=g), torch.rand(2, 6, 3, 96, 96, generator=g)
    fa, ff = flatten_sequences(a, f)
    assert torch.equal(fa, torch.cat([a[:, i] for i in range(3)], dim=0)) and torch.equal(ff, torch.cat([f[:, :, i] for i in range(3)], dim=0))
    x = torch.rand(6, 3, 96, 96, generator=g)
    assert torch.equal(unflatten_sequences(x, 2, 3), torch.stack(torch.split(x, 2, dim=0), dim=2))
    with pytest.raises(ValueError, match="differ in B or T"):
        flatten_sequences(a, f[:, :, :2])


def test_mel_windows_against_literal_loops():
    from n3dt.wav2lip import chunk, chunk_start, segmented_mels
    g = torch.Generator().manual_seed(9)
    for fps in (25.0, 25, 30.0, 29.97, 12.5):
        n_frames = 40
        T = int(80.0 * n_frames / float(fps)) + 3
        mel = torch.rand(80, T, generator=g)
        spec = mel.numpy().T.copy()  # the reference's orig_mel: [T, 80]
        for frame_id in (0, 1, 2, n_frames - 8, n_frames - 7, n_frames - 6, n_frames - 5, n_frames - 4, n_frames - 3, n_frames - 2, n_frames - 1):
            # get_segmented_mels over crop_audio_window
            want = []
            start_frame_num = frame_id + 1
            if start_frame_num - 2 < 0:
                start_frame_num = 3
            for i in range(start_frame_num, start_frame_num + 5):
                start_idx = int(80. * ((i - 2) / float(fps)))
                m = spec[start_idx:start_idx + 16, :]
                if m.shape[0] != 16:
                    want = None
                    break
                want.append(m.T)
            got = segmented_mels(mel, frame_id, fps)
            assert (got is None) == (want is None), (fps, frame_id)
            if want is not None:
                assert tuple(got.shape) == (5, 80, 16) and np.array_equal(got.numpy(), np.asarray(want))
            # main's chunk
            mel_idx_multiplier = 80. / fps
            start_idx = int(frame_id * mel_idx_multiplier)
            if start_idx + 16 > T:
                want_chunk = spec.T[:, T - 16:]
            else:
                want_chunk = spec.T[:, start_idx:start_idx + 16]
            assert np.array_equal(chunk(mel, frame_id, fps).numpy(), want_chunk) and chunk_start(T, frame_id, fps) in (start_idx, T - 16)
        assert segmented_mels(mel, n_frames + 5, fps) is None
        assert chunk_start(T, n_frames + 50, fps) == T - 16
    assert torch.equal(segmented_mels(torch.arange(80.0 * 200).reshape(80, 200), 0, 25.0)[0, 0], torch.arange(3.0, 19.0))  # frame 0 -> 3 - 2 = 1


# the window counts of the GPU tests: one, the fixture's three, and 65, which crosses a 64-row tile on the 1 x 1 and 3 x 3 maps
COUNTS = (1, 3, 65)


def test_index_walk_on_the_host_under_sanitizers(tmp_path):
    """csrc/wav2lip_core.h -- the functions the convolution kernel takes its classes, rows, halo cells, taps, residual reads and
    stores from -- over the kernel's full grid on the CPU, all 51 blocks, n = 1, 3, 65, the maps in their chain form (concatenation
    buffers with their row stride and channel offset).  A stand-alone program with its own main, built here with the host compiler
    under -fsanitize=address,undefined and run directly.  A read outside a buffer ends it through the sanitizer; a tap that is not
    the (transposed) convolution's, an element stored twice or never -- halo cells, concatenation slices and all parity classes
    included -- or a packed weight read where the pack did not write it fails the program's own check.  Where the compiler has no
    sanitizer runtimes the indices are still checked, on an unsanitised build, and only the sanitizer claim is skipped."""
    from n3dt.wav2lip import block_shapes
    found = _host_compiler(tmp_path)
    if found is None:
        pytest.skip("no host C++ compiler found (tried $CXX, g++, c++, clang++)")
    cxx, flags = found
    exe = tmp_path / "wav2lip_core_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                           [os.path.join(REPO, "tests", "wav2lip_core_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)] + [str(n) for n in COUNTS], capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0 and not run.stderr.strip(), "sanitizer or program error:\n" + run.stderr
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()]
    assert [tuple(r[:2]) for r in rows] == [(n, b) for n in COUNTS for b in range(51)]
    shapes = block_shapes()
    classes = {32: 9, 34: 4, 37: 4, 40: 4, 43: 4, 46: 4}
    for r in rows:  # the extents are the table's, which the fixture pins to the reference's class
        n, b = r[:2]
        (cin, hi, wi), (cout, ho, wo) = shapes[b]
        assert r[2:6] == [hi, wi, ho, wo] and r[8] == cout
        assert r[10] == classes.get(b, 1)
        assert r[12] == n * r[6] * r[7] * cout  # every cell of the padded output, once
        assert r[11] > 0
    if not flags:
        pytest.skip("%s cannot link -fsanitize=address,undefined: the index walk was checked (it holds), the sanitizer claim was not" % cxx)
