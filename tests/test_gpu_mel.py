"""The audio front end on the GPU: n3dt.MelFrontend / MelStream / audio.clip_audiostyle (n3dt_mel_spectrogram, n3dt_mel_windows,
csrc/mel.hip) against the float64 restatement's recorded fixtures (tests/golden/mel.*, tools/gen_golden_mel.py).

Tolerance.  The kernel works in float64 like the restatement; the two differ in the order of the DFT's and the basis product's
sums and in the device's sqrt and log10.  Three float64 evaluation orders on the CPU (rfft, the DFT through BLAS, the DFT term
by term) agree with an 80-bit evaluation to 5.7e-13 in normalised mel units, and the host build of the kernel's own arithmetic
(tests/test_mel_cpu.py) sits at 4.4e-13 on the 999-sample fixture.  The bound is the project's bound for its float64 pins, 1e-9 absolute.  The fp32 output
is the float64 output rounded once, so it is compared bitwise; so is everything the streaming form, a shifted signal, a second
call and a graph replay give."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9
LENGTHS = (401, 800, 999, 1000, 3201, 16000, 40000)


def dev():
    return torch.device("cuda:0")


def gpu(a):
    return torch.as_tensor(a).to(dev())


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("mel")


@pytest.fixture(scope="module")
def front():
    from n3dt import MelFrontend
    return MelFrontend()


@pytest.fixture(scope="module")
def offline(fixture, front):
    """{length: (wav on the device, melspectrogram in float64)}: computed once, never modified"""
    data, _ = fixture
    out = {}
    for L in LENGTHS:
        wav = gpu(data["len%d/wav" % L])
        out[L] = (wav, front.melspectrogram(wav, dtype=torch.float64))
    return out


@pytest.mark.parametrize("L", LENGTHS)
def test_fixtures_in_float64_and_fp32(fixture, front, offline, L):
    data, _ = fixture
    want = data["len%d/mel" % L]
    wav, m64 = offline[L]
    assert m64.dtype == torch.float64 and m64.is_cuda and tuple(m64.shape) == (80, 1 + L // 200) == want.shape
    err = float(np.abs(m64.cpu().numpy() - want).max())
    print("len%d: max |d mel| %.3e (bound %.0e)" % (L, err, TOL))
    assert err <= TOL
    m32 = front.melspectrogram(wav)
    assert m32.dtype == torch.float32 and torch.equal(m32, m64.to(torch.float32))
    # the clips are exact on both sides: the same entries sit at -4 and at +4
    for clip in (-4.0, 4.0):
        assert np.array_equal(m64.cpu().numpy() == clip, want == clip), clip


@pytest.mark.parametrize("L", [401, 800, 999, 1000])
def test_boundary_lengths_reflect_on_both_sides(fixture, offline, L):
    """Every frame of these signals reads reflected samples on one side or on both (401: all three frames on both)."""
    data, _ = fixture
    want = data["len%d/mel" % L]
    got = offline[L][1].cpu().numpy()
    T = 1 + L // 200
    assert got.shape == (80, T)
    for t in (0, 1, T - 2, T - 1):
        err = float(np.abs(got[:, t] - want[:, t]).max())
        print("len%d frame %d: %.3e" % (L, t, err))
        assert err <= TOL, t


def _stream(front, wav, sizes, dtype=torch.float64):
    s = front.stream(dtype=dtype)
    cols, pos = [], 0
    for n in sizes:
        out = s.push(wav[pos:pos + n].contiguous())
        assert out.dtype == dtype and out.shape[0] == 80
        pos += n
        # frame t is out once 200 t + 401 samples are in
        assert s.next_frame == (0 if pos < 401 else (pos - 401) // 200 + 1)
        cols.append(out)
    assert pos == wav.shape[0]
    cols.append(s.flush())
    return torch.cat(cols, dim=1)


def _blocks(L, size):
    return [size] * (L // size) + ([L % size] if L % size else [])


@pytest.mark.parametrize("L,size", [(3201, 1), (3201, 199), (3201, 200), (3201, 201), (3201, 1000),
                                    (16000, 199), (16000, 200), (16000, 201), (16000, 1000)])
def test_stream_in_fixed_blocks_is_bitwise_the_offline_result(front, offline, L, size):
    wav, want = offline[L]
    assert torch.equal(_stream(front, wav, _blocks(L, size)), want)


@pytest.mark.parametrize("L", [3201, 16000])
def test_stream_in_a_random_partition_and_flush_alone(front, offline, L):
    wav, want = offline[L]
    rng = np.random.default_rng(L + 1)
    sizes = []
    while sum(sizes) < L:  # empty blocks, single samples and blocks of several frames
        sizes.append(min(int(rng.choice([0, 1, 7, 93, 200, 333, 1024])), L - sum(sizes)))
    assert 0 in sizes and 1 in sizes and max(sizes) > 800
    assert torch.equal(_stream(front, wav, sizes), want)
    assert torch.equal(_stream(front, wav, [L]), want)                       # one push, then flush
    s = front.stream(dtype=torch.float64)                                    # a push too short for any frame: flush gives it all
    assert s.push(wav[:400].contiguous()).shape == (80, 0)
    s2 = front.stream(dtype=torch.float32)
    got32 = torch.cat([s2.push(wav[:L // 2].contiguous()), s2.push(wav[L // 2:].contiguous()), s2.flush()], dim=1)
    assert got32.dtype == torch.float32 and torch.equal(got32, want.to(torch.float32))
    with pytest.raises(ValueError, match="after flush"):
        s2.push(wav[:10].contiguous())


def test_frames_do_not_depend_on_their_position_in_the_signal(front, offline):
    """Frames t >= 3 of wav read samples 200 and later only (and multiply sample 200 t - 400, whose pre-emphasis differs at the
    cut, by the window's exact 0): they are frames t - 1 of wav[200:].  The frames that reflect about the end are left out."""
    wav, m = offline[16000]
    shifted = front.melspectrogram(wav[200:].contiguous(), dtype=torch.float64)
    assert shifted.shape[1] == m.shape[1] - 1
    last = (16000 - 400) // 200  # 200 t + 399 <= L - 1
    assert last == 78 and torch.equal(m[:, 3:last + 1], shifted[:, 2:last])


def test_two_calls_and_a_graph_replay_give_the_same_bits(front, offline):
    wav, m = offline[16000]
    assert torch.equal(front.melspectrogram(wav, dtype=torch.float64), m)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = front.melspectrogram(wav, dtype=torch.float64)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, m)


def test_nan_samples_give_nan_frames_and_nothing_else(front, offline):
    wav = offline[3201][0].clone()
    wav[1700] = float("nan")
    m = front.melspectrogram(wav, dtype=torch.float64)
    bad = torch.isnan(m).all(dim=0).cpu().numpy()
    # samples 1700 and (through the pre-emphasis) 1701 are read by the frames with 200 t - 400 <= 1701 and 200 t + 399 >= 1700
    want = np.array([200 * t - 400 <= 1701 and 200 * t + 399 >= 1700 for t in range(17)])
    assert np.array_equal(bad, want) and not torch.isnan(m[:, torch.as_tensor(~want).to(dev())]).any()


@pytest.mark.parametrize("L", [16000, 40000])
def test_windows_equal_the_recorded_windows(fixture, front, offline, L):
    data, manifest = fixture
    case = next(c for c in manifest["cases"] if c["length"] == L)
    m64 = offline[L][1]
    m32 = m64.to(torch.float32)
    rec64 = gpu(data["len%d/mel" % L])
    rec32 = rec64.to(torch.float32)
    T = m64.shape[1]
    assert len(case["windows"]) == 4
    for w in case["windows"]:
        got = front.windows(m32, w["frame_ids"], fps=w["fps"], rule=w["rule"])
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(w["frame_ids"]), 80, 16)
        # against the device's own spectrogram bitwise: the gather moves values, it computes nothing
        starts = w["starts"]
        cols = torch.as_tensor([[min(max(s + c, 0), T - 1) for c in range(16)] for s in starts], device=dev())
        assert torch.equal(got, m32[:, cols].permute(1, 0, 2))
        assert torch.equal(front.windows(m64, w["frame_ids"], fps=w["fps"], rule=w["rule"]), got)  # float64 in: rounded at the store
        # the recorded windows were cut from the restatement's spectrogram: from that very spectrogram, bitwise, in either dtype
        assert np.array_equal(front.windows(rec32, w["frame_ids"], fps=w["fps"], rule=w["rule"]).cpu().numpy(), data[w["key"]])
        assert np.array_equal(front.windows(rec64, w["frame_ids"], fps=w["fps"], rule=w["rule"]).cpu().numpy(), data[w["key"]])
        if w["rule"] == "chunk":
            assert starts[-1] == T - 16 and torch.equal(got[-1], m32[:, T - 16:])
        else:
            assert starts[0] < -1 and starts[1] < -1
            for f in (0, 1):  # the window starts before the signal: its first columns repeat column 0
                k = -starts[f]
                assert torch.equal(got[f, :, :k + 1], m32[:, :1].expand(80, k + 1))


def test_a_caller_supplied_basis_replaces_the_built_in_one(offline):
    """Half the basis is half the mel amplitude exactly: every value that is clipped on neither side moves by 8 * 20 log10(0.5) / 100."""
    import n3dt
    wav, m = offline[16000]
    half = n3dt.MelFrontend(mel_basis=n3dt.mel_basis() * np.float32(0.5)).melspectrogram(wav, dtype=torch.float64)
    free = (m.abs() < 4.0) & (half.abs() < 4.0)
    assert float(free.double().mean()) > 0.4
    shift = 8.0 * 20.0 * np.log10(0.5) / 100.0
    err = float((half - m - shift)[free].abs().max())
    print("half basis: max deviation from the shift %.3e" % err)
    assert err <= TOL
    assert bool((half <= m).all())


@pytest.mark.parametrize("per", [1, 4])
def test_clip_audiostyle_is_the_recipe_by_hand(front, offline, per):
    import n3dt
    torch.manual_seed(0)
    a2s = n3dt.Audio2style().to(dev()).eval()
    wav = offline[16000][0]
    n_frames = 6
    got = n3dt.audio.clip_audiostyle(a2s, front, wav, n_frames, fps=25.0, frames_per_sequence=per)
    assert tuple(got.shape) == (n_frames, 64) and got.dtype == torch.float32
    windows = front.windows(front.melspectrogram(wav), range(n_frames), fps=25.0, rule="chunk")
    with torch.no_grad():
        by_hand = torch.cat([a2s(windows[i:i + per]) for i in range(0, n_frames, per)])
    assert torch.equal(got.detach(), by_hand)
    assert not a2s.training  # the module's mode is the caller's


def test_short_signals_and_wrong_dtypes_raise(front, offline):
    wav = offline[800][0]
    with pytest.raises(ValueError, match="at least 401"):
        front.melspectrogram(wav[:400].contiguous())
    with pytest.raises(ValueError, match="float32"):
        front.melspectrogram(wav.double())
    with pytest.raises(ValueError, match="contiguous"):
        front.melspectrogram(wav[::2])
    s = front.stream()
    assert s.push(wav[:400].contiguous()).shape == (80, 0)
    with pytest.raises(ValueError, match="received 400 samples"):
        s.flush()
    with pytest.raises(ValueError, match="at least 16"):
        front.windows(offline[1000][1], [0])  # 6 mel frames: no 16-column chunk
    assert tuple(front.windows(offline[1000][1], [0, 1, 2, 9], rule="centered").shape) == (4, 80, 16)
