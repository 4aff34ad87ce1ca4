"""The wrappers' per-device cache of packed weights on the GPU (n3dt._host.PackedCache): its rule on a build made of torch ops alone,
then the three classes that gained the rule with it -- SyncNet, LPIPS and VGGPerceptualLoss pack again after an in-place update of
a weight, and VGGPerceptualLoss orders a second stream behind its pack.  Everything is asserted bitwise; the shapes are each
library's smallest."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=g)).to(dev())


def byte_cache(source):
    """a cache whose value is a uint8 copy of the 16 float32 values of `source`, and the list its builds are counted in"""
    from n3dt._host import PackedCache
    builds = []

    def build(device, on_device):
        builds.append(len(on_device))
        buf = torch.zeros(64, dtype=torch.uint8, device=device)
        if on_device:
            assert on_device[0].device == device and on_device[0].is_contiguous()
            buf.copy_(on_device[0].view(torch.uint8))
        return buf, on_device

    return PackedCache(lambda: [source] if source is not None else [], build), builds


def bytes_of(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def test_a_hit_returns_the_same_buffer_and_an_in_place_update_or_clear_builds_again():
    t = torch.arange(16, dtype=torch.float32)
    cache, builds = byte_cache(t)
    first = cache.get(dev())
    assert cache.get(dev()) is first and cache.get(torch.device("cuda", 0)) is first and builds == [1]
    assert torch.equal(first.cpu(), bytes_of(t))
    t.add_(1)
    second = cache.get(dev())
    assert second is not first and builds == [1, 1] and cache.get(dev()) is second
    assert torch.equal(second.cpu(), bytes_of(t)) and not torch.equal(second.cpu(), first.cpu())
    cache.clear()
    third = cache.get(dev())
    assert third is not second and builds == [1, 1, 1] and torch.equal(third.cpu(), bytes_of(t))


def test_a_get_on_a_side_stream_right_behind_the_first_get_sees_the_packed_bytes():
    """No proof of the wait either: a 64-byte copy may be done before the side stream reads, ordered or not."""
    t = torch.arange(16, dtype=torch.float32) * 0.37
    cache, builds = byte_cache(t)
    side = torch.cuda.Stream()
    first = cache.get(dev())  # builds on the current stream; the host does not wait
    with torch.cuda.stream(side):
        again = cache.get(dev())
        seen = again.clone()
    torch.cuda.synchronize()
    assert again is first and builds == [1]
    assert torch.equal(seen.cpu(), bytes_of(t))


def test_nothing_watched_never_builds_again():
    cache, builds = byte_cache(None)
    first = cache.get(dev())
    with torch.cuda.stream(torch.cuda.Stream()):
        assert cache.get(dev()) is first
    assert cache.get(dev()) is first and builds == [0]
    torch.cuda.synchronize()


def syncnet_case():
    from n3dt import SyncNet, synthetic as syn
    from n3dt.syncnet import FACE_SHAPE, MEL_SHAPE
    mel, faces = rand((1,) + MEL_SHAPE, 1, -4.0, 4.0), rand((1,) + FACE_SHAPE, 2)  # one window

    def run(net):  # both embeddings and the cosine, [1, 1025]
        return torch.cat([e.double() for e in net(mel, faces)] + [net.cos(mel, faces)[:, None]], 1)

    return syn.syncnet_state_dict(3), "face_encoder.0.conv_block.0.bias", SyncNet, run


def lpips_case():
    from n3dt import LPIPS, synthetic as syn
    pred, gt = rand((1, 3, 31, 31), 4), rand((1, 3, 31, 31), 5)  # the library's smallest
    return syn.lpips_alex_state_dict(6), "lin0.model.1.weight", LPIPS, lambda lp: torch.cat([lp(pred, gt)[None], lp.layers(pred, gt)])


def vgg_run(f, pred, gt):
    """the term and the input gradient, flattened into one tensor"""
    x = pred.clone().requires_grad_(True)
    term = f(x, gt)
    term.backward()
    return torch.cat([term.detach().reshape(1), x.grad.reshape(-1)])


def vgg_case(precision):
    from n3dt import synthetic as syn
    from n3dt.perceptual import VGGPerceptualLoss
    pred, gt = rand((1, 3, 16, 16), 7), rand((1, 3, 16, 16), 8)  # B = 1, P = 16: the library's lower bound
    return syn.vgg16_features_state_dict(9), "features.0.bias", lambda sd: VGGPerceptualLoss(sd, precision=precision), lambda f: vgg_run(f, pred, gt)


CASES = {"syncnet": syncnet_case, "lpips": lpips_case, "vgg-fp32": lambda: vgg_case("fp32"), "vgg-bf16": lambda: vgg_case("bf16")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_repack_follows_the_weights_version(case):
    weights, key, make, run = CASES[case]()
    sd = {k: v.clone() for k, v in weights.items()}
    net = make(sd)
    before = run(net)
    sd[key].add_(0.5)  # in place: the version counter moves, the next call packs again
    after = run(net)
    fresh = run(make(sd))
    assert bool(torch.isfinite(before).all()) and bool(torch.isfinite(after).all())
    assert not torch.equal(before, after) and torch.equal(after, fresh)
    net.repack()  # still works, and changes nothing
    assert torch.equal(run(net), fresh)


def test_vgg_first_use_on_a_side_stream_then_a_call_on_the_default_stream():
    """The pack is enqueued on the side stream; the call on the default stream follows with no host synchronisation between and
    has to wait for it on the device.  The expected values come from a third object, used and synchronised on its own.
    Written to pass, run once: at this size an unordered read may well find the pack finished, so a pass does not prove the
    wait -- a failure would disprove it."""
    from n3dt import synthetic as syn
    from n3dt.perceptual import VGGPerceptualLoss
    sd = syn.vgg16_features_state_dict(10)
    pred, gt = rand((1, 3, 16, 16), 11), rand((1, 3, 16, 16), 12)
    want = vgg_run(VGGPerceptualLoss(sd, precision="fp32"), pred, gt)
    torch.cuda.synchronize()
    f = VGGPerceptualLoss(sd, precision="fp32")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = vgg_run(f, pred, gt)
    on_default = vgg_run(f, pred, gt)
    torch.cuda.synchronize()
    assert float(want[0]) > 0.0 and float(want[1:].abs().max()) > 0.0
    assert torch.equal(on_side, want) and torch.equal(on_default, want)
