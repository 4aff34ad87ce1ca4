"""Host side of n3dt.FlatAdam, no GPU: the new exports, the chunk / arena layout as a pure function of sizes, the state-dict
conversion to and from torch.optim.Adam's form, and the documented refusals."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1,), (3,), (63,), (64,), (65,), (4096,), (4097,), ()]  # numels 1, 3, 63, 64, 65, 4096, 4097 and a 0-dim scalar


def test_new_symbols_are_declared_and_exported():
    from n3dt import _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "n3dt.h")).read()
    declared = set(re.findall(r"\b(n3dt_flat_adam_[a-z0-9_]+)\s*\(", header))
    assert declared == {"n3dt_flat_adam_step", "n3dt_flat_adam_record_bytes"}
    for name in declared:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.n3dt_abi_version() == 5
    # the table records the Python side writes are the ones the library reads
    assert [L.n3dt_flat_adam_record_bytes(i) for i in range(4)] == [ctypes.sizeof(_lib.AdamTensor), ctypes.sizeof(_lib.AdamChunk),
                                                                     ctypes.sizeof(_lib.AdamGroup), 0]


def test_entry_point_refuses_null_tables_and_empty_work_lists():
    """Validation is host code and runs before anything is enqueued."""
    from n3dt import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(256)
    assert L.n3dt_flat_adam_step(None, d, 1, d, 1, d, None) == -1 and b"NULL" in L.n3dt_last_error()
    assert L.n3dt_flat_adam_step(d, None, 1, d, 1, d, None) == -1
    assert L.n3dt_flat_adam_step(d, d, 1, None, 1, d, None) == -1
    assert L.n3dt_flat_adam_step(d, d, 1, d, 1, None, None) == -1
    assert L.n3dt_flat_adam_step(d, d, 0, d, 1, d, None) == -1 and b"n_chunks" in L.n3dt_last_error()
    assert L.n3dt_flat_adam_step(d, d, -3, d, 1, d, None) == -1
    assert L.n3dt_flat_adam_step(d, d, 1, d, 0, d, None) == -1 and b"n_groups" in L.n3dt_last_error()
    assert L.n3dt_flat_adam_step(d, d, 1, d, _lib.ADAM_MAX_GROUPS + 1, d, None) == -1


def test_chunks_tile_every_tensor_once_and_offsets_follow_the_gradient_arena():
    from n3dt import optim, parallel
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    numels = [p.numel() for p in params]
    assert numels == [1, 3, 63, 64, 65, 4096, 4097, 1]
    arena = parallel.FlatGrads(params)
    offsets, total = optim.arena_offsets(numels)
    assert offsets == arena.offsets and total == arena.flat.numel()
    assert all(o % 64 == 0 for o in offsets)  # 256-byte slices
    chunks = optim.build_chunks(numels)
    covered = [torch.zeros(n, dtype=torch.int32) for n in numels]
    for t, start, length in chunks:
        assert 0 <= t < len(numels) and length >= 1 and length <= optim.CHUNK
        assert 0 <= start and start + length <= numels[t], "a chunk crosses its tensor"
        covered[t][start:start + length] += 1
    for c in covered:
        assert bool((c == 1).all())
    assert [t for t, _, _ in chunks] == sorted(t for t, _, _ in chunks)
    assert sum(1 for t, _, _ in chunks if t == 6) == 2 and sum(1 for t, _, _ in chunks if t == 5) == 1  # 4097 -> 4096 + 1
    assert optim.build_chunks([0, 5]) == [(1, 0, 5)]


def _adam_state_dict(steps=3):
    gen = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in SHAPES[:5]]
    opt = torch.optim.Adam([{"params": params[:2]}, {"params": params[2:], "lr": 1e-7, "betas": (0.5, 0.999), "weight_decay": 1e-2}], lr=1e-4)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return params, opt


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_state_dict_conversion_round_trip_is_the_identity():
    from n3dt import optim
    _, opt = _adam_state_dict()
    sd = opt.state_dict()
    unified = optim.unify_state(sd)
    assert unified["step"] == 3 and sorted(unified["state"]) == [0, 1, 2, 3, 4]
    assert all(set(v) == {"exp_avg", "exp_avg_sq"} for v in unified["state"].values())
    back = optim.torch_state(unified)
    assert _same(back, sd)
    # `step` as a Python number or a float64 tensor reads the same
    sd2 = {"state": {k: dict(v, step=3 if k % 2 else torch.tensor(3.0, dtype=torch.float64)) for k, v in sd["state"].items()},
           "param_groups": sd["param_groups"]}
    assert optim.unify_state(sd2)["step"] == 3
    # and torch.optim.Adam takes the converted dict back
    params, _ = _adam_state_dict(0)
    fresh = torch.optim.Adam([{"params": params[:2]}, {"params": params[2:]}])
    fresh.load_state_dict(back)
    assert _same(fresh.state_dict(), sd)


def test_differing_per_parameter_steps_raise():
    from n3dt import optim
    _, opt = _adam_state_dict()
    sd = opt.state_dict()
    sd["state"][1]["step"] = torch.tensor(4.0)
    with pytest.raises(ValueError, match="share one step counter"):
        optim.unify_state(sd)


def test_param_groups_match_torch_adam_before_any_step():
    from n3dt import FlatAdam
    params, opt = _adam_state_dict(0)
    flat = FlatAdam([{"params": params[:2]}, {"params": params[2:], "lr": 1e-7, "betas": (0.5, 0.999), "weight_decay": 1e-2}], lr=1e-4)
    assert _same(flat.state_dict(), opt.state_dict())  # no state yet, identical groups


def test_documented_refusals():
    from n3dt import FlatAdam
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="amsgrad"):
        FlatAdam([p], amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        FlatAdam([{"params": [p], "amsgrad": True}])
    with pytest.raises(ValueError, match="float32"):
        FlatAdam([torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))])
    opt = FlatAdam([p], lr=1e-3)  # a CPU parameter: refused when the step would have to run (there is no CPU path)
    p.grad = torch.ones(8)
    with pytest.raises(ValueError, match="GPU"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(8))
    with pytest.raises(ValueError, match="GPU"):
        opt.load_state_dict(torch.optim.Adam([p]).state_dict())
