"""Host side of FlatAdam's guarded step (max_grad_norm / skip_nonfinite), no GPU: argument validation, the additions to the C
ABI and their ctypes mirror, the entry point's refusals, and make_flat_optimizer's pass-through."""
import ctypes
import math
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param():
    return torch.nn.Parameter(torch.zeros(8))


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, -math.inf, math.nan, torch.tensor(1.0), "1.0", True])
def test_max_grad_norm_must_be_a_positive_python_number(bad):
    from n3dt import FlatAdam
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatAdam([_param()], max_grad_norm=bad)
    opt = FlatAdam([_param()], max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = bad
    assert opt.max_grad_norm == 1.0


def test_accepted_values_and_defaults():
    from n3dt import FlatAdam
    opt = FlatAdam([_param()])
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and not opt.guarded
    assert FlatAdam([_param()], max_grad_norm=math.inf).guarded
    assert FlatAdam([_param()], max_grad_norm=2).max_grad_norm == 2.0
    assert FlatAdam([_param()], skip_nonfinite=True).guarded
    opt.max_grad_norm = 0.5
    assert opt.guarded
    opt.max_grad_norm = None
    assert not opt.guarded
    # the options are not hyper-parameters of a group: the state dict stays torch.optim.Adam's
    params = [_param()]
    assert FlatAdam(params, max_grad_norm=1.0, skip_nonfinite=True).state_dict() == torch.optim.Adam(params).state_dict()


def test_guard_symbols_are_declared_exported_and_mirrored():
    from n3dt import _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "n3dt.h")).read()
    assert '#include "n3dt_flat_adam_guard.h"' in header
    guard_h = open(os.path.join(REPO, "include", "n3dt_flat_adam_guard.h")).read()
    declared = set(re.findall(r"^(?:size_t|int) (n3dt_[a-z0-9_]+)\(", guard_h, flags=re.M))
    assert declared == {"n3dt_flat_adam_guard_bytes", "n3dt_flat_adam_guarded_step"} == set(_lib.GUARD_EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    assert L.n3dt_abi_version() == 5
    assert L.n3dt_flat_adam_guard_bytes() == ctypes.sizeof(_lib.AdamGuard) == 32
    # field for field against the header's struct
    body = re.search(r"typedef struct N3dtAdamGuard \{(.*?)\} N3dtAdamGuard;", guard_h, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t) ([a-z_]+);", body, flags=re.M)
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.AdamGuard._fields_)
    # what the host may write comes first
    assert _lib.AdamGuard.max_grad_norm.offset == 0 and _lib.AdamGuard.skip_nonfinite.offset == 4 and _lib.GUARD_HOST_BYTES == 8
    # the existing records did not move
    assert [L.n3dt_flat_adam_record_bytes(i) for i in range(3)] == [48, 16, 48]


def test_guarded_entry_point_refuses_what_the_plain_one_refuses():
    from n3dt import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(256)
    ok = [d, d, 1, d, 1, d, d, d, None]
    for i in (0, 1, 3, 5, 6, 7):  # each pointer NULL in turn
        args = list(ok)
        args[i] = None
        assert L.n3dt_flat_adam_guarded_step(*args) == -1, i
        assert b"n3dt_flat_adam_guarded_step" in L.n3dt_last_error() and b"NULL" in L.n3dt_last_error()
    for n_chunks in (0, -3):
        args = list(ok)
        args[2] = n_chunks
        assert L.n3dt_flat_adam_guarded_step(*args) == -1 and b"n_chunks" in L.n3dt_last_error()
    for n_groups in (0, _lib.ADAM_MAX_GROUPS + 1):
        args = list(ok)
        args[4] = n_groups
        assert L.n3dt_flat_adam_guarded_step(*args) == -1 and b"n_groups" in L.n3dt_last_error()
    for i, off in ((0, 4), (1, 4), (3, 4), (5, 2), (6, 4), (7, 2)):  # misaligned tables / counter / partials / guard
        args = list(ok)
        args[i] = ctypes.c_void_p(256 + off)
        assert L.n3dt_flat_adam_guarded_step(*args) == -1 and b"aligned" in L.n3dt_last_error(), i


def test_make_flat_optimizer_forwards_the_options():
    from n3dt import FlatAdam
    from n3dt.train import make_flat_optimizer
    net = torch.nn.Linear(3, 2)
    opt, sched = make_flat_optimizer(net, lr=3e-4, max_grad_norm=0.25, skip_nonfinite=True)
    assert isinstance(opt, FlatAdam) and opt.max_grad_norm == 0.25 and opt.skip_nonfinite is True
    assert opt.param_groups[0]["lr"] == 3e-4 and opt.modules == [net] and sched.optimizer is opt
    opt, _ = make_flat_optimizer(net)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and not opt.guarded
    with pytest.raises(ValueError, match="max_grad_norm"):
        make_flat_optimizer(net, max_grad_norm=-1.0)
