"""The host layer the frozen networks' wrappers share: the per-device cache of packed weights, the size
queries' zero-means-error rule, the chunk loop, the strict state-dict mechanics and the input check.  Plain functions and one small
class; every wrapper keeps its own tables, its own policy and its own wording.
"""
import torch

from . import ops
from ._lib import check, lib


class PackedCache(object):
    """What a wrapper keeps on each device, built once per device and again when a watched tensor has been written in place.

    `tensors()` gives the watched (weight) tensors, possibly none; `build(device, on_device)` takes them on the device, contiguous
    and in the same order, enqueues the pack on the current stream and returns (value, temporaries).  `get(device)` is the value:
    built on the stream that is current at first use, or again when the tuple of the tensors' `_version` counters has moved.  The
    temporaries are read by the pack on that stream, so the allocator is told not to hand them out before it has run.  A call on
    another stream waits for the pack's event first (under a graph capture torch has already ordered the capture stream behind
    it).  `clear()` forgets every device."""

    def __init__(self, tensors, build):
        self.tensors, self.build = tensors, build
        self.clear()

    def clear(self):
        self._built = {}

    def get(self, device):
        key = (device.type, device.index)
        stream = torch.cuda.current_stream(device)
        versions = tuple(t._version for t in self.tensors())
        if key not in self._built or self._built[key][3] != versions:
            value, temporaries = self.build(device, [t.to(device).contiguous() for t in self.tensors()])
            for t in temporaries:
                t.record_stream(stream)
            done = torch.cuda.Event()
            done.record(stream)
            self._built[key] = (value, stream.cuda_stream, done, versions)
        value, pack_stream, done, _ = self._built[key]
        if stream.cuda_stream != pack_stream and not torch.cuda.is_current_stream_capturing():
            stream.wait_event(done)
        return value


def pack(entry, nbytes, device, *args):
    """a new uint8 buffer of nbytes on `device`, filled by the library's `entry`(*args, buffer, stream) on the current stream"""
    packed = torch.empty(nbytes, dtype=torch.uint8, device=device)
    check(getattr(lib(), entry)(*args, ops._ptr(packed), ops._stream()), entry)
    return packed


def count_or_raise(n):
    """a size query's answer; 0 is its refusal, worded by the library"""
    if n == 0:
        raise ValueError(lib().n3dt_last_error().decode())
    return n


def workspace(role, nbytes, device):
    """the current stream's scratch buffer of `role`, at least nbytes (a size query's answer) long"""
    return ops.WORKSPACE.get(role, count_or_raise(nbytes), device)


def chunks(n, cap, chunk=None):
    """(first, count) of the calls that cover n items, at most cap -- and at most `chunk`, but at least 1 -- each"""
    if chunk is not None:
        cap = max(1, min(cap, int(chunk)))
    for i in range(0, n, cap):
        yield i, min(cap, n - i)


def open_state_dict(who, obj, unwrap=(), strip_module=False, paths=True, expected=None):
    """The state dict behind `obj`: a path (with `paths`) is loaded onto the CPU, a dict holding a dict under one of the `unwrap`
    names gives that one, `strip_module` drops a leading `module.` from the keys.  Anything else is a TypeError that names what
    `who` expected."""
    if paths and (isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__")):
        obj = torch.load(obj, map_location="cpu")
    if not isinstance(obj, dict):
        raise TypeError("%s: expected %s, got %s" % (who, expected or ("a state dict or a path" if paths else "a state dict"), type(obj).__name__))
    for name in unwrap:
        if name in obj and isinstance(obj[name], dict):
            obj = obj[name]
    if strip_module:
        obj = {(k[len("module."):] if isinstance(k, str) and k.startswith("module.") else k): v for k, v in obj.items()}
    return obj


def only_keys(who, keys, want):
    for key in keys:
        if key not in want:
            raise KeyError("%s: unexpected key %r" % (who, key))


def take(who, sd, key, shapes, alt_keys=()):
    """sd[key] -- or the first of alt_keys the dict holds -- detached, if it is a tensor of one of `shapes` (one shape, or a list
    whose first the refusal names)"""
    name = next((k for k in (key,) + tuple(alt_keys) if k in sd), None)
    if name is None:
        nor = " (nor %s)" % ", ".join(repr(k) for k in alt_keys) if alt_keys else ""
        raise KeyError("%s: the state dict has no key %r%s" % (who, key, nor))
    t = sd[name]
    shapes = [shapes] if isinstance(shapes, tuple) else list(shapes)
    if not torch.is_tensor(t) or tuple(t.shape) not in shapes:
        raise ValueError("%s: %r has shape %s, expected %s" % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, shapes[0]))
    return t.detach()


def gpu_tensor(who, name, x, dtype=None, shape=None, wants=None, empty=None, copy=True):
    """x detached and contiguous, if it is a GPU tensor of `dtype` and `shape` where given (None: any size, the first at least 1).
    `wants` words the refusal, "<who>: <name> must be <wants>, got ..."; with `empty`, a first size of 0 is refused as
    "<who>: <name> <empty>" instead.  copy=False gives x itself: the caller has checks of its own to make before anything is copied."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("%s: %s must be a GPU tensor (there is no CPU path)" % (who, name))
    fits = dtype is None or x.dtype == dtype
    if shape is not None:
        fits = fits and x.dim() == len(shape) and all(s is None or s == d for s, d in zip(shape, x.shape)) and (empty is not None or x.shape[0] >= 1)
    if not fits:
        raise ValueError("%s: %s must be %s, got %s %s" % (who, name, wants or "%s %s" % (dtype, list(shape)), x.dtype, tuple(x.shape)))
    if empty is not None and x.shape[0] < 1:
        raise ValueError("%s: %s %s" % (who, name, empty))
    return x.detach().contiguous() if copy else x


def gpu_images(who, name, x, min_hw):
    """x [n,3,H,W] float32 on the GPU, min_hw <= H, W <= 4096, detached and contiguous"""
    x = gpu_tensor(who, name, x, torch.float32, (None, 3, None, None), "float32 [n,3,H,W]", copy=False)
    if min(x.shape[2:]) < min_hw or max(x.shape[2:]) > 4096:
        raise ValueError("%s: %s must be %d..4096 pixels high and wide, got %d x %d" % (who, name, min_hw, x.shape[2], x.shape[3]))
    return x.detach().contiguous()
