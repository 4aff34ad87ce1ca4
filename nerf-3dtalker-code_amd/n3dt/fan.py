"""The AWing FAN landmark detector on libn3dt: frames to 68 landmarks (the reference's KeypointExtractor network --
s_face3d/util/my_awing_arch.py, FAN over HourGlass / ConvBlock / CoordConvTh with calculate_points behind it, as
s_face3d/extract_kp_videos_safe.py runs it), frozen and inference-only (n3dt_fan_*, csrc/fan.hip).

`FAN` takes the CALLER'S weights under the keys of the reference's class.  The pretrained alignment_WFLW_4HG.pth has never been run
through this code; facexlib's landmark_98_to_68 (the default table below is written from memory of it), RetinaFace's boxes (the box
stays the caller's: S3FD.boxes gives one), cv2.resize's byte arithmetic and Preprocesser.crop are parity unpinned.  There is no CPU
path, no training mode and no gradient.
"""
import ctypes

import torch

from . import ops
from ._host import PackedCache, chunks, count_or_raise, gpu_tensor, only_keys, open_state_dict, pack, take, workspace
from ._lib import FAN_MAX_CONVS, FanParams, check, lib

IMG = 256
HEAT = 64
CELLS = HEAT * HEAT
FRONT_CONVS, STACK_CONVS = 12, 47
FRONT_BLOCKS, STACK_BLOCKS = 6, 19
POOL_BLOCK, UPADD_BLOCK = 4, 5
BN_PARTS = ("weight", "bias", "running_mean", "running_var")
HG_BLOCKS = ("b1_4", "b2_4", "b1_3", "b2_3", "b1_2", "b2_2", "b1_1", "b2_1", "b2_plus_1", "b3_1", "b3_2", "b3_3", "b3_4")  # state-dict order
GATE_LEVEL = 0.05


def _map_98_to_68():
    """68 rows of two source indices whose mean is taken -- facexlib's landmark_98_to_68 as remembered, NOT pinned against it"""
    rows = [(i, i) for i in range(0, 33, 2)]                                        # 0-16: the jaw, every second point
    rows += [(33, 33), (34, 41), (35, 40), (36, 39), (37, 38)]                      # 17-21: left eyebrow
    rows += [(42, 50), (43, 49), (44, 48), (45, 47), (46, 46)]                      # 22-26: right eyebrow
    rows += [(i, i) for i in range(51, 60)]                                         # 27-35: nose
    rows += [(i, i) for i in (60, 61, 63, 64, 65, 67)]                              # 36-41: left eye
    rows += [(i, i) for i in (68, 69, 71, 72, 73, 75)]                              # 42-47: right eye
    rows += [(i, i) for i in range(76, 96)]                                         # 48-67: mouth
    return tuple(rows)


MAP_98_TO_68 = _map_98_to_68()


def conv_table(num_modules, num_landmarks):
    """[(conv name, bn name or None, C_in of the K loop, C_out, kernel, has bias, weight's channel count)] indexed as
    csrc/fan_core.h's fan_conv; None where the last stack has no bl / al"""
    N = num_landmarks

    def cb(name, cin, cout):
        rows = [(name + ".conv1", name + ".bn1", cin, cout // 2, 3, False, cin), (name + ".conv2", name + ".bn2", cout // 2, cout // 4, 3, False, cout // 2),
                (name + ".conv3", name + ".bn3", cout // 4, cout // 4, 3, False, cout // 4)]
        if cin != cout:
            rows.append((name + ".downsample.2", name + ".downsample.0", cin, cout, 1, False, cin))
        return rows

    t = [("conv1.conv", "bn1", 3, 64, 7, True, 6)] + cb("conv2", 64, 128) + cb("conv3", 128, 128) + cb("conv4", 128, 256)
    for s in range(num_modules):
        t.append(("m%d.coordconv.conv" % s, None, 256, 256, 1, True, 259 if s == 0 else 261))
        for b in HG_BLOCKS:
            t += cb("m%d.%s" % (s, b), 256, 256)
        t += cb("top_m_%d" % s, 256, 256)
        t.append(("conv_last%d" % s, "bn_end%d" % s, 256, 256, 1, True, 256))
        t.append(("l%d" % s, None, 256, N + 1, 1, True, 256))
        if s < num_modules - 1:
            t += [("bl%d" % s, None, 256, 256, 1, True, 256), ("al%d" % s, None, N + 1, 256, 1, True, N + 1)]
        else:
            t += [None, None]
    return t


def state_dict_keys(num_modules=4, num_landmarks=98):
    """{key: shape} of every tensor of the reference's FAN(num_modules, num_landmarks=...), in its state-dict order"""
    keys = {}
    N = num_landmarks

    def conv(name, cout, cin, k, bias):
        keys[name + ".weight"] = (cout, cin, k, k)
        if bias:
            keys[name + ".bias"] = (cout,)

    def bn(name, c):
        for part in BN_PARTS:
            keys["%s.%s" % (name, part)] = (c,)
        keys[name + ".num_batches_tracked"] = ()

    def cb(name, cin, cout):
        bn(name + ".bn1", cin)
        conv(name + ".conv1", cout // 2, cin, 3, False)
        bn(name + ".bn2", cout // 2)
        conv(name + ".conv2", cout // 4, cout // 2, 3, False)
        bn(name + ".bn3", cout // 4)
        conv(name + ".conv3", cout // 4, cout // 4, 3, False)
        if cin != cout:
            bn(name + ".downsample.0", cin)
            conv(name + ".downsample.2", cout, cin, 1, False)

    conv("conv1.conv", 64, 6, 7, True)
    bn("bn1", 64)
    cb("conv2", 64, 128)
    cb("conv3", 128, 128)
    cb("conv4", 128, 256)
    for s in range(num_modules):
        conv("m%d.coordconv.conv" % s, 256, 259 if s == 0 else 261, 1, True)
        for b in HG_BLOCKS:
            cb("m%d.%s" % (s, b), 256, 256)
        cb("top_m_%d" % s, 256, 256)
        conv("conv_last%d" % s, 256, 256, 1, True)
        bn("bn_end%d" % s, 256)
        conv("l%d" % s, N + 1, 256, 1, True)
        if s < num_modules - 1:
            conv("bl%d" % s, 256, 256, 1, True)
            conv("al%d" % s, 256, N + 1, 1, True)
    return keys


def block_names(num_modules=4):
    """the blocks of `FAN.block` in its order"""
    names = ["conv1", "conv2", "conv3", "conv4", "avg_pool", "upsample_add"]
    for s in range(num_modules):
        names += ["m%d.coordconv" % s] + ["m%d.%s" % (s, b) for b in HG_BLOCKS] + ["top_m_%d" % s, "conv_last%d" % s, "l%d" % s]
        if s < num_modules - 1:
            names += ["bl%d" % s, "al%d" % s]
    return names


def block_index(name, num_modules=4):
    """the library's block number of a name of block_names() (the numbering leaves room for the bl / al a last stack lacks)"""
    front = ["conv1", "conv2", "conv3", "conv4", "avg_pool", "upsample_add"]
    if name in front:
        return front.index(name)
    for s in range(num_modules):
        per = ["m%d.coordconv" % s] + ["m%d.%s" % (s, b) for b in HG_BLOCKS] + ["top_m_%d" % s, "conv_last%d" % s, "l%d" % s, "bl%d" % s, "al%d" % s]
        if name in per:
            return FRONT_BLOCKS + s * STACK_BLOCKS + per.index(name)
    raise ValueError("FAN: no block %r" % (name,))


def block_shape(b, num_landmarks, Hi, Wi):
    """(C_in, C_out, Ho, Wo, takes a skip) of library block b on an Hi x Wi input"""
    N = num_landmarks
    if b == 0:
        return 3, 64, Hi // 2, Wi // 2, False
    if b in (1, 2, 3):
        cin, cout = ((64, 128), (128, 128), (128, 256))[b - 1]
        return cin, cout, Hi, Wi, False
    if b == POOL_BLOCK:
        return 256, 256, Hi // 2, Wi // 2, False
    if b == UPADD_BLOCK:
        return 256, 256, Hi * 2, Wi * 2, True
    t = (b - FRONT_BLOCKS) % STACK_BLOCKS
    if t == 16:
        return 256, N + 1, Hi, Wi, False
    if t == 18:
        return N + 1, 256, Hi, Wi, True
    return 256, 256, Hi, Wi, t == 17


def coords(dim):
    """the xx, yy, rr channels [3, dim, dim] as AddCoordsTh computes them, in fp32: xx the ROW coordinate, yy the column's"""
    r = torch.arange(dim, dtype=torch.int32).float() / (dim - 1)
    r = r * 2 - 1
    xx = r[:, None].expand(dim, dim).contiguous()
    yy = r[None, :].expand(dim, dim).contiguous()
    rr = torch.sqrt(torch.pow(xx, 2) + torch.pow(yy, 2))
    rr = rr / torch.max(rr)
    return torch.stack((xx, yy, rr))


def load_fan(obj, num_modules=4, num_landmarks=98):
    """{key: float32 tensor} from a state dict with the reference's keys, a dict holding one under 'state_dict', or the path of such
    a file (loaded onto the CPU).  Strict: a missing key, a key the network does not have and a wrongly shaped tensor are refused
    with the key; num_batches_tracked is accepted (also absent) and ignored."""
    obj = open_state_dict("load_fan", obj, unwrap=("state_dict",))
    want = state_dict_keys(num_modules, num_landmarks)
    only_keys("load_fan", obj, want)
    # a float32 tensor stays the caller's: its version counter is watched
    return {key: take("load_fan", obj, key, shape).float() for key, shape in want.items() if not key.endswith("num_batches_tracked")}


class FAN(object):
    """The reference's FAN(num_modules, num_landmarks=...) on libn3dt, with caller-supplied weights (see load_fan).

    `net.forward(x)` is `FAN.forward`'s first result: [n,3,256,256] BGR in [0,1] -> the list of every stack's heat maps
    [n,N+1,64,64]; the boundary gates it used stay in `net.last_gates` (uint8 [n,num_modules-1,64,64]), and `gates=` supplies them
    instead.  `net.points(heatmaps)` is calculate_points per frame; `net.landmarks(frames, boxes)` the chain of
    KeypointExtractor.extract_keypoint behind the caller's face box.  Runs without gradients, stream-ordered, without a host
    synchronisation, bitwise reproducible; a frame's result depends neither on its position in the batch nor on how a clip is
    split into calls (the carry-forward apart, which is sequential by definition)."""

    def __init__(self, weights, num_modules=4, num_landmarks=98, end_relu=False, map98to68=None):
        if not isinstance(num_modules, int) or not 1 <= num_modules <= 4:
            raise ValueError("FAN: num_modules must be 1..4, got %r" % (num_modules,))
        if not isinstance(num_landmarks, int) or not 1 <= num_landmarks <= 127:
            raise ValueError("FAN: num_landmarks must be 1..127, got %r" % (num_landmarks,))
        self.num_modules, self.num_landmarks, self.end_relu = num_modules, num_landmarks, bool(end_relu)
        self.weights = load_fan(weights, num_modules, num_landmarks)
        self.table = conv_table(num_modules, num_landmarks)
        if map98to68 is None:
            map98to68 = MAP_98_TO_68 if num_landmarks == 98 else None
        if map98to68 is not None:
            m = torch.as_tensor(map98to68, dtype=torch.int32)
            if m.dim() != 2 or m.shape[1] != 2 or not 1 <= m.shape[0] <= 1024 or int(m.min()) < 0 or int(m.max()) >= num_landmarks:
                raise ValueError("FAN: map98to68 must be [P,2] source indices below num_landmarks")
            map98to68 = m.contiguous()
        self.map98to68 = map98to68
        self._packed = PackedCache(lambda: list(self.weights.values()), self._pack)
        self._maps = {}
        self.last_gates = None

    def repack(self):
        self._packed.clear()

    def block_names(self):
        """the names `block` takes, in the chain's order"""
        return block_names(self.num_modules)

    def _pack(self, device, tensors):
        dev = dict(zip(self.weights, tensors))
        c256, c64 = coords(IMG).to(device), coords(HEAT).to(device)
        p = FanParams()
        p.num_modules, p.num_landmarks = self.num_modules, self.num_landmarks
        p.coords256, p.coords64 = c256.data_ptr(), c64.data_ptr()
        for j, row in enumerate(self.table):
            if row is None:
                continue
            conv, bn, _, _, _, bias, _ = row
            p.weight[j] = dev[conv + ".weight"].data_ptr()
            if bias:
                p.bias[j] = dev[conv + ".bias"].data_ptr()
            if bn is not None:
                p.bn_weight[j], p.bn_bias[j], p.bn_mean[j], p.bn_var[j] = (dev["%s.%s" % (bn, part)].data_ptr() for part in BN_PARTS)
        nbytes = lib().n3dt_fan_packed_bytes(self.num_modules, self.num_landmarks)
        return pack("n3dt_fan_pack", nbytes, device, ctypes.byref(p)), tensors + [c256, c64]

    def _packed_for(self, device):
        return self._packed.get(device)

    def max_images(self):
        """images one call takes: the library's workspace budget"""
        return count_or_raise(lib().n3dt_fan_max_images(self.num_modules, self.num_landmarks))

    @torch.no_grad()
    def forward(self, x, gates=None, chunk=None):
        """x [n,3,256,256] float32 BGR in [0,1] -> [heat maps [n,N+1,64,64]] * num_modules.  gates: uint8 [n,num_modules-1,64,64]
        taken instead of the device's own; either way `last_gates` holds what was used.  `chunk` caps the images per call
        (default: the workspace budget); results do not depend on it."""
        x = gpu_tensor("FAN.forward", "x", x, torch.float32, (None, 3, IMG, IMG))
        n, dev, M, N = x.shape[0], x.device, self.num_modules, self.num_landmarks
        slots = max(M - 1, 1)
        if gates is not None:
            used = gpu_tensor("FAN.forward", "gates", gates, torch.uint8, (n, M - 1, HEAT, HEAT)).clone() if M > 1 else None
        else:
            used = torch.empty(n, M - 1, HEAT, HEAT, dtype=torch.uint8, device=dev) if M > 1 else None
        packed = self._packed_for(dev)
        calls = list(chunks(n, self.max_images(), chunk))
        heat = None if len(calls) == 1 else [torch.empty(n, N + 1, HEAT, HEAT, dtype=torch.float32, device=dev) for _ in range(M)]
        for i, m in calls:
            ws = workspace("fan", lib().n3dt_fan_workspace_bytes(M, N, m), dev)
            g = used[i:i + m] if used is not None else torch.empty(m, slots, CELLS, dtype=torch.uint8, device=dev)
            out = torch.empty(M, m, N + 1, HEAT, HEAT, dtype=torch.float32, device=dev)
            check(lib().n3dt_fan_fwd(M, N, int(self.end_relu), m, ops._ptr(packed), ops._ptr(x[i:]), int(gates is None), ops._ptr(g), ops._ptr(out),
                                     ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_fan_fwd")
            if heat is None:
                heat = list(out.unbind(0))
            else:
                for s in range(M):
                    heat[s][i:i + m].copy_(out[s])
        self.last_gates = used
        return heat

    __call__ = forward

    @torch.no_grad()
    def points(self, heatmaps):
        """calculate_points per frame (as get_landmarks calls it: B = 1): heatmaps [n,N,64,64] float32 -> (points [n,N,2] float64
        (x, y) in heat-map cells, status [n] int32: 2 where a landmark's argmax is cell 4095 -- the reference raises IndexError
        there -- and the frame's points are all -1).  A view [:, :N] of a [n,N+1,64,64] tensor is taken as it is."""
        h = heatmaps
        gpu_tensor("FAN.points", "heatmaps", h, copy=False)
        if h.dtype != torch.float32 or h.dim() != 4 or h.shape[0] < 1 or not 1 <= h.shape[1] <= 127 or tuple(h.shape[2:]) != (HEAT, HEAT):
            raise ValueError("FAN.points: heatmaps must be float32 [n,N,64,64] with N in 1..127, got %s %s" % (h.dtype, tuple(h.shape)))
        h = h.detach()
        if h.stride()[1:] != (CELLS, HEAT, 1) or h.stride(0) < h.shape[1] * CELLS:
            h = h.contiguous()
        n, N = h.shape[:2]
        pts = torch.empty(n, N, 2, dtype=torch.float64, device=h.device)
        status = torch.empty(n, dtype=torch.int32, device=h.device)
        check(lib().n3dt_fan_points(n, N, ops._ptr(h), h.stride(0) if n > 1 else N * CELLS, ops._ptr(pts), ops._ptr(status), ops._stream()), "n3dt_fan_points")
        return pts, status

    @torch.no_grad()
    def crops(self, frames, boxes=None):
        """frames [F,3,H,W] float32 RGB; boxes int32 [F,4] = (y1, y2, x1, x2), None: the whole frame -> ([F,3,256,256] BGR, the
        boxes used): each box resampled bilinearly with half-pixel centres; a bad box gives zeros"""
        frames = gpu_tensor("FAN.crops", "frames", frames, torch.float32, (None, 3, None, None))
        F, _, H, W = frames.shape
        if not 1 <= H <= 4096 or not 1 <= W <= 4096:
            raise ValueError("FAN.crops: frames must be 1..4096 pixels high and wide")
        if boxes is None:
            boxes = torch.tensor([0, H, 0, W], dtype=torch.int32, device=frames.device).repeat(F, 1)
        boxes = gpu_tensor("FAN.crops", "boxes", boxes, torch.int32, (F, 4))
        out = torch.empty(F, 3, IMG, IMG, dtype=torch.float32, device=frames.device)
        check(lib().n3dt_fan_crops(F, H, W, ops._ptr(frames), ops._ptr(boxes), ops._ptr(out), ops._stream()), "n3dt_fan_crops")
        return out, boxes

    @torch.no_grad()
    def tail(self, pts, decode_status, boxes, H, W, convert=True, carry=True):
        """points in heat-map cells -> image pixels: times the box's (w / 64, h / 64), 98 -> 68 through the table (rounded to fp32
        as facexlib's float32 array does, the box's integer origin added in fp32; convert=False: float64 throughout), a failed
        frame -1, the carry-forward -> ([F,P,2] float64, status [F] int32: decode's 2 | 4 for a bad box)"""
        pts = gpu_tensor("FAN.tail", "pts", pts, torch.float64, (None, self.num_landmarks, 2))
        F, dev = pts.shape[0], pts.device
        decode_status = gpu_tensor("FAN.tail", "decode_status", decode_status, torch.int32, (F,))
        boxes = gpu_tensor("FAN.tail", "boxes", boxes, torch.int32, (F, 4))
        table = None
        if convert:
            if self.map98to68 is None:
                raise ValueError("FAN.tail: convert=True needs a map98to68 (the default exists for 98 landmarks only)")
            key = (dev.type, dev.index)
            if key not in self._maps:
                self._maps[key] = self.map98to68.to(dev)
            table = self._maps[key]
        P = table.shape[0] if table is not None else self.num_landmarks
        out = torch.empty(F, P, 2, dtype=torch.float64, device=dev)
        status = torch.empty(F, dtype=torch.int32, device=dev)
        check(lib().n3dt_fan_tail(F, self.num_landmarks, P, int(H), int(W), ops._ptr(pts), ops._ptr(decode_status), ops._ptr(boxes), ops._ptr(table),
                                  int(bool(carry)), ops._ptr(out), ops._ptr(status), ops._stream()), "n3dt_fan_tail")
        return out, status

    def landmarks(self, frames, boxes=None, convert=True, carry=True, chunk=None):
        """frames [F,3,H,W] float32 RGB in [0,1] on the GPU; boxes int32 [F,4] = (y1, y2, x1, x2) as S3FD.boxes gives them, None:
        the whole frame -> (landmarks [F,68,2] float64 image pixels (x, y) -- [F,N,2] with convert=False -- and status [F] int32).
        A frame with a bad box (4) or the reference's IndexError case (2) is -1, the reference's no-face value, and with carry=True
        takes the points of the last good frame before it.  The heat maps of the last stack stay in `last_heatmaps`."""
        crops, boxes = self.crops(frames, boxes)
        heat = self.forward(crops, chunk=chunk)[-1]
        self.last_heatmaps = heat
        pts, st = self.points(heat[:, :self.num_landmarks])
        return self.tail(pts, st, boxes, frames.shape[2], frames.shape[3], convert, carry)

    @torch.no_grad()
    def block(self, b, x, skip=None, gates=None):
        """block b (a name of block_names(num_modules)) alone on x [n,C_in,Hi,Wi] -> [n,C_out,Ho,Wo].  A ConvBlock, conv_last, l
        take any size; conv1 256 x 256 and a coordconv 64 x 64 only (from the second stack on with gates uint8 [n,64,64]); avg_pool
        even sizes; upsample_add takes the lower map as x and the upper, twice as large, as skip; bl and al take what is added to
        them as skip"""
        who = "FAN.block"
        idx = block_index(b, self.num_modules) if isinstance(b, str) else b
        if not isinstance(idx, int) or b not in block_names(self.num_modules):
            raise ValueError("%s: block must be one of block_names(%d), got %r" % (who, self.num_modules, b))
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            raise ValueError("%s: x must be a float32 GPU tensor [n,C,H,W]" % who)
        n, C, Hi, Wi = x.shape
        cin, cout, Ho, Wo, takes_skip = block_shape(idx, self.num_landmarks, Hi, Wi)
        if C != cin or n < 1 or Ho < 1 or Wo < 1:
            raise ValueError("%s: block %s takes [n,%d,H,W] with a non-empty output, got %s" % (who, b, cin, tuple(x.shape)))
        if takes_skip != (skip is not None):
            raise ValueError("%s: upsample_add, bl and al, and no other block, take a skip" % who)
        if skip is not None:
            skip = gpu_tensor(who, "skip", skip, torch.float32, (n, cout, Ho, Wo))
        if gates is not None:
            gates = gpu_tensor(who, "gates", gates, torch.uint8, (n, HEAT, HEAT))
        x = x.detach().contiguous()
        packed = self._packed_for(x.device)
        M, N = self.num_modules, self.num_landmarks
        ws = workspace("fan_block", lib().n3dt_fan_block_workspace_bytes(idx, M, N, n, Hi, Wi), x.device)
        out = torch.empty(n, cout, Ho, Wo, dtype=torch.float32, device=x.device)
        check(lib().n3dt_fan_block(idx, M, N, int(self.end_relu), n, Hi, Wi, ops._ptr(packed), ops._ptr(x), ops._ptr(skip), ops._ptr(gates), ops._ptr(out),
                                   ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream()), "n3dt_fan_block")
        return out
