"""On-device training augmentation: the reference's VOCDatasetv2(train=True) + ToTensor() (src/dataloader.py:68-75,
148-178, 224-275) as host parameter draws plus ONE HIP call per batch (mcamd_augment, csrc/augment.hip).

Per image the reference crops with a +-jitter box (outside the source reads black), resizes the crop to the network
input with PIL's default bicubic filter, flips left-right at random, distorts hue / saturation / exposure through PIL's
HSV conversion and three 256-entry point LUTs, and moves the boxes with it.  Here the host only draws the parameters
(same `random` calls in the same order), builds Pillow's fixed-point resampling tables and the three LUTs exactly as
Pillow does, and packs them with the raw uint8 sources into one buffer; the device does the pixels.  The result is
bit-equal to `ToTensor()(data_augmentation(...)[0])`.

  draw_params / transform_labels   -- the reference's random draws and fill_truth_detection, in float64
  resample_table / point_luts      -- Pillow's bicubic coefficient tables and Image.point's LUTs
  pack_batch / collate             -- one uint8 buffer: descriptors | tables | LUTs | sources (runs in loader workers)
  pack_resident                    -- the same batch for sources that already live on the device (data.ResidentImages):
                                      descriptors | (dhue, dsat, dexp), the tables and LUTs built by mcamd_augment_tables
  DeviceAugmenter                  -- one H2D copy and one mcamd_augment call on the current stream -> (x, target)
"""
import ctypes as C
import functools
import math
import random
from collections import namedtuple

import numpy as np
import torch

from . import _lib

MAX_BOXES = 50
PRECISION_BITS = 22          # Pillow's Resample.c, 8-bit path: 32 - 8 - 2
JITTER, HUE, SATURATION, EXPOSURE = 0.2, 0.1, 1.5, 1.5   # dataloader.py:69-72

AugParams = namedtuple("AugParams", "pleft pright ptop pbot swidth sheight flip dx dy sx sy dhue dsat dexp")


def _rand_scale(rng, s):
    scale = rng.uniform(1, s)
    if rng.randint(1, 10000) % 2:
        return scale
    return 1. / scale


def draw_params(rng, ow, oh, jitter=JITTER, hue=HUE, saturation=SATURATION, exposure=EXPOSURE):
    """data_augmentation's random draws (dataloader.py:148-178) from `rng`, in the reference's call order."""
    dw = int(ow * jitter)
    dh = int(oh * jitter)
    pleft = rng.randint(-dw, dw)
    pright = rng.randint(-dw, dw)
    ptop = rng.randint(-dh, dh)
    pbot = rng.randint(-dh, dh)
    swidth = ow - pleft - pright
    sheight = oh - ptop - pbot
    sx = float(swidth) / ow
    sy = float(sheight) / oh
    flip = rng.randint(1, 10000) % 2
    dx = (float(pleft) / ow) / sx
    dy = (float(ptop) / oh) / sy
    dhue = rng.uniform(-hue, hue)
    dsat = _rand_scale(rng, saturation)
    dexp = _rand_scale(rng, exposure)
    return AugParams(pleft, pright, ptop, pbot, swidth, sheight, flip, dx, dy, sx, sy, dhue, dsat, dexp)


def resize_params(ow, oh):
    """The identity geometry: the whole ow x oh picture, no flip (with distort=False: Image.resize + ToTensor())."""
    return AugParams(0, -1, 0, -1, ow + 1, oh + 1, 0, 0., 0., 1., 1., 0., 1., 1.)


def sample_rng(seed, epoch, index):
    """The per-sample generator: a function of (seed, epoch, index) only, never of the worker or the rank."""
    return random.Random("augment:%d:%d:%d" % (seed, epoch, index))


def transform_labels(boxes, p):
    """fill_truth_detection (dataloader.py:224-266) as getData calls it (1./sx, 1./sy: line 274) -> float32 [250]."""
    label = np.zeros((MAX_BOXES, 5))
    if boxes is not None and np.size(boxes):
        bs = np.array(boxes, dtype=np.float64).reshape(-1, 5)
        sx, sy, dx, dy = 1. / p.sx, 1. / p.sy, p.dx, p.dy
        cc = 0
        for i in range(bs.shape[0]):
            c, x, y, w, h = (float(v) for v in bs[i])
            x1, y1 = x - w / 2, y - h / 2
            x2, y2 = x + w / 2, y + h / 2
            x1 = min(0.999, max(0, x1 * sx - dx))
            y1 = min(0.999, max(0, y1 * sy - dy))
            x2 = min(0.999, max(0, x2 * sx - dx))
            y2 = min(0.999, max(0, y2 * sy - dy))
            x, y, w, h = (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1
            if p.flip:
                x = 0.999 - x
            if w < 0.001 or h < 0.001:
                continue
            label[cc] = (c, x, y, w, h)
            cc += 1
            if cc >= MAX_BOXES:
                break
    return torch.from_numpy(label.reshape(-1)).float()


def _bicubic(x):
    """Pillow's bicubic_filter (a = -0.5), elementwise in float64 with the same operation order."""
    x = np.abs(x)
    near = ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * -0.5
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=4096)
def resample_table(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter over the whole input
    (Image.resize without a box) -> (ksize, int32 [out_size][ksize + 2]: first tap, tap count, ksize coefficients).
    A pass Pillow skips (same size) gets the identity table, which gives the same bytes."""
    if in_size == out_size:
        t = np.zeros((out_size, 3), np.int32)
        t[:, 0] = np.arange(out_size)
        t[:, 1] = 1
        t[:, 2] = 1 << PRECISION_BITS
        return 1, t
    scale = float(np.float32(in_size)) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = 0.0 + (np.arange(out_size) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(ksize)
    w = _bicubic((((taps[None, :] + xmin[:, None]).astype(np.float64) - center[:, None]) + 0.5) * ss)
    w = np.where(taps[None, :] < xmax[:, None], w, 0.0)
    ww = np.zeros(out_size)
    for t in range(ksize):                 # Pillow sums in tap order
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, np.trunc(-0.5 + w * (1 << PRECISION_BITS)), np.trunc(0.5 + w * (1 << PRECISION_BITS)))
    t = np.empty((out_size, ksize + 2), np.int32)
    t[:, 0], t[:, 1], t[:, 2:] = xmin, xmax, k
    return ksize, t


def table_taps(n_in, n_out):
    """The ksize of resample_table(n_in, n_out) from the two sizes alone."""
    if n_in == n_out:
        return 1
    return int(math.ceil(2 * max(float(np.float32(n_in)) / n_out, 1))) * 2 + 1


def point_luts(dhue, dsat, dexp):
    """The H, S, V tables Image.point builds from distort_image's functions (dataloader.py:114-131): the function at
    0..255, Python's round (half to even), a clip to 0..255.  Hue wraps at 255 (change_hue), not 256."""
    i = np.arange(256, dtype=np.float64)
    h = i + dhue * 255
    h = np.where(h > 255, h - 255, h)
    h = np.where(h < 0, h + 255, h)
    luts = np.stack([h, i * dsat, i * dexp])
    return np.clip(np.round(luts), 0, 255).astype(np.uint8)


def _align(n, a=256):
    return (n + a - 1) // a * a


class PackedBatch:
    """One uint8 buffer: [B descriptors | int32 tables | uint8 LUTs | uint8 sources], 256-byte aligned sections, plus
    the float32 targets.  Built on the host (in loader workers when it comes from `collate`); DataLoader(pin_memory=True)
    pins it through pin_memory().
    A batch of pack_resident has no source section (src_off is an offset into the resident buffer of `resident_bytes`
    bytes); with `hsv_at` set it has no tables or LUTs either: coef_at and lut_at are then offsets into a device
    workspace of `lut_at + lut_bytes` bytes that mcamd_augment_tables fills from the float64 [B][3] section at hsv_at."""
    resident_bytes = hsv_at = None

    def __init__(self, buf, B, shape, coef_at, coef_elems, lut_at, src_at, tmp_bytes, target):
        self.buf, self.B, self.shape, self.target = buf, B, shape, target
        self.coef_at, self.coef_elems, self.lut_at, self.src_at, self.tmp_bytes = coef_at, coef_elems, lut_at, src_at, tmp_bytes
        self.lut_bytes = 768 * B

    def pin_memory(self):
        self.buf, self.target = self.buf.pin_memory(), self.target.pin_memory()
        return self


def _describe(d, b, src_h, src_w, p, shape, coef_elems, tmp_bytes, who):
    """The geometry of descriptor d (image b of a batch): source size, crop, flip, the workspace rows and the place and
    tap counts of its two tables -> (coef_elems, tmp_bytes) after this image."""
    W, H = shape
    d.src_h, d.src_w = src_h, src_w
    d.crop_x, d.crop_y = p.pleft, p.ptop
    d.crop_w, d.crop_h = p.swidth - 1, p.sheight - 1          # crop box (pleft, ptop, pleft+swidth-1, ptop+sheight-1)
    d.flip = int(p.flip)
    if d.crop_w >= 1 and d.crop_h > 100 * d.crop_w:
        # Pillow resamples a crop this tall and narrow vertically first (a different rounding); a +-20 % jitter
        # crop of a real image never is one
        raise ValueError("%s: crop %d x %d of source %d is over 100x taller than wide" % (who, d.crop_w, d.crop_h, b))
    if d.crop_w >= 1 and d.crop_h >= 1:                        # an empty crop is left to mcamd_augment to reject
        d.tmp_off, tmp_bytes = tmp_bytes, tmp_bytes + _align(d.crop_h * W * 4, 16)
        d.hk, d.hcoef_off = table_taps(d.crop_w, W), coef_elems
        coef_elems += W * (d.hk + 2)
        d.vk, d.vcoef_off = table_taps(d.crop_h, H), coef_elems
        coef_elems += H * (d.vk + 2)
    return coef_elems, tmp_bytes


def _host_tables(descs, shape):
    """The resample_table tables of every non-empty crop, in descriptor order (horizontal, vertical)."""
    W, H = shape
    return [resample_table(n_in, n_out)[1].reshape(-1) for d in descs if d.crop_w >= 1 and d.crop_h >= 1
            for n_in, n_out in ((d.crop_w, W), (d.crop_h, H))]


def pack_batch(sources, params, shape, targets=None):
    """sources: B uint8 [h][w][3] arrays; params: B AugParams; shape = (W, H) as in Image.resize."""
    W, H = shape
    B = len(sources)
    if B != len(params) or B < 1:
        raise ValueError("pack_batch: %d sources, %d parameter sets" % (B, len(params)))
    descs = (_lib.AugmentDesc * B)()
    luts = []
    coef_elems = src_bytes = tmp_bytes = 0
    for b, (s, p) in enumerate(zip(sources, params)):
        if s.dtype != np.uint8 or s.ndim != 3 or s.shape[2] != 3:
            raise ValueError("pack_batch: source %d is %s %s, not uint8 [h][w][3]" % (b, s.dtype, s.shape))
        d = descs[b]
        d.src_off, src_bytes = src_bytes, src_bytes + _align(s.nbytes, 16)
        coef_elems, tmp_bytes = _describe(d, b, s.shape[0], s.shape[1], p, (W, H), coef_elems, tmp_bytes, "pack_batch")
        d.lut_off = 768 * b
        luts.append(point_luts(p.dhue, p.dsat, p.dexp))
    tables = _host_tables(descs, (W, H))
    coef_at = _align(C.sizeof(descs))
    lut_at = _align(coef_at + 4 * coef_elems)
    src_at = _align(lut_at + 768 * B)
    buf = torch.empty(src_at + src_bytes, dtype=torch.uint8)
    a = buf.numpy()
    C.memmove(a.ctypes.data, descs, C.sizeof(descs))
    if tables:
        a[coef_at:coef_at + 4 * coef_elems].view(np.int32)[:] = np.concatenate(tables)
    a[lut_at:lut_at + 768 * B] = np.concatenate(luts).reshape(-1)
    for b, s in enumerate(sources):
        o = src_at + descs[b].src_off
        a[o:o + s.nbytes] = s.reshape(-1)
    if targets is None:
        targets = torch.zeros(B, MAX_BOXES * 5)
    return PackedBatch(buf, B, (W, H), coef_at, coef_elems, lut_at, src_at, tmp_bytes, targets)


def pack_resident(resident, indices, params, shape, targets=None, distort=True, device_tables=True):
    """pack_batch for sources that live on the device: `resident` is a data.ResidentImages (or its host_index: only
    `offsets`, `sizes` and `nbytes` are read), `indices` the B pictures.  The buffer has no source section, src_off is
    the resident offset and every other descriptor field is what pack_batch sets.  distort=False: no HSV step
    (lut_off = -1, no LUTs).  device_tables=True: the tables and LUTs are not built here; their places are offsets
    into a device workspace and the buffer carries float64 [B][3] (dhue, dsat, dexp) for mcamd_augment_tables."""
    W, H = shape
    B = len(indices)
    if B != len(params) or B < 1:
        raise ValueError("pack_resident: %d indices, %d parameter sets" % (B, len(params)))
    descs = (_lib.AugmentDesc * B)()
    coef_elems = tmp_bytes = 0
    for b, (i, p) in enumerate(zip(indices, params)):
        d = descs[b]
        d.src_off = int(resident.offsets[i])
        h, w = (int(v) for v in resident.sizes[i])
        coef_elems, tmp_bytes = _describe(d, b, h, w, p, (W, H), coef_elems, tmp_bytes, "pack_resident")
        d.lut_off = 768 * b if distort else -1
    lut_bytes = 768 * B if distort else 0
    if targets is None:
        targets = torch.zeros(B, MAX_BOXES * 5)
    if device_tables:
        hsv_at = _align(C.sizeof(descs))
        buf = torch.empty(hsv_at + 24 * B, dtype=torch.uint8)
        a = buf.numpy()
        a[hsv_at:].view(np.float64)[:] = np.array([(p.dhue, p.dsat, p.dexp) for p in params], np.float64).reshape(-1)
        coef_at, lut_at = 0, _align(4 * coef_elems)           # in the workspace
    else:
        coef_at = _align(C.sizeof(descs))
        lut_at = _align(coef_at + 4 * coef_elems)
        buf = torch.empty(lut_at + lut_bytes, dtype=torch.uint8)
        a = buf.numpy()
        tables = _host_tables(descs, (W, H))
        if tables:
            a[coef_at:coef_at + 4 * coef_elems].view(np.int32)[:] = np.concatenate(tables)
        if distort:
            a[lut_at:] = np.concatenate([point_luts(p.dhue, p.dsat, p.dexp) for p in params]).reshape(-1)
    C.memmove(a.ctypes.data, descs, C.sizeof(descs))
    pb = PackedBatch(buf, B, (W, H), coef_at, coef_elems, lut_at, buf.numel(), tmp_bytes, targets)
    pb.lut_bytes, pb.resident_bytes = lut_bytes, int(resident.nbytes)
    if device_tables:
        pb.hsv_at = hsv_at
    return pb


def collate(items, shape):
    """DataLoader collate_fn body for VOCAugment / SyntheticAugment items (source, boxes, params): the sources stay
    ragged, the labels are transformed here, and the whole batch is packed (in the worker) for DeviceAugmenter."""
    targets = torch.stack([transform_labels(boxes, p) for _, boxes, p in items])
    return pack_batch([s for s, _, _ in items], [p for _, _, p in items], shape, targets)


def collate_fn(shape):
    """A picklable collate_fn for loader workers."""
    return functools.partial(collate, shape=tuple(shape))


def augment_launch(pb, dev_buf, tmp, out, stream=None, resident=None, workspace=None):
    """mcamd_augment for a PackedBatch whose bytes are in `dev_buf` (device uint8), on `stream` (a hipStream_t as an
    int; default: the current torch stream).  A batch of pack_resident takes its sources from `resident` (the device
    uint8 buffer of data.ResidentImages) and, packed with device_tables, has mcamd_augment_tables build its tables and
    LUTs in `workspace` (device uint8, lut_at + lut_bytes bytes) first."""
    W, H = pb.shape
    hb, db = pb.buf.data_ptr(), dev_buf.data_ptr()
    st = _lib.stream_ptr() if stream is None else C.c_void_p(stream)
    if pb.resident_bytes is None:
        src, src_bytes = db + pb.src_at, pb.buf.numel() - pb.src_at
    else:
        if resident is None or resident.numel() != pb.resident_bytes:
            raise ValueError("batch packed for a resident buffer of %d bytes, got %s"
                             % (pb.resident_bytes, None if resident is None else resident.numel()))
        src, src_bytes = resident.data_ptr(), pb.resident_bytes
    tables = db
    if pb.hsv_at is not None:
        if workspace is None or workspace.numel() < pb.lut_at + pb.lut_bytes:
            raise ValueError("batch packed for device tables needs a workspace of %d bytes" % (pb.lut_at + pb.lut_bytes))
        tables = workspace.data_ptr()
        _lib.check(_lib.lib().mcamd_augment_tables(hb, db, db + pb.hsv_at, pb.B, H, W, tables + pb.coef_at, pb.coef_elems,
                                                   tables + pb.lut_at if pb.lut_bytes else None, pb.lut_bytes, st),
                   "mcamd_augment_tables")
    bt = _lib.AugmentBatch(desc=hb, desc_dev=db, src=src, src_bytes=src_bytes,
                      coef=tables + pb.coef_at, coef_elems=pb.coef_elems,
                      lut=tables + pb.lut_at if pb.lut_bytes else None, lut_bytes=pb.lut_bytes,
                      tmp=tmp.data_ptr(), tmp_bytes=tmp.numel(),
                      out=out.data_ptr(), B=pb.B, H=H, W=W)
    _lib.check(_lib.lib().mcamd_augment(C.byref(bt), st), "mcamd_augment")


class DeviceAugmenter:
    """Batch front end: PackedBatch -> (x fp32 [B][3][H][W], target fp32 [B][250]) on `device`,
    enqueued on the current stream with no host synchronisation.  With `resident` (a data.ResidentImages on the
    device) it also takes the batches of pack_resident: one small H2D copy (descriptors, and the tables and LUTs or
    the three numbers they are built from), mcamd_augment_tables when the batch asks for it, then mcamd_augment
    reading the resident buffer."""

    def __init__(self, shape=(416, 416), device="cuda", resident=None):
        self.shape, self.device = tuple(shape), torch.device(device)
        self.resident = None if resident is None else resident.buf

    def __call__(self, batch):
        if not isinstance(batch, PackedBatch):
            raise TypeError("DeviceAugmenter takes a PackedBatch (augment.collate / pack_batch)")
        if batch.shape != self.shape:
            raise ValueError("batch packed for %s, augmenter shape %s" % (batch.shape, self.shape))
        if not batch.buf.is_pinned():
            batch.pin_memory()
        W, H = self.shape
        dev_buf = batch.buf.to(self.device, non_blocking=True)
        tmp = torch.empty(max(batch.tmp_bytes, 1), dtype=torch.uint8, device=self.device)
        x = torch.empty(batch.B, 3, H, W, dtype=torch.float32, device=self.device)
        ws = None
        if batch.hsv_at is not None:
            ws = torch.empty(max(batch.lut_at + batch.lut_bytes, 1), dtype=torch.uint8, device=self.device)
        augment_launch(batch, dev_buf, tmp, x, resident=self.resident, workspace=ws)
        return x, batch.target.to(self.device, non_blocking=True)


def synthetic_source(w, h, seed):
    """A deterministic uint8 [h][w][3] test image from an integer formula (smooth gradients, edges and texture)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    c = np.arange(3, dtype=np.int64)[None, None, :]
    s = int(seed) % 9973
    v = (x[..., None] * (3 + c) + y[..., None] * (5 + 2 * c) + s * 37 + ((x[..., None] * y[..., None] + s) >> (3 + c))
         + 64 * (((x[..., None] // (7 + c)) + (y[..., None] // 11)) % 2))
    return (v & 255).astype(np.uint8)
