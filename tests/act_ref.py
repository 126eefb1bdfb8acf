"""Float64 restatement of mcamd_bn_act_fwd (include/mcamd.h, mcamd_act_desc): every destination AS STORED, bit for bit.

torch on the CPU only.  The activation is  v = leaky(fl32(y [+ border[class(h, w)]]) * scale + shift):  the affine sum is taken
in float64 and rounded ONCE to fp32, the negative branch is the exact product z32 * fl32(slope) rounded once.  On the operand
grid of tests/act_cases.py (`exactness`) that is the number any fp32 evaluation order gives, fused or not.

Replaces, for the comparison, nn.BatchNorm2d's affine step + nn.LeakyReLU + nn.MaxPool2d(2, 2) + Reorg of the reference
network (src/nets.py:802-821, 648-667); `anchor` ties the restatement to torch's own operators in float64.
"""
import collections

import torch
import torch.nn.functional as F

PLAIN, POOL, REORG = 0, 1, 2
F8 = torch.float8_e4m3fn
SENT16 = 0x7F7F          # fp16 NaN; both bytes are the e4m3 NaN code, which no store produces
SENT8 = 0x7F
# region labels of an expected image (per fp16 unit / per byte)
UNWRITTEN, HI, LO, THIRD, LO8, X8, TWIN, POOL_ACT = range(8)
REGION = ("unwritten", "hi", "lo", "third plane", "lo8", "x8", "twin", "pool_act")


def fl32(t):
    """float64 -> the nearest fp32 value, kept in float64"""
    return t.float().double()


def border_class(H, W):
    """[H][W] int64: bit 0 h == 0, bit 1 h == H - 1, bit 2 w == 0, bit 3 w == W - 1 (mcamd_act_desc.border)"""
    h = torch.arange(H).view(H, 1)
    w = torch.arange(W).view(1, W)
    return (h == 0) * 1 + (h == H - 1) * 2 + (w == 0) * 4 + (w == W - 1) * 8


def affine(c, op, rnd=fl32):
    """z as fp32 values in float64, NCHW (rnd: the rounding of every step; `anchor` passes none)"""
    y = op.y
    if op.border is not None:
        cls = border_class(c.H, c.W)                                      # [H][W]
        y = rnd(y + op.border.double()[cls].permute(2, 0, 1).unsqueeze(0))
    return rnd(y * op.scale.double().view(1, -1, 1, 1) + op.shift.double().view(1, -1, 1, 1))


def activation(c, op, rnd=fl32):
    """v as fp32 values in float64, NCHW, full resolution"""
    z = affine(c, op, rnd)
    s = torch.tensor(op.slope, dtype=torch.float32).double()
    return torch.where(z > 0, z, rnd(z * s))


def window(v):
    """[4][B][C][H/2][W/2]: the 2x2 windows in (h, w) scan order"""
    return torch.stack([v[:, :, hs::2, ws::2] for hs in (0, 1) for ws in (0, 1)])


def mapped(c, v):
    """what dst holds, before storage: v, its 2x2 maximum, or the reorg'ed channels (hs * 2 + ws) * C + c at (h / 2, w / 2)"""
    if c.mode == PLAIN:
        return v
    if c.mode == POOL:
        return window(v).amax(0)
    return torch.cat(list(window(v)), 1)


def anchor(c, op):
    """largest deviation of the restatement WITHOUT its fp32 roundings, i.e. in plain float64, from torch's operators on the
    same affine values: the border classes, the activation and the destination mapping"""
    def none(t):
        return t
    z = affine(c, op, none)
    s = float(torch.tensor(op.slope, dtype=torch.float32))
    v = F.leaky_relu(z, s)
    mine = activation(c, op, none)
    err = float((mine - v).abs().max())
    if c.mode == POOL:
        err = max(err, float((mapped(c, mine) - F.max_pool2d(v, 2, 2)).abs().max()))
    elif c.mode == REORG:
        from oracle import darknet_ref as O
        err = max(err, float((mapped(c, mine) - O.reorg(v, 2)).abs().max()))
    return err


# ---------------------------------------------------------------------------------------------------------- storage
def bits16(h):
    return h.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def hi16(v):
    """fp16(clamp(v, +-65504)), as fp16"""
    return v.clamp(-65504.0, 65504.0).float().half()


def lo16(v):
    return (v - hi16(v).double()).float().half()


def e4m3(t):
    """codes (uint8) of float64 values: clamped to +-448, one rounding from fp32"""
    return t.float().clamp(-448.0, 448.0).to(F8).view(torch.uint8)


def lo8(v):
    return e4m3((v - hi16(v).double()) * 4096.0)


def x8(v):
    return e4m3(v * 2.0)


def twin16(v):
    """what the fp16 buffer beside a byte twin holds: deq(code) / 2"""
    return (x8(v).view(F8).float() * 0.5).half()


def half_prev_bits(b):
    """the next fp16 value below (bit patterns, int32): +-0 -> 0x8001, negative values bits + 1, positive bits - 1"""
    return torch.where((b & 0x7FFF) == 0, torch.full_like(b, 0x8001), torch.where((b & 0x8000) != 0, b + 1, b - 1))


def pool_act_bits(v):
    """The header's rule (mcamd_act_desc.pool_act), as bit patterns NCHW int32: the FIRST maximum of the unrounded window in scan
    order keeps fp16(v); every other element that rounds to the same fp16 value gets the next fp16 value below it; everything
    else is fp16(v)."""
    w = window(v)                                                         # [4][B][C][Ho][Wo]
    arg = torch.zeros(w.shape[1:], dtype=torch.int64)
    best = w[0].clone()
    for k in range(1, 4):
        gt = w[k] > best
        best = torch.where(gt, w[k], best)
        arg = torch.where(gt, torch.full_like(arg, k), arg)
    hb = bits16(hi16(w))
    top = torch.gather(hb, 0, arg.unsqueeze(0))[0]
    out = torch.empty_like(hb)
    for k in range(4):
        out[k] = torch.where((arg != k) & (hb[k] == top), half_prev_bits(top), hb[k])
    full = torch.empty(v.shape, dtype=torch.int32)
    for k in range(4):
        full[:, :, k >> 1::2, k & 1::2] = out[k]
    return full, (out != hb).sum().item()


# ---------------------------------------------------------------------------------------------------------- placement
def pixel_index(B, H, W, pad):
    """[B][H][W] int64: index of interior pixel (b, h, w) in a padded NHWC buffer -- the padded form [B][H+2][W+2] (pad 0) or
    the shared-halo form (pad 1: rows of W + 1 pixels, H + 1 rows per image, the pointer at pixel (0, -1, -1))"""
    pw = 1 if pad else 2
    b = torch.arange(B).view(B, 1, 1)
    h = torch.arange(H).view(1, H, 1)
    w = torch.arange(W).view(1, 1, W)
    return (b * (H + pw) + h + 1) * (W + pw) + w + 1


def pixels(B, H, W, pad):
    return B * (H + 1) * (W + 1) + W + 2 if pad else B * (H + 2) * (W + 2)


Image = collections.namedtuple("Image", "want region B H W ld pad")       # want / region: [pixels][ld] (int32 / uint8)


def _put(img, t, choff, label):
    """NCHW values (bit patterns / codes) -> channels [choff, choff + n) of every interior pixel"""
    n = t.shape[1]
    idx = pixel_index(img.B, img.H, img.W, img.pad).reshape(-1)
    img.want[idx, choff:choff + n] = t.permute(0, 2, 3, 1).reshape(-1, n).to(img.want.dtype)
    img.region[idx, choff:choff + n] = label


def _image16(B, H, W, ld, pad):
    n = pixels(B, H, W, pad)
    return Image(torch.full((n, ld), SENT16, dtype=torch.int32), torch.zeros((n, ld), dtype=torch.uint8), B, H, W, ld, pad)


def _image8(B, H, W, ld, pad):
    n = pixels(B, H, W, pad)
    return Image(torch.full((n, ld), SENT8, dtype=torch.int32), torch.zeros((n, ld), dtype=torch.uint8), B, H, W, ld, pad)


def _store16(B, H, W, ld, pad, v, planes, choff, plane, twin):
    """One fp16 destination in storage form `planes` (1: fp16(v), or deq(code) / 2 beside a byte twin)."""
    img = _image16(B, H, W, ld, pad)
    if planes == 1:
        _put(img, bits16(twin16(v) if twin else hi16(v)), choff, HI)
        return img
    _put(img, bits16(hi16(v)), choff, HI)
    if planes in (2, 3):
        _put(img, bits16(lo16(v)), choff + plane, LO)
        if planes == 3:
            _put(img, bits16(hi16(v)), choff + 2 * plane, THIRD)
        return img
    # 4: pixel byte 2 * plane + ci holds lo8, 3 * plane + ci holds x8, ci = the BUFFER channel; little-endian fp16 units
    by = torch.stack([img.want & 0xFF, img.want >> 8], 2).reshape(-1, 2 * ld)
    rg = torch.stack([img.region, img.region], 2).reshape(-1, 2 * ld)
    idx = pixel_index(B, H, W, pad).reshape(-1)
    n = v.shape[1]
    for code, base, label in ((lo8(v), 2 * plane, LO8), (x8(v), 3 * plane, X8)):
        by[idx, base + choff:base + choff + n] = code.permute(0, 2, 3, 1).reshape(-1, n).to(torch.int32)
        rg[idx, base + choff:base + choff + n] = label
    by = by.view(-1, ld, 2)
    rg = rg.view(-1, ld, 2)
    return Image(by[..., 0] | (by[..., 1] << 8), torch.maximum(rg[..., 0], rg[..., 1]), B, H, W, ld, pad)


def expected(c, op):
    """{"dst", "dst2", "pool_act", "dst_q8", "dst2_q8"} -> Image of every destination the case has, plus "moved": how many
    pool_act elements the strict-maximum rule changed."""
    v = activation(c, op)
    m = mapped(c, v)
    Hd, Wd = (c.H, c.W) if c.mode == PLAIN else (c.H // 2, c.W // 2)
    out = {"dst": _store16(c.B, Hd, Wd, c.dst_ld, c.dst_pad, m, c.planes, c.dst_choff, c.dst_plane, c.twin)}
    if c.twin:
        out["dst_q8"] = _image8(c.B, Hd, Wd, c.dst_ld, c.dst_pad)
        _put(out["dst_q8"], x8(m), c.dst_choff, TWIN)
    if c.dst2:
        out["dst2"] = _store16(c.B, c.H, c.W, c.dst2_ld, c.dst2_pad, v, c.planes2, c.dst2_choff, c.dst2_plane, c.twin2)
        if c.twin2:
            out["dst2_q8"] = _image8(c.B, c.H, c.W, c.dst2_ld, c.dst2_pad)
            _put(out["dst2_q8"], x8(v), c.dst2_choff, TWIN)
    if c.pool_act:
        img = _image16(c.B, c.H, c.W, c.pool_act_ld, c.pool_act_pad)
        bits, moved = pool_act_bits(v)
        _put(img, bits, 0, POOL_ACT)
        out["pool_act"], out["moved"] = img, moved
    return out


def interior(img, flat, choff, n):
    """channels [choff, choff + n) of the interior pixels of a [pixels][ld] array -> NCHW"""
    idx = pixel_index(img.B, img.H, img.W, img.pad)
    return flat[idx][..., choff:choff + n].permute(0, 3, 1, 2)


def first_mismatch(img, got):
    """None, or a description of the first element of `got` ([pixels][ld]) that differs from the image"""
    bad = (got != img.want).nonzero()
    if bad.numel() == 0:
        return None
    p, ch = int(bad[0, 0]), int(bad[0, 1])
    pw = 1 if img.pad else 2
    row, x = divmod(p, img.W + pw)
    b, y = divmod(row, img.H + pw)
    per = torch.bincount(img.region[got != img.want].long(), minlength=len(REGION)).tolist()
    return ("%d elements differ (%s); first at image %d channel %d y %d x %d (interior coordinates; -1 = halo): got 0x%04x want 0x%04x, "
            "%s region" % (bad.shape[0], ", ".join("%s %d" % (REGION[r], n) for r, n in enumerate(per) if n), b, ch, y - 1, x - 1,
                           int(got[p, ch]), int(img.want[p, ch]), REGION[int(img.region[p, ch])]))
