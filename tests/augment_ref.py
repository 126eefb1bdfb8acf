"""numpy restatement of the reference's PIL augmentation chain (src/dataloader.py:148-178 + ToTensor()), the yardstick
of tests/test_augment_*.py: crop (outside reads 0) -> Pillow's two fixed-point bicubic passes from the
augment.resample_table tables -> flip -> Pillow's Convert.c RGB->HSV, the point LUTs, HSV->RGB.  The HSV functions
restate Convert.c's float / double arithmetic; test_augment_cpu.py checks them against PIL on all 2^24 colours."""
import numpy as np

from modelcompression_amd.augment import PRECISION_BITS, point_luts, resample_table

f32, f64 = np.float32, np.float64


def crop(src, x0, y0, w, h):
    out = np.zeros((h, w, 3), np.uint8)
    sh, sw = src.shape[:2]
    ys, xs, ye, xe = max(0, y0), max(0, x0), min(sh, y0 + h), min(sw, x0 + w)
    if ye > ys and xe > xs:
        out[ys - y0:ye - y0, xs - x0:xe - x0] = src[ys:ye, xs:xe]
    return out


def apply_pass(img, table, axis):
    """One Pillow 8-bit resampling pass of a uint8 [h][w][3] image along `axis` (1 horizontal, 0 vertical)."""
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((table.shape[0],) + a.shape[1:], np.int64)
    for o in range(table.shape[0]):
        first, cnt = int(table[o, 0]), int(table[o, 1])
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for t in range(cnt):
            acc += a[first + t] * int(table[o, 2 + t])
        out[o] = acc
    return np.moveaxis(np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def resize(img, W, H):
    """Image.resize((W, H)) (bicubic) of a uint8 [h][w][3] image: horizontal pass, then vertical."""
    h, w = img.shape[:2]
    return apply_pass(apply_pass(img, resample_table(w, W)[1], 1), resample_table(h, H)[1], 0)


def rgb2hsv(rgb):
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    eq = maxc == minc
    cr = np.where(eq, f32(1), (maxc - minc).astype(f32))
    s = (maxc - minc).astype(f32) / np.where(maxc == 0, f32(1), maxc.astype(f32))
    rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
    h = np.where(r == maxc, (bc - gc).astype(f64),
                 np.where(g == maxc, 2.0 + rc.astype(f64) - bc.astype(f64), 4.0 + gc.astype(f64) - rc.astype(f64)))
    h = np.fmod(h.astype(f32).astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.where(eq, 0, np.clip(np.trunc(h.astype(f64) * 255.0), 0, 255)).astype(np.uint8)
    us = np.where(eq, 0, np.clip(np.trunc(s.astype(f64) * 255.0), 0, 255)).astype(np.uint8)
    return np.stack([uh, us, maxc.astype(np.uint8)], -1)


def hsv2rgb(hsv):
    h, s, v = (hsv[..., i] for i in range(3))
    hf = h.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int32)
    f = (hf - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32)
    vv = v.astype(f32).astype(f64)

    def rnd(x):                                       # C round(): half away from zero (x >= 0 here)
        return np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)
    p = rnd(vv * (1.0 - fs.astype(f64)))
    q = rnd(vv * (1.0 - (fs * f).astype(f64)))
    t = rnd(vv * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))
    v8, k = v.astype(np.uint8), i % 6
    cond = [k == 0, k == 1, k == 2, k == 3, k == 4]
    rgb = np.stack([np.select(cond, [v8, q, p, p, t], v8), np.select(cond, [t, v8, v8, q, p], p),
                    np.select(cond, [p, p, t, v8, v8], q)], -1)
    return np.where((s == 0)[..., None], v8[..., None], rgb).astype(np.uint8)


def distort(rgb, luts, chunk=1 << 20):
    """RGB -> HSV -> the [3][256] LUTs -> RGB, in chunks of pixels."""
    flat = rgb.reshape(-1, 3)
    out = np.empty_like(flat)
    for a in range(0, flat.shape[0], chunk):
        hsv = rgb2hsv(flat[a:a + chunk])
        hsv = np.stack([luts[0][hsv[:, 0]], luts[1][hsv[:, 1]], luts[2][hsv[:, 2]]], -1)
        out[a:a + chunk] = hsv2rgb(hsv)
    return out.reshape(rgb.shape)


def augment(src, p, shape):
    """uint8 [H][W][3] output of data_augmentation(Image.fromarray(src), shape, ...) for drawn parameters p."""
    W, H = shape
    img = resize(crop(src, p.pleft, p.ptop, p.swidth - 1, p.sheight - 1), W, H)
    if p.flip:
        img = img[:, ::-1]
    return distort(np.ascontiguousarray(img), point_luts(p.dhue, p.dsat, p.dexp))
