"""The YOLOv2 region loss of the reference (src/nets.py:282-635, build_targets + RegionLoss.forward) in float64 NumPy, as
the reference's own loops over images and ground-truth boxes (vectorised over the cells only).  It shares no code with the
package: it is what csrc/region_loss.hip and the torch restatement in region_loss.py are compared against, per element.

Kept from the reference, on purpose:
  * the boxes of the IoU tests are exp(exp(o)) * anchor (double exponential, nets.py:511-512, 546-547);
  * tw, th = gw / anchor, no logarithm (nets.py:429-430);
  * conf_mask enters the loss as its square root on both sides of a squared error = as itself (nets.py:582, 598);
  * an image's rows end at the first x == 0 (nets.py:326, 370);
  * the boxes are written in order, so the later of two boxes in one cell / anchor wins (nets.py:418-436);
  * the best anchor is the first strict maximum of the shape IoU, and best_n = -1 = the last anchor when no IoU is
    above 0 (nets.py:375-409);
  * tx = gx - int(gx) with the unclamped integer (nets.py:424); the cell index itself is clamped to the grid (the
    reference would raise for x == 1.0, the kernel clamps);
  * the best IoU of a cell is a maximum that ignores NaN (the reference's NaN compares false against the threshold,
    which is the same decision);
  * a class label outside [0, C) gives no class term and a zero class gradient (the kernel's documented behaviour; the
    reference's CrossEntropyLoss would raise).
The reference evaluates in float32, where exp(exp(o)) * anchor overflows to inf for o above 4.4855; that overflow is a
property of the operation's number format, so it is kept: a box size beyond the largest float32 is inf here as well.
Everything else is float64 arithmetic on the given numbers.
"""
import numpy as np

MAX_BBOX = 50
FLT_MAX = float(np.finfo(np.float32).max)
EPS32 = float(np.finfo(np.float32).eps)


class Result(object):
    """loss, grad [B, A*(5+C), H, W], counts (nGT, nCorrect); scale (per gradient element, see region_loss_ref), loss_abs,
    margins (3 numbers); info: what the input exercised (counts of cells / boxes) and the assigned-cell mask."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _iou(x1, y1, w1, h1, x2, y2, w2, h2):
    """bbox_iou / bbox_ious(x1y1x2y2=False), nets2_utils.py:63-131."""
    mx = np.minimum(x1 - w1 / 2.0, x2 - w2 / 2.0)
    Mx = np.maximum(x1 + w1 / 2.0, x2 + w2 / 2.0)
    my = np.minimum(y1 - h1 / 2.0, y2 - h2 / 2.0)
    My = np.maximum(y1 + h1 / 2.0, y2 + h2 / 2.0)
    cw = w1 + w2 - (Mx - mx)
    ch = h1 + h2 - (My - my)
    carea = np.where((cw <= 0) | (ch <= 0), 0.0, cw * ch)
    return carea / (w1 * h1 + w2 * h2 - carea)


def _f32_range(v):
    return np.where(v > FLT_MAX, np.inf, v)


def region_loss_ref(out, target, anchors, A, C, scales, thresh):
    """out [B, A*(5+C), H, W], target [B, 250] rows of (class, x, y, w, h), anchors: a flat list of at least A (w, h)
    pairs, scales = (coord, noobject, object, class).

    `scale` is, for every gradient element, the gradient's formula with every subtraction of two like quantities replaced
    by the sum of their magnitudes (x - tx -> |x| + |gx| + |int(gx)|, since tx is itself such a difference; 1 - x ->
    1 + x; conf - tconf -> conf + |tconf|; p_c - [c == tcls] -> p_c + [c == tcls]): a float32 evaluation is expected
    within a small multiple of eps32 * scale of `grad`.  `loss_abs` is the same for the loss (only the cross-entropy's
    lse - o_tcls has a difference).
    `margins` are the three comparisons a float32 evaluation may decide differently:
      [0] min |best IoU - thresh| over all cells of images with boxes,
      [1] min (best - second best anchor IoU) over all boxes that have an anchor IoU above 0 (with none above 0 every
          anchor IoU is exactly 0 in any precision and the last anchor is taken), inf for A == 1,
      [2] min |IoU - 0.5| over the boxes counted for nCorrect (all valid boxes; NaN IoUs are never counted)."""
    out = np.asarray(out, dtype=np.float64)
    B, ch, H, W = out.shape
    assert ch == A * (5 + C)
    o = out.reshape(B, A, 5 + C, H, W)
    tg = np.asarray(target, dtype=np.float64).reshape(B, MAX_BBOX, 5)
    step = len(anchors) // A
    aw = np.array([float(np.float32(anchors[step * n])) for n in range(A)])
    ah = np.array([float(np.float32(anchors[step * n + 1])) for n in range(A)])
    coord_s, noobj_s, obj_s, cls_s = (float(np.float32(s)) for s in scales)
    thresh = float(np.float32(thresh))

    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x = 1.0 / (1.0 + np.exp(-o[:, :, 0]))
        y = 1.0 / (1.0 + np.exp(-o[:, :, 1]))
        w = np.exp(o[:, :, 2])
        h = np.exp(o[:, :, 3])
        conf = 1.0 / (1.0 + np.exp(-o[:, :, 4]))
        px = x + np.arange(W, dtype=np.float64).reshape(1, 1, 1, W)
        py = y + np.arange(H, dtype=np.float64).reshape(1, 1, H, 1)
        pw = _f32_range(_f32_range(np.exp(w)) * aw.reshape(1, A, 1, 1))
        ph = _f32_range(_f32_range(np.exp(h)) * ah.reshape(1, A, 1, 1))

        shape = (B, A, H, W)
        conf_mask = np.full(shape, noobj_s)
        cm = np.zeros(shape)
        tx, ty, tw, th, tconf = (np.zeros(shape) for _ in range(5))
        tx_abs, ty_abs = np.zeros(shape), np.zeros(shape)
        tcls = np.zeros(shape, dtype=np.int64)
        owner = np.full(shape, -1, dtype=np.int64)          # the row that wrote the cell last
        clamped = np.zeros(shape, dtype=bool)
        fallback = np.zeros(shape, dtype=bool)
        margins = [np.inf, np.inf, np.inf]
        nGT = nCorrect = n_overwritten = n_ignored_rows = 0

        for b in range(B):
            T = 0
            while T < MAX_BBOX and tg[b, T, 1] != 0:
                T += 1
            n_ignored_rows += int(np.count_nonzero(tg[b, T + 1:, 1])) if T < MAX_BBOX else 0
            # nets.py:322-347: silence the no-object penalty where a prediction overlaps some ground truth
            best = np.zeros((A, H, W))
            for t in range(T):
                gx, gy, gw, gh = tg[b, t, 1] * W, tg[b, t, 2] * H, tg[b, t, 3] * W, tg[b, t, 4] * H
                best = np.fmax(best, _iou(px[b], py[b], pw[b], ph[b], gx, gy, gw, gh))
            if T:
                conf_mask[b][best > thresh] = 0.0
                margins[0] = min(margins[0], float(np.min(np.abs(best - thresh))))
            # nets.py:368-438
            for t in range(T):
                nGT += 1
                gx, gy, gw, gh = tg[b, t, 1] * W, tg[b, t, 2] * H, tg[b, t, 3] * W, tg[b, t, 4] * H
                gi, gj = int(gx), int(gy)
                best_iou, best_n, ious = 0.0, -1, []
                for n in range(A):
                    v = float(_iou(0.0, 0.0, aw[n], ah[n], 0.0, 0.0, gw, gh))
                    ious.append(v)
                    if v > best_iou:
                        best_iou, best_n = v, n
                if best_n >= 0 and A > 1:
                    top = sorted((v for v in ious if v == v), reverse=True)
                    margins[1] = min(margins[1], top[0] - top[1])
                bn = best_n if best_n >= 0 else A - 1
                ci, cj = min(max(gi, 0), W - 1), min(max(gj, 0), H - 1)
                iou = float(_iou(gx, gy, gw, gh, px[b, bn, cj, ci], py[b, bn, cj, ci], pw[b, bn, cj, ci], ph[b, bn, cj, ci]))
                if iou == iou:
                    margins[2] = min(margins[2], abs(iou - 0.5))
                if iou > 0.5:
                    nCorrect += 1
                if owner[b, bn, cj, ci] >= 0:
                    n_overwritten += 1
                owner[b, bn, cj, ci] = t
                cm[b, bn, cj, ci] = 1.0
                conf_mask[b, bn, cj, ci] = obj_s
                tx[b, bn, cj, ci], ty[b, bn, cj, ci] = gx - gi, gy - gj
                tx_abs[b, bn, cj, ci], ty_abs[b, bn, cj, ci] = abs(gx) + abs(gi), abs(gy) + abs(gj)
                tw[b, bn, cj, ci], th[b, bn, cj, ci] = gw / aw[bn], gh / ah[bn]
                tconf[b, bn, cj, ci] = iou
                tcls[b, bn, cj, ci] = int(tg[b, t, 0])                  # truncates towards zero, as .long() does
                clamped[b, bn, cj, ci] = (ci != gi) or (cj != gj)
                fallback[b, bn, cj, ci] = best_n < 0

        # nets.py:594-600 and its derivative with respect to the logits
        inv = 1.0 / B
        grad = np.zeros_like(o)
        scale = np.zeros_like(o)
        dx, dy, dw, dh, dc = x - tx, y - ty, w - tw, h - th, conf - tconf
        cell = coord_s * cm * 0.5 * (dx * dx + dy * dy + dw * dw + dh * dh) + conf_mask * 0.5 * dc * dc
        cell_abs = cell.copy()
        grad[:, :, 0] = coord_s * cm * dx * x * (1.0 - x) * inv
        grad[:, :, 1] = coord_s * cm * dy * y * (1.0 - y) * inv
        grad[:, :, 2] = coord_s * cm * dw * w * inv
        grad[:, :, 3] = coord_s * cm * dh * h * inv
        grad[:, :, 4] = conf_mask * dc * conf * (1.0 - conf) * inv
        scale[:, :, 0] = coord_s * cm * (x + tx_abs) * x * (1.0 + x) * inv
        scale[:, :, 1] = coord_s * cm * (y + ty_abs) * y * (1.0 + y) * inv
        scale[:, :, 2] = coord_s * cm * (w + tw) * w * inv
        scale[:, :, 3] = coord_s * cm * (h + th) * h * inv
        scale[:, :, 4] = conf_mask * (conf + np.abs(tconf)) * conf * (1.0 + conf) * inv
        in_range = (cm == 1.0) & (tcls >= 0) & (tcls < C)
        for b, n, j, i in zip(*np.nonzero(in_range)):
            oc = o[b, n, 5:, j, i]
            m = oc.max()
            lse = m + np.log(np.exp(oc - m).sum())
            p = np.exp(oc - lse)
            hot = np.zeros(C)
            hot[tcls[b, n, j, i]] = 1.0
            grad[b, n, 5:, j, i] = cls_s * (p - hot) * inv
            scale[b, n, 5:, j, i] = cls_s * (p + hot) * inv
            cell[b, n, j, i] += cls_s * (lse - oc[tcls[b, n, j, i]])
            cell_abs[b, n, j, i] += cls_s * (abs(lse) + abs(oc[tcls[b, n, j, i]]))

    has_boxes = (tg[:, 0, 1] != 0).reshape(B, 1, 1, 1)
    info = dict(
        assigned=cm == 1.0,
        silenced=int(np.count_nonzero((conf_mask == 0.0) & (cm == 0.0) & has_boxes)) if noobj_s != 0.0 else 0,
        overwritten=n_overwritten, clamped=int(clamped.sum()), fallback=int(fallback.sum()),
        out_of_range=int(np.count_nonzero((cm == 1.0) & ~in_range)), ignored_rows=n_ignored_rows,
        inf_boxes=int(np.count_nonzero((~np.isfinite(pw) | ~np.isfinite(ph)) & has_boxes)),
        truncated_labels=int(sum(1 for b, n, j, i in zip(*np.nonzero(cm == 1.0))
                                 if tg[b, owner[b, n, j, i], 0] != int(tg[b, owner[b, n, j, i], 0]))))
    return Result(loss=float(cell.sum() * inv), grad=grad.reshape(out.shape), counts=(nGT, nCorrect),
                  scale=scale.reshape(out.shape), loss_abs=float(cell_abs.sum() * inv), margins=tuple(margins), info=info)
