"""A numpy restatement of the contract of csrc/voc_eval.hip (include/mcamd.h), and the generated inputs the
tests of it share: crafted rows / probs / nkept as mcamd_detect would leave them, their ground truth, and a devkit on disk.

    q          float('%f' % v) of an fp32 value
    emit       the records predict() writes as text lines
    match      the stable order (class, descending q(score), image, row) and voc_eval's matching per (image, class)
    curves     rec, prec and PASCALVOCEval.voc_ap's 11-point AP of one class's flags
"""
import os

import numpy as np

from modelcompression_amd.predict import PASCALVOCEval

CLASSES = PASCALVOCEval(None, '', '', None, '', '', '', '', '').VOC_CLASSES
NEITHER, TP, FP = 0, 1, 2


def q(v):
    """float('%f' % v), v fp32: v * 1e6 is exact in a double, rint rounds ties to even as the C library's printf does."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    return np.rint(v.astype(np.float64) * 1e6) / 1e6


def emit(rows, probs, nkept, conf_thresh, first_image, sizes):
    """One record (class, s6 = q(score) * 1e6, image, row, x1, y1, x2, y2) per line that predict() writes, in its order."""
    two, conf = np.float32(2), np.float32(conf_thresh)
    out = []
    for b in range(rows.shape[0]):
        W, H = np.float32(sizes[b][0]), np.float32(sizes[b][1])
        for r in range(int(nkept[b])):
            x, y, w, h = rows[b, r, :4]
            box = q(np.array([(x - w / two) * W, (y - h / two) * H, (x + w / two) * W, (y + h / two) * H], dtype=np.float32))
            top = int(rows[b, r, 6])
            for c in range(probs.shape[2]):
                if probs[b, r, c] > conf or c == top:
                    out.append((c, int(np.rint(np.float64(probs[b, r, c]) * 1e6)), first_image + b, r) + tuple(box))
    return out


def make_key(c, s6, image, r):
    return (c << 56) | ((1000000 - s6) << 36) | (image << 11) | r


def match(records, gt, ovthresh=0.5):
    """records of emit (any order), gt = per global image a list of (class, difficult, (xmin, ymin, xmax, ymax)) in annotation
    order.  Returns (keys int64, flags uint8, class int) in the total order; the arithmetic is voc_eval's, line by line."""
    order = sorted(records, key=lambda t: (t[0], -t[1], t[2], t[3]))
    det = {}
    keys, flags, cls = [], [], []
    for c, s6, image, r, x1, y1, x2, y2 in order:
        R = [o for o in gt[image] if o[0] == c]
        BBGT = np.array([o[2] for o in R]).astype(float)
        difficult = [bool(o[1]) for o in R]
        done = det.setdefault((image, c), [False] * len(R))
        bb, ovmax = np.array([x1, y1, x2, y2]).astype(float), -np.inf
        if BBGT.size > 0:
            iw = np.maximum(np.minimum(BBGT[:, 2], bb[2]) - np.maximum(BBGT[:, 0], bb[0]) + 1., 0.)
            ih = np.maximum(np.minimum(BBGT[:, 3], bb[3]) - np.maximum(BBGT[:, 1], bb[1]) + 1., 0.)
            inters = iw * ih
            uni = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) +
                   (BBGT[:, 2] - BBGT[:, 0] + 1.) * (BBGT[:, 3] - BBGT[:, 1] + 1.) - inters)
            overlaps = inters / uni
            ovmax, jmax = np.max(overlaps), int(np.argmax(overlaps))
        flag = NEITHER
        if ovmax > ovthresh:
            if not difficult[jmax]:
                if not done[jmax]:
                    flag, done[jmax] = TP, True
                else:
                    flag = FP
        else:
            flag = FP
        keys.append(make_key(c, s6, image, r)), flags.append(flag), cls.append(c)
    return np.array(keys, dtype=np.int64), np.array(flags, dtype=np.uint8), np.array(cls, dtype=np.int64)


def count_npos(gt, num_classes):
    npos = np.zeros(num_classes, dtype=np.int32)
    for objs in gt:
        for c, difficult, _ in objs:
            npos[c] += not difficult
    return npos


def curves(flags, npos):
    """rec, prec, ap of one class from its flags in order, as voc_eval's last lines compute them."""
    if len(flags) == 0:
        return np.zeros(0), np.zeros(0), 0.0
    tp, fp = np.cumsum((flags == TP).astype(float)), np.cumsum((flags == FP).astype(float))
    rec = tp / float(max(int(npos), 1))
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, PASCALVOCEval.voc_ap(None, rec, prec, True)


# ------------------------------------------------------------------------------------------------------ generated inputs
def _grid_objects(rng, W, H, n, num_classes):
    """n objects on an 8 x 8 grid of a W x H image: classes cycle over five, every seventh is difficult, and objects 10
    and 11 are the same box of the same class (np.argmax takes the first)."""
    objs = []
    cw, ch = W // 8, H // 8
    for j in range(n):
        gx, gy = j % 8, j // 8
        box = (gx * cw + 3, gy * ch + 3, gx * cw + cw - 6, gy * ch + ch - 5)
        objs.append((j % 5 % num_classes, int(j % 7 == 6), box))
    if n > 11:
        objs[11] = (objs[10][0], 0, objs[10][2])
    return objs


def _row_for(box, W, H):
    """(x, y, w, h) fp32, relative, of a pixel box (x1, y1, x2, y2)."""
    x1, y1, x2, y2 = box
    return np.array([(x1 + x2) / 2.0 / W, (y1 + y2) / 2.0 / H, (x2 - x1) / float(W), (y2 - y1) / float(H)], dtype=np.float32)


class Case:
    """rows [B, N, 8], probs [B, N, C], nkept [B] (numpy), sizes [(W, H)], gt (per image, see match), conf_thresh."""


def craft_case(seed=0, N=256, C=20, ties=False, conf_thresh=0.005):
    """Four images.  0: ground truth but nkept = 0.  1: nkept = N, 64 objects.  2: no ground truth.  3: a 64 x 64 image with
    a detection of IoU exactly 0.5, two identical objects, double hits, and a difficult object.
    Rows at or beyond nkept are NaN / 1e30.  Scores are distinct after q() unless `ties`.  The ground truth has classes
    0 .. 4 only, and class C - 1 has no record."""
    rng = np.random.RandomState(seed)
    B = 4
    k = Case()
    k.sizes = [(353, 500), (500, 375), (500, 333), (64, 64)]
    k.gt = [_grid_objects(rng, 353, 500, 9, C), _grid_objects(rng, 500, 375, 64, C), [],
            [(0, 0, (10, 10, 19, 19)),            # a 10 x 10 object (+1 convention)
             (1, 0, (30, 30, 50, 50)), (1, 0, (30, 30, 50, 50)),          # twice the same
             (2, 1, (5, 40, 25, 60)),             # difficult
             (3, 0, (40, 5, 60, 25))]]
    k.nkept = np.array([0, N, min(40, N), min(64, N)], dtype=np.int32)
    k.conf_thresh, k.first_image = conf_thresh, 0
    rows = np.full((B, N, 8), np.nan, dtype=np.float32)
    probs = np.full((B, N, C), 1e30, dtype=np.float32)
    assert int(k.nkept.sum()) * C <= 19990
    low = rng.permutation(19990) + 10                            # others: 0.00001 .. 0.019999, a quarter <= conf_thresh
    high = rng.permutation(959999)[:B * N] + 20000               # the arg-max class: 0.02 .. 0.979998
    li = hi = 0
    for b in range(B):
        W, H = k.sizes[b]
        for r in range(int(k.nkept[b])):
            if k.gt[b] and rng.rand() < 0.7:
                c, _, box = k.gt[b][rng.randint(len(k.gt[b]))]
                box = np.array(box, dtype=np.float64) + rng.uniform(-6, 6, 4) * (rng.rand() < 0.8)
            else:
                c = rng.randint(C - 1)
                x1, y1 = rng.uniform(0, W * 0.7), rng.uniform(0, H * 0.7)
                box = np.array([x1, y1, x1 + rng.uniform(4, W * 0.3), y1 + rng.uniform(4, H * 0.3)])
            rows[b, r, :4] = _row_for(box, W, H)
            for cc in range(C):
                probs[b, r, cc] = np.float32(low[li] / 1e6)
                li += 1
            probs[b, r, c] = np.float32(high[hi] / 1e6)
            probs[b, r, C - 1] = np.float32(3e-6)                # the last class is never emitted: a class without records
            hi += 1
            rows[b, r, 4], rows[b, r, 5], rows[b, r, 6], rows[b, r, 7] = 0.9, probs[b, r, c], c, r
    n3 = int(k.nkept[3])
    assert n3 >= 12
    # image 3, by hand.  Row 0: a 10 x 5 detection inside the 10 x 10 object: IoU exactly 0.5, which is not > 0.5 -> fp
    rows[3, 0, :4] = [14.5 / 64, 12 / 64, 9 / 64, 4 / 64]
    # rows 1, 2: two hits on the object of class 0: the better one is the tp, the other an fp
    rows[3, 1, :4] = rows[3, 2, :4] = _row_for((10, 10, 19, 19), 64, 64)
    # rows 3, 4, 5: hits on the doubled object of class 1: tp on the first copy, then fp twice (the second copy never matches)
    rows[3, 3, :4] = rows[3, 4, :4] = rows[3, 5, :4] = _row_for((30, 30, 50, 50), 64, 64)
    # row 6: the difficult object -> neither;  row 7: class 3's object -> tp
    rows[3, 6, :4] = _row_for((5, 40, 25, 60), 64, 64)
    rows[3, 7, :4] = _row_for((40, 5, 60, 25), 64, 64)
    for r, c in ((0, 0), (1, 0), (2, 0), (3, 1), (4, 1), (5, 1), (6, 2), (7, 3)):
        old = int(rows[3, r, 6])
        probs[3, r, old], probs[3, r, c] = probs[3, r, c], probs[3, r, old]
        probs[3, r, c] = np.float32((990000 + 100 * r) / 1e6)    # ahead of every other row of the image
        rows[3, r, 5], rows[3, r, 6] = probs[3, r, c], c
    # rows 8, 9: the arg-max class is forced to one whose probability is below conf_thresh; it is emitted all the same
    for r in (8, 9):
        c = (int(rows[3, r, 6]) + 1) % (C - 1)
        probs[3, r, c] = np.float32((r - 7) / 1e6)
        assert probs[3, r, c] <= np.float32(conf_thresh)
        rows[3, r, 6] = c
    k.forced = [(3, 8, int(rows[3, 8, 6])), (3, 9, int(rows[3, 9, 6]))]
    if ties:
        # equal fp32 scores within an image, across images, and two fp32 values that q() rounds to the same six decimals
        probs[3, 2, 0] = probs[3, 1, 0]
        probs[3, 4, 1] = probs[3, 3, 1]
        probs[2, 5, 1] = probs[1, 7, 1] = probs[3, 3, 1]
        probs[1, 9, 4] = np.float32(0.5)
        probs[1, 3, 4] = np.nextafter(np.float32(0.5), np.float32(1))
        probs[2, 0, 4] = np.nextafter(np.float32(0.5), np.float32(0))
    k.rows, k.probs = rows, probs
    return k


def tie_free(records):
    """No two records of one class share q(score)."""
    seen = set((t[0], t[1]) for t in records)
    return len(seen) == len(records)


XML = """<annotation><filename>%s</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>
"""
OBJ = ("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
       "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>")


def write_devkit(root, ids, sizes, gt, extra=(), images=None):
    """VOC2007/{Annotations, ImageSets/Main/test.txt, JPEGImages} under root: image i has ids[i], sizes[i], gt[i]; `extra`
    = (id, objects) pairs that are in the image set (they count towards npos) but not in the evaluation list.  images[i]
    (uint8 HWC, optional) is the picture; a grey one otherwise.  Returns (pascal_dir, list file)."""
    from PIL import Image
    base = os.path.join(str(root), 'VOC2007')
    for d in ('Annotations', 'ImageSets/Main', 'JPEGImages'):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    paths = []
    for i, name in enumerate(ids):
        W, H = sizes[i]
        body = ''.join(OBJ % ((CLASSES[c], d) + tuple(box)) for c, d, box in gt[i])
        with open(os.path.join(base, 'Annotations', name + '.xml'), 'w') as f:
            f.write(XML % (name, W, H, body))
        pix = images[i] if images is not None else np.full((H, W, 3), 128, dtype=np.uint8)
        paths.append(os.path.join(base, 'JPEGImages', name + '.png'))
        Image.fromarray(pix).save(paths[-1])
    for name, objs in extra:
        body = ''.join(OBJ % ((CLASSES[c], d) + tuple(box)) for c, d, box in objs)
        with open(os.path.join(base, 'Annotations', name + '.xml'), 'w') as f:
            f.write(XML % (name, 100, 100, body))
    with open(os.path.join(base, 'ImageSets', 'Main', 'test.txt'), 'w') as f:
        f.write(''.join(n + '\n' for n in list(ids) + [n for n, _ in extra]))
    listfile = os.path.join(str(root), 'eval_list.txt')
    with open(listfile, 'w') as f:
        f.write(''.join(p + '\n' for p in paths))
    return str(root), listfile


# ----------------------------------------------------------------------------------------- end to end on a generated devkit
def make_images(seed, n):
    """n small pictures (uint8 HWC) of different sizes: coloured rectangles, noise over everything."""
    rng = np.random.RandomState(seed)
    images, sizes = [], []
    for i in range(n):
        W, H = int(rng.randint(48, 129)), int(rng.randint(48, 129))
        pix = np.zeros((H, W, 3), dtype=np.int64) + rng.randint(0, 192, 3)
        for _ in range(rng.randint(2, 7)):
            x, y = rng.randint(0, W - 8), rng.randint(0, H - 8)
            pix[y:y + rng.randint(8, H), x:x + rng.randint(8, W)] = rng.randint(0, 192, 3)
        pix = (pix + rng.randint(0, 64, (H, W, 3))).astype(np.uint8)      # no two cells see the same pixels: no tied scores
        images.append(pix), sizes.append((W, H))
    return images, sizes


def ground_truth_from_detections(rows, probs, nkept, sizes, seed, per_image=8):
    """Ground truth made of a model's own detections (numpy, as mcamd_detect wrote them): of the first rows of each image
    every other one becomes an object of its arg-max class, its corners rounded to ints; a third of those are shifted by a
    quarter of their size (IoU with the detection near the 0.5 threshold) and every fifth is difficult."""
    rng = np.random.RandomState(seed)
    gt = []
    for b, (W, H) in enumerate(sizes):
        objs = []
        for r in range(min(int(nkept[b]), 2 * per_image)):
            if rng.rand() < 0.5:
                continue
            x, y, w, h = [float(v) for v in rows[b, r, :4]]
            box = np.array([(x - w / 2) * W, (y - h / 2) * H, (x + w / 2) * W, (y + h / 2) * H])
            if rng.rand() < 1 / 3.:
                box += np.array([w * W, h * H, w * W, h * H]) * rng.uniform(0.15, 0.35) * rng.choice([-1, 1])
            objs.append((int(rows[b, r, 6]), int(rng.rand() < 0.2), tuple(int(v) for v in np.rint(box))))
        gt.append(objs)
    return gt
