"""VOC07 mAP on the device: what PASCALVOCEval._do_python_eval computes from the detection files (voc_eval + voc_ap with
use_07_metric=True), from what mcamd_detect leaves on the device instead (csrc/voc_eval.hip).

    gt = VOCGroundTruth(ev.parse_rec, annopath, imagesetfile, eval_files, class_names, device)
    acc = DeviceVOCEval(gt, num_classes)
    for each batch:  acc.add(rows, probs, nkept, first_image, conf_thresh)      # no host synchronisation
    aps, mAP = acc.finish()                                                     # one
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import McamdError
from .nets2_utils import get_image_size


class VOCGroundTruth:
    """The ground truth of an evaluation list as the device table mcamd_voc_match reads, built once on the host.

    parse_rec     PASCALVOCEval.parse_rec
    annopath      '.../Annotations/{:s}.xml'
    imagesetfile  the image set voc_eval counts npos over (one id per line)
    eval_files    image paths in evaluation order; image i of the evaluation is eval_files[i]
    class_names   class c is class_names[c]; objects of other names take no part (voc_eval filters by name)
    default_size  (width, height) of an image whose header get_image_size cannot read
    """

    def __init__(self, parse_rec, annopath, imagesetfile, eval_files, class_names, device, default_size=None):
        with open(imagesetfile) as f:
            imagenames = [x.strip() for x in f.readlines()]
        recs = {n: parse_rec(annopath.format(n)) for n in imagenames}
        index = {name: c for c, name in enumerate(class_names)}
        npos = np.zeros(len(class_names), dtype=np.int32)
        for n in imagenames:                                  # as voc_eval counts: once per line of the image set
            for obj in recs[n]:
                if obj['name'] in index and not obj['difficult']:
                    npos[index[obj['name']]] += 1
        ids = [os.path.basename(p).split('.')[0] for p in eval_files]
        seen = set()
        for i in ids:
            if i not in recs:
                raise McamdError("VOCGroundTruth: evaluation image `%s` is not in the image set %s" % (i, imagesetfile))
            if i in seen:
                raise McamdError("VOCGroundTruth: evaluation image `%s` is listed twice" % i)
            seen.add(i)
        objs = [[o for o in recs[i] if o['name'] in index] for i in ids]
        for i, o in zip(ids, objs):
            if len(o) > ops.VOC_MAX_OBJECTS:
                raise McamdError("VOCGroundTruth: image `%s` has %d objects, at most %d" % (i, len(o), ops.VOC_MAX_OBJECTS))
        M, G = len(ids), max([1] + [len(o) for o in objs])
        box = np.zeros((M, G, 4), dtype=np.int32)
        cls = np.full((M, G), 255, dtype=np.uint8)
        dif = np.zeros((M, G), dtype=np.uint8)
        cnt = np.zeros(M, dtype=np.int32)
        size = np.zeros((M, 2), dtype=np.int32)
        for m, (path, o) in enumerate(zip(eval_files, objs)):
            cnt[m] = len(o)
            for g, obj in enumerate(o):
                box[m, g], cls[m, g], dif[m, g] = obj['bbox'], index[obj['name']], bool(obj['difficult'])
            wh = get_image_size(path) or default_size
            if not wh:
                raise McamdError("VOCGroundTruth: cannot read the size of `%s`" % path)
            size[m] = wh
        self.ids, self.num_images, self.num_classes, self.max_objects = ids, M, len(class_names), G
        self.npos_host = npos
        self.box, self.cls, self.difficult, self.count, self.size, self.npos = (
            torch.from_numpy(a).to(device) for a in (box, cls, dif, cnt, size, npos))


class DeviceVOCEval:
    """Accumulates detection records on the device and turns them into per-class AP.  `capacity` records are held; more
    make finish() raise."""

    def __init__(self, gt, num_classes, capacity=1 << 22, ovthresh=0.5):
        if num_classes != gt.num_classes:
            raise McamdError("DeviceVOCEval: %d classes, the ground truth has %d" % (num_classes, gt.num_classes))
        dev = gt.box.device
        self.gt, self.num_classes, self.capacity, self.ovthresh = gt, num_classes, int(capacity), float(ovthresh)
        # unused slots hold the largest key, so the sort needs no count on the host
        self.keys = torch.full((self.capacity,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        self.flags = torch.zeros(self.capacity, dtype=torch.uint8, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)
        self._sorted = None

    def add(self, rows, probs, nkept, first_image, conf_thresh):
        """The batch's detections as mcamd_detect wrote them; image b of the batch is image first_image + b of the
        ground truth.  No host synchronisation."""
        B, g = rows.shape[0], self.gt
        if first_image < 0 or first_image + B > g.num_images:
            raise McamdError("DeviceVOCEval.add: images %d .. %d, the ground truth has %d"
                             % (first_image, first_image + B - 1, g.num_images))
        sl = slice(first_image, first_image + B)
        ops.voc_match(rows, probs, nkept, conf_thresh, self.ovthresh, first_image, g.box[sl], g.cls[sl], g.difficult[sl],
                      g.count[sl], g.size[sl], self.keys, self.flags, self.counters)
        self._sorted = None

    def _run(self, want_curves):
        keys, order = torch.sort(self.keys)
        flags = self.flags[order]
        res = ops.voc_ap(keys, flags, self.counters, self.gt.npos, want_curves)
        self._sorted = (keys, flags)
        return res

    def finish(self):
        """(aps float64 ndarray [num_classes], mAP float) after one synchronisation."""
        ap = self._run(False)
        out = torch.cat((ap, self.counters.double())).cpu().numpy()       # the one copy
        aps, count, lost = out[:self.num_classes].copy(), int(out[-2]), int(out[-1])
        if lost:
            raise McamdError("DeviceVOCEval: %d detection records exceed the capacity of %d (%d lost); raise `capacity`"
                             % (count, self.capacity, lost))
        self.num_records = count
        return aps, float(np.mean(aps))

    def records(self):
        """(keys int64, flags uint8) of the records in sorted order, on the host (tests)."""
        if self._sorted is None:
            self._run(False)
        n = min(int(self.counters[0]), self.capacity)
        return self._sorted[0][:n].cpu().numpy(), self._sorted[1][:n].cpu().numpy()

    def curves(self, c):
        """(rec, prec) float64 ndarrays of class c, as voc_eval returns them (tests)."""
        _, rec, prec = self._run(True)
        keys = self.records()[0]
        lo, hi = np.searchsorted(keys, [c << ops.VOC_KEY_CLASS_SHIFT, (c + 1) << ops.VOC_KEY_CLASS_SHIFT])
        return rec[lo:hi].cpu().numpy(), prec[lo:hi].cpu().numpy()
