"""Minimal data sources for the train / predict entry points.

The reference's data pipeline (src/dataloader.py: PIL/cv2/torchvision augmentation) is outside
the hot path; these are just enough to drive it:
  * VOCList     -- images listed in a darknet-style list file, labels from the sibling
                   `labels/*.txt` files (cls x y w h, normalised), resized to the network input
                   with PIL only, target = 50 x 5 floats as dataloader.py:83-96 builds it;
  * SyntheticDetection -- seeded random images/boxes of the same shapes (benchmarks, smoke runs,
                   and whenever VOC is not on disk);
  * VOCAugment  -- the reference's VOCDatasetv2(train=True) (dataloader.py:68-75): decode, labels and the
                   augmentation parameters only; the pixels are augmented on the device (augment.py), batches
                   come from augment.collate_fn(shape) and go through augment.DeviceAugmenter;
  * SyntheticAugment -- seeded varied-size uint8 sources with boxes for the same path, without VOC;
  * ResidentImages -- every picture of a list decoded ONCE into one device uint8 buffer; ResidentAugment and
                   ResidentList are VOCAugment and VOCList over it: their items carry an index, never pixels, their
                   `collate` packs descriptors only (augment.pack_resident) and augment.DeviceAugmenter(resident=...)
                   resamples straight from the buffer, so the loader needs no worker processes.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from .augment import draw_params, pack_resident, resize_params, sample_rng, synthetic_source, transform_labels

MAX_BOXES = 50


def label_path_for(imgpath):
    p = imgpath.replace('images', 'labels').replace('JPEGImages', 'labels')
    return os.path.splitext(p)[0] + '.txt'


class VOCList(Dataset):
    def __init__(self, listfile, shape=(416, 416), train=True):
        with open(listfile) as f:
            self.lines = [l.strip() for l in f if l.strip()]
        self.shape, self.train = shape, train

    def __len__(self):
        return len(self.lines)

    def __getitem__(self, i):
        from PIL import Image
        path = self.lines[i]
        img = Image.open(path).convert('RGB').resize(self.shape)
        x = torch.from_numpy(np.asarray(img, dtype=np.float32).transpose(2, 0, 1) / 255.0)
        target = torch.zeros(MAX_BOXES * 5)
        lp = label_path_for(path)
        if os.path.exists(lp) and os.path.getsize(lp):
            lab = np.loadtxt(lp).reshape(-1, 5)[:MAX_BOXES]
            target[:lab.size] = torch.from_numpy(lab.astype(np.float32).reshape(-1))
        return x, target


class SyntheticDetection(Dataset):
    def __init__(self, n, shape=(416, 416), seed=0, num_classes=20):
        self.n, self.shape, self.seed, self.nc = n, shape, seed, num_classes

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        x = torch.rand(3, self.shape[1], self.shape[0], generator=g)
        nb = int(torch.randint(1, 6, (1,), generator=g))
        target = torch.zeros(MAX_BOXES * 5)
        for b in range(nb):
            wh = torch.rand(2, generator=g) * 0.4 + 0.05
            xy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
            target[b * 5:(b + 1) * 5] = torch.tensor([float(torch.randint(0, self.nc, (1,), generator=g)), xy[0], xy[1], wh[0], wh[1]])
        return x, target


def read_boxes(lp):
    """cls x y w h rows of a label file as float64 [n][5] (empty when the file is missing or empty)."""
    if os.path.exists(lp) and os.path.getsize(lp):
        return np.loadtxt(lp).reshape(-1, 5)
    return np.zeros((0, 5))


class _AugmentSource(Dataset):
    """Items (uint8 [h][w][3] source, float64 [n][5] boxes, augment.AugParams); the parameters are drawn from a
    generator seeded by (seed, epoch, index), so a batch does not depend on the worker count or the world size."""
    epoch = 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _item(self, i, src, boxes):
        return src, boxes, draw_params(sample_rng(self.seed, self.epoch, i), src.shape[1], src.shape[0])


class VOCAugment(_AugmentSource):
    def __init__(self, listfile, shape=(416, 416), seed=0):
        with open(listfile) as f:
            self.lines = [l.strip() for l in f if l.strip()]
        self.shape, self.seed = tuple(shape), seed

    def __len__(self):
        return len(self.lines)

    def __getitem__(self, i):
        from PIL import Image
        path = self.lines[i]
        src = np.asarray(Image.open(path).convert('RGB'))
        return self._item(i, src, read_boxes(label_path_for(path)))


class SyntheticAugment(_AugmentSource):
    def __init__(self, n, shape=(416, 416), seed=0, num_classes=20):
        self.n, self.shape, self.seed, self.nc = n, tuple(shape), seed, num_classes

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = np.random.default_rng([self.seed, i])
        w, h = (int(v) for v in g.integers(160, 640, 2))
        nb = int(g.integers(1, 6))
        wh = g.random((nb, 2)) * 0.4 + 0.05
        xy = g.random((nb, 2)) * (1 - wh) + wh / 2
        boxes = np.concatenate([g.integers(0, self.nc, (nb, 1)).astype(np.float64), xy, wh], 1)
        return self._item(i, synthetic_source(w, h, self.seed * 1000003 + i), boxes)


def _decode(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def _size(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


class ResidentImages:
    """The decoded pictures of `paths` in ONE uint8 buffer on `device`: HWC, rows of w * 3 bytes, picture i at byte
    `offsets[i]` (16-byte aligned), `sizes[i]` = (h, w); `offsets` (int64) and `sizes` stay on the host.  Each file is
    decoded once, as VOCList / VOCAugment decode it, by `num_workers` threads (at most 16; 0: the calling thread), and
    copied in chunks of CHUNK_BYTES through two pinned staging buffers, so the host never holds the whole set."""
    CHUNK_BYTES = 64 << 20

    def __init__(self, paths, device, num_workers=4):
        self.paths = list(paths)
        workers = max(0, min(int(num_workers), 16))
        if workers:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(workers) as pool:
                self._build(list(pool.map(_size, self.paths)), lambda idx: pool.map(_decode, [self.paths[i] for i in idx]),
                            device)
        else:
            self._build([_size(p) for p in self.paths], lambda idx: (_decode(self.paths[i]) for i in idx), device)

    @classmethod
    def from_sources(cls, sources, device):
        """The same buffer from uint8 [h][w][3] arrays (tests, the synthetic sets)."""
        self = cls.__new__(cls)
        self.paths = None
        for i, s in enumerate(sources):
            if s.dtype != np.uint8 or s.ndim != 3 or s.shape[2] != 3:
                raise ValueError("ResidentImages: source %d is %s %s, not uint8 [h][w][3]" % (i, s.dtype, s.shape))
        self._build([s.shape[:2] for s in sources], lambda idx: (sources[i] for i in idx), device)
        return self

    def _build(self, sizes, fetch, device):
        """sizes: (h, w) per picture; fetch(indices) -> their uint8 [h][w][3] arrays, in order."""
        self.device = torch.device(device)
        self.sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        n = len(self.sizes)
        padded = (self.sizes[:, 0] * self.sizes[:, 1] * 3 + 15) // 16 * 16
        ends = np.cumsum(padded)
        self.offsets = (ends - padded).astype(np.int64)
        self.nbytes = int(ends[-1]) if n else 0
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)
        on_gpu = self.device.type == "cuda"
        chunk = max(self.CHUNK_BYTES, int(padded.max()) if n else 0)
        staging = [torch.zeros(min(chunk, self.nbytes), dtype=torch.uint8) for _ in range(2 if on_gpu else 1)]
        if on_gpu:
            staging = [t.pin_memory() for t in staging]
        events = [None, None]
        lo, turn = 0, 0
        while lo < n:
            hi = lo + 1                                  # pictures [lo, hi): as many as the staging buffer holds
            while hi < n and ends[hi] - self.offsets[lo] <= chunk:
                hi += 1
            base, size = int(self.offsets[lo]), int(ends[hi - 1] - self.offsets[lo])
            if events[turn] is not None:
                events[turn].synchronize()               # the copy that last read this staging buffer
            stage = staging[turn].numpy()
            for i, img in zip(range(lo, hi), fetch(range(lo, hi))):
                if img.shape != (self.sizes[i, 0], self.sizes[i, 1], 3) or img.dtype != np.uint8:
                    raise ValueError("ResidentImages: picture %d decodes to %s %s, its header says %s"
                                     % (i, img.dtype, img.shape, tuple(self.sizes[i])))
                o = int(self.offsets[i]) - base
                stage[o:o + img.size] = img.reshape(-1)
                stage[o + img.size:o + int(padded[i])] = 0     # the padding up to the next picture
            self.buf[base:base + size].copy_(staging[turn][:size], non_blocking=on_gpu)
            if on_gpu:
                events[turn] = torch.cuda.Event()
                events[turn].record()
                turn ^= 1
            lo = hi
        if on_gpu:
            torch.cuda.current_stream(self.device).synchronize()

    def __len__(self):
        return len(self.sizes)

    def source(self, i):
        """Picture i as a uint8 [h][w][3] array on the host (a copy)."""
        h, w = (int(v) for v in self.sizes[i])
        o = int(self.offsets[i])
        return self.buf[o:o + h * w * 3].cpu().numpy().reshape(h, w, 3)


def read_targets(label_paths):
    """VOCList's target of every label file: float32 [n][250], the first 50 rows of the file, zero-filled."""
    targets = torch.zeros(len(label_paths), MAX_BOXES * 5)
    for i, lp in enumerate(label_paths):
        if os.path.exists(lp) and os.path.getsize(lp):
            lab = np.loadtxt(lp).reshape(-1, 5)[:MAX_BOXES]
            targets[i, :lab.size] = torch.from_numpy(lab.astype(np.float32).reshape(-1))
    return targets


class _ResidentSet(Dataset):
    """Keeps the host tables of a ResidentImages only (never the device buffer: the set may be handed to loader
    workers).  Batches come from collate_fn=self.collate and go through augment.DeviceAugmenter(shape, device, resident)."""

    def __init__(self, resident, shape):
        self.offsets, self.sizes, self.nbytes, self.shape = resident.offsets, resident.sizes, resident.nbytes, tuple(shape)

    def __len__(self):
        return len(self.sizes)


class ResidentAugment(_ResidentSet):
    """VOCAugment without the pixels: items (index, boxes, AugParams) with the same per-(seed, epoch, index) draws;
    `boxes` holds the float64 [n][5] rows of every picture (read_boxes of its label file)."""
    epoch = 0

    def __init__(self, resident, boxes, shape=(416, 416), seed=0):
        super().__init__(resident, shape)
        if len(boxes) != len(resident):
            raise ValueError("ResidentAugment: %d box lists for %d pictures" % (len(boxes), len(resident)))
        self.boxes, self.seed = list(boxes), seed

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __getitem__(self, i):
        h, w = (int(v) for v in self.sizes[i])
        return i, self.boxes[i], draw_params(sample_rng(self.seed, self.epoch, i), w, h)

    def collate(self, items):
        targets = torch.stack([transform_labels(boxes, p) for _, boxes, p in items])
        return pack_resident(self, [i for i, _, _ in items], [p for _, _, p in items], self.shape, targets)


class ResidentList(_ResidentSet):
    """VOCList without the pixels: items (index, target), the raw 50 x 5 target of the label file; the batch is resized
    on the device with no crop, flip or distortion (Image.resize + /255, bit for bit).  `label_paths` may also be a
    float32 [n][250] tensor of targets (the synthetic sets have no files)."""

    def __init__(self, resident, label_paths, shape=(416, 416)):
        super().__init__(resident, shape)
        self.targets = label_paths if torch.is_tensor(label_paths) else read_targets(label_paths)
        if len(self.targets) != len(resident):
            raise ValueError("ResidentList: %d targets for %d pictures" % (len(self.targets), len(resident)))

    def __getitem__(self, i):
        return i, self.targets[i]

    def collate(self, items):
        idx = [i for i, _ in items]
        params = [resize_params(int(self.sizes[i, 1]), int(self.sizes[i, 0])) for i in idx]
        return pack_resident(self, idx, params, self.shape, torch.stack([t for _, t in items]), distort=False)
