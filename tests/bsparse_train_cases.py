"""The cases of tests/test_bsparse_train_instances_gpu.py: launches of mcamd_conv_fwd_bsparse_raw (with and without the
BatchNorm statistics), mcamd_conv_dgrad_bsparse and mcamd_bsparse_lists_dgrad (csrc/conv_bsparse.hip: bsparse_kernel<64 |
128, 64, 3, MCAMD_EPI_RAW_F16> and <64 | 128, 32, 4, MCAMD_EPI_RAW_F16>), their operands, masks and exact references.

Both directions are one implicit GEMM with N output columns and K-side channels `kreal` (padded to `kpad`): the forward has
N = cout over cin, the dgrad N = cin over cout_p with the taps flipped.  Weights and masks are therefore drawn in GEMM
("view") coordinates [N][kpad][k][k] with bsparse_cases.build_mask -- the mask kinds and the per-tile list lengths mean the
same thing in either direction -- and turned into the OIHW tensors the library packs.  The references are
conv_cases.reference for "fwd-raw16-stats" / "fwd-raw16" / "dgrad-raw16" and must meet conv_cases.exactness;
test_bsparse_train_cases_cpu.py proves the coverage on the CPU.  Test-side only."""
import collections
import zlib

import numpy as np
import torch

from modelcompression_amd import ops
import bsparse_cases as BC
import bsparse_ref as R
import conv_cases as CC
from bsparse_cases import ALL, RANDOM, BM_ENV, MASK_KINDS, ring_lengths  # noqa: F401
from conv_cases import DRAWS, _draw, exactness, Operands  # noqa: F401

INSTANCES = BC.INSTANCES                          # (bm, bk, stages) of bsparse_kernel<BM, BK, NSTAGE, MCAMD_EPI_RAW_F16>
FORMS = ("fwd-stats", "fwd", "dgrad")             # forward with statistics, forward without, dgrad
_EPI = {"fwd-stats": "fwd-raw16-stats", "fwd": "fwd-raw16", "dgrad": "dgrad-raw16"}
SAT_ROW = 5                                       # the output channel of the planted overflow
SAT_W, SAT_POS, SAT_NEG = 32.0, 64.0, -256.0      # 64 channels or more: 64 * 32 * 64 = 131072; 64 * 32 * -256 = -524288

SAT_W_STATS, SAT_CH_STATS = 128.0, 32             # stats_saturate_case: 32 channels * 128 * +-64 = +-262144 (+ 128 * the rest)

_FIELDS = "name form B H W k cin cout pad ld choff y_ld y_choff bm mask counts overflow draw wdraw expect"
_View = collections.namedtuple("_View", "cout cin k ntiles nchunks kb mask counts ntaps")


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch on the device's lists (and one with all_chunks).  form: FORMS.  ld / choff: the operand slice (x forward,
    dy dgrad; ld 0: the whole buffer); y_ld / y_choff: the output slice of [M][y_ld].  pad: the form of the operand.  bm:
    the setting of MCAMD_BSPARSE_BM.  mask / counts: bsparse_cases.Case's, over the tiles and chunks of THIS GEMM.
    (epi, fwd, n, M, k_tap, ktot, stem, concurrent: what conv_cases.reference / exactness read.)"""
    __slots__ = ()
    stem, concurrent, dst = 0, False, "plain"

    def __str__(self):
        return self.name

    @property
    def base(self):
        return self.name.split(".")[0]

    @property
    def epi(self):
        return _EPI[self.form]

    @property
    def fwd(self):
        return self.form != "dgrad"

    @property
    def dgrad(self):
        return self.form == "dgrad"

    @property
    def stats(self):
        return self.form == "fwd-stats"

    @property
    def n(self):
        return self.cout if self.fwd else self.cin

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def kreal(self):
        return self.cin if self.fwd else self.cout

    @property
    def kpad(self):
        return ops.round_up(self.kreal, 32)

    k_tap = kpad

    @property
    def kb(self):
        return R.block_kb(self.kpad)

    @property
    def ntaps(self):
        return self.k * self.k

    @property
    def ktot(self):
        return self.ntaps * self.kpad

    @property
    def nchunks(self):
        return self.ktot // self.kb

    @property
    def ntiles(self):
        return -(-self.n // R.FILTERS)

    @property
    def view(self):
        return _View(self.n, self.kpad, self.k, self.ntiles, self.nchunks, self.kb, self.mask, self.counts, self.ntaps)


def case(name, form, B, H, W, k, cin, cout, bm, mask="block", counts=(), pad=0, choff=0, y_choff=0, overflow=False, draw="d1",
         wdraw=None):
    assert form in FORMS and mask in MASK_KINDS and cin % 32 == 0 and cout % 8 == 0
    fwd = form != "dgrad"
    n, kpad = (cout, cin) if fwd else (cin, ops.round_up(cout, 32))
    ld = ops.round_up(choff + kpad + 8, 32) if choff else 0
    y_ld = ops.round_up(y_choff + n + 8, 32) if y_choff else 0
    kb = R.block_kb(kpad)
    assert mask != "block" or len(counts) == -(-n // R.FILTERS), name
    return Case("%s.m%d" % (name, bm), form, B, H, W, k, cin, cout, pad, ld, choff, y_ld, y_choff, bm, mask, tuple(counts), overflow,
                draw, wdraw or draw, (bm, kb, 3 if kb == 64 else 4))


def geom_of(c):
    if c.fwd:
        return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.ld or c.cin, c.choff, pad=c.pad)
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.cin, 0, pad=c.pad)        # (x_ld: unused by dgrad)


def apply_env(c, setenv):
    setenv(BM_ENV, str(c.bm))


def info_of(c):
    return ops.conv_bsparse_train_info(geom_of(c), c.dgrad)


# ---------------------------------------------------------------------------------------------------------------------
# the dgrad packing and its lists, restated in numpy
# ---------------------------------------------------------------------------------------------------------------------
def pack_dgrad(w, mask=None):
    """fp16 [round_up(cin, 256)][khw * cout_p] dgrad packing of an OIHW tensor (include/mcamd.h): row c, column kpos(t, n) =
    (n / kb) * khw * kb + t * kb + n % kb over cout_p = round_up(cout, 32) holds w[n][c][k-1-ty][k-1-tx], t = ty * k + tx."""
    cout, cin = w.shape[:2]
    v = np.asarray(w, np.float32).reshape(cout, cin, -1)
    if mask is not None:
        v = v * np.asarray(mask, np.float32).reshape(v.shape)
    khw, cp = v.shape[2], (cout + 31) // 32 * 32
    kb = R.block_kb(cp)
    d = np.zeros((cin, cp, khw), np.float32)
    d[:, :cout] = v[:, :, ::-1].transpose(1, 0, 2)             # flipped tap: (k-1-ty) * k + (k-1-tx) = khw - 1 - t
    out = np.zeros(((cin + 255) // 256 * 256, khw * cp), np.float16)
    out[:cin] = d.reshape(cin, cp // kb, kb, khw).transpose(0, 1, 3, 2).reshape(cin, khw * cp).astype(np.float16)
    return out


def lists_ref(c, o):
    """(packed fp16, count, list): bsparse_ref.chunk_lists on the numpy packing of the direction"""
    packed = R.pack_fwd(o.w.numpy(), o.mask.numpy()) if c.fwd else pack_dgrad(o.w.numpy(), o.mask.numpy())
    return (packed,) + R.chunk_lists(packed, c.n, c.kb)


# ---------------------------------------------------------------------------------------------------------------------
# operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
def from_view(c, t):
    """[N][kpad][k][k] in GEMM coordinates -> the OIHW tensor: itself forward; dgrad: w[n][c][ty][tx] = view[c][n][k-1-ty][k-1-tx]"""
    t = t[:, :c.kreal]
    return t.contiguous() if c.fwd else t.permute(1, 0, 2, 3).flip(2, 3).contiguous()


def operands(c, gaussian=False, plant=True):
    """conv_cases.Operands: act = x [B][cin][H][W] forward, dy [B][cout][H][W] dgrad; w, mask OIHW; planted [(b, channel, h, w,
    sign)] of an `overflow` case."""
    gen = torch.Generator().manual_seed(zlib.crc32(c.base.encode()))
    if gaussian:
        act = torch.randn(c.B, c.kreal, c.H, c.W, generator=gen)
        wv = torch.randn(c.n, c.kpad, c.k, c.k, generator=gen) * (4.0 / c.ktot) ** 0.5
        wv = wv + 0.5 * torch.sign(wv)
    else:
        act = _draw(gen, DRAWS[c.draw], (c.B, c.kreal, c.H, c.W))
        wv = _draw(gen, DRAWS[c.wdraw], (c.n, c.kpad, c.k, c.k))
        wv[wv == 0] = 1.0                                      # every kept weight counts
    mv, wv = BC.build_mask(c.view, gen, wv)
    planted = []
    if c.overflow and not gaussian:
        assert c.k == 1 and c.kreal >= 64 and c.mask == "block" and c.counts[0] == ALL
        # (with statistics: a heavier filter on a few planted channels, so that the other filters' sums of y^2 stay small)
        wv[SAT_ROW] = SAT_W_STATS if c.stats else SAT_W
        chans = slice(0, SAT_CH_STATS) if c.stats else slice(None)
        if plant:
            if c.stats:                     # (nothing else at the planted pixels: every filter's value there is a multiple of 64)
                act[0, :, 1, 2] = 0.0
                act[c.B - 1, :, c.H - 1, c.W - 2] = 0.0
            act[0, chans, 1, 2] = SAT_POS
            if c.stats:                     # (half as many channels again: the two accumulators do not cancel in the sum)
                act[c.B - 1, :SAT_CH_STATS * 3 // 2, c.H - 1, c.W - 2] = -SAT_POS
            else:
                act[c.B - 1, :, c.H - 1, c.W - 2] = SAT_NEG
            planted = [(0, SAT_ROW, 1, 2, 1.0), (c.B - 1, SAT_ROW, c.H - 1, c.W - 2, -1.0)]
    return Operands(act, from_view(c, wv), from_view(c, mv), None, None, None, planted)


_CACHE = {}


def operands_and_reference(c, plant=True):
    """Once per process and case; shared by the tests and never modified."""
    key = (c.name, plant)
    if key not in _CACHE:
        o = operands(c, plant=plant)
        _CACHE[key] = (o, CC.reference(c, o))
    return _CACHE[key]


def stats_reference(ref):
    """(sum y, sum y^2) per channel over all pixels, from the values AS STORED (fp16, clamped where the case saturates): what
    mcamd_conv_fwd's "fwd-raw16-stats" epilogue sums.  Without clamping it is conv_cases.reference's s1 / s2."""
    return ref.y.sum((0, 2, 3)), (ref.y * ref.y).sum((0, 2, 3))


def stats_saturate_case(inst):
    """A forward WITH statistics that clamps two elements of channel SAT_ROW: sums of the stored values (+-65504) and sums
    of the accumulators (262144 / -1048576 and the like) differ there, so the convention is visible.  Not one of TRAIN_CASES:
    condition 3 of conv_cases.exactness cannot hold for that channel (65504^2 > 2^24); stats_saturate_exactness() states
    what holds in its place."""
    bm, bk, _ = inst
    return case("stats-saturate-k%d" % bk, "fwd-stats", 2, 13, 13, 1, 128 if bk == 64 else 96, 72, bm, counts=(ALL, RANDOM),
                overflow=True, draw="d3")


def stats_saturate_exactness(c, o, ref):
    """Violations of: conditions 1 and 2 of conv_cases.exactness; condition 3 for every channel but SAT_ROW, on the stored
    values; and for SAT_ROW: every stored value is a multiple of 32 (the filter is 128 everywhere, 65504 = 32 * 2047), so every y^2 -- 65504^2 =
    2^10 (2^22 - 2^12 + 1) included -- is a multiple of 1024, and sum |y| / 32 and sum y^2 / 1024 over all pixels are below
    2^24: every partial sum in every order is a multiple of the unit with fewer than 24 bits, an exact fp32 number."""
    s1, s2 = stats_reference(ref)
    others = s2.clone()
    others[SAT_ROW] = 0
    bad = CC.exactness(c, o, ref._replace(s1=s1, s2=others))
    y = ref.y[:, SAT_ROW]
    if not bool((y % 32 == 0).all()):
        bad.append("the saturated channel holds values that are no multiples of 32")
    if not (float(y.abs().sum()) / 32 < 2 ** 24 and float(s2[SAT_ROW]) / 1024 < 2 ** 24):
        bad.append("the saturated channel's sums exceed 24 bits of their unit")
    if not (float(s1[SAT_ROW]) != float(ref.acc[:, SAT_ROW].sum()) and float(s2[SAT_ROW]) != float((ref.acc[:, SAT_ROW] ** 2).sum())):
        bad.append("stored values and accumulators have the same sums: the convention is not visible")
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the cases: the same rows on the 64-row and on the 128-row M tile, for K chunks of 64 and of 32, in every form
# ---------------------------------------------------------------------------------------------------------------------
_LENGTHS = (0, 1, 2, 3, 4, 5, ALL)


def _rows(form, bk, bm):
    """Forward: N = cout in {136, 72, 40, 64} over cin (64 / 128: chunks of 64; 96 / 32: chunks of 32).  dgrad: N = cin in {128,
    96, 32, 64} over cout (64 / 40 -> cout_p 64: chunks of 64; 72 / 136 -> cout_p 96 / 160: chunks of 32)."""
    fwd = form != "dgrad"
    tag = "%s-k%d" % (form, bk)

    def mk(name, B, H, W, k, n, kreal, **kw):
        cin, cout = (kreal, n) if fwd else (n, kreal)
        return case("%s-%s" % (tag, name), form, B, H, W, k, cin, cout, bm, **kw)

    big = 136 if fwd else 128                    # 3 / 2 tiles, the last one ragged forward
    nt = -(-big // 64)
    k3 = (64 if bk == 64 else 96) if fwd else (64 if bk == 64 else 72)          # K-side channels of the 3x3 rows
    k3b = k3 if fwd else (40 if bk == 64 else 136)                             # ... with a ragged cout_p in the dgrad
    k1 = (128 if bk == 64 else 96) if fwd else (64 if bk == 64 else 72)
    L = _LENGTHS + (RANDOM, ALL)
    rows = [
        mk("len0", 2, 13, 13, 3, big, k3, counts=L[0:nt], pad=1, y_choff=8, draw="d2"),
        mk("len1", 2, 8, 8, 3, big, k3b, counts=L[nt:2 * nt], choff=32, draw="d2"),
        mk("len2", 2, 13, 13, 3, big, k3, counts=L[2 * nt:3 * nt], draw="d2"),
        mk("len3", 2, 8, 8, 3, big, k3, counts=(L[6:9] if fwd else L[6:8]), pad=1, y_choff=16, choff=32),
        mk("unstructured", 2, 13, 13, 1, 72 if fwd else 96, k1, mask="unstructured", pad=1, draw="d3"),
        mk("negzero", 2, 8, 8, 3, 40 if fwd else 32, k3b, mask="negzero", draw="d3"),
        mk("single", 2, 8, 8, 3, 64, k3, mask="single", pad=1, draw="d3"),
    ]
    if form != "fwd-stats":                      # (the statistics reference is taken from unclamped values)
        rows.append(mk("saturate", 2, 13, 13, 1, 72 if fwd else 96, k1, counts=(ALL, RANDOM), overflow=True, draw="d3"))
    if form == "fwd":                            # the launch without statistics: the 1x1 rows and one list-length row
        rows = [r for r in rows if r.base.split("-")[-1] in ("len2", "unstructured", "saturate")]
    return rows


TRAIN_CASES = [c for form in FORMS for bk in (64, 32) for bm in (64, 128) for c in _rows(form, bk, bm)]


def foreign_case(form, inst):
    """the launch of the foreign-list test on an instance: one tile, 3x3 taps (9 chunks of 64 or 27 of 32)"""
    bm, bk, _ = inst
    kreal = (64 if bk == 64 else 96) if form != "dgrad" else (64 if bk == 64 else 72)
    cin, cout = (kreal, 64) if form != "dgrad" else (64, kreal)
    return case("foreign-%s-k%d" % (form, bk), form, 1, 6, 6, 3, cin, cout, bm, "unstructured", draw="d3")
