"""BatchNorm + LeakyReLU fused into the split-operand 1x1 forward behind it (mcamd_bn_act_conv1x1_fwd, csrc/bn_conv1x1.hip)
against the two launches it replaces, ops.bn_act_fwd + ops.conv_fwd_raw32, on the same inputs: the consumer's raw output y,
its statistics slab and the stored hi plane must be EQUAL bit for bit -- same MFMA instructions in the same K order, same
persistent slots, same epilogue, same conversion expressions.  No tolerance.

Inputs: fp32 y of the producer from a seeded normal, scaled so that some activations pass 65 504 (sat_half) and about half
are negative (both LeakyReLU sides); scale with a zero and a negative entry; slope 0.1.  The destination is prefilled with a
sentinel in the interior and in the lo plane and zeros in the halo: afterwards the halo is still zero and the lo plane
still the sentinel (the fused launch stores interior pixels of the hi plane only).

Shapes, the smallest at which each mechanism can fail: one ragged tile with one K block per part; conv4's channel form with
a full and a ragged tile and an image boundary inside a tile; conv7's form (512 threads, four K blocks per part); more M
tiles than persistent slots (a workgroup keeps its sums across two tiles); no statistics slab.  Refused pairs return an
error from the launch entry and launch nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops  # noqa: E402
from modelcompression_amd import _lib as L  # noqa: E402

SLOPE = 0.1
SENTINEL = 7.25


class Pair:
    """A PLAIN producer of P channels (raw fp32 output, coefficients) and the 1x1 consumer P -> cout behind it."""

    def __init__(self, dev, B, H, W, P, cout, seed=0):
        self.dev, self.B, self.H, self.W, self.P, self.cout = dev, B, H, W, P, cout
        self.M = B * H * W
        gen = torch.Generator().manual_seed(seed)
        # |y| <= 8e4, scale in [0.5, 1.5): some activations beyond the fp16 maximum (hi saturates), none beyond twice it (lo =
        # fp16(v - hi) stays finite); about half negative
        self.y = (torch.randn(self.M, P, generator=gen) * 3e4).clamp_(-8e4, 8e4).to(dev)
        scale = torch.rand(P, generator=gen) + 0.5
        scale[1], scale[P // 2] = 0.0, -0.75
        self.scale, self.shift = scale.to(dev), torch.randn(P, generator=gen).to(dev)
        self.ld = 2 * P                                  # hi | lo planes, P apart
        self.g = ops.geom(B, H, W, 1, 3 * P, cout, self.ld, 0, 0, 0, 2 * P)
        w = (torch.randn(cout, P, 1, 1, generator=gen) * 0.05).to(dev).contiguous()
        nf, _ = ops.packed_elems(self.g)
        self.wp = torch.zeros(nf, dtype=torch.float16, device=dev)
        table = ops.pack_table([dict(w=w, dst_fwd=self.wp, cout=cout, cin=P, ksize=1, split=1)], dev)
        ops.pack_many(*table)
        self._keep = (w, table)

    def act_args(self, dst):
        return ((self.B, self.H, self.W, self.P, self.y, self.P, 0, self.scale, self.shift, SLOPE, L.DST_PLAIN, dst, self.ld, 0),
                dict(planes=2, dst_plane=self.P, dst_pad=0))

    def act_geom(self, **over):
        kw = dict(planes=2, dst_plane=self.P, dst_pad=0)
        kw.update(over)
        return ops.act_geom(self.B, self.H, self.W, self.P, self.P, 0, SLOPE, L.DST_PLAIN, self.ld, 0, **kw)

    def dst(self):
        buf = ops.alloc_padded(self.B, self.H, self.W, self.ld, self.dev)
        ops.padded_view(buf, self.B, self.H, self.W, self.ld)[:, 1:-1, 1:-1, :] = SENTINEL
        return buf

    def outputs(self, stats, rows):
        y = torch.full((self.M, self.cout), float("nan"), device=self.dev)
        slab = torch.full((rows, 2, ops.round_up(self.cout, 256)), float("nan"), device=self.dev) if stats else None
        return y, slab

    def two_kernels(self, stats=True):
        dst = self.dst()
        a, kw = self.act_args(dst)
        ops.bn_act_fwd(*a, **kw)
        y, slab = self.outputs(stats, ops.stats_rows(self.g, L.EPI_RAW_F32))
        ops.conv_fwd_raw32(self.g, dst, self.wp, y, self.cout, 0, slab)
        return dst, y, slab

    def fused(self, stats=True):
        dst = self.dst()
        a, kw = self.act_args(dst)
        rows = ops.bn_act_conv1x1_stats_rows(self.act_geom(), self.g)
        assert rows > 0
        y, slab = self.outputs(stats, rows)
        ops.bn_act_conv1x1_fwd(a, kw, self.g, self.wp, y, self.cout, 0, slab)
        return dst, y, slab, rows


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_pair(p, stats=True):
    dst0, y0, slab0 = p.two_kernels(stats)
    dst1, y1, slab1, rows = p.fused(stats)
    torch.cuda.synchronize()
    B, H, W, P = p.B, p.H, p.W, p.P
    v0, v1 = (ops.padded_view(d, B, H, W, p.ld) for d in (dst0, dst1))
    hi0, hi1 = v0[:, 1:-1, 1:-1, :P], v1[:, 1:-1, 1:-1, :P]
    # the inputs exercise what they claim to
    assert (hi0.float().abs() == 65504).any() and (hi0 < 0).float().mean() > 0.3 and (hi0 > 0).float().mean() > 0.3
    assert torch.isfinite(y0).all()
    assert torch.equal(bits(hi0), bits(hi1)), "hi plane"
    assert torch.equal(bits(y0), bits(y1)), "raw output: max |d| %g" % (y0 - y1).abs().max().item()
    if stats:
        assert slab0.shape[0] == rows
        assert torch.equal(bits(slab0[:, :, :p.cout]), bits(slab1[:, :, :p.cout])), "statistics slab"
        assert torch.isfinite(slab1[:, :, :p.cout]).all()
    # only interior pixels of the hi plane were written
    assert (v1[:, 1:-1, 1:-1, P:] == SENTINEL).all(), "lo plane touched"
    halo = v1.clone()
    halo[:, 1:-1, 1:-1, :] = 0
    assert (halo == 0).all(), "halo touched"
    return rows


@pytest.mark.parametrize("B,H,W,P,cout", [
    (1, 3, 5, 64, 64),        # one ragged tile (M = 15), one K block per part
    (2, 9, 8, 128, 64),       # conv4's channel form, M = 144: a full tile + a ragged one, an image boundary inside a tile
    (3, 7, 7, 256, 128),      # conv7's form, M = 147
], ids=["m15-64to64", "m144-128to64", "m147-256to128"])
def test_fused_equals_two_kernels(dev, B, H, W, P, cout):
    p = Pair(dev, B, H, W, P, cout)
    assert ops.bn_act_conv1x1_ok(p.act_geom(), p.g)
    check_pair(p)


def test_persistent_workgroup_takes_two_tiles(dev):
    """More M tiles than statistics rows: a workgroup keeps its partial sums across the tiles of its slot."""
    P, cout = 128, 64
    probe = ops.geom(1, 512, 512, 1, 3 * P, cout, 2 * P, 0, 0, 0, 2 * P)
    d = ops.act_geom(1, 512, 512, P, P, 0, SLOPE, L.DST_PLAIN, 2 * P, 0, planes=2, dst_plane=P, dst_pad=0)
    cap = ops.bn_act_conv1x1_stats_rows(d, probe)           # the row count saturates at the launch's slot target
    W = (128 * cap) // 512 + 1                              # the smallest 512-row image above 128 x rows pixels
    p = Pair(dev, 1, 512, W, P, cout)
    rows = check_pair(p)
    assert rows == cap and p.M > 128 * rows


def test_no_statistics_slab(dev):
    check_pair(Pair(dev, 2, 9, 8, 128, 64), stats=False)


def test_refusals(dev):
    """Cout beyond one column tile, Cin no multiple of 64, a shared-halo destination, an x_f8 consumer: refused by the
    predicate; the launch entry returns an error (nothing is launched: the outputs keep their prefill)."""
    p = Pair(dev, 2, 9, 8, 128, 64)
    B, H, W, P = p.B, p.H, p.W, p.P
    cases = {
        "cout256": (p.act_geom(), ops.geom(B, H, W, 1, 3 * P, 256, 2 * P, 0, 0, 0, 2 * P)),
        "cin96": (ops.act_geom(B, H, W, 96, 96, 0, SLOPE, L.DST_PLAIN, 192, 0, planes=2, dst_plane=96, dst_pad=0),
                  ops.geom(B, H, W, 1, 288, 64, 192, 0, 0, 0, 192)),
        "shared-halo": (p.act_geom(dst_pad=1), ops.geom(B, H, W, 1, 3 * P, 64, 2 * P, 0, 0, 1, 2 * P)),
        "x_f8": (p.act_geom(planes=4), ops.geom(B, H, W, 1, 2 * P, 64, 2 * P, 0, 0, 0, 0, x_f8=P)),
    }
    for name, (d, g) in cases.items():
        assert not ops.bn_act_conv1x1_ok(d, g), name
        assert ops.bn_act_conv1x1_stats_rows(d, g) == 0, name
    # the launch entry refuses too: descriptors with real pointers, geometry of each refused case
    y = torch.full((p.M, 256), -3.0, device=dev)
    for name, (_, g) in cases.items():
        dst = p.dst()
        a, kw = p.act_args(dst)
        if name == "shared-halo":
            kw = dict(kw, dst_pad=1)
        with pytest.raises(L.McamdError):
            ops.bn_act_conv1x1_fwd(a, kw, g, p.wp, y, 256, 0, None)
        torch.cuda.synchronize()
        assert (y == -3.0).all() and (ops.padded_view(dst, B, H, W, p.ld)[:, 1:-1, 1:-1, :] == SENTINEL).all(), name
