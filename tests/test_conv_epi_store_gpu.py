"""The store every forward implicit-GEMM kernel shares (csrc/conv_epi.h: store_pad_tile) writes its slice and nothing else.

The other kernel tests compare halo and out-of-slice channels with zero in zero-allocated buffers, which a stray store of
zeros passes.  Here every destination -- halo, guard bands and all channels -- is filled with a non-zero sentinel before
the launch; afterwards (a) every element outside the interior pixels x [choff, choff + cdst) still holds the sentinel and
(b) the slice is bit-equal to the same launch into a zero-initialised buffer.  No tolerance: the values themselves are
checked by test_kernels_gpu.py, test_sparse_kernels_gpu.py and test_q8_kernels_gpu.py.

Shapes: B=2, H=6, W=10 -- M = 120 is less than one 128-row tile, so the tile is ragged in M and the pooled test
4 * idx < M matters -- with 72 and 264 filters (a ragged last channel tile against the 32-, 64-, 128- and 256-wide
tiles), 1x1 and 3x3, every destination form, a channel offset inside a wider destination; and one dense shape that takes
the ping-pong tile."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops, _lib as L  # noqa: E402
from util import to_padded  # noqa: E402

B, H, W, CIN = 2, 6, 10, 64
OFF, OFF2 = 8, 32                   # channel offsets of the slices in y and y2
SENT16, SENT8 = 7.0, 0x5a           # fp16 7.0; a non-zero e4m3 code
DSTS = ["plain", "pool", "pool+y2", "reorg"]
ROUTE_PP = ops.ROUTE_PP              # mcamd_conv_route_info: the ping-pong kernel


def whole(buf):
    """The buffer with the guard bands in front of and behind it: everything a stray store could reach."""
    return torch.empty(0, dtype=buf.dtype, device=buf.device).set_(buf.untyped_storage())


@functools.lru_cache(maxsize=None)
def operands(dev, entry, b, h, w, cin, cout, k):
    """Input, packed weights and epilogue coefficients of one (entry point, shape): shared by its destination forms."""
    gen = torch.Generator().manual_seed(cin + cout + k)
    wt = (torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5).to(dev).contiguous()
    coef = ((torch.rand(cout, generator=gen) + 0.5).to(dev), (torch.randn(cout, generator=gen) * 0.2).to(dev))
    ld = ops.round_up(cin, 32)
    g = ops.geom(b, h, w, k, cin, cout, ld)
    if entry == "q8":
        assert ops.conv_fwd_q8_ok(g)
        # e4m3 codes of |x| < 4 with either sign, halo 0x00
        codes = torch.randint(0, 0x48, (b, h, w, cin), generator=gen) | (torch.randint(0, 2, (b, h, w, cin), generator=gen) << 7)
        x = ops.alloc_padded_q8(b, h, w, ld, dev)
        x.view(b, h + 2, w + 2, ld)[:, 1:-1, 1:-1, :cin] = codes.to(torch.uint8).to(dev)
        return g, x, ops.pack_q8(g, wt), coef
    x, _ = to_padded(torch.randn(b, cin, h, w, generator=gen).to(dev))
    if entry == "sparse24":
        assert ops.conv_fwd_sparse24_ok(g)
        # a valid 2:4 mask: two of every four consecutive input channels, rotating with the filter
        keep = (torch.arange(cin).view(1, cin) + torch.arange(cout).view(cout, 1)) % 4 < 2
        mask = keep.view(cout, cin, 1, 1).expand(cout, cin, k, k).float().contiguous().to(dev)
        return g, x, ops.pack_sparse24(g, wt, mask), coef
    return g, x, (ops.pack_weights(g, wt, None, True, False)[0],), coef


def launch(dev, entry, shape, cout, k, dst, f8, f8_2, fill):
    """One launch into destinations filled with `fill` (True: the sentinel, False: zero).
    Returns [(buffer, is_bytes, pixels (b, h, w), ld, choff, channels)] for y and, when present, y2."""
    b, h, w, cin = shape
    g, x, packed, (scale, shift) = operands(dev, entry, b, h, w, cin, cout, k)
    mode = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "pool+y2": L.DST_POOL, "reorg": L.DST_REORG}[dst]
    ho, wo = (h, w) if dst == "plain" else (h // 2, w // 2)
    cdst = 4 * cout if dst == "reorg" else cout
    ld, ld2 = ops.round_up(OFF + cdst + 8, 32), ops.round_up(OFF2 + cout + 8, 32)

    def alloc(bytes_, hh, ww, ld_):
        buf = ops.alloc_padded_q8(b, hh, ww, ld_, dev) if bytes_ else ops.alloc_padded(b, hh, ww, ld_, dev)
        if fill:
            whole(buf).fill_(SENT8 if bytes_ else SENT16)
        return buf

    y = alloc(f8, ho, wo, ld)
    y2 = alloc(f8_2, h, w, ld2) if dst == "pool+y2" else None
    kw = dict(dst_mode=mode, y2=y2, y2_ld=ld2 if y2 is not None else 0, y2_choff=OFF2 if y2 is not None else 0)
    if entry == "q8":
        ops.conv_fwd_q8(g, x, packed[0], packed[1], y, ld, OFF, scale, shift, 0.1, y_f8=f8, y2_f8=f8_2, **kw)
    elif entry == "sparse24":
        ops.conv_fwd_sparse24(g, x, packed[0], packed[1], y, ld, OFF, scale, shift, 0.1, **kw)
    else:
        ops.conv_fwd_padded(g, x, packed[0], y, ld, OFF, scale, shift, 0.1, **kw)
    torch.cuda.synchronize()
    out = [(y, f8, (b, ho, wo), ld, OFF, cdst)]
    if y2 is not None:
        out.append((y2, f8_2, (b, h, w), ld2, OFF2, cout))
    return out


def check(dev, entry, shape, cout, k, dst, f8=False, f8_2=False):
    dirty = launch(dev, entry, shape, cout, k, dst, f8, f8_2, True)
    clean = launch(dev, entry, shape, cout, k, dst, f8, f8_2, False)
    for (buf, bytes_, (b, h, w), ld, choff, c), (buf0, *_) in zip(dirty, clean):
        sent = SENT8 if bytes_ else SENT16
        n = b * (h + 2) * (w + 2) * ld
        all_ = whole(buf).clone()
        v = all_[buf.storage_offset():buf.storage_offset() + n].view(b, h + 2, w + 2, ld)
        got = v[:, 1:-1, 1:-1, choff:choff + c].clone()
        v[:, 1:-1, 1:-1, choff:choff + c] = sent
        assert bool((all_ == sent).all()), "an element outside the slice was written"
        ref = buf0[:n].view(b, h + 2, w + 2, ld)[:, 1:-1, 1:-1, choff:choff + c]
        assert bool((ref != 0).any()), "the launch wrote nothing"
        bits = torch.uint8 if bytes_ else torch.int16
        assert torch.equal(got.contiguous().view(bits), ref.contiguous().view(bits)), "slice differs from the zero-initialised launch"


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cout", [72, 264])
@pytest.mark.parametrize("entry", ["padded", "sparse24", "q8-f8", "q8-f16"])
def test_store_writes_its_slice_only(dev, entry, cout, k, dst):
    f8 = entry == "q8-f8"
    check(dev, entry.split("-")[0], (B, H, W, CIN), cout, k, dst, f8, f8)


def test_store_q8_mixed_destinations(dev):
    """y as e4m3 bytes, y2 as fp16: both LDS tiles of the quantised block's epilogue."""
    check(dev, "q8", (B, H, W, CIN), 72, 3, "pool+y2", True, False)


def test_store_q8_fp8_mfma_256_channel_tile(dev, setenv):
    """MCAMD_Q8_MFMA=1 reaches the 256-channel tile from 256 filters."""
    # (not asserted: no query reports the fp8 tile.  It is mcamd_conv_q8_launch's `a.N >= 256` branch under the switch,
    # csrc/conv_q8.hip; if that threshold moves, move the filter count of this case with it)
    setenv("MCAMD_Q8_MFMA", "1")
    check(dev, "q8", (B, H, W, CIN), 264, 3, "pool+y2", True, True)


def test_store_pingpong_tile(dev):
    """A dense shape on the ping-pong kernel (the 3 x 26 x 26 x 128 -> 256 pool + y2 case of
    test_conv_fwd_padded_pool_reorg_epilogue takes the 128-row kernel; with 58 images the same layer fills the 256 CUs with
    192 x 256 ping-pong tiles, the last one ragged in M)."""
    shape = (58, 26, 26, 128)
    g = operands(dev, "padded", *shape, 256, 3)[0]
    # (asked for this launch's own epilogue: the padded one with POOL)
    assert ops.conv_route_info(g, ops.DIR_FWD, L.EPI_PAD_F16, L.DST_POOL).kernel == ROUTE_PP
    check(dev, "padded", shape, 256, 3, "pool+y2")
