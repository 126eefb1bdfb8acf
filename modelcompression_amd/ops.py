"""Thin torch-tensor wrappers over the C-ABI (include/mcamd.h).

Tensors are only containers for device memory here (allocation + stream come
from PyTorch-ROCm); every compute call goes to libmcamd.so.
"""
import collections
import ctypes as C
import weakref

import torch

from . import _lib as L
from ._lib import (ConvGeom, ConvEpilogue, SplitkInfo, ActDesc, ActBwdDesc, DgradSums, ChanMap, PackJob, StemBlockDesc, FoldDesc, FoldJob, check, ptr,
                   stream_ptr)

HALF = torch.float16
SLACK = 64  # fp16 elements of zeroed slack after every activation buffer


def round_up(v, m):
    return (v + m - 1) // m * m


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.McamdError("modelcompression_amd compute ops need CUDA (MI355X) tensors; there is no CPU path")


def guard_elems(W, ld):
    """Zeroed guard band (elements) in front of and behind every padded buffer: the 9-tap wgrad kernel
    and the 9-tap forward/dgrad kernels read whole windows of (W+3 rounded up to 4) padded-pixel
    rows around their 32- / 128-row pixel tiles."""
    return (round_up(W + 3, 4) + 128) * ld + SLACK


_PAD_OF = {}     # data_ptr -> weak reference to the shared-halo buffer alloc_padded returned at that address


def alloc_padded(B, H, W, ld, device, pad=0):
    """Zeroed padded-NHWC fp16 buffer [B][H+2][W+2][ld], flat, with zeroed guard bands on both sides
    (the returned tensor is a view starting at padded pixel (0,0,0); its storage holds the guards).
    pad=1: the SHARED-HALO form (include/mcamd.h): B (H+1) (W+1) + W + 2 pixels, the pointer is pixel (0, -1, -1)."""
    n = (B * (H + 1) * (W + 1) + W + 2) * ld if pad else B * (H + 2) * (W + 2) * ld
    g = guard_elems(W, ld)
    full = torch.zeros(g + n + g, dtype=HALF, device=device)
    buf = full[g:g + n + SLACK]
    # the form travels ON the tensor object; the address registry serves other tensor objects over the same memory and is
    # validated by a weak reference, so an address reused after the buffer died never reports a stale form
    buf._mcamd_pad = 1 if pad else 0
    if pad:
        _PAD_OF[buf.data_ptr()] = weakref.ref(buf)
    else:
        _PAD_OF.pop(buf.data_ptr(), None)
    return buf


def pad_of(buf):
    form = getattr(buf, "_mcamd_pad", None)
    if form is not None:
        return form
    ref = _PAD_OF.get(buf.data_ptr())
    if ref is None:
        return 0
    if ref() is None:                      # the buffer that registered this address is gone
        del _PAD_OF[buf.data_ptr()]
        return 0
    return 1


def padded_view(buf, B, H, W, ld, pad=None):
    """[B][H+2][W+2][ld] view of a buffer from alloc_padded, pixel (h, w) at [:, h + 1, w + 1].  For the shared-halo form
    it is an OVERLAPPING strided view (a row's right halo pixel is the next row's left one): reads are what they look
    like; write interior pixels, or zeros to halo pixels, only."""
    if pad is None:
        pad = pad_of(buf)
    if pad:
        return torch.as_strided(buf, (B, H + 2, W + 2, ld), ((H + 1) * (W + 1) * ld, (W + 1) * ld, ld, 1))
    return buf[: B * (H + 2) * (W + 2) * ld].view(B, H + 2, W + 2, ld)


F8_WEXP_DEFAULT = 5      # weight exponent of the fp8 correction bytes for initialisation-sized weights (|w| <= 14)


def geom(B, H, W, ksize, cin, cout, x_ld, x_choff=0, stem=0, pad=0, x_wrap=0, x_f8=0, x_f8_wexp=F8_WEXP_DEFAULT):
    return ConvGeom(B, H, W, ksize, cin, cout, x_ld, x_choff, stem, pad, x_wrap, x_f8, x_f8_wexp if x_f8 else 0)


def conv_fwd_f8_ok(g):
    """Does mcamd_conv_fwd accept this geometry with fp8 correction terms (mcamd_conv_geom.x_f8)?"""
    return bool(L.lib().mcamd_conv_fwd_f8_ok(C.byref(g)))


def packed_elems(g):
    lib = L.lib()
    return int(lib.mcamd_packed_elems_fwd(C.byref(g))), int(lib.mcamd_packed_elems_dgrad(C.byref(g)))


def _chan_map(g, rows, cols):
    """mcamd_chan_map from optional int32 CUDA vectors (physical filter / input channel -> tensor index)."""
    if rows is None and cols is None:
        return None
    m = ChanMap()
    for name, v, n in (("rows", rows, g.cout), ("cols", cols, g.cin)):
        if v is not None:
            if v.dtype != torch.int32 or not v.is_cuda or not v.is_contiguous() or v.numel() != n:
                raise L.McamdError("channel map `%s` must be a contiguous CUDA int32 vector of %d entries" % (name, n))
            setattr(m, name, v.data_ptr())
    return C.byref(m)


def pack_weights(g, w, mask=None, want_fwd=True, want_dgrad=True, out_fwd=None, out_dgrad=None, rows=None, cols=None):
    """fp32 OIHW master (* mask) -> (fwd, dgrad) fp16 packings (layers.py:59 replacement).
    `rows` / `cols`: physical channel order of `g` (see mcamd_chan_map); w and mask stay in OIHW order."""
    _need_cuda(w, mask)
    assert w.dtype == torch.float32 and w.is_contiguous()
    nf, nd = packed_elems(g)
    if want_fwd and out_fwd is None:
        out_fwd = torch.empty(nf, dtype=HALF, device=w.device)
    if want_dgrad and not g.stem and out_dgrad is None:
        out_dgrad = torch.empty(nd, dtype=HALF, device=w.device)
    check(L.lib().mcamd_pack_weights(C.byref(g), ptr(w), ptr(mask), _chan_map(g, rows, cols), ptr(out_fwd) if want_fwd else None,
                                     ptr(out_dgrad) if (want_dgrad and not g.stem) else None, stream_ptr()),
          "mcamd_pack_weights")
    return out_fwd, out_dgrad


def pack_table(jobs, device):
    """jobs: list of dicts(w, mask, dst_fwd, dst_dgrad, rows, cols, cout, cin, ksize[, split]), one per layer ->
    (device table, njobs, total tiles) for `pack_many` (mcamd_pack_job array).  The tensors must stay alive and
    in place while the table is used."""
    arr = (PackJob * len(jobs))()
    total = 0
    for a, j in zip(arr, jobs):
        _need_cuda(j["w"], j.get("dst_fwd"), j.get("dst_dgrad"))
        assert j["w"].dtype == torch.float32 and j["w"].is_contiguous()
        a.w = j["w"].data_ptr()
        for name in ("mask", "dst_fwd", "dst_dgrad", "rows", "cols"):
            setattr(a, name, j[name].data_ptr() if j.get(name) is not None else None)
        a.first_tile, a.cout, a.cin, a.ksize = total, j["cout"], j["cin"], j["ksize"]
        a.split = int(j.get("split") or 0)      # 0 plain, 1 [w_hi | w_hi | w_lo], 2 [w_hi | w8 | wlo8] (mcamd_pack_job.split)
        a.f8_wexp = int(j.get("f8_wexp", F8_WEXP_DEFAULT))
        total += ((j["cout"] + 31) // 32) * ((j["cin"] + 31) // 32)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device), len(jobs), total


def pack_many(table, njobs, total):
    """Every (non-stem) layer's forward + dgrad packing in one launch (the master and the mask are read once);
    pads of the destinations must already be zero."""
    check(L.lib().mcamd_pack_weights_many(ptr(table), njobs, total, stream_ptr()), "mcamd_pack_weights_many")


def tile_info(g, dgrad=False, concurrent=False):
    out = (C.c_int32 * 4)()
    check(L.lib().mcamd_conv_tile_info(C.byref(g), (2 if concurrent else 1) if dgrad else 0, out), "mcamd_conv_tile_info")
    return tuple(out)


ConvRouteInfo = collections.namedtuple("ConvRouteInfo", "bm bn bk kernel rows")
DIR_FWD, DIR_DGRAD, DIR_DGRAD_CONCURRENT = 0, 1, 2      # `dir` of conv_route_info
ROUTE_IGEMM, ROUTE_STEM, ROUTE_PP, ROUTE_SMALL3X3, ROUTE_WIN3X3, ROUTE_WRES, ROUTE_SMALL3X3_SPLIT = 0, 1, 2, 4, 5, 6, 7


def conv_route_info(g, dir=DIR_FWD, mode=L.EPI_RAW_F16, dst_mode=L.DST_PLAIN, stats=False):
    """The kernel, tile and slab rows a forward / dgrad launch of `g` with this epilogue takes: mcamd_conv_route_info, the
    launches' own route function.  Needs no GPU."""
    out = (C.c_int32 * 5)()
    check(L.lib().mcamd_conv_route_info(C.byref(g), dir, mode, dst_mode, 1 if stats else 0, out), "mcamd_conv_route_info")
    return ConvRouteInfo(*out)


def stats_rows(g, mode=L.EPI_RAW_F16):
    """Rows of the BN partial-sum slab a forward launch of `g` writes with epilogue `mode` (RAW_F16 or RAW_F32)."""
    return int(L.lib().mcamd_conv_stats_rows_mode(C.byref(g), mode))


def _epi(mode, y, y_ld=0, y_choff=0, bias=None, stats=None, stats_rows_=0, stats_ld=0, scale=None, shift=None,
         slope=1.0, overflow=None, dst_mode=0, y2=None, y2_ld=0, y2_choff=0):
    e = ConvEpilogue()
    e.mode, e.y_ld, e.y_choff = mode, y_ld, y_choff
    e.y = y.data_ptr()
    e.bias = bias.data_ptr() if bias is not None else None
    e.stats = stats.data_ptr() if stats is not None else None
    e.stats_rows, e.stats_ld = stats_rows_, stats_ld
    e.scale = scale.data_ptr() if scale is not None else None
    e.shift = shift.data_ptr() if shift is not None else None
    e.slope = slope
    e.overflow = overflow.data_ptr() if overflow is not None else None
    e.dst_mode = dst_mode
    e.y2 = y2.data_ptr() if y2 is not None else None
    e.y2_ld, e.y2_choff = y2_ld, y2_choff
    return e


def conv_fwd_raw(g, x, wp, y, y_ld, y_choff=0, stats=None):
    """y[M][y_ld] fp16 raw conv output; `stats`: fp32 [stats_rows(g)][2][stats_ld] slab or None."""
    e = _epi(L.EPI_RAW_F16, y, y_ld, y_choff, stats=stats,
             stats_rows_=stats.shape[0] if stats is not None else 0,
             stats_ld=stats.shape[2] if stats is not None else 0)
    check(L.lib().mcamd_conv_fwd(C.byref(g), ptr(x), ptr(wp), C.byref(e), stream_ptr()), "mcamd_conv_fwd")


def conv_fwd_raw32(g, x, wp, y, y_ld, y_choff=0, stats=None):
    """y[M][y_ld] fp32: the unrounded accumulators (the "fp16x3" precision mode); `stats` as conv_fwd_raw, with
    stats_rows(g, EPI_RAW_F32) rows, summed from the fp32 values."""
    e = _epi(L.EPI_RAW_F32, y, y_ld, y_choff, stats=stats,
             stats_rows_=stats.shape[0] if stats is not None else 0,
             stats_ld=stats.shape[2] if stats is not None else 0)
    check(L.lib().mcamd_conv_fwd(C.byref(g), ptr(x), ptr(wp), C.byref(e), stream_ptr()), "mcamd_conv_fwd")


def conv_fwd_nchw(g, x, wp, y, bias=None):
    e = _epi(L.EPI_NCHW_F32, y, bias=bias)
    check(L.lib().mcamd_conv_fwd(C.byref(g), ptr(x), ptr(wp), C.byref(e), stream_ptr()), "mcamd_conv_fwd")


def conv_fwd_padded(g, x, wp, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None, y2_ld=0, y2_choff=0):
    """Inference: leaky(conv * scale + shift) straight into a padded NHWC buffer.  `dst_mode` = L.DST_POOL / L.DST_REORG fuses
    the MaxPool(2,2) / Reorg(2) that follows the block (y is then at the pooled resolution); `y2`: optional full-resolution copy."""
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff)
    check(L.lib().mcamd_conv_fwd(C.byref(g), ptr(x), ptr(wp), C.byref(e), stream_ptr()), "mcamd_conv_fwd")


def dgrad_sums_rows(g, concurrent=False):
    """Slab rows a conv_dgrad_raw launch of `g` writes when it takes its producer's BatchNorm-backward sums (dgrad_sums);
    0: the kernel that geometry gets cannot take them."""
    return int(L.lib().mcamd_conv_dgrad_sums_rows(C.byref(g), 1 if concurrent else 0))


def dgrad_sums(slab, act, act_ld, act_choff, act_pad, scale, shift, mean, invstd, slope, C_, ch_lo=0, y=None, y_ld=0, y_choff=0):
    """mcamd_dgrad_sums for conv_dgrad_raw(..., sums=): the PLAIN block whose C_ channels are the columns [ch_lo, ch_lo + C_)
    of the launch's output G; `slab` fp32 [dgrad_sums_rows(g, concurrent)][2][ld >= C_] receives sum g_z and sum g_z xhat,
    which bn_act_bwd(..., sums=slab) then takes instead of running its first pass.  The tensors must stay alive."""
    _need_cuda(slab, act, scale, shift, mean, invstd, y)
    assert slab.dtype == torch.float32 and slab.dim() == 3 and slab.shape[1] == 2 and slab.is_contiguous()
    assert y is None or y.dtype == torch.float32
    d = DgradSums()
    d.slab, d.rows, d.ld = slab.data_ptr(), slab.shape[0], slab.shape[2]
    d.act, d.act_ld, d.act_choff, d.act_pad = act.data_ptr(), act_ld, act_choff, act_pad
    d.scale, d.shift, d.mean, d.invstd = scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    d.slope = slope
    d.y, d.y_ld, d.y_choff = (y.data_ptr() if y is not None else None), y_ld, y_choff
    d.ch_lo, d.C = ch_lo, C_
    return d


def conv_dgrad_raw(g, dy, dy_ld, dy_choff, wpd, out, out_ld, out_choff=0, overflow=None, concurrent=False, sums=None):
    """`overflow`: optional int32[1] device flag, set when a (scaled) gradient was clamped to the fp16 range.
    `concurrent`: another stream has work for the CUs this launch leaves idle (mcamd_conv_epilogue.concurrent).
    `sums`: optional dgrad_sums(...) descriptor -- the launch also forms the BatchNorm-backward sums of the producer whose
    output gradient it stores (mcamd_conv_dgrad_sums)."""
    e = _epi(L.EPI_RAW_F16, out, out_ld, out_choff, overflow=overflow)
    e.concurrent = 1 if concurrent else 0
    if sums is not None:
        check(L.lib().mcamd_conv_dgrad_sums(C.byref(g), ptr(dy), dy_ld, dy_choff, ptr(wpd), C.byref(e), C.byref(sums), stream_ptr()),
              "mcamd_conv_dgrad_sums")
        return
    check(L.lib().mcamd_conv_dgrad(C.byref(g), ptr(dy), dy_ld, dy_choff, ptr(wpd), C.byref(e), stream_ptr()),
          "mcamd_conv_dgrad")


def conv_dgrad_nchw(g, dy, dy_ld, dy_choff, wpd, out):
    e = _epi(L.EPI_NCHW_F32, out)
    check(L.lib().mcamd_conv_dgrad(C.byref(g), ptr(dy), dy_ld, dy_choff, ptr(wpd), C.byref(e), stream_ptr()),
          "mcamd_conv_dgrad")


def wgrad_workspace_bytes(g):
    return int(L.lib().mcamd_conv_wgrad_workspace_bytes(C.byref(g)))


WgradPlanInfo = collections.namedtuple("WgradPlanInfo", "family tmo tnc taps kp ns nsplit pix_per_split rows_pad finish sg tiles grid")


def wgrad_plan_info(g, has_cmap=False):
    """The kernels mcamd_conv_wgrad launches for `g` (with a column map or without): mcamd_conv_wgrad_plan_info.  Needs no GPU."""
    out = (C.c_int32 * L.WGRAD_PLAN_INFO_N)()
    check(L.lib().mcamd_conv_wgrad_plan_info(C.byref(g), 1 if has_cmap else 0, out), "mcamd_conv_wgrad_plan_info")
    return WgradPlanInfo(*out)


def wgrad_generic_instances():
    """(TMo, TNc, TAPS, KP) of every wgrad_kernel instance in the library."""
    lib = L.lib()
    n = int(lib.mcamd_wgrad_generic_instances(None, 0))
    out = (C.c_int32 * (4 * n))()
    lib.mcamd_wgrad_generic_instances(out, n)
    return [tuple(out[4 * i:4 * i + 4]) for i in range(n)]


def conv_wgrad(g, x, dy, dy_ld, dy_choff, dw, mask=None, grad_scale=1.0, dbias=None, workspace=None, rows=None, cols=None):
    """`rows` / `cols`: physical channel order of `g`; dw / mask stay OIHW and rows outside `rows` are not written."""
    if workspace is None:
        workspace = torch.empty(wgrad_workspace_bytes(g), dtype=torch.uint8, device=dw.device)
    check(L.lib().mcamd_conv_wgrad(C.byref(g), ptr(x), ptr(dy), dy_ld, dy_choff, ptr(mask), _chan_map(g, rows, cols), grad_scale, ptr(dw),
                                   ptr(dbias), ptr(workspace), workspace.numel(), stream_ptr()), "mcamd_conv_wgrad")


# ... its list launch: the tiles and taps a block mask keeps (Darknet.sparse_train = "block-wgrad")
def conv_wgrad_bsparse_ok(g):
    """Does conv_wgrad_bsparse accept this geometry?  Needs no GPU."""
    return bool(L.lib().mcamd_conv_wgrad_bsparse_ok(C.byref(g)))


def wgrad_bsparse_elems(g):
    """(nt, 2 nt): int32 entries of the tile list and of the tap words, nt = (cout / 64) * (cin / 64)."""
    out = (C.c_int64 * 2)()
    check(L.lib().mcamd_wgrad_bsparse_elems(C.byref(g), out), "mcamd_wgrad_bsparse_elems")
    return int(out[0]), int(out[1])


def wgrad_bsparse_lists(g, mask, tiles=None, words=None, counts=None):
    """fp32 OIHW mask -> (tiles int32[nt], words int32[2 nt], counts int32[2]): the 64 x 64 tiles with any non-zero mask
    element, ascending, their tap words, and (kept tiles, kept (tile, tap) pairs): mcamd_wgrad_bsparse_lists; no host
    synchronisation."""
    _need_cuda(mask)
    nt, nw = wgrad_bsparse_elems(g)
    if mask.dtype != torch.float32 or not mask.is_contiguous() or mask.numel() != g.cout * g.cin * g.ksize * g.ksize:
        raise L.McamdError("wgrad_bsparse_lists: mask must be contiguous fp32 OIHW of the geometry's shape")
    tiles = torch.empty(nt, dtype=torch.int32, device=mask.device) if tiles is None else tiles
    words = torch.empty(nw, dtype=torch.int32, device=mask.device) if words is None else words
    counts = torch.empty(2, dtype=torch.int32, device=mask.device) if counts is None else counts
    if tiles.numel() != nt or words.numel() != nw or counts.numel() != 2:
        raise L.McamdError("wgrad_bsparse_lists: list sizes do not fit the geometry")
    check(L.lib().mcamd_wgrad_bsparse_lists(C.byref(g), ptr(mask), ptr(tiles), ptr(words), ptr(counts), stream_ptr()),
          "mcamd_wgrad_bsparse_lists")
    return tiles, words, counts


def wgrad_bsparse_full_lists(g, device):
    """(tiles, words) naming every tile with every tap: what a full-list launch runs on."""
    nt, nw = wgrad_bsparse_elems(g)
    return (torch.arange(nt, dtype=torch.int32, device=device),
            torch.full((nw,), 0x1ff if g.ksize == 3 else 1, dtype=torch.int32, device=device))


WgradBsparsePlan = collections.namedtuple("WgradBsparsePlan", "family kp ns nsplit pix_per_split finish sg bytes")


def conv_wgrad_bsparse_plan(g, kept_tiles):
    """What conv_wgrad_bsparse runs for `kept_tiles` listed tiles (mcamd_conv_wgrad_bsparse_plan).  Needs no GPU."""
    out = (C.c_int64 * L.WGRAD_BSPARSE_PLAN_N)()
    check(L.lib().mcamd_conv_wgrad_bsparse_plan(C.byref(g), int(kept_tiles), out), "mcamd_conv_wgrad_bsparse_plan")
    return WgradBsparsePlan(*(int(v) for v in out))


def conv_wgrad_bsparse(g, x, dy, dy_ld, dy_choff, dw, mask, tiles, words, ntiles, nsplit, grad_scale=1.0, dbias=None,
                       workspace=None):
    """conv_wgrad on the `ntiles` listed tiles (wgrad_bsparse_lists of the same mask) at `nsplit` pixel splits
    (conv_wgrad_bsparse_plan(g, ntiles).nsplit; a full-list launch takes the short lists' split count).  `ntiles` and
    `nsplit` are host integers: the launch never reads the counters back."""
    nt, nw = wgrad_bsparse_elems(g)
    _need_cuda(x, dy, mask, tiles, words)
    if tiles.dtype != torch.int32 or words.dtype != torch.int32 or tiles.numel() < ntiles or words.numel() < ntiles:
        raise L.McamdError("conv_wgrad_bsparse: tiles / words must be int32 lists of at least %d entries" % ntiles)
    if workspace is None:
        workspace = torch.empty(nsplit * g.cout * g.cin * g.ksize * g.ksize * 4, dtype=torch.uint8, device=dw.device)
    check(L.lib().mcamd_conv_wgrad_bsparse(C.byref(g), ptr(x), ptr(dy), dy_ld, dy_choff, ptr(mask), ptr(tiles), ptr(words),
                                           int(ntiles), int(nsplit), grad_scale, ptr(dw), ptr(dbias), ptr(workspace),
                                           workspace.numel(), stream_ptr()), "mcamd_conv_wgrad_bsparse")


def conv_bwd1x1_ok(g):
    """(ok, reason): does `g` have the one-launch backward (mcamd_conv_bwd1x1)?  `reason` says why not.  Needs no GPU."""
    why = C.c_char_p()
    ok = bool(L.lib().mcamd_conv_bwd1x1_ok(C.byref(g), C.byref(why)))
    return ok, (None if ok else why.value.decode())


def conv_bwd1x1_sums_rows(g):
    """Rows of the sums slab a conv_bwd1x1 launch of `g` writes (dgrad_sums(...) with that many rows); 0: refused geometry."""
    return int(L.lib().mcamd_conv_bwd1x1_sums_rows(C.byref(g)))


def conv_bwd1x1_wgrad_splits(g):
    """fp32 [cout][cin] splits of the weight gradient a conv_bwd1x1 launch of `g` leaves in its workspace; 0: refused."""
    return int(L.lib().mcamd_conv_bwd1x1_wgrad_splits(C.byref(g)))


def conv_bwd1x1_workspace_bytes(g):
    return int(L.lib().mcamd_conv_bwd1x1_workspace_bytes(C.byref(g)))


def conv_bwd1x1(g, x, dy, dy_ld, dy_choff, wpd, gin, g_ld, g_choff, dw, mask=None, grad_scale=1.0, dbias=None, workspace=None,
                overflow=None, sums=None):
    """The whole backward of a dense 1x1 block in one launch + the finish pass: gin as conv_dgrad_raw stores it (with
    `overflow`), dw / dbias as conv_wgrad, and with `sums` (dgrad_sums(...) over x itself, conv_bwd1x1_sums_rows(g) rows) the
    producer's BatchNorm-backward sums."""
    if workspace is None:
        workspace = torch.empty(conv_bwd1x1_workspace_bytes(g), dtype=torch.uint8, device=dw.device)
    check(L.lib().mcamd_conv_bwd1x1(C.byref(g), ptr(x), ptr(dy), dy_ld, dy_choff, ptr(wpd), ptr(gin), g_ld, g_choff, ptr(overflow),
                                    C.byref(sums) if sums is not None else None, ptr(mask), grad_scale, ptr(dw), ptr(dbias),
                                    ptr(workspace), workspace.numel(), stream_ptr()), "mcamd_conv_bwd1x1")


def _perm_ptr(perm, C_):
    if perm is None:
        return None
    if perm.dtype != torch.int32 or perm.numel() != C_ or not perm.is_contiguous() or not perm.is_cuda:
        raise L.McamdError("channel permutation must be a contiguous CUDA int32 vector of %d entries" % C_)
    return perm.data_ptr()


def bn_coeffs(stats, C_, count, gamma, beta, rmean, rvar, training, scale, shift, mean=None, invstd=None,
              momentum=0.1, eps=1e-5, perm=None, ones_channel=-1):
    """`perm` (int32 [C], optional): physical channel c uses gamma/beta/running_*[perm[c]].
    `ones_channel` >= 0: that physical channel gets scale 0 / shift 1 (the activation pass writes ones there)."""
    rows = stats.shape[0] if stats is not None else 0
    ld = stats.shape[2] if stats is not None else 0
    check(L.lib().mcamd_bn_coeffs_ex(ptr(stats), rows, ld, C_, count, ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar),
                                     momentum, eps, 1 if training else 0, ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
                                     _perm_ptr(perm, C_), ones_channel, stream_ptr()), "mcamd_bn_coeffs_ex")


def _fold_desc(w, mask, rows, cols, beta, slope, n, cin_k, aug):
    _need_cuda(w, mask, rows, cols, beta)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4 and w.shape[2] == w.shape[3]
    assert beta.dtype == torch.float32 and beta.numel() == w.shape[1]
    d = FoldDesc()
    d.w = w.data_ptr()
    d.mask = mask.data_ptr() if mask is not None else None
    for name, v, cnt in (("rows", rows, n), ("cols", cols, w.shape[1])):
        if v is not None:
            if v.dtype != torch.int32 or not v.is_contiguous() or v.numel() != cnt:
                raise L.McamdError("fold: channel map `%s` must be a contiguous CUDA int32 vector of %d entries" % (name, cnt))
            setattr(d, name, v.data_ptr())
    d.beta, d.slope = beta.data_ptr(), slope
    assert aug.dtype == torch.float32 and aug.is_contiguous() and aug.dim() == 4 and aug.shape[0] == n and aug.shape[1] > cin_k
    d.n, d.cin_t, d.cin_k, d.cin_aug, d.ksize = n, w.shape[1], cin_k, aug.shape[1], w.shape[2]
    return d


def fold_weights(w, mask, rows, cols, beta, slope, n, cin_k, waug):
    """Augmented weights [n][cin_aug >= cin_k + 1][k][k] of a consumer whose dead input channels are folded into one channel of
    ones (include/mcamd.h, mcamd_fold_desc): kept inputs gathered, the last column = sum_c leaky(beta_c) W[:, c]."""
    d = _fold_desc(w, mask, rows, cols, beta, slope, n, cin_k, waug)
    check(L.lib().mcamd_fold_weights(C.byref(d), ptr(waug), stream_ptr()), "mcamd_fold_weights")


def fold_table(jobs, device):
    """jobs: list of dicts(w, mask, rows, cols, beta, slope, n, cin_k, waug) -> (device table, njobs, total blocks) for
    `fold_many` (mcamd_fold_job array).  The tensors must stay alive and in place while the table is used."""
    arr = (FoldJob * len(jobs))()
    total = 0
    for a, j in zip(arr, jobs):
        a.d = _fold_desc(j["w"], j["mask"], j["rows"], j["cols"], j["beta"], j["slope"], j["n"], j["cin_k"], j["waug"])
        a.waug = j["waug"].data_ptr()
        a.first_block = total
        total += j["n"]
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device), len(jobs), total


def fold_many(table, njobs, total):
    """Every folding layer's augmented weights in one launch."""
    check(L.lib().mcamd_fold_weights_many(ptr(table), njobs, total, stream_ptr()), "mcamd_fold_weights_many")


def unfold_wgrad(w, mask, rows, cols, beta, slope, n, cin_k, dwaug, dw, prod_dbeta, prod_dgamma, accumulate=False):
    """Augmented weight gradient -> OIHW dW (x mask; the folded column expands to the dead inputs), and the producer's
    dbeta (dgamma = 0) for its dead channels."""
    d = _fold_desc(w, mask, rows, cols, beta, slope, n, cin_k, dwaug)
    check(L.lib().mcamd_unfold_wgrad(C.byref(d), ptr(dwaug), ptr(dw), ptr(prod_dbeta), ptr(prod_dgamma), 1 if accumulate else 0,
                                     stream_ptr()), "mcamd_unfold_wgrad")


def _act_desc(B, H, W, C_, y, y_ld, y_choff, scale, shift, slope, mode, dst, dst_ld, dst_choff=0, dst2=None,
              dst2_ld=0, dst2_choff=0, border=None, planes=1, dst_plane=0, dst2_plane=0, dst_pad=0, dst2_pad=0, planes2=0,
              pool_act=None, pool_act_ld=0, pool_act_pad=0, dst_q8=None, dst2_q8=None):
    """mcamd_act_desc of bn_act_fwd's arguments."""
    d = ActDesc()
    d.y_dtype = 1 if y.dtype == torch.float32 else 0
    d.planes, d.dst_plane, d.dst2_plane, d.planes2 = planes, dst_plane, dst2_plane, planes2
    d.dst_pad, d.dst2_pad = dst_pad, dst2_pad
    d.B, d.H, d.W, d.C = B, H, W, C_
    d.y, d.y_ld, d.y_choff = y.data_ptr(), y_ld, y_choff
    d.scale, d.shift, d.slope, d.mode = scale.data_ptr(), shift.data_ptr(), slope, mode
    d.dst, d.dst_ld, d.dst_choff = dst.data_ptr(), dst_ld, dst_choff
    d.dst2 = dst2.data_ptr() if dst2 is not None else None
    d.dst2_ld, d.dst2_choff = dst2_ld, dst2_choff
    if border is not None:
        if border.dtype != torch.float32 or tuple(border.shape) != (16, C_) or not border.is_contiguous():
            raise L.McamdError("bn_act_fwd: border table must be contiguous fp32 [16, %d]" % C_)
        d.border = border.data_ptr()
    if pool_act is not None:
        d.pool_act, d.pool_act_ld, d.pool_act_pad = pool_act.data_ptr(), pool_act_ld, pool_act_pad
    d.dst_q8 = dst_q8.data_ptr() if dst_q8 is not None else None
    d.dst2_q8 = dst2_q8.data_ptr() if dst2_q8 is not None else None
    return d


def bn_act_fwd(B, H, W, C_, y, y_ld, y_choff, scale, shift, slope, mode, dst, dst_ld, dst_choff=0, dst2=None,
               dst2_ld=0, dst2_choff=0, border=None, planes=1, dst_plane=0, dst2_plane=0, dst_pad=0, dst2_pad=0, planes2=0,
               pool_act=None, pool_act_ld=0, pool_act_pad=0, dst_q8=None, dst2_q8=None):
    """`dst_q8` / `dst2_q8`: byte twins of dst / dst2 (same geometry) that receive the e4m3 codes q(2 v) while the fp16
    buffer receives deq(code) / 2 (mcamd_act_desc.dst_q8: the fp8 quantisation-aware training forward; fp32 y, planes 1).
    `border`: optional fp32 [16, C] table added to the raw conv output by border class (slim models).
    `pool_act` (mode pool): padded fp16 buffer that receives the full-resolution activation for the block's backward pass
    (mcamd_act_desc.pool_act; bn_act_bwd(..., act=pool_act)).
    `y` may be fp16 or fp32 (conv_fwd_raw / conv_fwd_raw32).  planes=3: split (hi | lo | hi) activation storage of
    the "fp16x3" precision mode with plane strides dst_plane / dst2_plane (include/mcamd.h, mcamd_act_desc.planes)."""
    d = _act_desc(**locals())
    check(L.lib().mcamd_bn_act_fwd(C.byref(d), stream_ptr()), "mcamd_bn_act_fwd")


ActInstance = collections.namedtuple("ActInstance", "mode fixed y32 planes planes2 q8 items grid")


def bn_act_fwd_instance(B, H, W, C_, y, y_ld, y_choff, scale, shift, slope, mode, dst, dst_ld, dst_choff=0, dst2=None,
                        dst2_ld=0, dst2_choff=0, border=None, planes=1, dst_plane=0, dst2_plane=0, dst_pad=0, dst2_pad=0,
                        planes2=0, pool_act=None, pool_act_ld=0, pool_act_pad=0, dst_q8=None, dst2_q8=None):
    """The kernel instance bn_act_fwd launches for these arguments (mcamd_bn_act_fwd_instance: host logic only, needs no
    GPU -- the tensors only say which pointers are given and whether y is fp32); raises what bn_act_fwd would raise."""
    d = _act_desc(**locals())
    r = L.ActInstance()
    check(L.lib().mcamd_bn_act_fwd_instance(C.byref(d), C.byref(r)), "mcamd_bn_act_fwd_instance")
    return ActInstance(r.mode, bool(r.fixed), bool(r.y32), r.planes, r.planes2, bool(r.q8), r.items, r.grid)


class _NoPtr:
    """Stands for a device buffer where only the geometry is asked (bn_act_conv1x1_ok needs no GPU)."""
    dtype = torch.float32

    @staticmethod
    def data_ptr():
        return None


def act_geom(B, H, W, C_, y_ld, y_choff, slope, mode, dst_ld, dst_choff=0, **kw):
    """The geometry half of bn_act_fwd's arguments as a descriptor without pointers (fp32 y): for bn_act_conv1x1_ok."""
    return _act_desc(B, H, W, C_, _NoPtr, y_ld, y_choff, _NoPtr, _NoPtr, slope, mode, _NoPtr, dst_ld, dst_choff, **kw)


def bn_act_conv1x1_ok(d, g):
    """Whether the activation pass `d` (act_geom(...) / the arguments of bn_act_fwd) and the 1x1 forward `g` behind it have
    a fused launch (mcamd_bn_act_conv1x1_ok: host logic only)."""
    return bool(L.lib().mcamd_bn_act_conv1x1_ok(C.byref(d), C.byref(g)))


def bn_act_conv1x1_stats_rows(d, g):
    """Rows of the statistics slab bn_act_conv1x1_fwd writes (0 when the pair is refused)."""
    return int(L.lib().mcamd_bn_act_conv1x1_stats_rows(C.byref(d), C.byref(g)))


BnConv1x1Info = collections.namedtuple("BnConv1x1Info", "bn cb threads rows num_mtiles grid lds_bytes")


def bn_act_conv1x1_info(d, g):
    """The bn_conv1x1_kernel<bn, cb> instance and launch dimensions bn_act_conv1x1_fwd takes for the pair
    (mcamd_bn_act_conv1x1_info: host logic only, needs no GPU); raises what the launch would raise for a refused pair."""
    r = L.BnConv1x1Instance()
    check(L.lib().mcamd_bn_act_conv1x1_info(C.byref(d), C.byref(g), C.byref(r)), "mcamd_bn_act_conv1x1_info")
    return BnConv1x1Info(r.bn, r.cb, r.threads, r.rows, r.num_mtiles, r.grid, r.lds_bytes)


def bn_act_conv1x1_fwd(act_args, act_kw, g, wp, y, y_ld, y_choff=0, stats=None):
    """bn_act_fwd(*act_args, **act_kw) and conv_fwd_raw32(g, dst, wp, y, y_ld, y_choff, stats) in one launch
    (mcamd_bn_act_conv1x1_fwd): bit-equal y and stats; of the activation only the hi plane is stored."""
    d = _act_desc(*act_args, **act_kw)
    e = _epi(L.EPI_RAW_F32, y, y_ld, y_choff, stats=stats,
             stats_rows_=stats.shape[0] if stats is not None else 0,
             stats_ld=stats.shape[2] if stats is not None else 0)
    check(L.lib().mcamd_bn_act_conv1x1_fwd(C.byref(d), C.byref(g), ptr(wp), C.byref(e), stream_ptr()),
          "mcamd_bn_act_conv1x1_fwd")


def bn_act_bwd(B, H, W, C_, y, y_ld, y_choff, scale, shift, mean, invstd, slope, mode, g, g_ld, g_choff, dy, dy_ld,
               dy_choff, dgamma, dbeta, grad_scale=1.0, g2=None, g2_ld=0, g2_choff=0, workspace=None, dy_keep=None,
               perm=None, overflow=None, skip_dead_from=0, dy_pad=0, act=None, act_ld=0, act_choff=0, act_pad=0,
               pool_out=None, pool_out_ld=0, pool_out_choff=0, pool_out_pad=0, sums=None):
    """`act` (PLAIN blocks): the stored fp16 activation in its padded buffer -- the pre-activation is recovered from it
    and `y` is not read (mcamd_act_bwd_desc.act).
    `pool_out` (MaxPool blocks with `act` or an fp32 `y`, no g2): the pooled fp16 activation in the consumer's padded buffer -- the pass
    that forms the per-channel sums reads it instead of the full-resolution copy or `y` (mcamd_act_bwd_desc.pool_out).
    `sums` (PLAIN blocks with `act`, no g2): fp32 [rows][2][ld] slab that already holds the per-channel sums -- written by the
    conv_dgrad_raw(..., sums=) launch that stored `g` -- so the pass that forms them is skipped (mcamd_act_bwd_desc.sums)."""
    d = ActBwdDesc()
    if sums is not None:
        assert sums.dtype == torch.float32 and sums.dim() == 3 and sums.shape[1] == 2 and sums.is_contiguous()
        d.sums, d.sums_rows, d.sums_ld = sums.data_ptr(), sums.shape[0], sums.shape[2]
    d.skip_dead_param_grads = int(skip_dead_from)
    d.dy_pad = dy_pad
    d.B, d.H, d.W, d.C = B, H, W, C_
    if act is not None:
        d.act, d.act_ld, d.act_choff, d.act_pad = act.data_ptr(), act_ld, act_choff, act_pad
    if pool_out is not None:
        d.pool_out, d.pool_out_ld, d.pool_out_choff, d.pool_out_pad = pool_out.data_ptr(), pool_out_ld, pool_out_choff, pool_out_pad
    d.y, d.y_ld, d.y_choff = (y.data_ptr() if y is not None else None), y_ld, y_choff
    d.scale, d.shift, d.mean, d.invstd = scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    d.slope, d.mode = slope, mode
    d.g, d.g_ld, d.g_choff = g.data_ptr(), g_ld, g_choff
    d.g2 = g2.data_ptr() if g2 is not None else None
    d.g2_ld, d.g2_choff = g2_ld, g2_choff
    d.dy, d.dy_ld, d.dy_choff = dy.data_ptr(), dy_ld, dy_choff
    d.dgamma = dgamma.data_ptr() if dgamma is not None else None
    d.dbeta = dbeta.data_ptr() if dbeta is not None else None
    d.grad_scale = grad_scale
    d.dy_keep = dy_keep.data_ptr() if dy_keep is not None else None
    d.chan_perm = _perm_ptr(perm, C_)
    d.y_dtype = 1 if (y is not None and y.dtype == torch.float32) else 0
    d.overflow = overflow.data_ptr() if overflow is not None else None
    need = int(L.lib().mcamd_bn_act_bwd_workspace_bytes(C.byref(d)))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=g.device)
    check(L.lib().mcamd_bn_act_bwd(C.byref(d), ptr(workspace), workspace.numel(), stream_ptr()), "mcamd_bn_act_bwd")


def bn_act_bwd_workspace_bytes(C_):
    d = ActBwdDesc()
    d.C = C_
    return int(L.lib().mcamd_bn_act_bwd_workspace_bytes(C.byref(d)))


def stem_block_workspace_bytes():
    return int(L.lib().mcamd_stem_block_workspace_bytes())


def _stem_desc(B, H, W, x, wp, gamma, beta, scale, shift, mean, invstd, slope):
    _need_cuda(x, wp, scale, shift)
    d = StemBlockDesc()
    d.B, d.H, d.W = B, H, W
    d.x, d.wp = x.data_ptr(), wp.data_ptr()
    d.gamma = gamma.data_ptr() if gamma is not None else None
    d.beta = beta.data_ptr() if beta is not None else None
    d.scale, d.shift = scale.data_ptr(), shift.data_ptr()
    d.save_mean = mean.data_ptr() if mean is not None else None
    d.save_invstd = invstd.data_ptr() if invstd is not None else None
    d.slope = slope
    return d


def stem_block_fwd(B, H, W, x, wp, gamma, beta, rmean, rvar, training, scale, shift, mean, invstd, slope, dst, dst_ld,
                   dst_choff, workspace, momentum=0.1, eps=1e-5, cout=32, planes=1, x_lo=None, wp_lo=None):
    """The first block in one call: conv1 (3 -> 32, 3x3) + BatchNorm + LeakyReLU + MaxPool(2,2) from the NHWC4 image
    `x` to the pooled padded-NHWC `dst`; the raw conv output is never stored (include/mcamd.h, mcamd_stem_block_desc).
    training: batch statistics from the image windows' Gram matrix, scale / shift / mean / invstd are written
    (`dst` None: that half only).  `x_lo` / `wp_lo`: split operands (training must be False: scale / shift are read)."""
    d = _stem_desc(B, H, W, x, wp, gamma, beta, scale, shift, mean, invstd, slope)
    d.running_mean = rmean.data_ptr() if rmean is not None else None
    d.running_var = rvar.data_ptr() if rvar is not None else None
    d.momentum, d.eps, d.training = momentum, eps, 1 if training else 0
    d.cout, d.planes = cout, planes
    d.dst, d.dst_ld, d.dst_choff = (dst.data_ptr() if dst is not None else None), dst_ld, dst_choff
    d.x_lo = x_lo.data_ptr() if x_lo is not None else None
    d.wp_lo = wp_lo.data_ptr() if wp_lo is not None else None
    check(L.lib().mcamd_stem_block_fwd(C.byref(d), ptr(workspace), workspace.numel() if workspace is not None else 0,
                                       stream_ptr()), "mcamd_stem_block_fwd")


def stem_block_stats_rows(B, H, W):
    d = StemBlockDesc()
    d.B, d.H, d.W = B, H, W
    return int(L.lib().mcamd_stem_block_stats_rows(C.byref(d)))


StemLaunchInfo = collections.namedtuple("StemLaunchInfo", "grid items per_pass per_wave passes")
StemPlanInfo = collections.namedtuple("StemPlanInfo", "fwd fwd_planes stats gram bwd")


def stem_block_plan_info(B, H, W):
    """How the first block's five persistent launches divide B x H x W (workgroups, work items, items per pass, items of
    the busiest wave, passes): mcamd_stem_block_plan_info, the launches' own grid function.  Needs no GPU."""
    d = StemBlockDesc()
    d.B, d.H, d.W = B, H, W
    out = (C.c_int32 * L.STEM_PLAN_INFO_N)()
    check(L.lib().mcamd_stem_block_plan_info(C.byref(d), out), "mcamd_stem_block_plan_info")
    return StemPlanInfo(*(StemLaunchInfo(*out[4 * i:4 * i + 4], -(-out[4 * i + 1] // out[4 * i + 2])) for i in range(5)))


def stem_block_stats(B, H, W, x, wp, stats, x_lo=None, wp_lo=None):
    """Per-channel partial sums / sums of squares of the first block's conv output (split operands with `x_lo` /
    `wp_lo`) into the fp32 slab `stats` [stem_block_stats_rows][2][ld]: what bn_coeffs takes.  Nothing else is written."""
    _need_cuda(x, wp, stats)
    assert stats.dtype == torch.float32 and stats.dim() == 3 and stats.shape[1] == 2 and stats.is_contiguous()
    d = StemBlockDesc()
    d.B, d.H, d.W = B, H, W
    d.x, d.wp = x.data_ptr(), wp.data_ptr()
    d.x_lo = x_lo.data_ptr() if x_lo is not None else None
    d.wp_lo = wp_lo.data_ptr() if wp_lo is not None else None
    d.cout = 32
    check(L.lib().mcamd_stem_block_stats(C.byref(d), ptr(stats), stats.shape[0], stats.shape[2], stream_ptr()),
          "mcamd_stem_block_stats")


def nchw_to_nhwc4_split(src, hi, lo):
    """fp32 NCHW 3-channel image -> padded NHWC4 fp16 images hi = fp16(v), lo = fp16(v - hi)."""
    _need_cuda(src, hi, lo)
    assert src.dtype == torch.float32 and src.is_contiguous() and src.shape[1] == 3
    B, _, H, W = src.shape
    check(L.lib().mcamd_nchw_f32_to_nhwc4_split(ptr(src), B, H, W, ptr(hi), ptr(lo), stream_ptr()), "mcamd_nchw_f32_to_nhwc4_split")


def pack_stem_split(w, mask, wp_hi, wp_lo):
    """Stem packing of fp16(w * mask) and of the residual fp16(w * mask - hi) (split operands of the first block)."""
    _need_cuda(w, wp_hi, wp_lo)
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape[1:]) == (3, 3, 3)
    check(L.lib().mcamd_pack_stem_split(ptr(w), ptr(mask), w.shape[0], ptr(wp_hi), ptr(wp_lo), stream_ptr()), "mcamd_pack_stem_split")


def stem_block_bwd(B, H, W, x, wp, gamma, scale, shift, mean, invstd, slope, g, g_ld, g_choff, dw, dgamma, dbeta, workspace,
                   mask=None, grad_scale=1.0):
    """Backward of stem_block_fwd (training mode) from the gradient `g` wrt the pooled output: dW (OIHW, x mask),
    dgamma, dbeta.  `workspace` must be the one the forward call of this step used."""
    _need_cuda(g, dw)
    d = _stem_desc(B, H, W, x, wp, gamma, None, scale, shift, mean, invstd, slope)
    d.g, d.g_ld, d.g_choff = g.data_ptr(), g_ld, g_choff
    d.mask = mask.data_ptr() if mask is not None else None
    d.grad_scale = grad_scale
    d.dw = dw.data_ptr()
    d.dgamma = dgamma.data_ptr() if dgamma is not None else None
    d.dbeta = dbeta.data_ptr() if dbeta is not None else None
    check(L.lib().mcamd_stem_block_bwd(C.byref(d), ptr(workspace), workspace.numel(), stream_ptr()), "mcamd_stem_block_bwd")


def nchw_to_padded(src, dst, dst_ld, dst_choff=0, mul=1.0, overflow=None, pad=0):
    """fp32 NCHW tensor -> channels [choff, choff+C) of a padded NHWC fp16 buffer (pad=1: shared-halo form)."""
    _need_cuda(src, dst)
    assert src.dtype == torch.float32 and src.is_contiguous()
    B, C_, H, W = src.shape
    if pad:
        check(L.lib().mcamd_nchw_f32_to_padded_nhwc_f16_pad(ptr(src), B, C_, H, W, mul, ptr(dst), dst_ld, dst_choff, 1,
                                                            ptr(overflow), stream_ptr()), "mcamd_nchw_f32_to_padded_nhwc_f16_pad")
        return
    check(L.lib().mcamd_nchw_f32_to_padded_nhwc_f16(ptr(src), B, C_, H, W, mul, ptr(dst), dst_ld, dst_choff,
                                                    ptr(overflow), stream_ptr()), "mcamd_nchw_f32_to_padded_nhwc_f16")


def nchw_to_padded_split(src, dst, dst_ld, dst_choff, plane):
    """fp32 NCHW image -> hi | lo | hi planes (`plane` channels apart) of a padded NHWC fp16 buffer."""
    _need_cuda(src, dst)
    assert src.dtype == torch.float32 and src.is_contiguous()
    B, C_, H, W = src.shape
    check(L.lib().mcamd_nchw_f32_to_padded_nhwc_f16_split(ptr(src), B, C_, H, W, ptr(dst), dst_ld, dst_choff, plane,
                                                          stream_ptr()), "mcamd_nchw_f32_to_padded_nhwc_f16_split")


def stem_conv_f32_stats_rows():
    return int(L.lib().mcamd_stem_conv_f32_stats_rows())


def stem_conv_f32(x, w, mask, weff_scratch, y, y_ld, stats=None):
    """The first convolution (3 -> 32 channels, 3x3, pad 1) in fp32 from the fp32 NCHW image: y fp32 [B*H*W][y_ld];
    `stats` fp32 [stem_conv_f32_stats_rows()][2][ld] receives the per-workgroup sums for mcamd_bn_coeffs."""
    _need_cuda(x, w, mask, weff_scratch, y, stats)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[1] == 3
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape[1:]) == (3, 3, 3)
    assert mask is None or (mask.dtype == torch.float32 and mask.is_contiguous() and mask.shape == w.shape)
    assert weff_scratch.dtype == torch.float32 and weff_scratch.numel() >= w.numel() and y.dtype == torch.float32
    B, _, H, W = x.shape
    assert y.numel() >= B * H * W * y_ld
    srows, sld = (stats.shape[0], stats.shape[2]) if stats is not None else (0, 0)
    check(L.lib().mcamd_stem_conv_f32(ptr(x), B, H, W, ptr(w), ptr(mask), w.shape[0], ptr(weff_scratch), ptr(y), y_ld, ptr(stats),
                                      srows, sld, stream_ptr()), "mcamd_stem_conv_f32")


def region_loss(output, target, anchors, num_anchors, num_classes, coord_scale, noobject_scale, object_scale, class_scale, thresh,
                want_counts=False):
    """Loss (0-dim fp32 tensor), d(loss)/d(output) and optionally the (nGT, nCorrect) counters of the YOLOv2 region loss in
    one library call (include/mcamd.h, mcamd_region_desc; reference nets.py:282-635)."""
    _need_cuda(output, target)
    assert output.dtype == torch.float32 and output.is_contiguous() and output.dim() == 4
    B, ch, H, W = output.shape
    if ch != num_anchors * (5 + num_classes):
        raise L.McamdError("region_loss: %d channels, expected %d anchors x (5 + %d classes)" % (ch, num_anchors, num_classes))
    tgt = target.detach().to(device=output.device, dtype=torch.float32).contiguous().view(B, -1)
    if tgt.shape[1] % 5 or len(anchors) < 2 * num_anchors:
        raise L.McamdError("region_loss: target rows must hold (class, x, y, w, h) boxes; anchors %d pairs" % num_anchors)
    d = L.RegionDesc()
    d.output, d.target = output.data_ptr(), tgt.data_ptr()
    d.B, d.H, d.W, d.num_anchors, d.num_classes, d.max_boxes = B, H, W, num_anchors, num_classes, tgt.shape[1] // 5
    step = len(anchors) // num_anchors
    for n in range(num_anchors):
        d.anchors[2 * n], d.anchors[2 * n + 1] = float(anchors[step * n]), float(anchors[step * n + 1])
    d.coord_scale, d.noobject_scale, d.object_scale = float(coord_scale), float(noobject_scale), float(object_scale)
    d.class_scale, d.thresh = float(class_scale), float(thresh)
    loss = torch.empty((), dtype=torch.float32, device=output.device)
    grad = torch.empty_like(output)
    counts = torch.zeros(2, dtype=torch.int32, device=output.device) if want_counts else None
    ws = torch.empty(int(L.lib().mcamd_region_loss_workspace_bytes(B)), dtype=torch.uint8, device=output.device)
    check(L.lib().mcamd_region_loss(C.byref(d), ptr(loss), ptr(grad), ptr(counts), ptr(ws), ws.numel(), stream_ptr()),
          "mcamd_region_loss")
    return loss, grad, counts


def distill_loss(student, teacher, num_anchors, num_classes, obj_scale=1.0, box_scale=1.0, cls_scale=1.0, temperature=1.0):
    """(loss, grad): the objectness-scaled distillation loss of the student's logits against the teacher's (0-dim fp32
    tensor) and d(loss)/d(student), in one library call (include/mcamd.h, mcamd_distill_desc; csrc/distill_loss.hip)."""
    if student.device != teacher.device:
        raise L.McamdError("distill_loss: student on %s, teacher on %s" % (student.device, teacher.device))
    _need_cuda(student, teacher)
    if tuple(student.shape) != tuple(teacher.shape) or student.dim() != 4:
        raise L.McamdError("distill_loss: student logits %s, teacher logits %s: both must be one [B, A*(5+C), H, W] shape"
                           % (tuple(student.shape), tuple(teacher.shape)))
    B, ch, H, W = student.shape
    if ch != num_anchors * (5 + num_classes):
        raise L.McamdError("distill_loss: %d channels, expected %d anchors x (5 + %d classes)" % (ch, num_anchors, num_classes))
    s = student.detach().contiguous().float()
    t = teacher.detach().contiguous().float()
    d = L.DistillDesc()
    d.student, d.teacher = s.data_ptr(), t.data_ptr()
    d.B, d.H, d.W, d.num_anchors, d.num_classes = B, H, W, num_anchors, num_classes
    d.obj_scale, d.box_scale, d.cls_scale, d.temperature = float(obj_scale), float(box_scale), float(cls_scale), float(temperature)
    loss = torch.empty((), dtype=torch.float32, device=s.device)
    grad = torch.empty_like(s)
    ws = torch.empty(int(L.lib().mcamd_distill_loss_workspace_bytes(B, num_anchors)), dtype=torch.uint8, device=s.device)
    check(L.lib().mcamd_distill_loss(C.byref(d), ptr(loss), ptr(grad), ptr(ws), ws.numel(), stream_ptr()), "mcamd_distill_loss")
    return loss, grad


# ------------------------------------------------------------------ detection post-processing (csrc/detect.hip)
DETECT_MAX_ROWS = 2048      # rows (cells x anchors) per image the kernels hold in LDS


def _detect_desc(output, anchors, num_anchors, num_classes, conf_thresh=0.0, nms_thresh=0.0):
    _need_cuda(output)
    assert output.dtype == torch.float32 and output.is_contiguous() and output.dim() == 4
    B, ch, H, W = output.shape
    if ch != num_anchors * (5 + num_classes):
        raise L.McamdError("detect: %d channels, expected %d anchors x (5 + %d classes)" % (ch, num_anchors, num_classes))
    if num_anchors < 1 or len(anchors) < 2 * num_anchors:
        raise L.McamdError("detect: %d anchor values for %d anchors" % (len(anchors), num_anchors))
    d = L.DetectDesc()
    d.output = output.data_ptr()
    d.B, d.H, d.W, d.num_anchors, d.num_classes = B, H, W, num_anchors, num_classes
    step = len(anchors) // num_anchors
    for n in range(min(num_anchors, 8)):
        d.anchors[2 * n], d.anchors[2 * n + 1] = float(anchors[step * n]), float(anchors[step * n + 1])
    d.conf_thresh, d.nms_thresh = float(conf_thresh), float(nms_thresh)
    return d, B, H * W * num_anchors


def region_decode(output, anchors, num_anchors, num_classes):
    """head [B, N, 7], cls_conf [B, N, C] of nets2_utils.region_boxes_tensors in one library call (mcamd_region_decode)."""
    d, B, N = _detect_desc(output, anchors, num_anchors, num_classes)
    head = torch.empty(B, N, 7, dtype=torch.float32, device=output.device)
    cls = torch.empty(B, N, num_classes, dtype=torch.float32, device=output.device)
    check(L.lib().mcamd_region_decode(C.byref(d), ptr(head), ptr(cls), stream_ptr()), "mcamd_region_decode")
    return head, cls


def nms(boxes, conf, nms_thresh):
    """(order int32 [B, n], kept uint8 [B, n]) of nets2_utils.nms_tensors in one library call (mcamd_nms)."""
    _need_cuda(boxes, conf)
    boxes, conf = boxes.detach().float().contiguous(), conf.detach().float().contiguous()
    assert boxes.dim() == 3 and boxes.shape[2] == 4 and conf.shape == boxes.shape[:2]
    B, n = conf.shape
    order = torch.empty(B, n, dtype=torch.int32, device=boxes.device)
    kept = torch.empty(B, n, dtype=torch.uint8, device=boxes.device)
    check(L.lib().mcamd_nms(ptr(boxes), ptr(conf), B, n, float(nms_thresh), ptr(order), ptr(kept), stream_ptr()), "mcamd_nms")
    return order, kept


def detect(output, anchors, num_anchors, num_classes, conf_thresh, nms_thresh, want_decode=False):
    """Decode, threshold, sort, greedy NMS and compaction in one launch (mcamd_detect): rows [B, N, 8], probs [B, N, C],
    nkept int32 [B]; rows at or beyond nkept[b] are unspecified.  want_decode adds the full (head, cls_conf)."""
    d, B, N = _detect_desc(output, anchors, num_anchors, num_classes, conf_thresh, nms_thresh)
    dev = output.device
    rows = torch.empty(B, N, 8, dtype=torch.float32, device=dev)
    probs = torch.empty(B, N, num_classes, dtype=torch.float32, device=dev)
    nkept = torch.empty(B, dtype=torch.int32, device=dev)
    head = torch.empty(B, N, 7, dtype=torch.float32, device=dev) if want_decode else None
    cls = torch.empty(B, N, num_classes, dtype=torch.float32, device=dev) if want_decode else None
    check(L.lib().mcamd_detect(C.byref(d), ptr(rows), ptr(probs), ptr(nkept), ptr(head), ptr(cls), stream_ptr()), "mcamd_detect")
    return (rows, probs, nkept, head, cls) if want_decode else (rows, probs, nkept)


# ------------------------------------------------------------------ VOC07 evaluation (csrc/voc_eval.hip)
VOC_MAX_OBJECTS = 64        # ground-truth objects per image: one lane of a wave each
VOC_KEY_CLASS_SHIFT, VOC_KEY_SCORE_SHIFT, VOC_KEY_IMAGE_SHIFT = 56, 36, 11      # key layout, include/mcamd.h


def _voc_tensor(t, dtype, shape, name):
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise L.McamdError("voc_match: `%s` must be a contiguous %s tensor of shape %s, got %s %s"
                           % (name, dtype, tuple(shape), t.dtype, tuple(t.shape)))


def voc_match(rows, probs, nkept, conf_thresh, ovthresh, first_image, gt_box, gt_cls, gt_difficult, gt_count, image_size,
              keys, flags, counters):
    """Append the batch's detection records (64-bit sort key, tp / fp / neither flag) to keys / flags (mcamd_voc_match);
    counters int64 [2] = records so far, records lost to the capacity.  No allocation, no host synchronisation."""
    _need_cuda(rows, probs, nkept, gt_box, gt_cls, gt_difficult, gt_count, image_size, keys, flags, counters)
    if rows.dim() != 3 or probs.dim() != 3 or gt_box.dim() != 3:
        raise L.McamdError("voc_match: rows [B, N, 8], probs [B, N, C] and gt_box [B, G, 4] expected")
    B, N, C_ = probs.shape
    G = gt_box.shape[1]
    _voc_tensor(rows, torch.float32, (B, N, 8), "rows")
    _voc_tensor(probs, torch.float32, (B, N, C_), "probs")
    _voc_tensor(nkept, torch.int32, (B,), "nkept")
    _voc_tensor(gt_box, torch.int32, (B, G, 4), "gt_box")
    _voc_tensor(gt_cls, torch.uint8, (B, G), "gt_cls")
    _voc_tensor(gt_difficult, torch.uint8, (B, G), "gt_difficult")
    _voc_tensor(gt_count, torch.int32, (B,), "gt_count")
    _voc_tensor(image_size, torch.int32, (B, 2), "image_size")
    _voc_tensor(keys, torch.int64, (keys.numel(),), "keys")
    _voc_tensor(flags, torch.uint8, (keys.numel(),), "flags")
    _voc_tensor(counters, torch.int64, (2,), "counters")
    d = L.VocMatchDesc()
    d.rows, d.probs, d.nkept = rows.data_ptr(), probs.data_ptr(), nkept.data_ptr()
    d.B, d.N, d.C, d.G = B, N, C_, G
    d.conf_thresh, d.ovthresh, d.first_image = float(conf_thresh), float(ovthresh), int(first_image)
    d.gt_box, d.gt_cls, d.gt_difficult = gt_box.data_ptr(), gt_cls.data_ptr(), gt_difficult.data_ptr()
    d.gt_count, d.image_size = gt_count.data_ptr(), image_size.data_ptr()
    d.keys, d.flags, d.capacity, d.counters = keys.data_ptr(), flags.data_ptr(), keys.numel(), counters.data_ptr()
    check(L.lib().mcamd_voc_match(C.byref(d), stream_ptr()), "mcamd_voc_match")


def voc_ap(keys, flags, counters, npos, want_curves=False):
    """Per-class VOC07 AP (float64 [C]) of the records SORTED by key (mcamd_voc_ap); want_curves adds rec and prec at the
    records' sorted positions (float64, the capacity long)."""
    _need_cuda(keys, flags, counters, npos)
    _voc_tensor(keys, torch.int64, (keys.numel(),), "keys")
    _voc_tensor(flags, torch.uint8, (keys.numel(),), "flags")
    _voc_tensor(counters, torch.int64, (2,), "counters")
    _voc_tensor(npos, torch.int32, (npos.numel(),), "npos")
    ap = torch.empty(npos.numel(), dtype=torch.float64, device=keys.device)
    rec = torch.zeros(keys.numel(), dtype=torch.float64, device=keys.device) if want_curves else None
    prec = torch.zeros(keys.numel(), dtype=torch.float64, device=keys.device) if want_curves else None
    check(L.lib().mcamd_voc_ap(ptr(keys), ptr(flags), ptr(counters), keys.numel(), ptr(npos), npos.numel(), ptr(ap), ptr(rec),
                               ptr(prec), stream_ptr()), "mcamd_voc_ap")
    return (ap, rec, prec) if want_curves else ap


# ------------------------------------------------------------------ launch plans
class Plan:
    """A recorded sequence of library calls (include/mcamd.h, "Launch plans"), replayed with one call per segment."""

    def __init__(self, streams):
        self.streams = list(streams)
        self._arr = (C.c_void_p * len(self.streams))(*[s.cuda_stream for s in self.streams])
        self.handle = None
        self.key = None
        self.keep = None          # whatever must stay alive while the plan holds its pointers

    def __enter__(self):
        check(L.lib().mcamd_plan_begin(self._arr, len(self.streams)), "mcamd_plan_begin")
        return self

    def __exit__(self, et, ev, tb):
        h = L.lib().mcamd_plan_end()
        if et is not None:
            if h:
                L.lib().mcamd_plan_destroy(h)
            return False
        if not h:
            raise L.McamdError("recording a launch plan failed: %s" % L.lib().mcamd_last_error().decode())
        self.handle = h
        self.segments = int(L.lib().mcamd_plan_segments(h))
        self.launches = int(L.lib().mcamd_plan_launches(h))
        return False

    def mark(self):
        return int(L.lib().mcamd_plan_mark())

    def run(self, lo=0, hi=None):
        check(L.lib().mcamd_plan_run(self.handle, lo, self.segments if hi is None else hi, self._arr, len(self.streams)),
              "mcamd_plan_run")

    def __del__(self):
        h, self.handle = self.handle, None
        if h:
            try:
                L.lib().mcamd_plan_destroy(h)
            except Exception:
                pass


def stream_wait(waiter, signal):
    """`waiter` (torch stream) waits for everything enqueued so far on `signal`.  Recordable."""
    check(L.lib().mcamd_stream_wait(C.c_void_p(waiter.cuda_stream), C.c_void_p(signal.cuda_stream)), "mcamd_stream_wait")


def memset_zero(t):
    """Zero a contiguous tensor on the current stream through the library (recordable, unlike Tensor.zero_())."""
    assert t.is_contiguous()
    check(L.lib().mcamd_memset_zero(ptr(t), t.numel() * t.element_size(), stream_ptr()), "mcamd_memset_zero")


# ------------------------------------------------------------------ pruning
def step_flags(engine_flags, loss, transport_flag, flags, found):
    """train.StepGuard's device-side decision in one launch (mcamd_step_flags): flags = [any engine overflow, loss not finite,
    transport overflow] (the int flags read are reset), found = their sum.  All arguments but `flags` may be None / empty."""
    _need_cuda(flags, found, loss, transport_flag, *engine_flags)
    assert flags.dtype == torch.float32 and flags.numel() >= 3 and len(engine_flags) <= 8
    assert all(f.dtype == torch.int32 for f in engine_flags) and (transport_flag is None or transport_flag.dtype == torch.int32)
    assert loss is None or (loss.dtype == torch.float32 and loss.numel() == 1)
    arr = (C.c_void_p * max(1, len(engine_flags)))(*[f.data_ptr() for f in engine_flags])
    check(L.lib().mcamd_step_flags(arr, len(engine_flags), ptr(loss), ptr(transport_flag), ptr(flags), ptr(found), stream_ptr()),
          "mcamd_step_flags")


def kth_magnitude(tensors, k):
    """-> device fp32[2] = (s[k], s[min(k+1, n-1)]) of the ascending |w| over all tensors."""
    _need_cuda(*tensors)
    n = len(tensors)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    counts = (C.c_int64 * n)(*[t.numel() for t in tensors])
    dev = tensors[0].device
    out = torch.empty(2, dtype=torch.float32, device=dev)
    ws = torch.empty(int(L.lib().mcamd_kth_magnitude_workspace_bytes()), dtype=torch.uint8, device=dev)
    check(L.lib().mcamd_kth_magnitude(ptrs, counts, n, k, ptr(out), ptr(ws), ws.numel(), stream_ptr()),
          "mcamd_kth_magnitude")
    return out


def magnitude_mask(w, thr_dev):
    mask = torch.empty_like(w)
    check(L.lib().mcamd_magnitude_mask(ptr(w), w.numel(), ptr(thr_dev), ptr(mask), stream_ptr()), "mcamd_magnitude_mask")
    return mask


def filter_scores(w):
    O, I, kh, kw = w.shape
    scores = torch.empty(O, dtype=torch.float32, device=w.device)
    ws = torch.empty(int(L.lib().mcamd_filter_scores_workspace_bytes(O)), dtype=torch.uint8, device=w.device)
    check(L.lib().mcamd_filter_scores(ptr(w), O, I, kh, kw, ptr(scores), ptr(ws), ws.numel(), stream_ptr()),
          "mcamd_filter_scores")
    return scores


def filter_mean_square(w):
    O, I, kh, kw = w.shape
    ms = torch.empty(O, dtype=torch.float32, device=w.device)
    ws = torch.empty(int(L.lib().mcamd_filter_scores_workspace_bytes(O)), dtype=torch.uint8, device=w.device)
    check(L.lib().mcamd_filter_mean_square(ptr(w), O, I, kh, kw, ptr(ms), ptr(ws), ws.numel(), stream_ptr()),
          "mcamd_filter_mean_square")
    return ms


def filter_mask(keep_i32, shape):
    O = shape[0]
    per = 1
    for s in shape[1:]:
        per *= s
    mask = torch.empty(shape, dtype=torch.float32, device=keep_i32.device)
    check(L.lib().mcamd_filter_mask(ptr(keep_i32), O, per, ptr(mask), stream_ptr()), "mcamd_filter_mask")
    return mask


def count_zeros(tensors):
    dev = tensors[0].device
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    for t in tensors:
        check(L.lib().mcamd_count_zeros(ptr(t), t.numel(), ptr(out), stream_ptr()), "mcamd_count_zeros")
    return int(out.item())


def masked_residual(ws, masks):
    dev = ws[0].device
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    for w, m in zip(ws, masks):
        check(L.lib().mcamd_masked_residual(ptr(w), ptr(m), w.numel(), ptr(out), stream_ptr()), "mcamd_masked_residual")
    return float(out.item())


# ----------------------------------------------------------------------------- 2:4 structured sparsity
def nm_mask(w, old_mask=None, n=2, m=4):
    """N:M magnitude mask of an OIHW fp32 tensor (mcamd_nm_mask): per group of 4 consecutive input channels at a fixed
    (filter, tap), the 2 largest |w * old_mask| keep their old mask value; ties keep the lower channel."""
    _need_cuda(w, old_mask)
    O, I = w.shape[0], w.shape[1]
    khw = w.numel() // (O * I)
    mask = torch.empty_like(w)
    check(L.lib().mcamd_nm_mask(ptr(w), ptr(old_mask), O, I, khw, n, m, ptr(mask), stream_ptr()), "mcamd_nm_mask")
    return mask


def nm_violations(mask, out=None):
    """Device int32 count of the mask's groups of 4 input channels with more than 2 non-zeros (added to `out`)."""
    _need_cuda(mask)
    O, I = mask.shape[0], mask.shape[1]
    if out is None:
        out = torch.zeros(1, dtype=torch.int32, device=mask.device)
    check(L.lib().mcamd_nm_violations(ptr(mask), O, I, mask.numel() // (O * I), ptr(out), stream_ptr()), "mcamd_nm_violations")
    return out


def conv_fwd_sparse24_ok(g):
    """Does mcamd_conv_fwd_sparse24 accept this geometry?  (Shared by the engine and the tests.)"""
    return bool(L.lib().mcamd_conv_fwd_sparse24_ok(C.byref(g)))


def sparse24_elems(g):
    out = (C.c_int64 * 2)()
    check(L.lib().mcamd_sparse24_elems(C.byref(g), out), "mcamd_sparse24_elems")
    return int(out[0]), int(out[1])


Sparse24Info = collections.namedtuple("Sparse24Info", "bmw bnp bk stages mtiles ntiles grid")


def conv_fwd_sparse24_info(g):
    """The sparse24_kernel instance conv_fwd_sparse24 launches for `g` (a tile of bmw filters x bnp pixels, K chunks of bk,
    LDS ring stages), its tiles along the pixels and the filters and its grid: mcamd_conv_fwd_sparse24_info, the launch's
    own choice.  Needs no GPU."""
    out = (C.c_int32 * 7)()
    check(L.lib().mcamd_conv_fwd_sparse24_info(C.byref(g), out), "mcamd_conv_fwd_sparse24_info")
    return Sparse24Info(*out)


def pack_sparse24(g, w, mask=None, out_vals=None, out_idx=None):
    """fp32 OIHW master (* mask) -> (fp16 kept values, int16 index words) of the 2:4 forward (mcamd_pack_sparse24)."""
    _need_cuda(w, mask)
    assert w.dtype == torch.float32 and w.is_contiguous()
    nv, ni = sparse24_elems(g)
    if out_vals is None:
        out_vals = torch.empty(nv, dtype=HALF, device=w.device)
    if out_idx is None:
        out_idx = torch.empty(ni, dtype=torch.int16, device=w.device)
    if out_vals.numel() < nv or out_idx.numel() < ni:
        raise L.McamdError("pack_sparse24: destination too small")
    check(L.lib().mcamd_pack_sparse24(C.byref(g), ptr(w), ptr(mask), ptr(out_vals), ptr(out_idx), stream_ptr()),
          "mcamd_pack_sparse24")
    return out_vals, out_idx


def conv_fwd_sparse24(g, x, wsp, idx, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None, y2_ld=0,
                      y2_choff=0, overflow=None):
    """conv_fwd_padded on 2:4-packed weights (v_smfmac): the same inference epilogue, arguments and output.
    `overflow`: optional int32 flag, set to 1 when an output was clamped to +-65504."""
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    check(L.lib().mcamd_conv_fwd_sparse24(C.byref(g), ptr(x), ptr(wsp), ptr(idx), C.byref(e), stream_ptr()),
          "mcamd_conv_fwd_sparse24")


# ----------------------------------------------------------------------------- block sparsity
BLOCK_FILTERS = 64      # filters per block of block_prune = the N tile of conv_fwd_bsparse


def block_kb(cin):
    """Channels per block: the channel block of the packed K axis (include/mcamd.h), for cin % 32 == 0."""
    return 64 if cin % 64 == 0 else 32


def block_scores(w, old_mask=None):
    """float64 mean of (w * old_mask)^2 per block [fb][cb][tap] of an OIHW fp32 tensor with cin % 32 == 0
    (mcamd_block_scores: fixed summation order, no atomics)."""
    _need_cuda(w, old_mask)
    assert w.dtype == torch.float32 and w.is_contiguous() and (old_mask is None or old_mask.is_contiguous())
    O, I = w.shape[0], w.shape[1]
    khw = w.numel() // (O * I)
    scores = torch.empty(((O + BLOCK_FILTERS - 1) // BLOCK_FILTERS) * (I // block_kb(I)) * khw, dtype=torch.float64, device=w.device)
    check(L.lib().mcamd_block_scores(ptr(w), ptr(old_mask), O, I, khw, ptr(scores), stream_ptr()), "mcamd_block_scores")
    return scores


def block_mask(keep_i32, shape, old_mask=None):
    """old_mask (ones when None) with the blocks whose keep flag is 0 zeroed (mcamd_block_mask)."""
    _need_cuda(keep_i32, old_mask)
    O, I = shape[0], shape[1]
    khw = 1
    for s in shape[2:]:
        khw *= s
    nblocks = ((O + BLOCK_FILTERS - 1) // BLOCK_FILTERS) * (I // block_kb(I)) * khw
    if keep_i32.dtype != torch.int32 or not keep_i32.is_contiguous() or keep_i32.numel() != nblocks:
        raise L.McamdError("block_mask: keep must be a contiguous CUDA int32 vector of %d entries" % nblocks)
    mask = torch.empty(tuple(shape), dtype=torch.float32, device=keep_i32.device)
    check(L.lib().mcamd_block_mask(ptr(keep_i32), ptr(old_mask), O, I, khw, ptr(mask), stream_ptr()), "mcamd_block_mask")
    return mask


def conv_fwd_bsparse_ok(g):
    """Does mcamd_conv_fwd_bsparse accept this geometry?  (Shared by the engine and the tests.)"""
    return bool(L.lib().mcamd_conv_fwd_bsparse_ok(C.byref(g)))


def bsparse_elems(g):
    """(ntiles, ntiles * nchunks): int32 entries of the counts and of the lists."""
    out = (C.c_int64 * 2)()
    check(L.lib().mcamd_bsparse_elems(C.byref(g), out), "mcamd_bsparse_elems")
    return int(out[0]), int(out[1])


def bsparse_lists(g, wp, out_count=None, out_list=None):
    """Packed fp16 forward weights -> (count int32[ntiles], list int32[ntiles][nchunks]): per 64-filter tile the K chunks
    holding a non-zero weight, ascending (mcamd_bsparse_lists; no host synchronisation)."""
    _need_cuda(wp)
    nc, nl = bsparse_elems(g)
    if out_count is None:
        out_count = torch.empty(nc, dtype=torch.int32, device=wp.device)
    if out_list is None:
        out_list = torch.empty(nc, nl // nc, dtype=torch.int32, device=wp.device)
    if out_count.numel() != nc or out_list.numel() != nl or wp.numel() < packed_elems(g)[0]:
        raise L.McamdError("bsparse_lists: operand sizes do not fit the geometry")
    check(L.lib().mcamd_bsparse_lists(C.byref(g), ptr(wp), ptr(out_count), ptr(out_list), stream_ptr()), "mcamd_bsparse_lists")
    return out_count, out_list


BsparseInfo = collections.namedtuple("BsparseInfo", "bm bn bk stages mtiles ntiles grid")


def conv_fwd_bsparse_info(g):
    """The kernel instance conv_fwd_bsparse launches for `g`: a tile of bm pixels (MCAMD_BSPARSE_BM) x bn filters, K chunks
    of bk, LDS ring stages, its tiles along the pixels and the filters and its grid: mcamd_conv_fwd_bsparse_info, the
    launch's own choice.  Needs no GPU."""
    out = (C.c_int32 * 7)()
    check(L.lib().mcamd_conv_fwd_bsparse_info(C.byref(g), out), "mcamd_conv_fwd_bsparse_info")
    return BsparseInfo(*out)


def conv_fwd_bsparse(g, x, wp, count, lst, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None, y2_ld=0,
                     y2_choff=0, all_chunks=False, overflow=None):
    """conv_fwd_padded over the listed K chunks of each 64-filter tile (bsparse_lists): the same inference epilogue,
    arguments and output.  all_chunks=True (tests, tools/bsparse_bench.py) runs the same launch with full lists.
    `overflow`: optional int32 flag, set to 1 when an output was clamped to +-65504."""
    nc, nl = bsparse_elems(g)
    if all_chunks:
        nch = nl // nc
        count = torch.full((nc,), nch, dtype=torch.int32, device=x.device)
        lst = torch.arange(nch, dtype=torch.int32, device=x.device).repeat(nc, 1).contiguous()
    _need_cuda(x, count, lst)
    if count.dtype != torch.int32 or lst.dtype != torch.int32 or count.numel() != nc or lst.numel() != nl or not lst.is_contiguous():
        raise L.McamdError("conv_fwd_bsparse: count / list must be contiguous int32 of %d / %d entries" % (nc, nl))
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    check(L.lib().mcamd_conv_fwd_bsparse(C.byref(g), ptr(x), ptr(wp), ptr(count), ptr(lst), C.byref(e), stream_ptr()),
          "mcamd_conv_fwd_bsparse")


# ... the training form: raw fp16 epilogue, forward and dgrad (Darknet.sparse_train = "block")
def conv_bsparse_train_ok(g, dgrad=False):
    """Does conv_fwd_bsparse_raw (dgrad=False) / conv_dgrad_bsparse (dgrad=True) accept this geometry?  Needs no GPU."""
    return bool(L.lib().mcamd_conv_bsparse_train_ok(C.byref(g), 1 if dgrad else 0))


def conv_bsparse_train_info(g, dgrad=False):
    """BsparseInfo of the instance that launch takes (mcamd_conv_bsparse_train_info, the launch's own choice).  Needs no GPU."""
    out = (C.c_int32 * 7)()
    check(L.lib().mcamd_conv_bsparse_train_info(C.byref(g), 1 if dgrad else 0, out), "mcamd_conv_bsparse_train_info")
    return BsparseInfo(*out)


def bsparse_raw_stats_rows(g, dgrad=False):
    """Rows of the statistics slab of conv_fwd_bsparse_raw: one per pixel tile (0: geometry refused)."""
    return int(L.lib().mcamd_conv_bsparse_raw_stats_rows(C.byref(g), 1 if dgrad else 0))


def bsparse_elems_dgrad(g):
    """(ntiles, ntiles * nchunks) of the lists over the dgrad packing: ntiles = ceil(cin / 64), nchunks = k*k * cout_p / kb_d."""
    out = (C.c_int64 * 2)()
    check(L.lib().mcamd_bsparse_elems_dgrad(C.byref(g), out), "mcamd_bsparse_elems_dgrad")
    return int(out[0]), int(out[1])


def bsparse_lists_dgrad(g, wpd, out_count=None, out_list=None):
    """bsparse_lists on the packed dgrad weights: per 64-input-channel tile the K chunks (cout block, flipped tap) holding a
    non-zero weight, ascending (mcamd_bsparse_lists_dgrad; no host synchronisation)."""
    _need_cuda(wpd)
    nc, nl = bsparse_elems_dgrad(g)
    if out_count is None:
        out_count = torch.empty(nc, dtype=torch.int32, device=wpd.device)
    if out_list is None:
        out_list = torch.empty(nc, nl // nc, dtype=torch.int32, device=wpd.device)
    if out_count.numel() != nc or out_list.numel() != nl or wpd.numel() < packed_elems(g)[1]:
        raise L.McamdError("bsparse_lists_dgrad: operand sizes do not fit the geometry")
    check(L.lib().mcamd_bsparse_lists_dgrad(C.byref(g), ptr(wpd), ptr(out_count), ptr(out_list), stream_ptr()),
          "mcamd_bsparse_lists_dgrad")
    return out_count, out_list


def bsparse_full_lists(nc, nl, device):
    """(count, list) naming every chunk of every tile: what all_chunks=True launches on."""
    nch = nl // nc
    return (torch.full((nc,), nch, dtype=torch.int32, device=device),
            torch.arange(nch, dtype=torch.int32, device=device).repeat(nc, 1).contiguous())


def _check_lists(what, x, count, lst, nc, nl):
    _need_cuda(x, count, lst)
    if count.dtype != torch.int32 or lst.dtype != torch.int32 or count.numel() != nc or lst.numel() != nl or not lst.is_contiguous():
        raise L.McamdError("%s: count / list must be contiguous int32 of %d / %d entries" % (what, nc, nl))


def conv_fwd_bsparse_raw(g, x, wp, count, lst, y, y_ld, y_choff=0, stats=None, all_chunks=False, overflow=None):
    """conv_fwd_raw over the listed K chunks of each 64-filter tile: y[M][y_ld] fp16 raw (saturated, `overflow` flag);
    `stats`: fp32 [bsparse_raw_stats_rows(g)][2][stats_ld] slab or None.  all_chunks=True: the same launch on full lists."""
    nc, nl = bsparse_elems(g)
    if all_chunks:
        count, lst = bsparse_full_lists(nc, nl, x.device)
    _check_lists("conv_fwd_bsparse_raw", x, count, lst, nc, nl)
    e = _epi(L.EPI_RAW_F16, y, y_ld, y_choff, stats=stats, stats_rows_=stats.shape[0] if stats is not None else 0,
             stats_ld=stats.shape[2] if stats is not None else 0, overflow=overflow)
    check(L.lib().mcamd_conv_fwd_bsparse_raw(C.byref(g), ptr(x), ptr(wp), ptr(count), ptr(lst), C.byref(e), stream_ptr()),
          "mcamd_conv_fwd_bsparse_raw")


def conv_dgrad_bsparse(g, dy, dy_ld, dy_choff, wpd, count, lst, out, out_ld, out_choff=0, overflow=None, concurrent=False,
                       all_chunks=False):
    """conv_dgrad_raw over the listed K chunks of each 64-input-channel tile (bsparse_lists_dgrad).  `concurrent` is passed
    on and ignored by the library (one tile shape).  all_chunks=True: the same launch on full lists."""
    nc, nl = bsparse_elems_dgrad(g)
    if all_chunks:
        count, lst = bsparse_full_lists(nc, nl, dy.device)
    _check_lists("conv_dgrad_bsparse", dy, count, lst, nc, nl)
    e = _epi(L.EPI_RAW_F16, out, out_ld, out_choff, overflow=overflow)
    e.concurrent = 1 if concurrent else 0
    check(L.lib().mcamd_conv_dgrad_bsparse(C.byref(g), ptr(dy), dy_ld, dy_choff, ptr(wpd), ptr(count), ptr(lst), C.byref(e),
                                           stream_ptr()), "mcamd_conv_dgrad_bsparse")


# ----------------------------------------------------------------------------- split-K forward (low-batch inference)
def conv_fwd_splitk_info(g, mode, dst_mode=0, slices=0):
    """mcamd_splitk_info of a split-K forward of `g` with epilogue `mode` (L.EPI_PAD_F16 / L.EPI_RAW_F16): host logic only.
    slices = 0 asks the policy (info.slices == 1: it does not split this launch); > 0 sizes a forced slice count."""
    info = SplitkInfo()
    check(L.lib().mcamd_conv_fwd_splitk_info(C.byref(g), mode, dst_mode, slices, C.byref(info)), "mcamd_conv_fwd_splitk_info")
    return info


def _splitk(g, x, wp, e, slices, workspace):
    if workspace is None:
        info = conv_fwd_splitk_info(g, e.mode, e.dst_mode, slices)
        workspace = torch.empty(info.workspace_bytes // 4, dtype=torch.float32, device=x.device)
    _need_cuda(x, workspace)
    check(L.lib().mcamd_conv_fwd_splitk(C.byref(g), ptr(x), ptr(wp), C.byref(e), slices, ptr(workspace),
                                        workspace.numel() * workspace.element_size(), stream_ptr()), "mcamd_conv_fwd_splitk")
    return workspace


def conv_fwd_splitk(g, x, wp, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None, y2_ld=0, y2_choff=0,
                    slices=0, workspace=None, overflow=None):
    """conv_fwd_padded with the K axis cut into `slices` slices (0 = the policy's count): a partial launch into `workspace`
    (fp32, conv_fwd_splitk_info(...).workspace_bytes; None allocates one) and a finish launch with the same epilogue.
    `overflow`: optional int32 flag, set to 1 when an output was clamped to +-65504."""
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    return _splitk(g, x, wp, e, slices, workspace)


def conv_fwd_raw_splitk(g, x, wp, y, y_ld, y_choff=0, slices=0, workspace=None, overflow=None):
    """conv_fwd_raw(..., stats=None) with the K axis cut into `slices` slices: y[M][y_ld] fp16 raw conv output.
    `overflow`: as conv_fwd_splitk."""
    return _splitk(g, x, wp, _epi(L.EPI_RAW_F16, y, y_ld, y_choff, overflow=overflow), slices, workspace)


# ----------------------------------------------------------------------------- fp8 (e4m3) quantised inference
def conv_fwd_q8_ok(g):
    """Does mcamd_conv_fwd_q8 accept this geometry?  (Shared by the engine and the tests.)"""
    return bool(L.lib().mcamd_conv_fwd_q8_ok(C.byref(g)))


def q8_elems(g):
    out = (C.c_int64 * 2)()
    check(L.lib().mcamd_q8_elems(C.byref(g), out), "mcamd_q8_elems")
    return int(out[0]), int(out[1])


def alloc_padded_q8(B, H, W, ld, device, pad=0):
    """Zeroed padded-NHWC BYTE buffer [B][H+2][W+2][ld] of e4m3 activations (halo bytes 0x00 = +0), flat.
    pad=1: the shared-halo form, B (H+1) (W+1) + W + 2 pixels from pixel (0, -1, -1) (training engines, W <= 26)."""
    return torch.zeros(padded_pixels(B, H, W, pad) * ld, dtype=torch.uint8, device=device)


def padded_pixels(B, H, W, pad=0):
    """Pixels (halo included) of a padded activation buffer in the padded (0) / shared-halo (1) form."""
    return B * (H + 1) * (W + 1) + W + 2 if pad else B * (H + 2) * (W + 2)


def padded_view_q8(buf, B, H, W, ld, pad=0):
    """[B][H+2][W+2][ld] view of a byte buffer from alloc_padded_q8 (shared-halo form: overlapping, as padded_view)."""
    if pad:
        return torch.as_strided(buf, (B, H + 2, W + 2, ld), ((H + 1) * (W + 1) * ld, (W + 1) * ld, ld, 1))
    return buf[: B * (H + 2) * (W + 2) * ld].view(B, H + 2, W + 2, ld)


def pack_q8(g, w, mask=None, out_w=None, out_exp=None):
    """fp32 OIHW master (* mask) -> (e4m3 weight bytes in the kernel's K order, int32 exponent per filter) (mcamd_pack_q8)."""
    _need_cuda(w, mask)
    assert w.dtype == torch.float32 and w.is_contiguous()
    nw, ne = q8_elems(g)
    if out_w is None:
        out_w = torch.empty(nw, dtype=torch.uint8, device=w.device)
    if out_exp is None:
        out_exp = torch.empty(ne, dtype=torch.int32, device=w.device)
    if out_w.numel() < nw or out_exp.numel() < ne:
        raise L.McamdError("pack_q8: destination too small")
    check(L.lib().mcamd_pack_q8(C.byref(g), ptr(w), ptr(mask), ptr(out_w), ptr(out_exp), stream_ptr()), "mcamd_pack_q8")
    return out_w, out_exp


Q8_FORM_INFER, Q8_FORM_RAW, Q8_FORM_BORDER, Q8_FORM_SPARSE = 0, 1, 2, 3
Q8Info = collections.namedtuple("Q8Info", "bmw bnp f8mfma stages mtiles ntiles grid")


def conv_fwd_q8_info(g, form=Q8_FORM_INFER):
    """The kernel instance an fp8 block launches for `g` in `form` (Q8_FORM_INFER: conv_fwd_q8; Q8_FORM_RAW: conv_fwd_q8_raw;
    Q8_FORM_BORDER: conv_fwd_q8_slim with a table; Q8_FORM_SPARSE: conv_fwd_q8_sparse24): a tile of bmw filters x bnp pixels,
    whether MCAMD_Q8_MFMA selects the fp8 MFMA, LDS ring stages, its tiles along the pixels and the filters and its grid:
    mcamd_conv_fwd_q8_info, the launches' own choice.  Needs no GPU."""
    out = (C.c_int32 * 7)()
    check(L.lib().mcamd_conv_fwd_q8_info(C.byref(g), int(form), out), "mcamd_conv_fwd_q8_info")
    return Q8Info(*out)


def conv_fwd_q8(g, x8, wq, wexp, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None, y2_ld=0,
                y2_choff=0, y_f8=False, y2_f8=False, overflow=None):
    """The quantised block (mcamd_conv_fwd_q8): e4m3 activations x e4m3 weights, the inference epilogue of conv_fwd_padded
    with `y` / `y2` written as e4m3 bytes (y_f8 / y2_f8) or fp16.
    `overflow`: optional int32 flag, set to 1 when an fp16 output was clamped to +-65504 (bytes saturate silently)."""
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    check(L.lib().mcamd_conv_fwd_q8(C.byref(g), ptr(x8), ptr(wq), ptr(wexp), C.byref(e), int(bool(y_f8)), int(bool(y2_f8)),
                                    stream_ptr()), "mcamd_conv_fwd_q8")


# ... with the K axis cut into slices for low-batch inference (csrc/conv_q8_splitk.hip)
def conv_fwd_q8_splitk_info(g, dst_mode=0, slices=0):
    """mcamd_splitk_info of a split-K fp8 forward of `g`: host logic only.  slices = 0 asks the policy -- conv_fwd_splitk_info's,
    on chunks of 64 k (info.slices == 1: it does not split this launch); > 0 sizes a forced slice count."""
    info = SplitkInfo()
    check(L.lib().mcamd_conv_fwd_q8_splitk_info(C.byref(g), dst_mode, slices, C.byref(info)), "mcamd_conv_fwd_q8_splitk_info")
    return info


def conv_fwd_q8_splitk(g, x8, wq, wexp, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None, y2_ld=0,
                       y2_choff=0, y_f8=False, y2_f8=False, overflow=None, slices=0, workspace=None):
    """conv_fwd_q8 with the K axis cut into `slices` slices (0 = the policy's count): a partial launch into `workspace` (fp32,
    conv_fwd_q8_splitk_info(...).workspace_bytes; None allocates one) and a finish launch with the same epilogue and
    destination formats.  Returns the workspace."""
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    if workspace is None:
        info = conv_fwd_q8_splitk_info(g, dst_mode, slices)
        workspace = torch.empty(info.workspace_bytes // 4, dtype=torch.float32, device=x8.device)
    _need_cuda(x8, workspace)
    check(L.lib().mcamd_conv_fwd_q8_splitk(C.byref(g), ptr(x8), ptr(wq), ptr(wexp), C.byref(e), int(bool(y_f8)), int(bool(y2_f8)),
                                           slices, ptr(workspace), workspace.numel() * workspace.element_size(), stream_ptr()),
          "mcamd_conv_fwd_q8_splitk")
    return workspace


# ... over the non-zero K chunks of each 64-filter tile only (csrc/conv_q8_bsparse.hip)
def conv_fwd_q8_bsparse_ok(g):
    """Does mcamd_conv_fwd_q8_bsparse accept this geometry?  (Shared by the engine and the tests; needs no device.)"""
    return bool(L.lib().mcamd_conv_fwd_q8_bsparse_ok(C.byref(g)))


def q8_bsparse_elems(g):
    """(ntiles, ntiles * nchunks): int32 entries of the counts and of the lists (64-filter tiles, 64-byte chunks)."""
    out = (C.c_int64 * 2)()
    check(L.lib().mcamd_q8_bsparse_elems(C.byref(g), out), "mcamd_q8_bsparse_elems")
    return int(out[0]), int(out[1])


def q8_bsparse_lists(g, wq, out_count=None, out_list=None):
    """pack_q8's weight bytes -> (count int32[ntiles], list int32[ntiles][nchunks]): per 64-filter tile the 64-byte K chunks
    holding a non-zero e4m3 code, ascending (mcamd_q8_bsparse_lists; no host synchronisation)."""
    _need_cuda(wq)
    nc, nl = q8_bsparse_elems(g)
    if out_count is None:
        out_count = torch.empty(nc, dtype=torch.int32, device=wq.device)
    if out_list is None:
        out_list = torch.empty(nc, nl // nc, dtype=torch.int32, device=wq.device)
    if out_count.numel() != nc or out_list.numel() != nl or wq.dtype != torch.uint8 or wq.numel() < q8_elems(g)[0]:
        raise L.McamdError("q8_bsparse_lists: operand sizes do not fit the geometry")
    check(L.lib().mcamd_q8_bsparse_lists(C.byref(g), ptr(wq), ptr(out_count), ptr(out_list), stream_ptr()), "mcamd_q8_bsparse_lists")
    return out_count, out_list


def conv_fwd_q8_bsparse_info(g):
    """The kernel instance conv_fwd_q8_bsparse launches for `g` (Q8Info: always the 64 x 128 tile, 3 stages, the MFMA form
    MCAMD_Q8_MFMA selects): mcamd_conv_fwd_q8_bsparse_info.  Needs no GPU."""
    out = (C.c_int32 * 7)()
    check(L.lib().mcamd_conv_fwd_q8_bsparse_info(C.byref(g), out), "mcamd_conv_fwd_q8_bsparse_info")
    return Q8Info(*out)


def conv_fwd_q8_bsparse(g, x8, wq, wexp, count, lst, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None,
                        y2_ld=0, y2_choff=0, y_f8=False, y2_f8=False, overflow=None, all_chunks=False):
    """conv_fwd_q8 over the listed K chunks of each 64-filter tile (q8_bsparse_lists): the same operands, epilogue,
    destination formats and output.  all_chunks=True (tests, tools/bsparse_bench.py) runs the same launch with full lists."""
    nc, nl = q8_bsparse_elems(g)
    if all_chunks:
        nch = nl // nc
        count = torch.full((nc,), nch, dtype=torch.int32, device=x8.device)
        lst = torch.arange(nch, dtype=torch.int32, device=x8.device).repeat(nc, 1).contiguous()
    _need_cuda(x8, count, lst)
    if count.dtype != torch.int32 or lst.dtype != torch.int32 or count.numel() != nc or lst.numel() != nl or not lst.is_contiguous():
        raise L.McamdError("conv_fwd_q8_bsparse: count / list must be contiguous int32 of %d / %d entries" % (nc, nl))
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    check(L.lib().mcamd_conv_fwd_q8_bsparse(C.byref(g), ptr(x8), ptr(wq), ptr(wexp), ptr(count), ptr(lst), C.byref(e),
                                            int(bool(y_f8)), int(bool(y2_f8)), stream_ptr()), "mcamd_conv_fwd_q8_bsparse")


# ... of slim_export models: cin a multiple of 8 on zero-padded weight rows, border table in the epilogue
def conv_fwd_q8_slim_ok(g):
    """Does mcamd_conv_fwd_q8_slim accept this geometry?  (Shared by the engine and the tests; needs no device.)"""
    return bool(L.lib().mcamd_conv_fwd_q8_slim_ok(C.byref(g)))


def q8_slim_elems(g):
    out = (C.c_int64 * 2)()
    check(L.lib().mcamd_q8_slim_elems(C.byref(g), out), "mcamd_q8_slim_elems")
    return int(out[0]), int(out[1])


def pack_q8_slim(g, w, mask=None, out_w=None, out_exp=None):
    """pack_q8 into rows of round_up(cin, 64) channels per tap, pad channels 0x00 (mcamd_pack_q8_slim)."""
    _need_cuda(w, mask)
    assert w.dtype == torch.float32 and w.is_contiguous()
    nw, ne = q8_slim_elems(g)
    if out_w is None:
        out_w = torch.empty(nw, dtype=torch.uint8, device=w.device)
    if out_exp is None:
        out_exp = torch.empty(ne, dtype=torch.int32, device=w.device)
    if out_w.numel() < nw or out_exp.numel() < ne:
        raise L.McamdError("pack_q8_slim: destination too small")
    check(L.lib().mcamd_pack_q8_slim(C.byref(g), ptr(w), ptr(mask), ptr(out_w), ptr(out_exp), stream_ptr()), "mcamd_pack_q8_slim")
    return out_w, out_exp


def conv_fwd_q8_slim(g, x8, wq, wexp, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None, y2_ld=0,
                     y2_choff=0, y_f8=False, y2_f8=False, border=None, border_ld=0, overflow=None):
    """conv_fwd_q8 for cin % 8 == 0 from pack_q8_slim's rows, with the fp32 [16][border_ld] table `border` (or None) added to
    the raw value by pixel class in the epilogue (mcamd_conv_fwd_q8_slim).  `overflow`: as conv_fwd_q8."""
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    if border is not None:
        assert border.dtype == torch.float32 and border.is_contiguous()
        border_ld = border_ld or border.shape[-1]
    check(L.lib().mcamd_conv_fwd_q8_slim(C.byref(g), ptr(x8), ptr(wq), ptr(wexp), C.byref(e), ptr(border), int(border_ld),
                                         int(bool(y_f8)), int(bool(y2_f8)), stream_ptr()), "mcamd_conv_fwd_q8_slim")


def cast_q8(src, pixels, src_ld, src_choff, C_, dst, dst_ld, dst_choff=0, write_back=False):
    """fp16 channel slice of `pixels` pixels -> e4m3(2 x) bytes (mcamd_cast_q8): the fp16 -> fp8 edge of the fp8 engine.
    `write_back` (training, mcamd_cast_q8_train): the fp16 slice is overwritten with deq(code) / 2."""
    fn = L.lib().mcamd_cast_q8_train if write_back else L.lib().mcamd_cast_q8
    check(fn(ptr(src), pixels, src_ld, src_choff, C_, ptr(dst), dst_ld, dst_choff, stream_ptr()),
          "mcamd_cast_q8_train" if write_back else "mcamd_cast_q8")


def conv_fwd_q8_stats_rows(g):
    """Rows of the statistics slab conv_fwd_q8_raw writes for `g` (mcamd_conv_fwd_q8_stats_rows)."""
    return int(L.lib().mcamd_conv_fwd_q8_stats_rows(C.byref(g)))


def conv_fwd_q8_raw(g, x8, wq, wexp, y, y_ld, y_choff=0, stats=None):
    """The training form of the quantised block (mcamd_conv_fwd_q8, MCAMD_EPI_RAW_F32): y[M][y_ld] fp32 = 2^-(e_f + 1) x
    the sum of byte products; `stats`: fp32 [conv_fwd_q8_stats_rows(g)][2][stats_ld] slab of the fp32 values, or None."""
    e = _epi(L.EPI_RAW_F32, y, y_ld, y_choff, stats=stats,
             stats_rows_=stats.shape[0] if stats is not None else 0,
             stats_ld=stats.shape[2] if stats is not None else 0)
    check(L.lib().mcamd_conv_fwd_q8(C.byref(g), ptr(x8), ptr(wq), ptr(wexp), C.byref(e), 0, 0, stream_ptr()), "mcamd_conv_fwd_q8")


def fakequant_q8(g, w, mask, wexp, out=None):
    """fp32 OIHW w_q = deq(q(w * mask * 2^e_f)) * 2^-e_f from the exponents pack_q8 wrote (mcamd_fakequant_q8)."""
    _need_cuda(w, mask, wexp)
    assert w.dtype == torch.float32 and w.is_contiguous()
    if out is None:
        out = torch.empty_like(w)
    check(L.lib().mcamd_fakequant_q8(C.byref(g), ptr(w), ptr(mask), ptr(wexp), ptr(out), stream_ptr()), "mcamd_fakequant_q8")
    return out


# ----------------------------------------------------------------------------- 2:4-sparse fp8 quantised inference
def conv_fwd_q8_sparse24_ok(g):
    """Does mcamd_conv_fwd_q8_sparse24 accept this geometry?  (Shared by the engine and the tests.)"""
    return bool(L.lib().mcamd_conv_fwd_q8_sparse24_ok(C.byref(g)))


def q8_sparse24_elems(g):
    """(kept bytes, 32-bit index words, int32 exponents) of the 2:4 fp8 packing."""
    out = (C.c_int64 * 3)()
    check(L.lib().mcamd_q8_sparse24_elems(C.byref(g), out), "mcamd_q8_sparse24_elems")
    return int(out[0]), int(out[1]), int(out[2])


def pack_q8_sparse24(g, w, mask=None, out_w=None, out_idx=None, out_exp=None):
    """fp32 OIHW master (* mask) -> (kept e4m3 bytes, int32 index words, int32 exponent per filter) of the 2:4 fp8 forward
    (mcamd_pack_q8_sparse24)."""
    _need_cuda(w, mask)
    assert w.dtype == torch.float32 and w.is_contiguous()
    nw, ni, ne = q8_sparse24_elems(g)
    if out_w is None:
        out_w = torch.empty(nw, dtype=torch.uint8, device=w.device)
    if out_idx is None:
        out_idx = torch.empty(ni, dtype=torch.int32, device=w.device)
    if out_exp is None:
        out_exp = torch.empty(ne, dtype=torch.int32, device=w.device)
    if out_w.numel() < nw or out_idx.numel() < ni or out_exp.numel() < ne:
        raise L.McamdError("pack_q8_sparse24: destination too small")
    check(L.lib().mcamd_pack_q8_sparse24(C.byref(g), ptr(w), ptr(mask), ptr(out_w), ptr(out_idx), ptr(out_exp), stream_ptr()),
          "mcamd_pack_q8_sparse24")
    return out_w, out_idx, out_exp


def conv_fwd_q8_sparse24(g, x8, wq, idx, wexp, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None,
                         y2_ld=0, y2_choff=0, y_f8=False, y2_f8=False, overflow=None):
    """conv_fwd_q8 on 2:4-compressed e4m3 weights (mcamd_conv_fwd_q8_sparse24): the same arguments plus the index words,
    the same arithmetic and output.  `overflow`: as conv_fwd_q8."""
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    check(L.lib().mcamd_conv_fwd_q8_sparse24(C.byref(g), ptr(x8), ptr(wq), ptr(idx), ptr(wexp), C.byref(e), int(bool(y_f8)),
                                             int(bool(y2_f8)), stream_ptr()), "mcamd_conv_fwd_q8_sparse24")


# ----------------------------------------------------------------------------- 4-bit weights on the fp8 engine
def conv_fwd_q8_w4_ok(g):
    """Does mcamd_conv_fwd_q8_w4 accept this geometry?  (mcamd_conv_fwd_q8_ok's predicate; needs no device.)"""
    return bool(L.lib().mcamd_conv_fwd_q8_w4_ok(C.byref(g)))


def q8_w4_elems(g):
    """(code bytes, shift bytes, int32 exponents) of the 4-bit packing: 4.25 bits per weight."""
    out = (C.c_int64 * 3)()
    check(L.lib().mcamd_q8_w4_elems(C.byref(g), out), "mcamd_q8_w4_elems")
    return int(out[0]), int(out[1]), int(out[2])


def pack_q8_w4(g, w, mask=None, out_codes=None, out_shift=None, out_exp=None):
    """fp32 OIHW master (* mask) -> (e2m1 nibble codes, one shift byte per group of 32 input channels, int32 exponent per
    filter) of the 4-bit forward (mcamd_pack_q8_w4; the layout is stated in include/mcamd.h)."""
    _need_cuda(w, mask)
    assert w.dtype == torch.float32 and w.is_contiguous()
    nc, ng, ne = q8_w4_elems(g)
    if out_codes is None:
        out_codes = torch.empty(nc, dtype=torch.uint8, device=w.device)
    if out_shift is None:
        out_shift = torch.empty(ng, dtype=torch.uint8, device=w.device)
    if out_exp is None:
        out_exp = torch.empty(ne, dtype=torch.int32, device=w.device)
    if out_codes.numel() < nc or out_shift.numel() < ng or out_exp.numel() < ne:
        raise L.McamdError("pack_q8_w4: destination too small")
    check(L.lib().mcamd_pack_q8_w4(C.byref(g), ptr(w), ptr(mask), ptr(out_codes), ptr(out_shift), ptr(out_exp), stream_ptr()),
          "mcamd_pack_q8_w4")
    return out_codes, out_shift, out_exp


def unpack_q8_w4(g, codes, gshift, out_w=None):
    """The e4m3 bytes the 4-bit packing stands for, in pack_q8's layout (mcamd_unpack_q8_w4): conv_fwd_q8 on them with
    pack_q8_w4's exponents computes what conv_fwd_q8_w4 computes."""
    _need_cuda(codes, gshift)
    nw = q8_elems(g)[0]
    if out_w is None:
        out_w = torch.empty(nw, dtype=torch.uint8, device=codes.device)
    nc, ng, _ = q8_w4_elems(g)
    if out_w.numel() < nw or codes.numel() < nc or gshift.numel() < ng:
        raise L.McamdError("unpack_q8_w4: operand too small")
    check(L.lib().mcamd_unpack_q8_w4(C.byref(g), ptr(codes), ptr(gshift), ptr(out_w), stream_ptr()), "mcamd_unpack_q8_w4")
    return out_w


def conv_fwd_q8_w4_info(g):
    """The kernel instance conv_fwd_q8_w4 launches for `g`, as conv_fwd_q8_info reports the fp8 block's
    (mcamd_conv_fwd_q8_w4_info, the launch's own choice).  Needs no GPU."""
    out = (C.c_int32 * 7)()
    check(L.lib().mcamd_conv_fwd_q8_w4_info(C.byref(g), out), "mcamd_conv_fwd_q8_w4_info")
    return Q8Info(*out)


def conv_fwd_q8_w4(g, x8, codes, gshift, wexp, y, y_ld, y_choff=0, scale=None, shift=None, slope=1.0, dst_mode=0, y2=None,
                   y2_ld=0, y2_choff=0, y_f8=False, y2_f8=False, overflow=None):
    """conv_fwd_q8 on 4-bit weights (mcamd_conv_fwd_q8_w4): the same arguments with pack_q8_w4's codes and shift bytes in
    place of the weight bytes, the arithmetic of conv_fwd_q8 on unpack_q8_w4's bytes.  `overflow`: as conv_fwd_q8."""
    e = _epi(L.EPI_PAD_F16, y, y_ld, y_choff, scale=scale, shift=shift, slope=slope, dst_mode=dst_mode, y2=y2, y2_ld=y2_ld,
             y2_choff=y2_choff, overflow=overflow)
    check(L.lib().mcamd_conv_fwd_q8_w4(C.byref(g), ptr(x8), ptr(codes), ptr(gshift), ptr(wexp), C.byref(e), int(bool(y_f8)),
                                       int(bool(y2_f8)), stream_ptr()), "mcamd_conv_fwd_q8_w4")


def conv_fwd_q8_w4_raw(g, x8, codes, gshift, wexp, y, y_ld, y_choff=0, stats=None):
    """The training form of the 4-bit block (mcamd_conv_fwd_q8_w4_raw): conv_fwd_q8_raw's arguments with
    pack_q8_w4's codes, shift bytes and exponents in place of the weight bytes; y[M][y_ld] fp32 = 2^-(e4_f + 1) x the sum of byte
    products, `stats`: fp32 [conv_fwd_q8_stats_rows(g)][2][stats_ld] slab of the fp32 values, or None."""
    e = _epi(L.EPI_RAW_F32, y, y_ld, y_choff, stats=stats,
             stats_rows_=stats.shape[0] if stats is not None else 0,
             stats_ld=stats.shape[2] if stats is not None else 0)
    check(L.lib().mcamd_conv_fwd_q8_w4_raw(C.byref(g), ptr(x8), ptr(codes), ptr(gshift), ptr(wexp), C.byref(e), stream_ptr()),
          "mcamd_conv_fwd_q8_w4_raw")


def fakequant_q8_w4(g, codes, gshift, wexp, out=None):
    """fp32 OIHW w_q = grid[code] * 2^g * 2^-e4_f decoded from pack_q8_w4's operands (mcamd_fakequant_q8_w4): the values the
    4-bit forward multiplies."""
    _need_cuda(codes, gshift, wexp)
    nc, ng, ne = q8_w4_elems(g)
    if codes.numel() < nc or gshift.numel() < ng or wexp.numel() < ne:
        raise L.McamdError("fakequant_q8_w4: operand too small")
    if out is None:
        out = torch.empty(g.cout, g.cin, g.ksize, g.ksize, dtype=torch.float32, device=codes.device)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != g.cout * g.cin * g.ksize * g.ksize:
        raise L.McamdError("fakequant_q8_w4: destination must be contiguous fp32 [cout][cin][k][k]")
    check(L.lib().mcamd_fakequant_q8_w4(C.byref(g), ptr(codes), ptr(gshift), ptr(wexp), ptr(out), stream_ptr()),
          "mcamd_fakequant_q8_w4")
    return out


# ----------------------------------------------------------------------------- compressed model files (.mcz)
WZ_ELEM = {L.WZ_FP32: 4, L.WZ_FP16: 2, L.WZ_FP8: 1, L.WZ_CODE: 1, L.WZ_W4: 1}


def _wz_table(items, device, unpack):
    """items: dicts(w, mask, kind[, dense, kept, val0, word0, exp0, shift0]) -> (host mcamd_wz_seg array, its device copy, blocks,
    words, exps, bytes of every value array were every weight kept, shift bytes).  The running sums are the header's
    (include/mcamd.h)."""
    arr = (L.WzSeg * len(items))()
    blocks = words = exps = cap = shifts = 0
    for a, it in zip(arr, items):
        w, mask, kind = it["w"], it.get("mask"), int(it["kind"])
        _need_cuda(w, mask)
        if kind == L.WZ_CODE and (w.dtype != torch.uint8 or not w.is_contiguous() or w.numel() == 0):
            raise L.McamdError("wz: the codes of a WZ_CODE item must be a non-empty contiguous uint8 tensor of the weight's shape")
        if kind != L.WZ_CODE and (w.dtype != torch.float32 or not w.is_contiguous() or w.numel() == 0 or kind not in WZ_ELEM):
            raise L.McamdError("wz: weights must be non-empty contiguous fp32 tensors and kind one of %r" % sorted(WZ_ELEM))
        if kind == L.WZ_W4 and (w.dim() != 4 or w.shape[1] % 32):
            raise L.McamdError("wz: a WZ_W4 item must be an OIHW tensor with cin %% 32 == 0, got %r" % (tuple(w.shape),))
        if mask is not None and (mask.dtype != torch.float32 or not mask.is_contiguous() or mask.shape != w.shape):
            raise L.McamdError("wz: a mask must be a contiguous fp32 tensor of the weight's shape")
        n, nwords = w.numel(), (w.numel() + 63) // 64
        a.w, a.mask, a.n, a.cout = w.data_ptr(), (mask.data_ptr() if mask is not None else None), n, w.shape[0]
        a.kind = kind | (w.shape[2] * w.shape[3]) << 8 if kind == L.WZ_W4 else kind          # MCAMD_WZ_W4_KIND(taps)
        a.block0 = blocks
        a.word0, a.exp0 = (int(it.get("word0", words)), int(it.get("exp0", exps))) if unpack else (words, exps)
        a.shift0 = (int(it.get("shift0", shifts // 8)) if unpack else shifts // 8) if kind == L.WZ_W4 else 0
        a.dense = int(bool(it.get("dense", 0))) if unpack else 0
        a.kept, a.val0 = (int(it["kept"]), int(it["val0"])) if unpack else (0, 0)
        if not a.dense:
            words += nwords
        if kind in (L.WZ_FP8, L.WZ_W4):
            exps += w.shape[0]
        if kind == L.WZ_W4:
            shifts += round_up(n // 32, 8)
        blocks += (nwords + L.WZ_BLOCK_WORDS - 1) // L.WZ_BLOCK_WORDS
        cap += round_up(n * WZ_ELEM[kind], 8)
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    return arr, dev, blocks, words, exps, cap, shifts


def wz_pack(items):
    """items: one dict(w=fp32 OIHW master, mask=fp32 mask or None, kind=L.WZ_*) per layer, all through one table
    (mcamd_wz_pack_w4) -> device tensors (words int64 [sum ceil(n / 64)], counts int64 [len(items)], exps int32 [fp8 and 4-bit
    filters], values uint8): the bit words of segment s start at the running sum of ceil(n / 64), its exponents at the running
    sum of the fp8 and 4-bit segments' cout, its values at the byte offset the header's rule gives from the counts.  A table
    that holds a WZ_W4 item returns a fifth tensor, shifts uint8: the n / 32 shift bytes of each such segment, padded to 8, in
    order; its values are one byte per code."""
    dev = items[0]["w"].device
    arr, table, blocks, nwords, nexps, cap, nshifts = _wz_table(items, dev, False)
    words = torch.empty(nwords, dtype=torch.int64, device=dev)
    counts = torch.empty(len(items), dtype=torch.int64, device=dev)
    exps = torch.empty(max(nexps, 1), dtype=torch.int32, device=dev)
    values = torch.zeros(cap, dtype=torch.uint8, device=dev)
    shifts = torch.zeros(max(nshifts, 8), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(L.lib().mcamd_wz_workspace_bytes(blocks, len(items))), dtype=torch.uint8, device=dev)
    check(L.lib().mcamd_wz_pack_w4(arr, ptr(table), len(items), ptr(words), nwords, ptr(counts), ptr(exps), nexps, ptr(values), cap,
                                   ptr(ws), ws.numel(), stream_ptr(), ptr(shifts), nshifts), "mcamd_wz_pack_w4")
    if nshifts:
        return words, counts, exps[:nexps], values, shifts[:nshifts]
    return words, counts, exps[:nexps], values


def wz_unpack(items, words, exps, values, shifts=None):
    """items: one dict(w=fp32 OIHW tensor to fill, mask=fp32 tensor to fill or None, kind, dense, kept, val0) per layer;
    words (int64, the bit words of the non-dense items in order), exps (int32, the fp8 and 4-bit items' exponents in order),
    values (uint8, item s at byte val0; a WZ_W4 item: one byte per code) and shifts (uint8, the WZ_W4 items' shift bytes, each
    item's padded to 8) are device tensors or None when no item needs them (mcamd_wz_unpack_w4).  An item may name where its
    bit words, exponents and shift bytes start (word0, exp0: element offsets into `words` / `exps`; shift0: the byte offset
    into `shifts` divided by 8) in place of the running sums, which lets views of one uploaded file serve as every array."""
    dev = items[0]["w"].device
    _need_cuda(words, exps, values, shifts)
    arr, table, blocks, nwords, nexps, _, nshifts = _wz_table(items, dev, True)
    for t, dt, need, name in ((words, torch.int64, nwords, "words"), (exps, torch.int32, nexps, "exps"), (values, torch.uint8, 0, "values"),
                              (shifts, torch.uint8, nshifts, "shifts")):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise L.McamdError("wz_unpack: `%s` must be a contiguous %s tensor" % (name, dt))
        if need and t is None:
            raise L.McamdError("wz_unpack: `%s` needs %d entries" % (name, need))
    if values is None:
        values = torch.zeros(8, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(L.lib().mcamd_wz_workspace_bytes(blocks, len(items))), dtype=torch.uint8, device=dev)
    check(L.lib().mcamd_wz_unpack_w4(arr, ptr(table), len(items), ptr(words), words.numel() if words is not None else 0, ptr(exps),
                                     exps.numel() if exps is not None else 0, ptr(values), values.numel(), ptr(ws), ws.numel(),
                                     stream_ptr(), ptr(shifts), shifts.numel() if shifts is not None else 0), "mcamd_wz_unpack_w4")


# ----------------------------------------------------------------------------- Huffman-coded model files
def _hz_table(spans, device, encode=False):
    """spans: dicts(sym0, nsym, A[, nbits, word0, chunk0, popc_bits]) -> (host mcamd_hz_seg array, its device copy, workgroups,
    chunks, code words).  block0 is the header's running sum; word0 and chunk0 default to their running sums (encode lays both
    out that way)."""
    arr = (L.HzSeg * len(spans))()
    blocks = chunks = words = 0
    for a, sp in zip(arr, spans):
        nsym, nbits = int(sp["nsym"]), int(sp.get("nbits", 0))
        nc = (nsym + L.HZ_CHUNK - 1) // L.HZ_CHUNK
        a.sym0, a.nsym, a.nbits, a.A, a.popc_bits = int(sp["sym0"]), nsym, nbits, int(sp["A"]), int(sp.get("popc_bits", 0))
        a.block0 = blocks
        a.word0, a.chunk0 = (words, chunks) if encode else (int(sp.get("word0", words)), int(sp.get("chunk0", chunks)))
        blocks += (nc + L.HZ_GROUP - 1) // L.HZ_GROUP
        chunks += nc
        words += (nbits + 63) // 64
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    return arr, dev, blocks, chunks, words


def _hz_lengths(lengths, device):
    """A list of per-stream code lengths (uint8 arrays of up to 256 entries) -> uint8 [nseg][256] on the device."""
    import numpy as np
    table = np.zeros((len(lengths), 256), dtype=np.uint8)
    for row, l in zip(table, lengths):
        l = l.cpu().numpy() if isinstance(l, torch.Tensor) else np.asarray(l)
        row[:l.size] = l.reshape(-1)
    return torch.from_numpy(table).to(device)


def _hz_buffer(buf, name):
    _need_cuda(buf)
    if buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.dim() != 1:
        raise L.McamdError("%s: the symbols must be a contiguous 1-d uint8 tensor" % name)


def hz_histogram_at(buf, spans, dyn=None):
    """int64 [len(spans)][256]: how often every byte value occurs in each stream of the uint8 device tensor `buf`
    (mcamd_hz_histogram).  spans: dicts(sym0, nsym, A).  dyn (int64 [len(spans)][2] on the device, optional): sym0 and nsym of
    every stream as a device pass left them; a span's nsym is then the most the stream can have."""
    _hz_buffer(buf, "hz_histogram")
    arr, table, blocks, _, _ = _hz_table(spans, buf.device)
    if dyn is not None and (dyn.dtype != torch.int64 or not dyn.is_contiguous() or tuple(dyn.shape) != (len(spans), 2)
                            or dyn.device != buf.device):
        raise L.McamdError("hz_histogram: `dyn` must be a contiguous int64 [streams][2] tensor on the symbols' device")
    hist = torch.empty(len(spans), 256, dtype=torch.int64, device=buf.device)
    ws = torch.empty(int(L.lib().mcamd_hz_workspace_bytes(blocks, len(spans))), dtype=torch.uint8, device=buf.device)
    check(L.lib().mcamd_hz_histogram(arr, ptr(table), len(spans), ptr(buf), buf.numel(), ptr(dyn), ptr(hist), ptr(ws), ws.numel(),
                                     stream_ptr()), "mcamd_hz_histogram")
    return hist


def hz_encode_at(buf, spans, lengths):
    """(chunk_bit0 int32 [sum of chunks], bits int64 [sum of ceil(nbits / 64)]) of the streams of `buf` under `lengths` (one
    uint8 array per stream), both in span order (mcamd_hz_encode).  spans: dicts(sym0, nsym, A, nbits), nbits the sum of
    count * length over the stream's histogram."""
    _hz_buffer(buf, "hz_encode")
    arr, table, blocks, chunks, words = _hz_table(spans, buf.device, encode=True)
    ctab = torch.empty(max(chunks, 1), dtype=torch.int32, device=buf.device)
    bits = torch.zeros(max(words, 1), dtype=torch.int64, device=buf.device)
    lens = _hz_lengths(lengths, buf.device)
    ws = torch.empty(int(L.lib().mcamd_hz_workspace_bytes(blocks, len(spans))), dtype=torch.uint8, device=buf.device)
    check(L.lib().mcamd_hz_encode(arr, ptr(table), len(spans), ptr(buf), buf.numel(), ptr(lens), ptr(ctab), chunks, ptr(bits), words,
                                  ptr(ws), ws.numel(), stream_ptr()), "mcamd_hz_encode")
    return ctab[:chunks], bits[:words]


def hz_decode_at(spans, lengths, chunk_bit0, bits, out):
    """Decode the streams into the uint8 device tensor `out` (mcamd_hz_decode) -> stats int64 [len(spans)][2] on the device:
    [s][0] bit 0 = the stream is damaged, bit 1 = a decoded bit word has a bit set at or past popc_bits; [s][1] = the set
    bits among the first popc_bits.  spans: dicts(sym0, nsym, A, nbits, word0, chunk0[, popc_bits]): where the stream's
    symbols go in `out`, its code words lie in `bits` (int64) and its chunk table lies in `chunk_bit0` (int32)."""
    _hz_buffer(out, "hz_decode")
    _need_cuda(chunk_bit0, bits)
    if chunk_bit0.dtype != torch.int32 or bits.dtype != torch.int64 or not chunk_bit0.is_contiguous() or not bits.is_contiguous():
        raise L.McamdError("hz_decode: chunk_bit0 must be a contiguous int32 and bits a contiguous int64 tensor")
    arr, table, _, _, _ = _hz_table(spans, out.device)
    lens = _hz_lengths(lengths, out.device)
    stats = torch.empty(len(spans), 2, dtype=torch.int64, device=out.device)
    check(L.lib().mcamd_hz_decode(arr, ptr(table), len(spans), ptr(lens), ptr(chunk_bit0), chunk_bit0.numel(), ptr(bits), bits.numel(),
                                  ptr(out), out.numel(), ptr(stats), stream_ptr()), "mcamd_hz_decode")
    return stats


def _hz_cat(tensors, name):
    """A list of uint8 device tensors -> (one buffer with every tensor at a multiple of 8 bytes, the byte offsets)."""
    if not tensors:
        raise L.McamdError("%s: no stream" % name)
    for t in tensors:
        _hz_buffer(t, name)
    offs, total = [], 0
    for t in tensors:
        offs.append(total)
        total += round_up(t.numel(), 8)
    buf = torch.zeros(max(total, 8), dtype=torch.uint8, device=tensors[0].device)
    for t, o in zip(tensors, offs):
        buf[o:o + t.numel()] = t
    return buf, offs


def hz_histogram(streams):
    """streams: a list of 1-d uint8 device tensors -> int64 [len(streams)][256] on the device, their byte histograms."""
    buf, offs = _hz_cat(streams, "hz_histogram")
    return hz_histogram_at(buf, [dict(sym0=o, nsym=t.numel(), A=256) for t, o in zip(streams, offs)])


def hz_encode(streams, lengths, alphabets=None):
    """streams: a list of 1-d uint8 device tensors; lengths: per stream the uint8 code lengths of its alphabet (0 = absent,
    1..12; compress.huffman_lengths of its histogram) -> per stream dict(nsym, A, nbits, lengths, chunk_bit0 int32, bits
    int64), device tensors.  nbits comes from one read of the streams' histograms."""
    buf, offs = _hz_cat(streams, "hz_encode")
    alphabets = alphabets or [256] * len(streams)
    spans = [dict(sym0=o, nsym=t.numel(), A=int(A)) for t, o, A in zip(streams, offs, alphabets)]
    hist = hz_histogram_at(buf, spans).cpu().numpy()
    for sp, h, l in zip(spans, hist, lengths):
        l = (l.cpu().numpy() if isinstance(l, torch.Tensor) else l).reshape(-1)
        sp["nbits"] = int(sum(int(c) * int(x) for c, x in zip(h[:l.size], l)))
    ctab, bits = hz_encode_at(buf, spans, lengths)
    out, c0, b0 = [], 0, 0
    for sp, l in zip(spans, lengths):
        nc, nw = (sp["nsym"] + L.HZ_CHUNK - 1) // L.HZ_CHUNK, (sp["nbits"] + 63) // 64
        out.append(dict(nsym=sp["nsym"], A=sp["A"], nbits=sp["nbits"], lengths=l, chunk_bit0=ctab[c0:c0 + nc], bits=bits[b0:b0 + nw]))
        c0, b0 = c0 + nc, b0 + nw
    return out


def hz_decode(coded, out=None, offsets=None):
    """coded: a list of dict(nsym, A, nbits, lengths, chunk_bit0, bits) as hz_encode returns -> (the decoded streams, uint8
    device tensors; stats int64 [len(coded)][2] as hz_decode_at returns).  out / offsets: decode into the uint8 device tensor
    `out`, stream s at byte offsets[s] (a multiple of 8), instead of a fresh buffer."""
    if not coded:
        raise L.McamdError("hz_decode: no stream")
    dev = coded[0]["bits"].device
    ctab = torch.cat([c["chunk_bit0"].to(torch.int32).reshape(-1) for c in coded] + [torch.zeros(1, dtype=torch.int32, device=dev)])
    bits = torch.cat([c["bits"].to(torch.int64).reshape(-1) for c in coded] + [torch.zeros(1, dtype=torch.int64, device=dev)])
    if out is None:
        offsets, total = [], 0
        for c in coded:
            offsets.append(total)
            total += round_up(int(c["nsym"]), 8)
        out = torch.zeros(max(total, 8), dtype=torch.uint8, device=dev)
    spans, c0, b0 = [], 0, 0
    for c, o in zip(coded, offsets):
        spans.append(dict(sym0=int(o), nsym=int(c["nsym"]), A=int(c["A"]), nbits=int(c["nbits"]), word0=b0, chunk0=c0,
                          popc_bits=int(c.get("popc_bits", 0))))
        c0, b0 = c0 + c["chunk_bit0"].numel(), b0 + c["bits"].numel()
    stats = hz_decode_at(spans, [c["lengths"] for c in coded], ctab, bits, out)
    return [out[int(o):int(o) + int(c["nsym"])] for c, o in zip(coded, offsets)], stats


# ----------------------------------------------------------------------------- weight sharing
class WsTable:
    """Every layer of a weight-sharing pass through one mcamd_ws_seg table (include/mcamd.h), with the arrays the passes
    share: `codebook` fp32 [sum K], `sums` float64 and `counts` int64 of the same length, and the workspace.

    items: one dict(w=fp32 tensor, mask=fp32 tensor of its shape or None, codes=uint8 tensor of its shape, K=2^bits) per
    layer.  codebook: the flat fp32 tensor to work on (layer s at the running sum of K), allocated when None.  Built once;
    every method is one library call on the current stream with no host read."""

    def __init__(self, items, codebook=None):
        if not items:
            raise L.McamdError("ws: no layer given")
        dev = items[0]["w"].device
        arr = (L.WsSeg * len(items))()
        slabs = parts = cb = 0
        self.offsets = []
        for a, it in zip(arr, items):
            w, mask, codes, K = it["w"], it.get("mask"), it["codes"], int(it["K"])
            _need_cuda(w, mask, codes)
            if w.dtype != torch.float32 or not w.is_contiguous() or w.numel() == 0:
                raise L.McamdError("ws: weights must be non-empty contiguous fp32 tensors")
            if mask is not None and (mask.dtype != torch.float32 or not mask.is_contiguous() or mask.shape != w.shape):
                raise L.McamdError("ws: a mask must be a contiguous fp32 tensor of the weight's shape")
            if codes.dtype != torch.uint8 or not codes.is_contiguous() or codes.numel() != w.numel():
                raise L.McamdError("ws: codes must be a contiguous uint8 tensor with one entry per weight")
            n = w.numel()
            nsl = (n + L.WS_SLAB - 1) // L.WS_SLAB
            a.w, a.mask, a.codes = w.data_ptr(), (mask.data_ptr() if mask is not None else None), codes.data_ptr()
            a.n, a.K, a.cb0, a.slab0, a.part0 = n, K, cb, slabs, parts
            self.offsets.append(cb)
            slabs, parts, cb = slabs + nsl, parts + nsl * K, cb + K
        self.items, self.arr, self.nseg, self.cb = items, arr, len(items), cb
        # (pinned and non-blocking: building a table is no host synchronisation either)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)
        if codebook is None:
            codebook = torch.zeros(cb, dtype=torch.float32, device=dev)
        _need_cuda(codebook)
        if codebook.dtype != torch.float32 or not codebook.is_contiguous() or codebook.numel() < cb:
            raise L.McamdError("ws: the codebook must be a contiguous fp32 tensor of at least %d entries" % cb)
        self.codebook = codebook
        self.sums = torch.zeros(cb, dtype=torch.float64, device=dev)
        self.counts = torch.zeros(cb, dtype=torch.int64, device=dev)
        self.ws = torch.empty(int(L.lib().mcamd_ws_workspace_bytes(slabs, parts, len(items))), dtype=torch.uint8, device=dev)

    def layer_codebook(self, s):
        return self.codebook[self.offsets[s]:self.offsets[s] + int(self.items[s]["K"])]

    def init(self):
        check(L.lib().mcamd_ws_init(self.arr, ptr(self.table), self.nseg, ptr(self.codebook), self.codebook.numel(), ptr(self.ws),
                                    self.ws.numel(), stream_ptr()), "mcamd_ws_init")

    def iterate(self):
        check(L.lib().mcamd_ws_iterate(self.arr, ptr(self.table), self.nseg, ptr(self.codebook), self.codebook.numel(), ptr(self.sums),
                                       ptr(self.counts), ptr(self.ws), self.ws.numel(), stream_ptr()), "mcamd_ws_iterate")

    def assign(self):
        check(L.lib().mcamd_ws_assign(self.arr, ptr(self.table), self.nseg, ptr(self.codebook), self.codebook.numel(), stream_ptr()),
              "mcamd_ws_assign")

    def project(self):
        check(L.lib().mcamd_ws_project(self.arr, ptr(self.table), self.nseg, ptr(self.codebook), self.codebook.numel(), ptr(self.sums),
                                       ptr(self.counts), ptr(self.ws), self.ws.numel(), stream_ptr()), "mcamd_ws_project")

    def expand(self):
        check(L.lib().mcamd_ws_expand(self.arr, ptr(self.table), self.nseg, ptr(self.codebook), self.codebook.numel(), stream_ptr()),
              "mcamd_ws_expand")


# ----------------------------------------------------------------------------- Taylor importance
class TaylorTable:
    """Every layer of a Taylor-importance step through one mcamd_taylor_seg table (include/mcamd.h).

    items: one dict per segment.  A conv segment: w, g (fp32, the weight's shape, [cout][cin]...), optional bias and gbias
    (fp32 [cout]) and the optional outputs acc_w (fp32, the weight's shape), acc_b (float64 [blocks]), acc_f (float64 [cout]).
    A gate segment (gate=True): w = gamma, g = dgamma, bias = beta, gbias = dbeta (fp32 [C]) and acc_f (float64 [C]).
    steps: device int32 [1].  Built once; accumulate() is one library call on the current stream with no host read."""

    def __init__(self, items, steps):
        if not items:
            raise L.McamdError("taylor: no segment given")
        dev = items[0]["w"].device
        arr = (L.TaylorSeg * len(items))()
        wgs = 0
        for a, it in zip(arr, items):
            w, g, gate = it["w"], it["g"], bool(it.get("gate"))
            f32 = [w, g, it.get("bias"), it.get("gbias"), it.get("acc_w")]
            f64 = [it.get("acc_b"), it.get("acc_f")]
            _need_cuda(*f32, *f64)
            for t, dt in [(t, torch.float32) for t in f32] + [(t, torch.float64) for t in f64]:
                if t is not None and (t.dtype != dt or not t.is_contiguous() or t.device != dev):
                    raise L.McamdError("taylor: every array must be a contiguous %s tensor on one device" % dt)
            cout = w.shape[0]
            cin = 1 if gate or w.dim() < 2 else w.shape[1]
            khw = w.numel() // (cout * cin)
            want = {"g": w.numel(), "bias": cout, "gbias": cout, "acc_w": w.numel(), "acc_f": cout}
            if not gate and cin % 32 == 0:
                want["acc_b"] = ((cout + BLOCK_FILTERS - 1) // BLOCK_FILTERS) * (cin // block_kb(cin)) * khw
            for name, n in want.items():
                if it.get(name) is not None and it[name].numel() != n:
                    raise L.McamdError("taylor: %s holds %d entries, %d expected" % (name, it[name].numel(), n))
            a.w, a.g = w.data_ptr(), g.data_ptr()
            for name in ("bias", "gbias", "acc_w", "acc_b", "acc_f"):
                setattr(a, name, it[name].data_ptr() if it.get(name) is not None else None)
            a.kind, a.cout, a.cin, a.khw, a.wg0 = (L.TAYLOR_GATE if gate else L.TAYLOR_CONV), cout, cin, khw, wgs
            wgs += int(L.lib().mcamd_taylor_seg_workgroups(C.byref(a)))
        _need_cuda(steps)
        if steps.dtype != torch.int32 or steps.numel() != 1:
            raise L.McamdError("taylor: steps must be a device int32 scalar")
        self.items, self.arr, self.nseg, self.steps, self.workgroups = items, arr, len(items), steps, wgs
        # (pinned and non-blocking: building a table is no host synchronisation)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)

    def accumulate(self, skip=None):
        """One step: every accumulator += this step's term, steps += 1; nothing at all when *skip != 0 (device fp32 scalar)."""
        if skip is not None:
            _need_cuda(skip)
            if skip.dtype != torch.float32 or skip.numel() != 1:
                raise L.McamdError("taylor: skip must be a device fp32 scalar")
        check(L.lib().mcamd_taylor_accum(self.arr, ptr(self.table), self.nseg, ptr(skip), ptr(self.steps), stream_ptr()),
              "mcamd_taylor_accum")


# ----------------------------------------------------------------------------- proximal group lasso
class GroupProxTable:
    """Every layer of a proximal group-lasso step through one mcamd_gprox_seg table (include/mcamd.h).

    items: one dict per segment.  A block segment: w (fp32, [cout][cin]..., cin % 32 == 0) and optionally nz (int32
    [blocks]).  A gate segment (gate=True): w = gamma (fp32 [C]) and optionally nz (int32 [C]).  Built once; step() is one
    library call on the current stream with no host read and no allocation."""

    def __init__(self, items):
        if not items:
            raise L.McamdError("group_prox: no segment given")
        dev = items[0]["w"].device
        arr = (L.GproxSeg * len(items))()
        wgs = 0
        for a, it in zip(arr, items):
            w, nz, gate = it["w"], it.get("nz"), bool(it.get("gate"))
            _need_cuda(w, nz)
            if w.dtype != torch.float32 or not w.is_contiguous() or w.device != dev or w.numel() == 0:
                raise L.McamdError("group_prox: weights must be non-empty contiguous fp32 tensors on one device")
            cout = w.shape[0]
            cin = 1 if gate or w.dim() < 2 else w.shape[1]
            khw = w.numel() // (cout * cin)
            if gate:
                groups = cout
            else:
                if cin % 32 != 0:
                    raise L.McamdError("group_prox: blocks need cin %% 32 == 0 (cin %d)" % cin)
                groups = ((cout + BLOCK_FILTERS - 1) // BLOCK_FILTERS) * (cin // block_kb(cin)) * khw
            if nz is not None and (nz.dtype != torch.int32 or not nz.is_contiguous() or nz.device != dev or nz.numel() != groups):
                raise L.McamdError("group_prox: nz must be a contiguous int32 tensor of %d entries on the weights' device" % groups)
            a.w, a.nz = w.data_ptr(), (nz.data_ptr() if nz is not None else None)
            a.kind, a.cout, a.cin, a.khw, a.wg0 = (L.GPROX_GATE if gate else L.GPROX_BLOCK), cout, cin, khw, wgs
            wgs += int(L.lib().mcamd_gprox_seg_workgroups(C.byref(a)))
        self.items, self.arr, self.nseg, self.workgroups = items, arr, len(items), wgs
        # (pinned and non-blocking: building a table is no host synchronisation)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)

    def step(self, tau, skip=None):
        """One proximal step at tau = lr * lam: blocks take tau2 = tau * tau (float64), gates (float)tau; nothing at all is
        written when *skip != 0 (device fp32 scalar)."""
        if skip is not None:
            _need_cuda(skip)
            if skip.dtype != torch.float32 or skip.numel() != 1:
                raise L.McamdError("group_prox: skip must be a device fp32 scalar")
        tau = float(tau)
        check(L.lib().mcamd_group_prox(self.arr, ptr(self.table), self.nseg, tau * tau, tau, ptr(skip), stream_ptr()),
              "mcamd_group_prox")
