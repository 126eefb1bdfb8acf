"""CPU restatement of the 4-bit weight format of the fp8 engine (include/mcamd.h), test-side only, in float64 /
integer arithmetic.

  filter     e4_f = e_f - 1 with e_f = q8_ref.filter_exponents (0 for an all-zero filter); s = w * mask * 2^e4_f
  group      the 32 consecutive input channels [32 j, 32 j + 32) at one tap of one filter
  shift      the smallest integer g in [-5, 6] with max |s| over the group <= 6 * 2^g; -5 for an all-zero group
  code       bit 3 = sign, bits 0-2 = index into GRID of |s| / 2^g rounded to nearest, ties to the even mantissa bit (= the even
             index); a zero magnitude has no sign bit
  value      GRID[code] * 2^g -- an e4m3fn number, always: byte = q8_ref.q(value) is exact

The device layout (mcamd_pack_q8_w4): code rows [Npad][ktot / 2] -- chunk q of 64 positions of mcamd_pack_q8's order is 32
bytes, piece h = 0, 1 of 16; piece h holds positions p(h, t) = 16 h + t (t < 16), 32 + 16 h + t - 16 (t >= 16); byte i, d = i / 4,
b = i % 4: low nibble t = 8 d + b, high nibble t = 8 d + 4 + b -- and shift bytes g + 5 as [ktot / 64][Npad][2]."""
import torch

import q8_ref as R
from q8_sparse_ref import dense_rows

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
G_MIN, G_MAX = -5, 6


def filter_exponents(wm):
    """int32 [cout]: e4_f of the (already masked) OIHW weights."""
    e = R.filter_exponents(wm)
    zero = wm.detach().float().abs().flatten(1).amax(1) == 0
    return torch.where(zero, torch.zeros_like(e), e - 1).to(torch.int32)


def group_shift(amax):
    """float64 group maxima (any shape) -> int64 shifts: the smallest g in [G_MIN, G_MAX] with amax <= 6 * 2^g, by trying
    every g (no logarithm)."""
    g = torch.full(amax.shape, G_MAX, dtype=torch.int64)
    for cand in range(G_MAX - 1, G_MIN - 1, -1):
        g = torch.where(amax <= 6.0 * 2.0 ** cand, torch.full_like(g, cand), g)
    return g


def round_to_grid(v):
    """float64 magnitudes v >= 0 -> int64 grid indices: nearest entry of GRID, a tie to the even index; above 6 -> 7."""
    v = v.double()
    idx = torch.zeros(v.shape, dtype=torch.int64)
    for i in range(7):                                       # past the midpoint of entries i and i + 1: at least i + 1
        mid = float(GRID[i] + GRID[i + 1]) / 2.0             # (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5: exact)
        idx += ((v > mid) | ((v == mid) & (i % 2 == 1))).long()            # on it: up when the lower index is odd
    return idx


def quantise(w, mask=None):
    """(codes uint8 OIHW with bit 3 the sign, g int64 [cout][cin / 32][k][k], e4 int32 [cout], values float64 OIHW = GRID[code] *
    2^g in the scaled domain, bytes uint8 OIHW = q(values)) of weight * mask."""
    wm = w.detach().float() * (mask.float() if mask is not None else 1.0)
    cout, cin, k, _ = wm.shape
    assert cin % 32 == 0
    e4 = filter_exponents(wm)
    s = wm.double() * torch.pow(2.0, e4.double()).view(-1, 1, 1, 1)
    grp = s.abs().view(cout, cin // 32, 32, k, k)
    g = group_shift(grp.amax(2))
    gfull = g.unsqueeze(2).expand(cout, cin // 32, 32, k, k).reshape(cout, cin, k, k)
    step = torch.pow(2.0, gfull.double())
    idx = round_to_grid(s.abs() / step)
    neg = (s < 0) & (idx != 0)
    values = GRID[idx] * step * torch.where(neg, -1.0, 1.0)
    codes = (idx | (neg.long() << 3)).to(torch.uint8)
    return codes, g, e4, values, R.q(values)


def dequantised(values, e4):
    """fp32 OIHW weights the codes stand for: values * 2^-e4_f (exact in fp32)."""
    return (values * torch.pow(2.0, -e4.double()).view(-1, 1, 1, 1)).float()


# ------------------------------------------------------------------------------------------------ the device layout
def _perm():
    """position in the chunk's 32 code bytes x nibble -> position in the 64-k chunk"""
    lo, hi = [], []
    for h in range(2):
        for i in range(16):
            d, b = divmod(i, 4)
            for t, out in ((8 * d + b, lo), (8 * d + 4 + b, hi)):
                out.append(16 * h + t if t < 16 else 32 + 16 * h + t - 16)
    return torch.tensor(lo), torch.tensor(hi)


def code_rows(codes):
    """codes OIHW -> the device's rows uint8 [cout][ktot / 2]."""
    rows = dense_rows(codes)
    cout, ktot = rows.shape
    ch = rows.view(cout, ktot // 64, 64)
    lo, hi = _perm()
    return (ch[:, :, lo] | (ch[:, :, hi] << 4)).reshape(cout, ktot // 2)


def codes_of_rows(rows, cin, k):
    """the device's rows [cout][ktot / 2] -> 4-bit codes in mcamd_pack_q8's order, uint8 [cout][ktot]."""
    cout = rows.shape[0]
    ch = rows.view(cout, -1, 32)
    lo, hi = _perm()
    out = torch.zeros(cout, ch.shape[1], 64, dtype=torch.uint8)
    out[:, :, lo] = ch & 0x0F
    out[:, :, hi] = ch >> 4
    return out.reshape(cout, -1)


def shift_rows(g):
    """g [cout][cin / 32][k][k] -> the device's shift bytes uint8 [ktot / 64][cout][2] (g + 5)."""
    cout, ng, k, _ = g.shape
    t = (g + 5).view(cout, ng // 2, 2, k * k).permute(1, 3, 0, 2)          # [cb][tap][cout][2]
    return t.reshape(ng // 2 * k * k, cout, 2).to(torch.uint8)
