"""The MXFP4 activation cast (mcamd_cast_a4_mx, include/mcamd.h) restated in torch on the CPU: e4m3 bytes ->
e2m1 codes, one e8m0 scale byte per group of 32 consecutive channels, and the e4m3 bytes the pairs stand for.  Test-side only."""
import torch

from w4_ref import GRID, round_to_grid

S_MIN, S_MAX = -11, 7


def deq(b):
    """uint8 e4m3 codes (finite) -> float64 values"""
    return b.view(torch.float8_e4m3fn).double()


def shift(amax):
    """float64 group maxima -> int64: the smallest s with amax <= 6 * 2^s, by trying every s (no logarithm); 0 for a zero"""
    s = torch.full(amax.shape, S_MAX, dtype=torch.int64)
    for cand in range(S_MAX - 1, S_MIN - 1, -1):
        s = torch.where(amax <= 6.0 * 2.0 ** cand, torch.full_like(s, cand), s)
    return torch.where(amax == 0, torch.zeros_like(s), s)


def code(v, s):
    """float64 values and their group's shift -> (uint8 code with bit 3 the sign, float64 value the pair stands for)"""
    step = torch.pow(2.0, s.double())
    idx = round_to_grid(v.abs() / step)
    neg = (v < 0) & (idx != 0)
    return (idx | (neg.long() << 3)).to(torch.uint8), GRID[idx] * step * torch.where(neg, -1.0, 1.0)


def cast(x8):
    """uint8 [rows][cin] -> (codes uint8 [rows][cin], scale bytes uint8 [rows][cin / 32], the e4m3 bytes [rows][cin] they stand for)"""
    rows, cin = x8.shape
    v = deq(x8)
    s = shift(v.abs().view(rows, cin // 32, 32).amax(2))
    codes, values = code(v, s.repeat_interleave(32, 1))
    # (the one pair outside e4m3: +-448 = 3.5 * 2^7 is a tie and goes to 4 * 2^7 = 512; its byte here is the nearest, +-448)
    back = values.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn)
    assert torch.equal(back.double()[values.abs() != 512.0], values[values.abs() != 512.0]), "the pairs stand for e4m3 numbers"
    return codes, (127 + s).to(torch.uint8), back.view(torch.uint8)


def packed(codes, scales):
    """the layout mcamd.h states: code bytes [rows][cin / 2] (even channel in the low nibble), scale words [rows][cin / 64][4]"""
    rows, cin = codes.shape
    words = torch.zeros(rows, cin // 64, 4, dtype=torch.uint8)
    words[:, :, :2] = scales.view(rows, cin // 64, 2)
    return codes[:, 0::2] | (codes[:, 1::2] << 4), words.view(rows, cin // 16)
