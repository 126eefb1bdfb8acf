"""The quantisation rule of the MXFP4 activation cast (a4_ref) over its whole domain: all 254 finite e4m3 codes
under every shift s in [-11, 7] that does not saturate them."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a4_ref as A  # noqa: E402
from w4_ref import GRID  # noqa: E402

BYTES = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)
MIDS = (GRID[:-1] + GRID[1:]) / 2


def test_every_code_under_every_shift():
    v = A.deq(BYTES)
    n = 0
    for s in range(A.S_MIN, A.S_MAX + 1):
        keep = v.abs() <= 6.0 * 2.0 ** s
        x = v[keep]
        code, val = A.code(x, torch.full(x.shape, s))
        u, idx = x.abs() / 2.0 ** s, (code & 7).long()
        # an e4m3 number -- but for the format's maximum: +-448 = 3.5 * 2^7 is a tie and goes to the even 4 * 2^7 = 512
        odd = val.abs() > 448.0
        assert torch.equal(val[~odd].float().to(torch.float8_e4m3fn).double(), val[~odd]), "the value is an e4m3 number (s = %d)" % s
        assert bool((x[odd].abs() == 448.0).all()) and bool((val[odd].abs() == 512.0).all()) and int(odd.sum()) == (2 if s == 7 else 0)
        lo, hi = GRID[(idx - 1).clamp(min=0)], GRID[(idx + 1).clamp(max=7)]
        # (no further from its grid entry than the midpoint to either neighbour: half a grid step at that entry)
        assert bool(((u >= (lo + GRID[idx]) / 2) & (u <= (GRID[idx] + hi) / 2)).all()), "within half a grid step (s = %d)" % s
        tie = (u.view(-1, 1) == MIDS.view(1, -1)).any(1)
        assert bool((idx[tie] % 2 == 0).all()), "ties go to the even mantissa bit"
        assert bool(((code >> 3 == 1) == ((x < 0) & (idx != 0))).all()), "a zero magnitude carries no sign"
        n += int(tie.sum())
    assert n > 0, "the domain holds ties"


def test_a_groups_shift_never_saturates():
    v = A.deq(BYTES).abs()
    s = A.shift(v)
    nz = v > 0
    assert int(s.min()) >= A.S_MIN and int(s.max()) <= A.S_MAX
    assert bool((v <= 6.0 * torch.pow(2.0, s.double())).all()) and bool((v[nz] > 3.0 * torch.pow(2.0, s[nz].double())).all())
    assert bool((s[~nz] == 0).all())
