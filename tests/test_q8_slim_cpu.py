"""fp8 inference of slim_export models, host side: the four entry points exist at every layer, the geometry
predicate mcamd_conv_fwd_q8_slim_ok (needs no device), the operand sizes, and the restatement q8_slim_ref.py against
q8_ref.py and against itself in float32."""
import os
import re

import pytest
import torch

from modelcompression_amd import ops, _lib as L
import q8_ref as R
import q8_slim_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcamd_conv_fwd_q8_slim_ok", "mcamd_q8_slim_elems", "mcamd_pack_q8_slim", "mcamd_conv_fwd_q8_slim"]


def test_entry_points_declared_exported_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    lib = L.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in mcamd.h"
        assert name in L.SIGNATURES, name + " is not in _lib.SIGNATURES"
        assert getattr(lib, name) is not None, name + " is not exported"
        assert callable(getattr(ops, name[len("mcamd_"):])), name + " has no wrapper in ops"


def geom(B, H, W, k, cin, cout, x_ld, x_choff=0, stem=0, pad=0, wrap=0):
    return ops.geom(B, H, W, k, cin, cout, x_ld, x_choff, stem, pad, wrap)


@pytest.mark.parametrize("case", [(1, 13, 13, 3, 72, 40, 128), (1, 13, 13, 3, 40, 24, 64), (1, 13, 13, 1, 136, 72, 192),
                                  (1, 13, 13, 3, 128, 64, 128), (1, 13, 13, 3, 72, 40, 256, 128)])
def test_slim_predicate_accepts(case):
    assert ops.conv_fwd_q8_slim_ok(geom(*case))
    assert ops.conv_fwd_q8_slim_ok(geom(*case, pad=1))


def test_slim_predicate_rejects():
    assert not ops.conv_fwd_q8_slim_ok(geom(1, 13, 13, 3, 72, 40, 96)), "the pad crosses x_ld"
    assert not ops.conv_fwd_q8_slim_ok(geom(1, 13, 13, 3, 60, 40, 128)), "cin 60"
    assert not ops.conv_fwd_q8_slim_ok(geom(1, 13, 13, 3, 72, 60, 128)), "cout 60"
    assert not ops.conv_fwd_q8_slim_ok(geom(1, 13, 13, 3, 3, 32, 4, 0, 1)), "the stem"
    assert not ops.conv_fwd_q8_slim_ok(geom(1, 13, 13, 5, 72, 40, 128)), "ksize 5"
    assert not ops.conv_fwd_q8_slim_ok(geom(1, 13, 13, 3, 192, 64, 128, 0, 0, 0, 128)), "x_wrap"
    assert not ops.conv_fwd_q8_slim_ok(geom(1, 13, 13, 3, 72, 40, 256, 8)), "x_choff 8"
    assert not ops.conv_fwd_q8_slim_ok(geom(1, 13, 13, 3, 72, 40, 120)), "x_ld % 16"
    assert not ops.conv_fwd_q8_slim_ok(geom(0, 13, 13, 3, 72, 40, 128)), "empty batch"


def test_dense_predicates_still_reject_ragged_cin():
    for cin in (32, 96):
        g = geom(1, 13, 13, 3, cin, 64, 128)
        assert not ops.conv_fwd_q8_ok(g) and not ops.conv_fwd_q8_sparse24_ok(g)
        assert ops.conv_fwd_q8_slim_ok(g)
    assert ops.conv_fwd_q8_ok(geom(1, 13, 13, 3, 128, 64, 128))


@pytest.mark.parametrize("k,cin,cout,ld", [(3, 72, 40, 128), (1, 136, 72, 192), (3, 128, 264, 128), (3, 40, 8, 64)])
def test_q8_slim_elems(k, cin, cout, ld):
    npad = ops.round_up(cout, 256)
    assert ops.q8_slim_elems(geom(2, 6, 6, k, cin, cout, ld)) == (npad * k * k * ops.round_up(cin, 64), npad)
    with pytest.raises(L.McamdError):
        ops.q8_slim_elems(geom(2, 6, 6, k, cin + 4, cout, ld))


def test_restatement_zero_table_is_q8_ref_block():
    B, H, W, cin, cout, k, _ = S.KERNEL_SHAPES[0]
    a8, w, mask, scale, shift, _ = S.make_case(B, H, W, cin, cout, k, seed=3, table=False)
    w8, e = R.quantise_weights(w, mask)
    want = R.block(a8, w8, e, scale, shift, R.SLOPE)
    assert torch.equal(S.block_border(a8, w8, e, scale, shift, None, R.SLOPE), want)
    assert torch.equal(S.block_border(a8, w8, e, scale, shift, torch.zeros(16, cout), R.SLOPE), want)


def test_restatement_class_map():
    m = S.class_map(3, 4)
    assert m.tolist() == [[5, 1, 1, 9], [4, 0, 0, 8], [6, 2, 2, 10]]
    assert S.class_map(1, 1).tolist() == [[15]] and S.class_map(1, 3).tolist() == [[7, 3, 11]]
    tab = torch.arange(16.0).view(16, 1).repeat(1, 2)
    assert torch.equal(S.border_map(tab, 3, 4)[0, 1], m.double())


@pytest.mark.parametrize("shape", S.KERNEL_SHAPES, ids=["-".join(str(v) for v in s) for s in S.KERNEL_SHAPES])
def test_restatement_float32_against_float64(shape):
    """The formula evaluated in float32 (an association the kernel may take) against the float64 judge on the kernel
    tests' inputs: inside the cap the kernel is held to, differing codes adjacent -- the cap leaves the formula alone."""
    B, H, W, cin, cout, k, dst = shape
    a8, w, mask, scale, shift, border = S.make_case(B, H, W, cin, cout, k, seed=sum(shape[:6]))
    assert border.shape == (16, cout) and bool((border != 0).any())
    w8, e = R.quantise_weights(w, mask)
    v64 = S.block_border(a8, w8, e, scale, shift, border, R.SLOPE)
    v32 = S.block_border(a8, w8, e, scale, shift, border, R.SLOPE, dtype=torch.float32)
    share, adjacent = R.byte_mismatch(R.store_bytes(v32, dst), R.store_bytes(v64, dst))
    print("%r: float32 vs float64 share of differing codes %.3g" % (shape, share))
    assert adjacent and share <= R.MISMATCH_CAP
    # ... and the table matters: without it far more codes than the cap differ
    v0 = S.block_border(a8, w8, e, scale, shift, None, R.SLOPE)
    assert R.byte_mismatch(R.store_bytes(v0, dst), R.store_bytes(v64, dst))[0] > 100 * R.MISMATCH_CAP
