"""Host logic of the fp4-operand form of the 4-bit weights (Darknet.precision = "fp8-w4-mx", csrc/conv_q8_w4_mx.hip, DESIGN.md
3zg): the cases of the GPU file reach its three instances whatever MCAMD_Q8_MFMA says, the predicate is mcamd_conv_fwd_q8_w4_ok's,
and the precision's rules that need no device.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import _lib as L, ops  # noqa: E402
import q8_cases as QC  # noqa: E402
import w4_cases as WC  # noqa: E402

MX_CASES = [c for c in WC.CASES if c.expect[1] == 1]


@pytest.mark.parametrize("mfma", ["0", "1"])
def test_cases_reach_the_three_instances_and_ok_agrees(setenv, mfma):
    setenv(QC.ENV, mfma)
    reached = set()
    for c in MX_CASES:
        g = QC.geom_of(c)
        r = ops.conv_fwd_q8_w4_mx_info(g)
        assert (r.f8mfma, r.bmw, r.bnp, r.stages) == (1, c.expect[2], 128, 3), c.name
        assert ops.conv_fwd_q8_w4_mx_ok(g) and ops.conv_fwd_q8_w4_ok(g)
        reached.add(r.bmw)
    assert reached == {256, 128, 64}
    bad = ops.geom(1, 208, 208, 3, 32, 64, 32)                             # conv2: cin % 64 != 0
    assert not ops.conv_fwd_q8_w4_mx_ok(bad) and not ops.conv_fwd_q8_w4_ok(bad)
    with pytest.raises(L.McamdError, match="mcamd_conv_fwd_q8_w4_mx_ok"):
        ops.conv_fwd_q8_w4_mx_info(bad)


def test_engine_accepts_the_precision_and_names_it():
    from modelcompression_amd import engine as E
    with pytest.raises(L.McamdError, match="'fp8-w4-mx'.*'fp8-w5'"):
        E.Engine(None, 1, 416, 416, "cpu", precision="fp8-w5")
    form = E._FORMS["q8_w4_mx"]
    assert isinstance(form, E._Q8) and (form.fwd, form.elems, form.packer) == ("conv_fwd_q8_w4_mx", "q8_w4_elems", "pack_q8_w4_mx")
    assert form.bufs == E._FORMS["q8_w4"].bufs and all(hasattr(ops, n) for n in (form.fwd, form.packer, "unpack_q8_w4_mx"))
    lay = E._Layer()
    lay.form = "q8_w4_mx"
    assert lay.q8_on and not lay.q8s_on and not lay.q8_slim and not lay.sk_on
