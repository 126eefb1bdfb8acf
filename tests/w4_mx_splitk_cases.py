"""The cases of tests/test_q8_w4_mx_splitk_kernels_gpu.py: launches of mcamd_conv_fwd_q8_w4_mx_splitk (csrc/conv_q8_w4_mx.hip,
DESIGN.md 3zi).  The shapes are rows of q8_splitk_cases._ROWS in their fp8-MFMA form (MCAMD_Q8_MFMA=1's arithmetic is the fp4
MFMA's: q8_cases.exactness applies condition 4) -- the smallest that reach the ragged last pixel tile, cout not a multiple of
64, one chunk per slice, uneven slices, every destination form and both store formats.  test_q8_w4_mx_splitk_cpu.py proves the
conditions of exactness per case without a GPU.  Test-side only."""
import q8_cases as QC
import q8_splitk_cases as SKC
import w4_cases as WC

POLICY = SKC.POLICY
# row letter of q8_splitk_cases._ROWS -> slice counts
SLICES = {"a": (1, 2, 5, 18, POLICY), "b": (1, 2, 3), "c": (1, 4, 9), "e": (1, 2), "g": (POLICY, 16), "h": (2,), "h.bytes": (2,)}
CASES = [SKC.SplitCase(sc.c, sc.chunks, SLICES[sc.c.name[3:-2]]) for sc in SKC.SPLITK_CASES
         if sc.c.mfma and sc.c.name[3:-2] in SLICES]
assert len(CASES) == len(SLICES)
LAUNCHES = [(sc, S) for sc in CASES for S in sc.slices]
launch_id, case_id = SKC.launch_id, SKC.case_id

_CACHE = {}


def operands_and_reference(c, plant=True):
    """q8_cases' operands with w4_cases' integer weight draws (5 and 7 round on the e2m1 grid, the shifts differ between
    groups) and w4_cases' float64 reference on the values the codes stand for.  The overflow rows keep q8_cases' own weights:
    their planted filter must stay all ones, and next to the planted activations (256) a weight draw up to 7 would leave the
    width the fp8 MFMA holds (condition 4); the d3 draw lies on the e2m1 grid.  Once per process and case, never modified."""
    key = (c.name, plant)
    if key not in _CACHE:
        o = QC.operands(c, plant=plant)
        if "overflow" not in c.special:
            o = o._replace(w=WC.operands(c).w)
        _CACHE[key] = (o, WC.reference(c, o)[0])
    return _CACHE[key]
