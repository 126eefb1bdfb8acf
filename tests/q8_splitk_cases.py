"""The cases of tests/test_q8_splitk_kernels_gpu.py: launches of mcamd_conv_fwd_q8_splitk (csrc/conv_q8_splitk.hip), built with
q8_cases.case(..., "dense", ...) so that q8_cases' operands, exact references and conditions of exactness apply as they are.
test_q8_splitk_cpu.py proves the conditions of exactness per case on the CPU; the GPU file runs them.  Test-side only.

Why the unsplit references apply to a split sum: q8_cases' operands make every partial sum in every order an fp32 number
(q8_cases.exactness, condition 1), so the S slab values and their sum in slice order are exact and the split sum equals the
unsplit one code for code.  Under MCAMD_Q8_MFMA=1 condition 4 keeps every product inside the width the fp8 MFMA holds, in any
grouping of the chunks."""
import collections

from modelcompression_amd import ops
import q8_cases as QC

POLICY = 0      # slices = 0: the library's policy

# (letter, image, k, cin, cout, keywords of q8_cases.case, chunks, slice counts)
_ROWS = [
    ("a", (1, 13, 13), 3, 128, 72, dict(fmt="f8", y_choff=8), 18, (1, 2, 5, 18, POLICY)),
    ("b", (2, 12, 14), 1, 192, 136, dict(dst="pool", fmt="f16", draw="d2"), 3, (1, 2, 3)),
    ("c", (2, 12, 14), 3, 64, 200, dict(dst="pool+y2", fmt="f8+f16", ld=128, choff=32, y2_choff=16, draw="d1"), 9, (1, 4, 7, 9)),
    ("d", (1, 16, 16), 1, 128, 48, dict(dst="pool+y2", fmt="f16+f8", draw="d2"), 2, (1, 2)),
    ("e", (1, 16, 16), 1, 128, 24, dict(dst="reorg", fmt="f8", y_choff=16, sa=-10), 2, (1, 2)),
    ("f", (2, 12, 14), 3, 64, 136, dict(dst="pool+y2", fmt="f8", special=("zeros",)), 9, (1, 3)),
    ("g", (1, 13, 13), 3, 1280, 256, dict(fmt="f8", draw="s4", wdraw="s4u"), 180, (POLICY, 16)),
    ("h", (2, 13, 13), 1, 128, 128, dict(fmt="f16", slope=1.0, special=("overflow",)), 2, (2,)),
    # (h) with a byte destination: the planted values saturate silently, the flag stays 0
    ("h.bytes", (2, 13, 13), 1, 128, 128, dict(fmt="f8", slope=1.0, special=("overflow",)), 2, (2,)),
]

SplitCase = collections.namedtuple("SplitCase", "c chunks slices")


def _unsplit_bmw(cout, mfma):
    """the tile mcamd_conv_fwd_q8 takes for the same launch (q8_cases.Case.expect; T2 compares against that kernel)"""
    if mfma and cout >= 256:
        return 256
    return 128 if cout >= 128 else 64


def _build():
    out = []
    for mfma in (0, 1):
        for (letter, (B, H, W), k, cin, cout, kw, chunks, slices) in _ROWS:
            kw = dict(kw)
            if kw.get("y_choff"):
                kw["y_ld"] = ops.round_up(kw["y_choff"] + (4 * cout if kw.get("dst") == "reorg" else cout) + 8, 32)
            if kw.get("y2_choff"):
                kw["y2_ld"] = ops.round_up(kw["y2_choff"] + cout + 8, 32)
            # (the part of the name in front of the first dot seeds the operands: both MFMA forms and (h) / (h.bytes) share them)
            base, _, rest = letter.partition(".")
            name = "sk-%s%s%s" % (base, "." + rest if rest else "", ".m" if mfma else "")
            c = QC.case(name, "dense", B, H, W, k, cin, cout, ("dense", mfma, _unsplit_bmw(cout, mfma)), mfma=mfma, **kw)
            assert c.ktot // 64 == chunks, (name, c.ktot // 64)
            out.append(SplitCase(c, chunks, tuple(slices)))
    return out


SPLITK_CASES = _build()
# (case, slices) pairs of T1
LAUNCHES = [(sc, S) for sc in SPLITK_CASES for S in sc.slices]


def launch_id(p):
    sc, S = p
    return "%s-S%s" % (sc.c.name, "policy" if S == POLICY else S)


def case_id(sc):
    return sc.c.name


def resolved(sc, S):
    """the slice count a launch with `S` runs: the policy's for POLICY (host logic, needs no GPU)"""
    return ops.conv_fwd_q8_splitk_info(QC.geom_of(sc.c), QC.DSTS["pool" if sc.c.dst == "pool+y2" else sc.c.dst], S).slices
