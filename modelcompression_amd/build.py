"""Build libmcamd.so (hand-written HIP for gfx950) in-tree with hipcc.

    python -m modelcompression_amd.build        # or __graft_entry__.build()

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels with the
repo snapshot to the GPU box.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libmcamd.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
COMMON = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-variable",
          "-fhip-fp32-correctly-rounded-divide-sqrt"]
SOURCES = {
    "api.hip": [],
    "conv_igemm.hip": [],
    "conv_igemm_pp.hip": [],
    "conv_sparse.hip": [],
    "conv_bsparse.hip": [],
    "conv_splitk.hip": [],
    # The fp8 forward family runs one K loop and one epilogue (csrc/conv_q8_loop.h): their results are bit-equal where the
    # tests say so because the same functions run.  The five files must still be compiled with EQUAL flags, so that the
    # shared epilogue expression (and the split-K finish kernel's restatement of it) contracts the same way in each.
    "conv_q8.hip": [],
    "conv_q8_sparse.hip": [],
    "conv_q8_splitk.hip": [],
    "conv_q8_bsparse.hip": [],
    "conv_q8_w4.hip": [],
    "conv_stem.hip": [],
    "conv_stem_block.hip": [],
    "conv_stem_f32.hip": [],
    "conv_small.hip": [],
    "conv_win.hip": [],
    "conv_wres.hip": [],
    "conv_wgrad.hip": [],
    "conv_wgrad_stem.hip": [],
    "conv_bwd1x1.hip": [],
    "bn_act.hip": [],
    "bn_conv1x1.hip": [],
    "fold.hip": [],
    "plan.hip": [],
    "region_loss.hip": [],
    "distill_loss.hip": [],
    "prune.hip": ["-ffp-contract=off"],   # pinned fp32 arithmetic: no FMA contraction
    "augment.hip": ["-ffp-contract=off"], # Pillow's float / double HSV arithmetic, operation by operation
    "detect.hip": ["-ffp-contract=off"],  # suppression decisions are pinned fp32 comparisons; one decode, bit for bit
    "voc_eval.hip": ["-ffp-contract=off"],  # voc_eval's float64 arithmetic, operation by operation
    "wpack.hip": ["-ffp-contract=off"],   # compressed model files: the stored codes are pinned conversions of weight * mask
    "wshare.hip": ["-ffp-contract=off"],  # weight sharing: float64 sums and divisions, operation by operation
    "huff.hip": [],                       # Huffman-coded model files: integer passes only
    "taylor.hip": ["-ffp-contract=off"],  # Taylor importance: pinned fp32 / float64 products and sums
    "group_prox.hip": ["-ffp-contract=off"],  # proximal group lasso: pinned float64 sums, one scale per block
}


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "mcamd.h"))
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _stale(o, [s] + headers):
            jobs.append([HIPCC] + COMMON + extra + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr))
        return r.stderr

    with ThreadPoolExecutor(max_workers=4) as ex:
        for err in ex.map(run, jobs):
            if verbose and err.strip():
                print(err)
    objs = [os.path.join(objdir, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _stale(OUT, objs):
        run([HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", OUT] + objs)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
