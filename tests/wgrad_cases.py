"""The weight-gradient cases of tests/test_wgrad_instances_gpu.py, and the enumeration of what mcamd_conv_wgrad can launch.

test_host_cpu.py proves on the CPU (through mcamd_conv_wgrad_plan_info, which is answered by the launch's own plan and
decision functions) that WGRAD_CASES reaches every compute-kernel instance and every finish-kernel instance the plan
rules can produce; test_wgrad_instances_gpu.py runs each case against an exact integer reference.  Test-side only."""
import collections

from modelcompression_amd import ops
from modelcompression_amd import _lib as L

ENV_DEFAULTS = {"MCAMD_WGRAD9": "1", "MCAMD_WGRAD9W": "1", "MCAMD_WGRAD9W_MINW": "40"}

_FIELDS = ("name B H W k cin cout stem pad x_ld x_choff dy_ld dy_choff cout_full perm_cols mask grad_scale dbias vmax env "
           "expect tags")


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_conv_wgrad.
    x_ld / dy_ld 0: the slice is the whole buffer (round_up(cin, 32) / rows_pad channels).  cout_full > 0: a row map that
    scatters the `cout` physical filters into a tensor of cout_full rows (the others stay unwritten); perm_cols: a column
    map (a permutation of the input channels).  vmax: operands are integers in [-vmax, vmax] (the stem image: [0, 2]).
    expect: (compute kernel, finish kernel) as compute_of / finish_of name them.  tags: the boundary conditions the case
    was written for, each re-derived from the query by boundary_tags()."""
    __slots__ = ()

    def __str__(self):
        return self.name


def case(name, B, H, W, k, cin, cout, expect, stem=0, pad=0, x_ld=0, x_choff=0, dy_ld=0, dy_choff=0, cout_full=0,
         perm_cols=False, mask=True, grad_scale=1.0, dbias=True, vmax=2, env=None, tags=()):
    return Case(name, B, H, W, k, cin, cout, stem, pad, x_ld, x_choff, dy_ld, dy_choff, cout_full, perm_cols, mask, grad_scale,
                dbias, vmax, dict(env or {}), expect, tuple(tags))


def geom_of(c):
    x_ld = c.x_ld or (4 if c.stem else ops.round_up(c.cin, 32))
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, x_ld, c.x_choff, stem=c.stem, pad=c.pad)


def apply_env(c, setenv):
    """Set the three plan switches for this case (the defaults where the case names none)."""
    for name, default in ENV_DEFAULTS.items():
        setenv(name, c.env.get(name, default))


def plan_of(c):
    return ops.wgrad_plan_info(geom_of(c), c.perm_cols)


def compute_of(p):
    """The compute kernel instance a plan names, with exactly the template arguments that instance has."""
    if p.family == L.WGRAD_GENERIC:
        return ("wgrad_kernel", p.tmo, p.tnc, p.taps, p.kp, p.ns)
    if p.family == L.WGRAD_STEM:
        return ("wgrad_stem_kernel", p.ns)
    if p.family == L.WGRAD_WIN:
        return ("wgrad_win_kernel", p.tmo // 32, p.ns)
    if p.family == L.WGRAD_NINE:
        return ("wgrad9_kernel", p.kp)
    assert p.family == L.WGRAD_NINE_WIDE, p
    return ("wgrad9w_kernel", p.kp, p.ns)


def finish_of(p, ksize, stem):
    kk = ksize * ksize
    if p.finish == L.WFIN_ROW:
        return ("wgrad_finish_row_kernel", kk)
    if p.finish == L.WFIN_VEC:
        return ("wgrad_finish_vec_kernel", kk, p.sg)
    assert p.finish == L.WFIN_GENERIC, p
    return ("wgrad_finish_kernel", p.sg)


def pixels_enumerated(c):
    """Products summed into one element of dW, halo pixels included (the 9-tap kernels enumerate padded pixels)."""
    pw = 1 if c.pad else 2
    return c.B * (c.H + pw) * (c.W + pw) + (c.W + 2 if c.pad else 0)


def boundary_tags(c, p):
    """The named boundary conditions this plan meets, from the query's nsplit / pix_per_split / tiles / grid alone."""
    t = set()
    M = c.B * c.H * c.W
    if p.nsplit == 1:
        t.add("nsplit==1")
    if p.nsplit > 64:
        t.add("nsplit>64")
    if p.grid != p.tiles * p.nsplit:
        t.add("idle-workgroups")
    if p.pix_per_split > 0 and p.nsplit > 1:
        n = pixels_enumerated(c) if p.family in (L.WGRAD_NINE, L.WGRAD_NINE_WIDE) else M
        if n % p.pix_per_split != 0:
            t.add("short-last-split")
    if p.finish == L.WFIN_ROW and p.nsplit == 16:
        t.add("row-finish-at-16-splits")
    if c.perm_cols and c.cin % 4 == 0 and p.nsplit == 17 and p.finish == L.WFIN_VEC:
        t.add("vec-finish-at-17-splits")
    row_bytes = c.cin * c.k * c.k * 4
    if c.perm_cols and c.cin % 4 == 0 and p.nsplit <= 16:
        if p.finish == L.WFIN_ROW and 60 * 1024 - 256 < row_bytes <= 60 * 1024:
            t.add("row-finish-just-under-60KB")
        if p.finish == L.WFIN_VEC and 60 * 1024 < row_bytes <= 60 * 1024 + 256:
            t.add("vec-finish-just-over-60KB")
    if p.finish == L.WFIN_GENERIC and c.perm_cols and c.cin % 4 != 0:
        t.add("generic-finish-by-cin%4-with-column-map")
    if p.finish == L.WFIN_GENERIC and c.stem:
        t.add("generic-finish-by-stem")
    return t


BOUNDARIES = ("nsplit==1", "nsplit>64", "idle-workgroups", "short-last-split", "row-finish-at-16-splits",
              "vec-finish-at-17-splits", "row-finish-just-under-60KB", "vec-finish-just-over-60KB",
              "generic-finish-by-cin%4-with-column-map", "generic-finish-by-stem")


def reachable(setenv):
    """Every (compute kernel instance, finish kernel instance) pair's two halves that the plan rules can name, as two
    sets, by asking the library over channel counts 8 .. 1344, both kernel sizes, the stem, image sizes from one tile to
    the training batch at 416 x 416, with and without a column map and under every setting of the three plan switches.
    The instance of the generic kernel depends on (cout, padded cin, taps) only (test_wgrad_instances_are_the_reachable_set
    walks all of those); the other families and the finish kernels also depend on the image, so the image list spans
    every threshold of the plan functions: W around 40 / 77 / 113 / 208, M around 4096, 1 .. > 64 splits."""
    chans = (8, 24, 32, 40, 56, 64, 96, 120, 128, 192, 256, 512, 1024, 1344)
    odd = (9, 41, 65)
    images = ((1, 8, 8), (2, 13, 13), (2, 16, 16), (3, 40, 48), (2, 50, 64), (1, 8, 80), (1, 8, 120), (2, 24, 40), (2, 40, 64),
              (3, 33, 96), (8, 26, 26), (64, 13, 13), (8, 52, 52), (7, 104, 104), (64, 104, 104), (16, 208, 208), (2, 256, 128),
              (64, 416, 416), (1, 8, 216))
    comp, fin = set(), set()
    for w9 in ("1", "0"):
        for w9w in ("1", "0"):
            for minw in ("8", "40"):
                setenv("MCAMD_WGRAD9", w9)
                setenv("MCAMD_WGRAD9W", w9w)
                setenv("MCAMD_WGRAD9W_MINW", minw)
                for (B, H, W) in images:
                    big = B * H * W > 1 << 20
                    for cout in chans:
                        p = ops.wgrad_plan_info(ops.geom(B, H, W, 3, 3, cout, 4, 0, stem=1))
                        comp.add(compute_of(p))
                        fin.add(finish_of(p, 3, 1))
                        for cin in (chans[:6] if big else chans + odd):
                            for k in (1, 3):
                                for cmap in (False, True):
                                    p = ops.wgrad_plan_info(ops.geom(B, H, W, k, cin, cout, ops.round_up(cin, 32)), cmap)
                                    comp.add(compute_of(p))
                                    fin.add(finish_of(p, k, 0))
    # the row kernel's LDS limit lies beyond those widths
    for cin in (1704, 1708):
        p = ops.wgrad_plan_info(ops.geom(1, 8, 8, 3, cin, 32, ops.round_up(cin, 32)), True)
        fin.add(finish_of(p, 3, 0))
    return comp, fin


G = "wgrad_kernel"
ROW, VEC, FIN = "wgrad_finish_row_kernel", "wgrad_finish_vec_kernel", "wgrad_finish_kernel"
MINW8 = {"MCAMD_WGRAD9W_MINW": "8"}

WGRAD_CASES = [
    # ---- the 19 instances of the generic kernel; operand forms and finish kernels spread over them ------------------------
    case("g32x32x9", 2, 12, 12, 3, 32, 32, ((G, 32, 32, 9, 32, 2), (VEC, 9, 1)), x_ld=48, x_choff=8, vmax=3,
         tags=("short-last-split", "idle-workgroups")),
    case("g32x32x3-stem", 2, 12, 20, 3, 3, 32, ((G, 32, 32, 3, 64, 3), (FIN, 1)), stem=1, vmax=3, grad_scale=256.0,
         tags=("generic-finish-by-stem", "nsplit==1")),
    case("g32x32x1-row-finish-16-splits", 16, 32, 32, 1, 32, 32, ((G, 32, 32, 1, 128, 3), (ROW, 1)), perm_cols=True, vmax=3,
         tags=("row-finish-at-16-splits",)),
    case("g32x32x1-vec-finish-17-splits", 17, 32, 32, 1, 32, 32, ((G, 32, 32, 1, 128, 3), (VEC, 1, 8)), perm_cols=True, vmax=3,
         dy_ld=64, dy_choff=24, dbias=False, tags=("vec-finish-at-17-splits", "idle-workgroups")),
    case("g32x64x9-row-finish-under-60KB", 1, 8, 8, 3, 1704, 32, ((G, 32, 64, 9, 32, 2), (ROW, 9)), perm_cols=True, vmax=3,
         grad_scale=256.0, tags=("row-finish-just-under-60KB", "nsplit==1")),
    case("g32x64x9-vec-finish-over-60KB", 1, 8, 8, 3, 1708, 32, ((G, 32, 64, 9, 32, 2), (VEC, 9, 1)), perm_cols=True, vmax=3,
         cout_full=48, tags=("vec-finish-just-over-60KB", "nsplit==1")),
    case("g32x64x1-folded-consumer-74-splits", 7, 104, 104, 1, 41, 32, ((G, 32, 64, 1, 128, 2), (FIN, 32)), perm_cols=True,
         vmax=3, dy_ld=64, dy_choff=32, tags=("generic-finish-by-cin%4-with-column-map", "nsplit>64", "short-last-split")),
    case("g32x128x3", 2, 12, 12, 3, 128, 32, ((G, 32, 128, 3, 32, 2), (VEC, 9, 1)), cout_full=80, vmax=3, grad_scale=256.0),
    case("g32x128x1", 2, 12, 12, 1, 128, 32, ((G, 32, 128, 1, 64, 2), (VEC, 1, 1)), x_ld=192, x_choff=64, vmax=3, mask=False,
         tags=("nsplit==1",)),
    case("g64x32x9", 2, 12, 12, 3, 32, 64, ((G, 64, 32, 9, 32, 2), (VEC, 9, 1)), dy_ld=96, dy_choff=16, vmax=3),
    case("g64x32x3-stem", 2, 12, 20, 3, 3, 64, ((G, 64, 32, 3, 64, 2), (FIN, 1)), stem=1, vmax=3, dbias=False,
         tags=("generic-finish-by-stem",)),
    case("g64x32x1", 2, 12, 12, 1, 32, 64, ((G, 64, 32, 1, 128, 2), (VEC, 1, 1)), cout_full=100, vmax=3),
    case("g64x64x3", 4, 52, 52, 3, 64, 56, ((G, 64, 64, 3, 32, 3), (VEC, 9, 8)), x_ld=128, x_choff=64, vmax=3,
         tags=("short-last-split", "idle-workgroups")),
    case("g64x64x1-folded-consumer", 4, 26, 26, 1, 41, 48, ((G, 64, 64, 1, 64, 3), (FIN, 8)), perm_cols=True, vmax=3,
         grad_scale=256.0, tags=("generic-finish-by-cin%4-with-column-map",)),
    case("g64x64x3-folded-consumer", 2, 12, 12, 3, 41, 48, ((G, 64, 64, 3, 32, 3), (FIN, 1)), perm_cols=True, vmax=3,
         cout_full=64, tags=("generic-finish-by-cin%4-with-column-map",)),
    case("g64x128x3", 2, 12, 12, 3, 128, 56, ((G, 64, 128, 3, 32, 2), (VEC, 9, 1)), vmax=3, dbias=False),
    case("g64x128x1", 4, 52, 52, 1, 128, 64, ((G, 64, 128, 1, 64, 2), (VEC, 1, 8)), vmax=3, dy_ld=128, dy_choff=64,
         tags=("short-last-split",)),
    case("g128x32x3", 2, 12, 12, 3, 32, 128, ((G, 128, 32, 3, 32, 3), (VEC, 9, 1)), vmax=3, grad_scale=256.0),
    case("g128x32x1", 2, 12, 12, 1, 32, 128, ((G, 128, 32, 1, 64, 2), (VEC, 1, 1)), vmax=3, x_ld=40, x_choff=8),
    case("g128x64x3-169-splits", 16, 52, 52, 3, 64, 120, ((G, 128, 64, 3, 32, 2), (VEC, 9, 32)), vmax=3,
         tags=("nsplit>64", "idle-workgroups")),
    case("g128x64x1-125-filters", 2, 12, 12, 1, 64, 125, ((G, 128, 64, 1, 64, 2), (VEC, 1, 1)), vmax=3, grad_scale=256.0),
    case("g128x128x1-batch-64", 64, 26, 26, 1, 512, 256, ((G, 128, 128, 1, 32, 3), (VEC, 1, 32)), vmax=3,
         tags=("nsplit>64", "short-last-split")),
    # ---- row kernel with both maps, a non-identity permutation and unwritten rows ---------------------------------------------
    case("g32x64x9-row-finish-both-maps", 2, 12, 12, 3, 40, 24, ((G, 32, 64, 9, 32, 2), (ROW, 9)), perm_cols=True, cout_full=96,
         vmax=3, tags=("short-last-split",)),
    case("g64x128x1-row-finish-both-maps", 2, 12, 20, 1, 256, 40, ((G, 64, 128, 1, 64, 2), (ROW, 1)), perm_cols=True,
         cout_full=64, vmax=3, x_ld=320, x_choff=32, tags=("nsplit==1",)),
    # ---- raw-window kernels --------------------------------------------------------------------------------------------------
    case("stem-5-splits", 2, 40, 64, 3, 3, 32, (("wgrad_stem_kernel", 4), (FIN, 8)), stem=1, vmax=3,
         tags=("generic-finish-by-stem",)),
    case("stem-676-splits", 4, 416, 416, 3, 3, 32, (("wgrad_stem_kernel", 4), (FIN, 32)), stem=1, vmax=2, grad_scale=256.0,
         tags=("generic-finish-by-stem", "nsplit>64")),
    case("win2", 3, 40, 48, 3, 32, 64, (("wgrad_win_kernel", 2, 6), (VEC, 9, 8)), vmax=3, x_ld=64, x_choff=32),
    case("win2-256-splits", 4, 208, 208, 3, 32, 64, (("wgrad_win_kernel", 2, 6), (VEC, 9, 32)), vmax=3, dy_ld=96, dy_choff=32,
         grad_scale=256.0, tags=("nsplit>64",)),
    case("win2-batch-64", 64, 208, 208, 3, 32, 64, (("wgrad_win_kernel", 2, 6), (VEC, 9, 32)), vmax=2, tags=("nsplit>64",)),
    case("win1-padded-cin", 2, 50, 64, 3, 24, 32, (("wgrad_win_kernel", 1, 6), (ROW, 9)), vmax=3, perm_cols=True, cout_full=40),
    # ---- 9-tap kernels, both halo forms ----------------------------------------------------------------------------------------
    case("nine64-batch-64", 64, 13, 13, 3, 256, 512, (("wgrad9_kernel", 64), (VEC, 9, 8)), vmax=3),
    case("nine64-shared-halo", 3, 13, 13, 3, 192, 64, (("wgrad9_kernel", 64), (VEC, 9, 1)), pad=1, vmax=3, x_ld=256, x_choff=64,
         tags=("short-last-split",)),
    case("nine64-one-split", 1, 13, 13, 3, 128, 256, (("wgrad9_kernel", 64), (VEC, 9, 1)), vmax=3, dy_ld=320, dy_choff=64,
         grad_scale=256.0, tags=("nsplit==1",)),
    case("nine64-column-map-23-splits", 8, 26, 26, 3, 192, 64, (("wgrad9_kernel", 64), (VEC, 9, 8)), pad=1, perm_cols=True, cout_full=72,
         vmax=3, tags=("short-last-split", "idle-workgroups")),
    case("nine32-313-splits", 8, 104, 104, 3, 64, 64, (("wgrad9_kernel", 32), (VEC, 9, 32)), vmax=3,
         tags=("nsplit>64", "short-last-split", "idle-workgroups")),
    case("nine32-shared-halo", 1, 8, 80, 3, 64, 64, (("wgrad9_kernel", 32), (ROW, 9)), pad=1, perm_cols=True, vmax=3,
         dy_ld=72, dy_choff=8, tags=("short-last-split",)),
    case("nine-wide3-shared-halo-230-splits", 8, 104, 104, 3, 64, 128, (("wgrad9w_kernel", 64, 3), (VEC, 9, 32)), pad=1, vmax=3,
         grad_scale=256.0, tags=("nsplit>64", "short-last-split", "idle-workgroups")),
    case("nine-wide3", 8, 52, 52, 3, 128, 256, (("wgrad9w_kernel", 64, 3), (VEC, 9, 8)), vmax=3, x_ld=192, x_choff=32,
         cout_full=300, tags=("short-last-split",)),
    case("nine-wide3-one-split", 2, 13, 13, 3, 64, 128, (("wgrad9w_kernel", 64, 3), (VEC, 9, 1)), env=MINW8, vmax=3,
         dbias=False, tags=("nsplit==1",)),
    case("nine-wide2", 1, 8, 120, 3, 64, 128, (("wgrad9w_kernel", 64, 2), (VEC, 9, 1)), vmax=3, dy_ld=136, dy_choff=8),
    case("nine-wide2-shared-halo", 2, 6, 160, 3, 128, 128, (("wgrad9w_kernel", 64, 2), (ROW, 9)), pad=1, perm_cols=True, vmax=3,
         grad_scale=256.0),
]

# nsplit > 1, one per split-K family: run twice on Gaussian data, bit-equal (tests "Deterministic (slab reduction, no atomics)")
DETERMINISM_CASES = ("g64x64x3", "nine64-column-map-23-splits", "nine-wide3")
