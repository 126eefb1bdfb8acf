"""A numpy restatement of the proximal group-lasso contract (include/mcamd.h), test-side only: one step of a
BLOCK segment and of a GATE segment in the documented float64 / float32 arithmetic, operation by operation, including the
lane order of the sums.  Also the shapes and the seeded data the CPU and the GPU tests share."""
import numpy as np

FILTERS = 64

# (cout, cin, khw): one full block, 9 taps and 1; a ragged last filter block; kb = 32 with a ragged block; several channel
# blocks and two filter blocks; 25 taps (the direct form)
BLOCKS = [(64, 64, 9), (64, 64, 1), (125, 64, 1), (96, 32, 9), (128, 192, 9), (70, 64, 25)]
GATES = [1, 255, 1024]
TAU = 0.05          # lr * lam of the seeded cases
# The bar a device result is held to on kept block elements, in fp32 steps from this restatement.  n2 is bit-defined (exact
# products, a pinned order), so the comparison with thr2 is exact.  s = 1 - sqrt(thr2 / n2) could differ by a few float64 steps
# if the device's float64 divide or square root were not correctly rounded, which would move the final fp32 rounding of w * s
# by at most one step: the derived bound is 1.  Measured on gfx950: 0 of 202 432 kept elements of the kernel cases and 0 of
# the mini model's 160 093 parameter elements differ at all, so the bar is equality.
MAX_ULP = 0


def wave_sum(x):
    """float64 [..., n] -> [...]: lane l adds elements l, l + 64, ... in ascending order starting from 0.0; the 64 lane sums are
    combined by s[l] = s[l] + s[l ^ d] for d = 32, 16, 8, 4, 2, 1."""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    lanes = np.zeros(x.shape[:-1] + (64,), np.float64)
    for first in range(0, n, 64):
        part = x[..., first:first + 64]
        lanes[..., :part.shape[-1]] = lanes[..., :part.shape[-1]] + part
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ d]
    return lanes[..., 0]


def block_dims(cout, cin, khw):
    kb = 64 if cin % 64 == 0 else 32
    assert cin % 32 == 0
    return (cout + FILTERS - 1) // FILTERS, cin // kb, kb


def nblocks(cout, cin, khw):
    nfb, ncb, _ = block_dims(cout, cin, khw)
    return nfb * ncb * khw


def block_prox(w, tau2):
    """(new weights float32 of w's shape, nz int32 [blocks])."""
    w = np.asarray(w, np.float32)
    cout, cin = w.shape[0], w.shape[1]
    w3 = w.reshape(cout, cin, -1)
    khw = w3.shape[2]
    nfb, ncb, kb = block_dims(cout, cin, khw)
    out = w3.copy()
    nz = np.zeros((nfb, ncb, khw), np.int32)
    tau2 = np.float64(tau2)
    with np.errstate(all="ignore"):
        for fb in range(nfb):
            rows = min(FILTERS, cout - FILTERS * fb)
            for cb in range(ncb):
                blk = w3[FILTERS * fb:FILTERS * fb + rows, kb * cb:kb * cb + kb, :].astype(np.float64)      # [r][c][tap]
                n2 = wave_sum((blk * blk).transpose(2, 0, 1).reshape(khw, rows * kb))                       # e = r * kb + c
                thr2 = tau2 * np.float64(rows * kb)
                for tap in range(khw):
                    if n2[tap] <= thr2:
                        out[FILTERS * fb:FILTERS * fb + rows, kb * cb:kb * cb + kb, tap] = np.float32(0.0)
                    else:
                        s = np.float64(1.0) - np.sqrt(thr2 / n2[tap])
                        out[FILTERS * fb:FILTERS * fb + rows, kb * cb:kb * cb + kb, tap] = (blk[:, :, tap] * s).astype(np.float32)
                        nz[fb, cb, tap] = 1
    return out.reshape(w.shape), nz.reshape(-1)


def gate_prox(gamma, tau):
    """(new gamma float32, nz int32): tau is rounded to float32 first; one float32 subtract."""
    gamma = np.asarray(gamma, np.float32)
    with np.errstate(all="ignore"):
        a = np.abs(gamma) - np.float32(tau)
        assert a.dtype == np.float32
        out = np.where(a > 0, np.copysign(a, gamma), np.where(a <= 0, np.float32(0.0), gamma)).astype(np.float32)
        nz = (~(a <= 0)).astype(np.int32)
    return out, nz


def block_weights(shape, tau, seed):
    """Seeded Gaussians whose per-block scale spans a decade around the threshold: a block's RMS equals `tau` at scale 1, so
    scales from 10^-0.5 to 10^0.5 put some blocks on each side.  A tensor of one block is kept (10^0.25), one of two has
    one block on each side (10^-0.25, 10^0.25)."""
    cout, cin, khw = shape
    rng = np.random.RandomState(seed)
    nfb, ncb, kb = block_dims(cout, cin, khw)
    exponent = rng.uniform(-0.5, 0.5, size=(nfb, ncb, khw))
    if exponent.size <= 2:
        exponent = np.array([-0.25, 0.25])[-exponent.size:].reshape(exponent.shape)
    scale = tau * 10.0 ** exponent
    per = np.repeat(np.repeat(scale, FILTERS, axis=0)[:cout], kb, axis=1)                                  # [cout][cin][khw]
    return (rng.standard_normal((cout, cin, khw)) * per).astype(np.float32)


def gate_weights(c, tau, seed):
    """Seeded gammas of both signs on both sides of tau, with one exactly at +tau and one at -tau (fp32) when c > 2."""
    rng = np.random.RandomState(seed)
    g = (rng.standard_normal(c) * 2.0 * tau).astype(np.float32)
    if c > 2:
        g[1], g[2] = np.float32(tau), -np.float32(tau)
    return g


def ulp_steps(a, b):
    """How many fp32 values apart a and b are, per element (int64); the same bits give 0."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
