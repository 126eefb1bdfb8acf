"""CPU restatement of the fp8 (OCP e4m3) inference arithmetic (include/mcamd.h), test-side only.

  q(v)        round-to-nearest-even to e4m3fn after clamping to [-448, 448]
  weights     per filter f of w = weight * mask: a = max |w_f|, (m, x) = frexp(a), e_f = 9 - x if m <= 0.875 else 8 - x
              (0 for an all-zero filter), w8 = q(w * 2^e_f)
  activations a8 = q(2 v), v the fp32 epilogue value (after BatchNorm, LeakyReLU and, for POOL, the window maximum)
  block       v = leaky(scale_f * 2^-(e_f + 1) * S + shift_f), S = sum a8 * w8

Bytes are uint8 tensors holding the e4m3 codes; `deq` gives their values.  MaxPool of bytes is taken on the
order-preserving key of the code (-0 below +0), which is what the kernel does: q is monotone, so this is q of the maximum.
"""
import torch
import torch.nn.functional as F

from oracle import darknet_ref as O

F8 = torch.float8_e4m3fn
SLOPE = float(torch.tensor(0.1, dtype=torch.float32))      # the fp32 value of the LeakyReLU slope


def q(v):
    """fp32 values -> e4m3 codes (uint8)."""
    return v.float().clamp(-448.0, 448.0).to(F8).view(torch.uint8)


def deq(b):
    """e4m3 codes (uint8) -> fp32 values."""
    return b.contiguous().view(F8).float()


def ordinal(b):
    """Signed position of a code on the e4m3 grid (+0 and -0 both 0): adjacent codes differ by one."""
    mag = (b & 0x7F).to(torch.int32)
    return torch.where((b & 0x80) != 0, -mag, mag)


def key(b):
    """Order-preserving key of a code: unsigned order = value order, -0 below +0."""
    b = b.to(torch.int32)
    return torch.where((b & 0x80) != 0, b ^ 0xFF, b ^ 0x80)


def unkey(k):
    k = k.to(torch.int32)
    return torch.where((k & 0x80) != 0, k ^ 0x80, k ^ 0xFF).to(torch.uint8)


def pool_bytes(b):
    """MaxPool(2, 2) of NCHW codes by value."""
    return unkey(F.max_pool2d(key(b).float(), 2, 2))


def filter_exponents(w):
    """int32 [cout]: e_f of every filter of the (already masked) OIHW weights."""
    a = w.detach().float().abs().flatten(1).amax(1)
    m, x = torch.frexp(a)
    e = torch.where(m <= 0.875, 9 - x, 8 - x)
    return torch.where(a == 0, torch.zeros_like(e), e).to(torch.int32)


def quantise_weights(w, mask=None):
    """(codes uint8 OIHW, exponents int32 [cout]) of weight * mask."""
    wm = w.detach().float() * (mask.float() if mask is not None else 1.0)
    e = filter_exponents(wm)
    scaled = (wm.double() * torch.pow(2.0, e.double()).view(-1, 1, 1, 1)).float()      # ldexp: exact
    return q(scaled), e


def block(a8, w8, e, scale, shift, slope=SLOPE, dtype=torch.float64):
    """One quantised block on codes: the fp32 epilogue value v (NCHW, full resolution) before any store."""
    k = w8.shape[-1]
    S = F.conv2d(deq(a8).to(dtype), deq(w8).to(dtype), None, 1, (k - 1) // 2)
    sc = scale.to(dtype) * torch.pow(2.0, -(e.to(dtype) + 1.0))
    v = S * sc.view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    v = torch.where(v > 0, v, v * slope)
    return v.float()


def store_bytes(v, dst="plain"):
    """The codes a byte destination receives: q(2 v), pooled / reorg'ed."""
    b = q(2.0 * v)
    if dst == "pool":
        return pool_bytes(b)
    if dst == "reorg":
        return O.reorg(b, 2)
    return b


def store_fp16(v, dst="plain"):
    """The values an fp16 destination receives (fp32 tensor of fp16-representable values)."""
    h = v.clamp(-65504.0, 65504.0).half().float()
    if dst == "pool":
        return F.max_pool2d(h, 2, 2)
    if dst == "reorg":
        return O.reorg(h, 2)
    return h


def byte_mismatch(got, ref):
    """(share of differing codes, do all differing codes sit on adjacent grid positions?)"""
    diff = got != ref
    n = int(diff.sum())
    if n == 0:
        return 0.0, True
    step = (ordinal(got[diff]) - ordinal(ref[diff])).abs().max()
    return n / got.numel(), bool(step <= 1)


MISMATCH_CAP = 1e-4      # share of output codes that may differ from the float64 reference's (each by one grid step)
# The same share for the kernel form on the block-scaled fp8 MFMA (MCAMD_Q8_MFMA=1).  That instruction keeps, inside a group
# of 8 products, 14 bits below the group's largest product (a product 2^-13 of the largest survives, one 2^-14
# of it does not), so its sum carries a relative error of the order of 2^-13 instead of fp32's 2^-24.  Neighbouring e4m3 codes
# are at least 2^-4 apart relative to the value, so an error of that size carries about 2^-13 / 2^-4 = 2^-9 of the values
# across a rounding boundary; one more factor of 2 for the part of the sum that the BatchNorm shift cancels.  From the width
# of the instruction and of the format, not from the shares the kernel gave.
FP8_MFMA_CAP = 2.0 ** -8


# ---------------------------------------------------------------------------
# whole forward: the blocks named in fp8_layers (conv numbers) quantised, the others as the fp16 engine runs them
# ---------------------------------------------------------------------------
def _structure(plan):
    srcs, readers = {}, {}
    for ind, op in enumerate(plan):
        t = op["type"]
        if t == "region":
            continue
        srcs[ind] = list(op["layers"]) if t == "route" else [ind - 1]
        for s in srcs[ind]:
            readers.setdefault(s, []).append(ind)
    return srcs, readers


def _formats(plan, fp8_layers):
    """ind -> True when the tensor op `ind` materialises is stored as e4m3 codes: its producing block and every block
    that reads it are fp8 blocks (a concatenation: every member's producer too)."""
    srcs, readers = _structure(plan)
    fp8 = set(fp8_layers)

    def producer(ind):
        if ind < 0:
            return None
        op = plan[ind]
        if op["type"] == "conv":
            return op["id"]
        if op["type"] in ("maxpool", "reorg"):
            return producer(ind - 1)
        if op["type"] == "route" and len(op["layers"]) == 1:
            return producer(op["layers"][0])
        return None

    def read_as_f8(ind, pooled):
        """Is every reader of tensor `ind` an fp8 block?  (`pooled` False: ignore the MaxPool / Reorg readers of a conv
        output -- they materialise a tensor of their own.)"""
        rs = [r for r in readers.get(ind, []) if pooled or plan[r]["type"] not in ("maxpool", "reorg")]
        if not rs:
            return False
        for r in rs:
            op = plan[r]
            if op["type"] == "conv":
                if op["id"] not in fp8:
                    return False
            elif op["type"] == "route":
                if not all(producer(m) in fp8 for m in op["layers"]) or not read_as_f8(r, True):
                    return False
            else:
                return False
        return True

    fmt = {}
    for ind, op in enumerate(plan):
        if op["type"] == "conv":
            fmt[ind] = producer(ind) in fp8 and read_as_f8(ind, False)
        elif op["type"] in ("maxpool", "reorg"):
            fmt[ind] = producer(ind) in fp8 and read_as_f8(ind, True)
    return fmt


def forward(blocks, state, x, fp8_layers, masks=None, dtype=torch.float64):
    """Logits (fp32 NCHW) of the fp8 engine's arithmetic on the CPU.  Tensors travel as fp32 VALUES that are exactly
    representable in their storage format (fp16, or e4m3 / 2), so an fp8 block's input codes are q(2 value) whichever
    format its input was stored in (the cast pass of an fp16 -> fp8 edge is that expression)."""
    plan = O.plan(blocks)
    fmt = _formats(plan, fp8_layers)
    fp8 = set(fp8_layers)
    outputs, raw, ci = {}, {}, 0
    x = x.half().float()

    def store(v, as_f8, dst="plain"):
        return deq(store_bytes(v, dst)) / 2.0 if as_f8 else store_fp16(v, dst)

    for ind, op in enumerate(plan):
        t = op["type"]
        if t == "conv":
            p, i = op["prefix"], op["id"]
            w = state[p + "conv%d.weight" % i].float()
            m = masks[ci] if masks is not None else None
            ci += 1
            if not op["bn"]:
                wm = (w * m if m is not None else w).half().to(dtype)
                x = (F.conv2d(x.to(dtype), wm, None, 1, op["pad"]) + state[p + "conv%d.bias" % i].to(dtype).view(1, -1, 1, 1)).float()
                outputs[ind] = x
                continue
            scale = state[p + "bn%d.weight" % i].float() / torch.sqrt(state[p + "bn%d.running_var" % i].float() + 1e-5)
            shift = state[p + "bn%d.bias" % i].float() - state[p + "bn%d.running_mean" % i].float() * scale
            slope = SLOPE if op["act"] == "leaky" else 1.0
            if i in fp8:
                w8, e = quantise_weights(w, m)
                v = block(q(2.0 * x), w8, e, scale, shift, slope, dtype)
            else:
                wm = (w * m if m is not None else w).half().to(dtype)
                v = F.conv2d(x.to(dtype), wm, None, 1, op["pad"]) * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
                v = torch.where(v > 0, v, v * slope).float()
            raw[ind] = v
            x = store(v, fmt[ind])
        elif t == "maxpool":
            assert op["size"] == 2 and op["stride"] == 2 and plan[ind - 1]["type"] == "conv"
            x = store(raw[ind - 1], fmt[ind], "pool")
        elif t == "reorg":
            assert op["stride"] == 2 and plan[ind - 1]["type"] == "conv"
            x = store(raw[ind - 1], fmt[ind], "reorg")
        elif t == "route":
            ls = op["layers"]
            x = outputs[ls[0]] if len(ls) == 1 else torch.cat((outputs[ls[0]], outputs[ls[1]]), 1)
        elif t == "region":
            continue
        outputs[ind] = x
    return x
