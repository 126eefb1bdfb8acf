"""CPU restatement of the fp8 quantisation-aware training arithmetic (include/mcamd.h), test-side only.

q, deq, the per-filter exponent e_f and the block formula are q8_ref's, unchanged.

  forward   a8 = q(2 x), (w8, e_f) = quantise_weights(weight, mask)
            y  = 2^-(e_f + 1) * sum a8 * w8                     raw output, fp32: conv(x_q, w_q), x_q = deq(a8) / 2,
                                                               w_q = deq(w8) * 2^-e_f
            scale, shift from the batch statistics of y (biased variance), v = leaky(scale * y + shift)
            byte destination: q(2 v) (pool: of the window maximum; reorg mapped); its fp16 twin: deq(byte) / 2
            fp16 -> fp8 edge: codes q(2 x16), the fp16 slice becomes deq(code) / 2
  backward  both quantisers are the identity (straight-through, no clipping mask):
            dX = dgrad(dY, w_q), dW = wgrad(dY, x_q) * mask
"""
import torch
import torch.nn.functional as F

import q8_ref as R

EPS = 1e-5


def x_q(a8):
    """The values the input codes stand for."""
    return R.deq(a8) / 2.0


def w_q(w8, e):
    """The values the weight codes stand for (fp32; the power of two is exact)."""
    return (R.deq(w8).double() * torch.pow(2.0, -e.double()).view(-1, 1, 1, 1)).float()


def fakequant(w, mask=None):
    """fp32 OIHW w_q of weight * mask (what mcamd_fakequant_q8 writes)."""
    w8, e = R.quantise_weights(w, mask)
    return w_q(w8, e)


def raw(a8, w8, e, dtype=torch.float64):
    """y = 2^-(e_f + 1) * sum a8 * w8, NCHW."""
    k = w8.shape[-1]
    S = F.conv2d(R.deq(a8).to(dtype), R.deq(w8).to(dtype), None, 1, (k - 1) // 2)
    return S * torch.pow(2.0, -(e.to(dtype) + 1.0)).view(1, -1, 1, 1)


def batch_coeffs(y, gamma, beta, eps=EPS):
    """(scale, shift, mean, biased var) of nn.BatchNorm2d in training mode on y (NCHW), in float64 -> fp32 coefficients."""
    yd = y.double()
    mean = yd.mean((0, 2, 3))
    var = yd.var((0, 2, 3), unbiased=False)
    scale = (gamma.double() / torch.sqrt(var + eps)).float()
    shift = (beta.double() - mean * scale.double()).float()
    return scale, shift, mean, var


def act(y, scale, shift, slope=R.SLOPE, dtype=torch.float64):
    """v = leaky(scale * y + shift) (fp32 result of a `dtype` evaluation)."""
    v = y.to(dtype) * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    return torch.where(v > 0, v, v * slope).float()


def train_block(a8, w8, e, gamma, beta, slope=R.SLOPE, eps=EPS, dtype=torch.float64):
    """(y, scale, shift, v fp32) of one training-mode block on codes; y in `dtype` (the kernel stores its fp32 rounding)."""
    y = raw(a8, w8, e, dtype)
    scale, shift, _, _ = batch_coeffs(y, gamma, beta, eps)
    return y, scale, shift, act(y, scale, shift, slope, dtype)


def store_pair(v, dst="plain"):
    """(codes of a byte destination, values of its fp16 twin)."""
    b = R.store_bytes(v, dst)
    return b, R.deq(b) / 2.0


def cast_train(x16):
    """The fp16 -> fp8 edge: (codes q(2 x16), the values written back over the fp16 slice)."""
    b = R.q(2.0 * x16.float())
    return b, R.deq(b) / 2.0


class QatConv(torch.autograd.Function):
    """conv(x_q, w_q) with both quantisers straight-through: x -> q(2 x) -> x_q, weight * mask -> (w8, e_f) -> w_q."""

    @staticmethod
    def forward(ctx, x, weight, mask):
        a8 = R.q(2.0 * x)
        w8, e = R.quantise_weights(weight, mask)
        xq, wq = x_q(a8).to(x.dtype), w_q(w8, e).to(x.dtype)
        ctx.save_for_backward(xq, wq, mask)
        ctx.pad = (weight.shape[-1] - 1) // 2
        return F.conv2d(xq, wq, None, 1, ctx.pad)

    @staticmethod
    def backward(ctx, g):
        xq, wq, mask = ctx.saved_tensors
        dx = torch.nn.grad.conv2d_input(xq.shape, wq, g, 1, ctx.pad)
        dw = torch.nn.grad.conv2d_weight(xq, wq.shape, g, 1, ctx.pad)
        if mask is not None:
            dw = dw * mask.to(dw.dtype)
        return dx, dw, None


# ---------------------------------------------------------------------------
# whole training-mode forward: the blocks named in fp8_layers in the fp8 arithmetic on batch statistics, the others as the
# fp16 engine trains them (fp16 operands, fp16 raw output, batch statistics of it, fp16 activations)
# ---------------------------------------------------------------------------
def forward_train(blocks, state, x, fp8_layers, masks=None, dtype=torch.float64):
    """Train-mode logits (fp32 NCHW) of the "fp8-qat" engine's arithmetic on the CPU.  Tensors travel as fp32 values that
    are exactly representable in their storage format, as in q8_ref.forward; running statistics are not updated."""
    from oracle import darknet_ref as O
    plan = O.plan(blocks)
    fmt = R._formats(plan, fp8_layers)
    fp8 = set(fp8_layers)
    outputs, rawv, ci = {}, {}, 0
    x = x.half().float()

    def store(v, as_f8, dst="plain"):
        return R.deq(R.store_bytes(v, dst)) / 2.0 if as_f8 else R.store_fp16(v, dst)

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
            gamma, beta = state[p + "bn%d.weight" % i].float(), state[p + "bn%d.bias" % i].float()
            slope = R.SLOPE if op["act"] == "leaky" else 1.0
            if i in fp8:
                w8, e = R.quantise_weights(w, m)
                v = train_block(R.q(2.0 * x), w8, e, gamma, beta, slope, dtype=dtype)[3]
            else:
                wm = (w * m if m is not None else w).half().to(dtype)
                y = F.conv2d(x.to(dtype), wm, None, 1, op["pad"]).half().float()
                scale, shift, _, _ = batch_coeffs(y, gamma, beta)
                v = act(y, scale, shift, slope, dtype)
            rawv[ind] = v
            x = store(v, fmt[ind])
        elif t == "maxpool":
            x = store(rawv[ind - 1], fmt[ind], "pool")
        elif t == "reorg":
            x = store(rawv[ind - 1], fmt[ind], "reorg")
        elif t == "route":
            ls = op["layers"]
            x = outputs[ls[0]] if len(ls) == 1 else torch.cat((outputs[ls[0]], outputs[ls[1]]), 1)
        elif t == "region":
            continue
        outputs[ind] = x
    return x
