"""CPU restatement of the 4-bit quantisation-aware training arithmetic (include/mcamd.h), test-side only: the
arithmetic of q8_qat_ref.py (3l) with the weight quantiser of w4_ref.py (3w).

  forward   a8 = q(2 x); (codes, g, e4_f) = w4_ref.quantise(weight, mask), re-done every step
            y  = conv(x_q, w_q), x_q = deq(a8) / 2, w_q = GRID[code] * 2^g * 2^-e4_f            raw output, fp32
               = 2^-(e4_f + 1) * sum a8 * W8x with W8x the e4m3 bytes of GRID[code] * 2^g (exact: powers of two)
            batch statistics, coefficients, byte / fp16-twin stores and the fp16 -> fp8 edge: q8_qat_ref's, unchanged
  backward  straight-through, no clipping mask: dX = dgrad(dY, w_q), dW = wgrad(dY, x_q) * mask -- a weight its group rounds to
            code 0 still receives its gradient
"""
import torch
import torch.nn.functional as F

import q8_ref as R
import q8_qat_ref as Q
import w4_ref as W


def fakequant(w, mask=None):
    """fp32 OIHW w_q of weight * mask (what mcamd_fakequant_q8_w4 writes from the packed operands)."""
    _, _, e4, values, _ = W.quantise(w, mask)
    return W.dequantised(values, e4)


def raw(a8, w, mask=None, dtype=torch.float64):
    """y = conv(x_q, w_q), NCHW, evaluated in `dtype` on the values themselves (no bytes, no exponents)."""
    k = w.shape[-1]
    return F.conv2d(Q.x_q(a8).to(dtype), fakequant(w, mask).to(dtype), None, 1, (k - 1) // 2)


def train_block(a8, w, mask, gamma, beta, slope=R.SLOPE, eps=Q.EPS, dtype=torch.float64):
    """(y, scale, shift, v fp32) of one training-mode block on input codes and fp32 master weights."""
    y = raw(a8, w, mask, dtype)
    scale, shift, _, _ = Q.batch_coeffs(y, gamma, beta, eps)
    return y, scale, shift, Q.act(y, scale, shift, slope, dtype)


class W4QatConv(torch.autograd.Function):
    """conv(x_q, w_q) with both quantisers straight-through: x -> q(2 x) -> x_q, weight * mask -> codes -> w_q."""

    @staticmethod
    def forward(ctx, x, weight, mask):
        xq, wq = Q.x_q(R.q(2.0 * x)).to(x.dtype), fakequant(weight, mask).to(x.dtype)
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


def dequantised_state(blocks, state, w4_layers, masks=None):
    """(state with the weights of the blocks `w4_layers` (conv numbers) replaced by their w_q, masks with those blocks' entries
    None): the "model B" of DESIGN.md 3w / 3x.  B's filter maxima are 128 or 192 times 2^-e4_f, so the fp8 quantiser picks e4_f + 1
    and its bytes are exactly twice the w4 values: every fp8-qat quantity of B equals the fp8-w4-qat quantity of the original."""
    from oracle import darknet_ref as O
    out = dict(state)
    mk = list(masks) if masks is not None else None
    ci = 0
    for op in O.plan(blocks):
        if op["type"] != "conv":
            continue
        if op["id"] in set(w4_layers):
            key = op["prefix"] + "conv%d.weight" % op["id"]
            out[key] = fakequant(state[key].float(), mk[ci] if mk is not None else None)
            if mk is not None:
                mk[ci] = None
        ci += 1
    return out, mk


def forward_train(blocks, state, x, w4_layers, masks=None, dtype=torch.float64):
    """Train-mode logits (fp32 NCHW) of the "fp8-w4-qat" engine's arithmetic on the CPU: q8_qat_ref.forward_train on the
    dequantised state (dequantised_state's argument; test_q8_w4_qat_cpu.py checks it block-wise)."""
    st, mk = dequantised_state(blocks, state, w4_layers, masks)
    return Q.forward_train(blocks, st, x, w4_layers, masks=mk, dtype=dtype)
