"""Knowledge distillation for the retraining steps (an addition beyond the reference, whose problem statement names
student-teacher methods next to pruning and estimation but implements none): the objectness-scaled distillation loss of a
YOLOv2 head against a frozen teacher's logits (Mehta and Ozturk, "Object detection at 200 FPS"; Chen et al., NeurIPS 2017).

Both operands are the region layer's logits [B, A*(5+C), H, W], anchor-major (x, y, w, h, obj, C classes).  Per prediction,
with student values s_k and teacher values t_k:
    q   = sig(t_4)                                      the teacher's objectness: a weight, never differentiated
    L_o = 1/2 (sig(s_4) - q)^2
    L_b = 1/2 [(sig(s_0) - sig(t_0))^2 + (sig(s_1) - sig(t_1))^2 + (s_2 - t_2)^2 + (s_3 - t_3)^2]     (w, h as raw logits)
    L_c = T^2 sum_c pt_c (log pt_c - log ps_c)          pt = softmax(t_5.. / T), ps = softmax(s_5.. / T)
    L   = 1/B sum_n [obj_scale L_o + q (box_scale L_b + cls_scale L_c)]
A raw-logit MSE would be dominated by the 840 of 845 predictions per image that are background; q silences them.
CUDA tensors take csrc/distill_loss.hip (loss and gradient in one launch pair); the torch restatement below is the path for
CPU tensors and the kernel's check.  Neither synchronises with the host.  A NaN or Inf logit in either operand gives a
non-finite loss, which train.StepGuard turns into a skipped step.
"""
import torch
import torch.nn as nn


class _DistillLossFn(torch.autograd.Function):
    """loss = mcamd_distill_loss(student, teacher); the kernel returns d(loss)/d(student) with it."""

    @staticmethod
    def forward(ctx, student, teacher, mod):
        from . import ops
        loss, grad = ops.distill_loss(student, teacher, mod.num_anchors, mod.num_classes, mod.obj_scale, mod.box_scale,
                                      mod.cls_scale, mod.temperature)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, go):
        (grad,) = ctx.saved_tensors
        return grad * go, None, None


class DistillLoss(nn.Module):
    def __init__(self, num_classes=20, anchors_cell=5, obj_scale=1., box_scale=1., cls_scale=1., temperature=1.):
        super(DistillLoss, self).__init__()
        if temperature <= 0:
            raise ValueError("DistillLoss: temperature %r must be positive" % (temperature,))
        self.num_classes = int(num_classes)
        self.num_anchors = int(anchors_cell)
        self.obj_scale = float(obj_scale)
        self.box_scale = float(box_scale)
        self.cls_scale = float(cls_scale)
        self.temperature = float(temperature)
        self.fused = True          # CUDA tensors: csrc/distill_loss.hip (False: the torch restatement on the device)

    @classmethod
    def from_model(cls, model, **kw):
        """The loss for a Darknet's region layer (its class and anchor counts)."""
        return cls(num_classes=model.num_classes, anchors_cell=model.num_anchors, **kw)

    def forward(self, student_logits, teacher_logits):
        if student_logits.is_cuda and self.fused and self.num_anchors <= 8:
            return _DistillLossFn.apply(student_logits, teacher_logits, self)
        if student_logits.shape != teacher_logits.shape:
            raise ValueError("DistillLoss: student logits %s, teacher logits %s" % (tuple(student_logits.shape),
                                                                                    tuple(teacher_logits.shape)))
        nB, nA, nC = student_logits.size(0), self.num_anchors, self.num_classes
        nH, nW = student_logits.size(2), student_logits.size(3)
        s = student_logits.reshape(nB, nA, 5 + nC, nH, nW)
        t = teacher_logits.detach().reshape(nB, nA, 5 + nC, nH, nW)
        tau = self.temperature
        q = torch.sigmoid(t[:, :, 4])
        l_o = 0.5 * (torch.sigmoid(s[:, :, 4]) - q) ** 2
        l_b = 0.5 * (((torch.sigmoid(s[:, :, 0:2]) - torch.sigmoid(t[:, :, 0:2])) ** 2).sum(2)
                     + ((s[:, :, 2:4] - t[:, :, 2:4]) ** 2).sum(2))
        log_ps = torch.log_softmax(s[:, :, 5:] / tau, dim=2)
        log_pt = torch.log_softmax(t[:, :, 5:] / tau, dim=2)
        l_c = (tau * tau) * (log_pt.exp() * (log_pt - log_ps)).sum(2)
        # a sigmoid maps an infinite logit to a finite 0 or 1: v - v is 0 for a finite v and NaN otherwise
        sd = s.detach()
        finite = (sd - sd).sum() + (t - t).sum()
        return (self.obj_scale * l_o + q * (self.box_scale * l_b + self.cls_scale * l_c)).sum() / nB + finite
