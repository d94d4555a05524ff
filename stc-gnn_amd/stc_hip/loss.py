"""ComboLoss of the reference trainer (``framework/Model_Trainer.py:9-23``): the loss whose backward
seeds the hot path's backward.

On ROCm fp32 tensors it is three HIP launches (``csrc/stc_loss.hip``, ABI v39): two forward (per-chunk partial sums, one fixed-order
fold), one backward, reading the prediction at its own strides -- the model's ``(horizon, B, N, C).transpose(0, 1)`` view is never copied.
Everything else (CPU tensors, other dtypes, a target that wants a gradient, layouts the kernels do not address, ``_FUSED = False``) runs
the plain torch ops below, unchanged."""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops

_FUSED = True            # ROCm fp32 operands go to the fused kernels (False: the torch ops, for A/B runs and tests); looked up per call


def _as3(t: torch.Tensor):
    """``t`` as a (batch, segments, seg) strided VIEW -- sample b is ``segments`` contiguous runs of ``seg`` elements -- or None where it has no
    such form: 1-D / 2-D contiguous (one run per sample), or dims [2:] contiguous with any non-overlapping strides of dims 0 and 1."""
    if t.dim() in (1, 2):
        if not t.is_contiguous():
            return None
        seg = t.shape[1] if t.dim() == 2 else 1
        return t.as_strided((t.shape[0], 1, seg), (seg, seg, 1))
    if t.dim() < 3:
        return None
    seg = 1
    for n, st in zip(reversed(t.shape[2:]), reversed(t.stride()[2:])):
        if n != 1 and st != seg:
            return None
        seg *= n
    batch, segments = t.shape[:2]
    sb, ss = t.stride()[:2]
    outer = sorted((st, n) for st, n in ((sb, batch), (ss, segments)) if n > 1)        # the runs must not overlap
    reach = seg
    for st, n in outer:
        if st < reach:
            return None
        reach = st * n
    return t.as_strided((batch, segments, seg), (sb if batch > 1 else segments * seg, ss if segments > 1 else seg, 1))


def combo_loss_supported(y_pred: torch.Tensor, y_true: torch.Tensor) -> bool:
    """Whether ``ComboLoss`` runs these operands on the fused kernels (asks for the kernel set only when the tensors are on a ROCm device)."""
    if not (_FUSED and y_pred.is_cuda and y_pred.device == y_true.device and y_pred.dtype == y_true.dtype == torch.float32
            and y_pred.shape == y_true.shape and y_pred.numel() > 0 and not y_true.requires_grad):
        return False
    if _as3(y_pred) is None or _as3(y_true) is None:
        return False
    return bool(getattr(ops.kernels(), 'combo_loss', False))


class _ComboLossFused(Function):
    """loss = stc_combo_loss_fwd_f32(p, y); saves p, y and the per-sample sums when ``save`` (grad mode on and p requires grad)."""

    @staticmethod
    def forward(ctx, p, y, save: bool):
        p3, y3 = _as3(p), _as3(y)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        sums = torch.empty(p3.shape[0], 2, dtype=torch.float64, device=p.device)
        ops.kernels().combo_loss_fwd(p3, y3, loss, sums)
        if save:
            ctx.save_for_backward(p, y, sums)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        p, y, sums = ctx.saved_tensors
        dp = torch.empty_like(p)                                   # p's strides where p is dense (the model's transposed view is)
        if dp.stride() != p.stride():
            dp = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device)
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        ops.kernels().combo_loss_bwd(_as3(p), _as3(y), sums, g, _as3(dp))
        return dp, None, None


class ComboLoss(nn.Module):
    """mean binary cross-entropy + Dice loss per sample, averaged over the batch."""

    def __init__(self):
        super().__init__()
        self.binary_crossentropy = nn.BCELoss(reduction='mean')

    def forward(self, y_pred: torch.Tensor, y_true: torch.Tensor):
        if combo_loss_supported(y_pred, y_true):
            return _ComboLossFused.apply(y_pred, y_true, torch.is_grad_enabled() and y_pred.requires_grad)
        return self.binary_crossentropy(y_pred, y_true) + self.dice_loss(y_pred, y_true)

    @staticmethod
    def _sample_sums(t: torch.Tensor) -> torch.Tensor:
        """Sum over everything but the batch dimension.  A (batch, n) -> (batch,) reduction gives the device one
        workgroup per sample (1.6 ms for 2 x 9.6 M elements on MI355X); two stages keep the whole GPU busy."""
        batch = t.shape[0]
        n = t.numel() // max(batch, 1)
        groups = 1
        while groups < 4096 and n % (2 * groups) == 0 and n // (2 * groups) >= 1024:
            groups *= 2
        flat = t.reshape(batch, groups, -1) if groups > 1 else t.reshape(batch, 1, -1)
        return flat.sum(-1).sum(-1)

    @classmethod
    def dice_loss(cls, y_pred: torch.Tensor, y_true: torch.Tensor):
        overlap = cls._sample_sums(y_pred * y_true)
        mass = cls._sample_sums(y_pred + y_true)
        return (1 - 2 * overlap / mass).mean()
