"""Rank-r ``MixedFusion`` of the learned graph generator (``STC_GNN.MixedFusion(n, rank=r)`` with ``FactorisedLinear`` layers):

    gate = sigmoid(U_A (V_A^T vec A) + b_A + U_P (V_P^T vec P) + b_P),   G = gate * A + (1 - gate) * P

On ROCm fp32 tensors it is two HIP launches forward and at most two backward (``csrc/stc_mixed_fusion_lr.hip``, ABI v40) instead of a dozen
torch launches forward and two to three times as many in autograd's backward.  Everything else (CPU tensors, other dtypes, misaligned views,
ranks above 64, ``_FUSED = False``) runs the torch expression of ``MixedFusion.forward``, unchanged."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import FUSION_LR_MAX_RANK

_FUSED = True            # ROCm fp32 operands go to the fused kernels (False: the torch ops, for A/B runs and tests); looked up per call


def mixed_fusion_lr_supported(A, P, UA, VA, bA, UP, VP, bP) -> bool:
    """Whether ``mixed_fusion_lr`` takes these operands: float32 on one ROCm device, contiguous parameters, everything 16-byte aligned,
    A and P (n, n) -- or 1-D of equal length D, the values of a graph on a sparsity pattern (``graph_mode='csr-learned'``: the kernels take any
    D) --, factors (D, r) with D = n^2 and 1 <= r <= 64, biases (D) (asks for the kernel set only when the tensors are on a device).
    No (n, r) is excluded by measurement: the kernels' replayed forward + backward was faster than the torch route at every pair
    measured (profiles/r12/mixed_fusion_lr_ab.txt)."""
    ts = (A, P, UA, VA, bA, UP, VP, bP)
    if not (_FUSED and all(isinstance(t, torch.Tensor) for t in ts) and ops._f32_on_gpu(ts) and all(t.device == A.device for t in ts)):
        return False
    square = A.dim() == 2 and A.shape[0] == A.shape[1]
    if not (square or A.dim() == 1) or P.shape != A.shape or A.numel() == 0 or UA.dim() != 2:      # 1-D: the stored values of a sparse graph (D = nnz)
        return False
    D, r = A.numel(), UA.shape[1]
    if not (1 <= r <= FUSION_LR_MAX_RANK and all(t.shape == (D, r) for t in (UA, VA, UP, VP)) and bA.shape == (D,) and bP.shape == (D,)):
        return False
    if not ops._laid_out(ts, ts[2:]):
        return False
    k = ops.kernels()
    return bool(getattr(k, 'mixed_fusion_lr', False)) and k.mixed_fusion_lr_supported(D, r)


class _MixedFusionLR(Function):
    """G from (A, P) and the six parameters in two launches; the backward forms only the gradients that are wanted."""

    @staticmethod
    def forward(ctx, A, P, UA, VA, bA, UP, VP, bP):
        A_, P_ = A.detach().contiguous(), P.detach().contiguous()
        gate, G, t = ops.kernels().mixed_fusion_lr_fwd(UA.detach(), VA.detach(), bA.detach(), UP.detach(), VP.detach(), bP.detach(), A_, P_)
        ctx.save_for_backward(A_, P_, UA, VA, UP, VP, gate, t)
        return G

    @staticmethod
    @once_differentiable
    def backward(ctx, dG):
        A, P, UA, VA, UP, VP, gate, t = ctx.saved_tensors
        need = ctx.needs_input_grad                                  # (A, P, U_A, V_A, b_A, U_P, V_P, b_P)
        if not any(need):
            return (None,) * 8
        if dG.dtype != torch.float32:
            dG = dG.to(torch.float32)
        dUA, dVA, dUP, dVP, db, dA, dP = ops.kernels().mixed_fusion_lr_bwd(
            UA.detach(), VA.detach(), UP.detach(), VP.detach(), A, P, gate, t, dG.detach().contiguous(),
            (need[2], need[3], need[5], need[6], need[0], need[1]))
        # both biases receive dpre (autograd copies a tensor it is handed twice before it keeps it as a .grad, as for ops._MixedFusion)
        return dA, dP, dUA, dVA, db if need[4] else None, dUP, dVP, db if need[7] else None


def mixed_fusion_lr(A, P, UA, VA, bA, UP, VP, bP):
    """``MixedFusion(n, rank=r)`` on the fused kernels; ask ``mixed_fusion_lr_supported`` first."""
    return _MixedFusionLR.apply(A, P, UA, VA, bA, UP, VP, bP)
