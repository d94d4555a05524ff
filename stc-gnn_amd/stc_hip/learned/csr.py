"""The learned spatial graph of ``MGP_Gen`` on a sparsity pattern -- that of the prior ``CsrGraph``, in the orientation of Gs itself:

    U, V    = tanh(alpha X Wu), tanh(alpha X Wv)            rows u_i, v_i of length KH = K h, K = B T  (``ops._MgpUV``, unchanged)
    score_e = <u_i, v_j> - <v_i, u_j>                       the reference's einsum pair (STC_GNN.py:231) sampled at entry e = (i, j)
    Ps_e    = softmax over the STORED entries of row i of relu(score)

``pattern`` is what ``stc_hip.graph.csr_pattern(graph, device)`` returns; every per-entry vector has nnz elements in its order.  On the full
pattern this is the reference's ``softmax(relu(P - P^T), -1)``, row-major.  No (N, N) matrix is formed.

On ROCm fp32 tensors with rows of a multiple of 4 floats the score, the softmax and their backwards are one HIP launch each
(``csrc/stc_mgp_csr.hip``); everything else -- CPU tensors, a kernel set without the entry points, rows the kernels do not take -- runs the
same expression on torch operations (``index_add`` / ``scatter_reduce``)."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops

_FUSED = True            # ROCm fp32 operands go to the kernels (False: the torch route, for A/B runs and tests); looked up per call


def mgp_csr_supported(U: torch.Tensor, V: torch.Tensor, pattern) -> bool:
    """Whether the kernels take these rows: float32 (R, ...) tensors of one shape on the pattern's ROCm device, rows of KH floats that
    ``stc_mgp_csr_supported`` accepts (asks for the kernel set only when the tensors are on a device)."""
    if not (_FUSED and ops._f32_on_gpu((U, V)) and U.shape == V.shape and U.dim() >= 2 and U.shape[0] == pattern['n'] and U.shape[0] > 0):
        return False
    if not (U.device == V.device == pattern['rowptr'].device):
        return False
    k = ops.kernels()
    return hasattr(k, 'mgp_csr_score') and k.mgp_csr_supported(U.shape[0], U[0].numel(), pattern['nnz'])


class _MgpCsrScore(Function):
    """score (nnz) from U, V (R, KH) in one launch; the backward gathers dU, dV per row over both orientations of the pattern in one launch
    and forms only what is wanted of them."""

    @staticmethod
    def forward(ctx, U, V, pattern):
        U_, V_ = U.detach().contiguous(), V.detach().contiguous()
        score = ops.kernels().mgp_csr_score(U_, V_, pattern['rowptr'], pattern['colidx'])
        ctx.save_for_backward(U_, V_)
        ctx.pattern = pattern
        return score

    @staticmethod
    @once_differentiable
    def backward(ctx, ds):
        need = ctx.needs_input_grad[:2]
        if not any(need):
            return None, None, None
        U_, V_ = ctx.saved_tensors
        p = ctx.pattern
        if ds.dtype != torch.float32:
            ds = ds.to(torch.float32)
        dU, dV = ops.kernels().mgp_csr_score_bwd(U_, V_, ds.detach().contiguous(), p['rowptr'], p['colidx'], p['t_rowptr'], p['t_colidx'], p['t_entry'])
        return dU if need[0] else None, dV if need[1] else None, None


class _MgpCsrSoftmax(Function):
    """Ps (nnz) = row softmax of relu(score) over the pattern's rows, one launch per direction."""

    @staticmethod
    def forward(ctx, score, pattern):
        s_ = score.detach().contiguous()
        Ps = ops.kernels().mgp_csr_softmax_fwd(s_, pattern['rowptr'])
        ctx.save_for_backward(s_, Ps)
        ctx.pattern = pattern
        return Ps

    @staticmethod
    @once_differentiable
    def backward(ctx, dPs):
        if not ctx.needs_input_grad[0]:
            return None, None
        s_, Ps = ctx.saved_tensors
        if dPs.dtype != torch.float32:
            dPs = dPs.to(torch.float32)
        return ops.kernels().mgp_csr_softmax_bwd(s_, Ps, dPs.detach().contiguous(), ctx.pattern['rowptr']), None


def _score_torch(U, V, pattern):
    u, v = U.flatten(1), V.flatten(1)
    rows, cols = pattern['rows'], pattern['cols']
    return (u.index_select(0, rows) * v.index_select(0, cols)).sum(-1) - (v.index_select(0, rows) * u.index_select(0, cols)).sum(-1)


def _softmax_torch(score, pattern):
    rows, n = pattern['rows'], pattern['n']
    r = torch.relu(score)
    # the row maximum only conditions the exponentials (the softmax does not depend on it): no gradient through it
    m = r.detach().new_zeros(n).scatter_reduce(0, rows, r.detach(), 'amax', include_self=True)
    ex = torch.exp(r - m.index_select(0, rows))
    den = ex.new_zeros(n).index_add(0, rows, ex)
    return ex / den.index_select(0, rows)


def mgp_csr_score(U, V, pattern):
    """score (nnz) of rows U, V (R, KH) or (R, K, h) at the pattern's entries: the kernels where they take the operands, else torch."""
    if mgp_csr_supported(U, V, pattern):
        return _MgpCsrScore.apply(U, V, pattern)
    return _score_torch(U, V, pattern)


def mgp_csr_softmax(score, pattern):
    """Ps (nnz): softmax of relu(score) over the stored entries of every row: the kernels for float32 ROCm vectors, else torch."""
    if (_FUSED and score.dim() == 1 and score.numel() == pattern['nnz'] > 0 and ops._f32_on_gpu((score,)) and score.device == pattern['rowptr'].device
            and hasattr(ops.kernels(), 'mgp_csr_softmax_fwd')):
        return _MgpCsrSoftmax.apply(score, pattern)
    return _softmax_torch(score, pattern)


def mgp_csr_front(X, Wu, Wv, pattern, alpha: float, reduce=None):
    """The learned spatial graph of one window on ``pattern``: Ps (nnz).  X (B, T, N, C) is the data window (rows = nodes, features =
    categories), Wu / Wv (C, h).  ``reduce``: applied once to the nnz scores before the softmax -- the batch-sum all-reduce of a sharded batch
    (the score is additive over the K = B T slices).  ``X`` gets no gradient: in grad mode an ``X`` that requires grad raises ``ValueError``."""
    if torch.is_grad_enabled() and X.requires_grad:
        raise ValueError('mgp_csr_front: X requires grad, and this operator returns no gradient for X (detach the data window)')
    if X.dim() != 4 or X.shape[2] != pattern['n']:
        raise ValueError(f'mgp_csr_front: X must be (B, T, N = {pattern["n"]}, C), got {tuple(X.shape)}')
    if ops.mgp_front_supported(X, Wu, Wv):
        U, V = ops._MgpUV.apply(X, Wu, Wv, 2, float(alpha))             # (N, K, h): one row of K h floats per node
    else:
        U = torch.tanh(alpha * torch.matmul(X, Wu)).flatten(0, 1).transpose(0, 1)
        V = torch.tanh(alpha * torch.matmul(X, Wv)).flatten(0, 1).transpose(0, 1)
    score = mgp_csr_score(U, V, pattern)
    if reduce is not None:
        score = reduce(score)
    return mgp_csr_softmax(score, pattern)
