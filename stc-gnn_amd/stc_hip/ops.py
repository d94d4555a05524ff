"""Autograd operators of the STC-GNN hot path, each a thin host sequence of HIP launches.

    bdg_dif      BDG_Dif.forward  (reference STC_GNN.py:31-47)  = SpMM hops + node kernel
    gru_gates    split / sigmoid / reset*H / second concat (STC_GNN.py:71-75)
    gru_blend    tanh + GRU blend (STC_GNN.py:76-78)
    concat2      torch.cat([Xt, Ht_1], -1) (STC_GNN.py:68)
    cheby_dense  BDG_Dif.cheby_poly on the small category graph (STC_GNN.py:24-29)
    mixed_fusion, mgp_front   the learned graph generator MGP_Gen (STC_GNN.py:210-261), at the end of the file; its rank-r fusion is ``stc_hip.fusion``

Decomposition of one BDG_Dif (K = Ks = Kc in the reference, kept separate here):

    Z_0 = X,  Z_1 = Gs^T X,  Z_k = 2 Gs^T Z_{k-1} - Z_{k-2}         K-1 CSR SpMM launches
    Y   = node(Z_0..Z_{K-1}; T_c(Gc), W, b)                         one fused node kernel

i.e. the Chebyshev recurrence runs on the FEATURES (never forms Gs^2; equal math because
polynomials of Gs commute with Gs) and the K*K*L concat is never written.  Backward:

    dZ_k, dW, db, dT_c = node_bwd(dY)
    for k = K-1 .. 2:   dZ_{k-1} += 2 Gs dZ_k ;  dZ_{k-2} -= dZ_k ;  dGs += 2 <Z_{k-1}, dZ_k>
    dX = dZ_0 + Gs dZ_1 ;  dGs += <Z_0, dZ_1>

All launches go to ``kernels()`` -- the ctypes front of libstc_hip.so.  There is no other
implementation in the product: without the built library or without a ROCm device the
first call raises ``StcError``.
"""
from __future__ import annotations

import enum
from types import SimpleNamespace
from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import SPMM_SUM_BF16_MAX_ADD, SPMM_SUM_MAX_ADD          # addends of stc_spmm_sum_bf16 / _f32
from .graph import SpatialOperand
from .small import (_alias, _check_guard, _guard, _out_slots, _refuse_differentiable, _stacks, _unpack, last_uses, small_graph_supported,
                    stc_small_graph, wavefront)

_kernels = None


def kernels():
    """The kernel set every operator launches through (HIP; created on first use)."""
    global _kernels
    if _kernels is None:
        from ._lib import HipKernels
        _kernels = HipKernels()
    return _kernels


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _cn(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else _c(t)                          # (an optional bias)


# ----------------------------------------------------------------------------- Chebyshev set of Gc
class _ChebyDense(Function):
    @staticmethod
    def forward(ctx, G, K: int):
        G = _c(G)
        T = G.new_empty((K,) + tuple(G.shape))
        kernels().cheby_dense_fwd(G, K, T)
        ctx.save_for_backward(G, T)
        return T

    @staticmethod
    @once_differentiable
    def backward(ctx, dT):
        G, T = ctx.saved_tensors
        dG = torch.empty_like(G)
        kernels().cheby_dense_bwd(G, T, dT.contiguous().clone(), dG)    # dT is consumed as scratch
        return dG, None


def cheby_dense(G: torch.Tensor, K: int) -> torch.Tensor:
    """(K, n, n) stack T_0..T_{K-1} of a small dense graph, matrix side as the reference."""
    if G.dim() != 2 or G.shape[0] != G.shape[1]:
        raise ValueError(f'category graph must be square, got {tuple(G.shape)}')
    return _ChebyDense.apply(G, K)


# ----------------------------------------------------------------------------- BDG_Dif
_NODE_PACK = True        # few categories (C <= 16): floor(16 / C) nodes per row tile of the matrix-core node kernels (``_node_pack``; tests flip it)
_PACK_SPLIT_ROWS = 1 << 18   # rows from which a node count that the tile does not divide is worth a second launch for its remainder


def _spatial_slabs(X, fwd_val, op: SpatialOperand, Ks: int):
    """[Z_0 = X, Z_1 = Gs^T X, Z_k = 2 Gs^T Z_{k-1} - Z_{k-2}]: the Ks-1 SpMM launches of one BDG_Dif."""
    k = kernels()
    B, N, C, L = X.shape
    F = C * L
    Zs = [X]
    for order in range(1, Ks):
        Zk = torch.empty_like(X)
        if order == 1:
            k.csr_spmm(op.fwd_rowptr, op.fwd_colidx, fwd_val, N, N, X.view(B, N, F), None, Zk.view(B, N, F), 1.0, 0.0, plan=op.fwd_plan)
        else:
            k.csr_spmm(op.fwd_rowptr, op.fwd_colidx, fwd_val, N, N, Zs[-1].view(B, N, F),
                       Zs[-2].view(B, N, F), Zk.view(B, N, F), 2.0, -1.0, plan=op.fwd_plan)
        Zs.append(Zk)
    return Zs


def _node_pack(X: torch.Tensor, Tc: torch.Tensor, Ks: int, Ho: int) -> int:
    """How many nodes one row tile of the matrix-core node kernels takes when the categories are few (C <= 16); 0: the route does not apply.
    The fp32-MFMA node kernels (csrc/stc_node_mfma.hip) work on tiles of 16 category rows and take a node of Cr <= 16 rows per tile; the node
    kernel is node-local (reference STC_GNN.py:38-45: the 2-mode product and the projection touch one node's C x L rows), so floor(16 / C)
    consecutive nodes ARE one node of p C categories whose category graph is block-diagonal -- same rows in memory, T_c repeated on the
    diagonal (``_block_diag``).  BASELINE configuration 2 (C = 8: two nodes per tile) otherwise runs the generic vector kernel: 35 / 181 us
    forward / backward for 13 / 32 + 8 on the matrix cores; the SF shape's C = 5 packs three nodes into 15 rows.  1: one node per tile
    (C > 8, or a small node count that p does not divide); 0: C > 16, a shape the matrix-core kernels do not take, bf16 rows, the switch
    off.  When p does not divide a LARGE node count the last (count mod p) nodes run one per tile in a second launch (``_packed_spans``)."""
    B, N, C, L = X.shape
    if not _NODE_PACK or X.dtype != torch.float32 or C > 16:
        return 0
    Kc = Tc.shape[0]
    if Ks != Kc or not 1 <= Ks <= 3 or Ho not in (16, 32) or L not in (20, 32):      # = fast_path_shape of csrc/stc_node_mfma.hip
        return 0
    p = 16 // C
    # a node count that p does not divide: the last nodes run one per tile in a launch of their own (``_packed_spans``) -- worth two more small
    # launches only when the packed part is large (N = 50 176, C = 5, 8 samples: 38.8 -> 59.3 samples/s; the SF shape's 3 200 nodes at order 3
    # with learned graphs: 10.1 ms with one node per tile, 11.2 with the split)
    return p if (B * N) % p == 0 or B * N * C >= _PACK_SPLIT_ROWS else 1


def _packed_spans(R: int, p: int):
    """[(first node, node count, nodes per tile)]: the nodes that fill whole tiles of p, then the remainder one node per tile."""
    main = R - R % p
    return [(0, main, p)] + ([(main, R - main, 1)] if main < R else []) if main else [(0, R, 1)]


def _cell_pack(k, R: int, C: int, Ks: int, Kc: int, L: int, h: int) -> int:
    """Nodes per row tile for the FUSED cell kernels of the per-cell path (gate math in the node kernels' epilogues / prologues): 1 where
    they take C itself, 16 / C where C divides 16 and the node count (the rows of 16 / C nodes are then exactly one tile: ``_node_pack``),
    0 where neither holds (the composed sequence: node kernel, gate kernel, node kernel, blend kernel)."""
    if k.cell_fused_supported(Ks, Kc, C, L, h):
        return 1
    if _NODE_PACK and C < 16 and 16 % C == 0 and R % (16 // C) == 0 and k.cell_fused_supported(Ks, Kc, 16, L, h):
        return 16 // C
    return 0


def _block_diag(Tc: torch.Tensor, p: int) -> torch.Tensor:
    """(Kc, C, C) -> (Kc, pC, pC) with T_c on the diagonal blocks: the category graph of p nodes taken as one."""
    Kc, C, _ = Tc.shape
    out = Tc.new_zeros(Kc, p, C, p, C)
    out.diagonal(dim1=1, dim2=3).copy_(Tc.unsqueeze(-1).expand(Kc, C, C, p))       # (diagonal view: (Kc, C, C, p))
    return out.view(Kc, p * C, p * C)


def _bdg_forward(X, W, b, Tc, fwd_val, op: SpatialOperand, Ks: int):
    """Launch sequence of one BDG_Dif forward on raw tensors; returns (Y, [Z_0..Z_{Ks-1}])."""
    k = kernels()
    B, N, C, L = X.shape
    Ho = W.shape[1]
    Zs = _spatial_slabs(X, fwd_val, op, Ks)
    Y = X.new_empty(B, N, C, Ho)
    p = max(1, _node_pack(X, Tc, Ks, Ho))
    R = B * N
    for lo, n, q in _packed_spans(R, p):
        k.bdg_node_fwd([z.view(R, C, L)[lo:lo + n].view(n // q, q * C, L) for z in Zs], Tc if q == 1 else _block_diag(Tc, q), W, b,
                       Y.view(R, C, Ho)[lo:lo + n].view(n // q, q * C, Ho))
    return Y, Zs


def _mix_grad(Zs, dY, W, Kc: int) -> torch.Tensor:
    """dT_c[p, d] = sum_r sum_o U_c[r, p, o] dY[r, d, o] with U_c = sum_n Z_n W_{n,c} (autograd of STC_GNN.py:38 w.r.t. the category graph) for few
    categories: ``stc_mix_dt_f32`` on the tiles of 16 rows the packed node kernels run on.  (As library GEMMs -- Q_n = Z_n^T . dY over the rows,
    then a contraction with W -- two launches of 41 us at configuration 2's shape, 64 workgroups each.)"""
    B, N, C, L = Zs[0].shape
    dTc = W.new_empty(Kc, C, C)
    kernels().mix_dT([z.view(B * N, C, L) for z in Zs], W, dY.view(B * N, C, W.shape[1]), dTc)
    return dTc


def _bdg_backward_slabs(dY, Zs, W, Tc, op: SpatialOperand, Ks: int, has_bias: bool, need_Tc: bool, need_val: bool, gates=None, cand=None, pack: int = 1):
    """Node-kernel backward and every hop of the Chebyshev recurrence but the last.

    Returns (g, dW, db | None, dTc | None, dval | None) with g = [g_0, g_1, ...] such that
    dX = g_0 + Gs.g_1 (g_1 absent for Ks = 1): the caller performs that last product, plain or with an
    element-wise consumer fused into its epilogue.
    """
    k = kernels()
    B, N, C, L = Zs[0].shape
    Ho = W.shape[1]
    F = C * L
    dZ = [torch.empty_like(Zs[0]) for _ in range(Ks)]
    dW = torch.empty_like(W)
    db = W.new_empty(Ho) if has_bias else None
    dTc = torch.empty_like(Tc) if need_Tc else None
    # pack > 1 (the fused prologue kernels on few categories, ``_cell_pack``): `pack` nodes are one node of pack * C categories, block-diagonal T_c
    rows = lambda ts: [t.view(B * N // pack, pack * C, t.shape[-1]) for t in ts]
    Tcp = Tc if pack == 1 else _block_diag(Tc, pack)
    if gates is not None:       # dY = gate pre-activation gradient, formed inside the kernel from (dCandIn, dU, H, U, R)
        dCandIn, Cand, H, U, Rg, dHnew, dH = gates   # dU = dHnew * (Cand - H); dH = dCandIn[h part] * R + dHnew * (1 - U); dXt stays in dCandIn
        dCandIn, Cand, H, U, Rg, dHnew, dH = rows((dCandIn, Cand, H, U, Rg, dHnew, dH))
        k.cell_gates_bwd(rows(Zs), Tcp, W, dCandIn, None, H, U, Rg, dHnew, rows(dZ), dW, db, None, dH, dH_in_scaled=True, Cand=Cand)
    elif cand is not None:      # dY = dHnew * U * (1 - Cand^2), formed inside the kernel
        k.cell_cand_bwd(rows(Zs), Tcp, W, *rows(cand), rows(dZ), dW, db)
    else:
        dY = _c(dY)
        rows = lambda ts: [t.view(B * N, C, t.shape[-1]) for t in ts]
        p = _node_pack(Zs[0], Tc, Ks, Ho)
        if p >= 1:
            # few categories: floor(16 / C) nodes per row tile of the matrix-core kernel (``_node_pack``); that kernel leaves dT_c to the caller
            R = B * N
            for i, (lo, n, q) in enumerate(_packed_spans(R, p)):
                dW_i, db_i = (dW, db) if i == 0 else (torch.empty_like(dW), None if db is None else torch.empty_like(db))
                k.bdg_node_bwd([z.view(R, C, L)[lo:lo + n].view(n // q, q * C, L) for z in Zs], Tc if q == 1 else _block_diag(Tc, q), W,
                               dY.view(R, C, Ho)[lo:lo + n].view(n // q, q * C, Ho), [z.view(R, C, L)[lo:lo + n].view(n // q, q * C, L) for z in dZ],
                               dW_i, db_i, None)
                if i:                                                    # (the remainder's share of the parameter gradients)
                    dW.add_(dW_i)
                    if db is not None:
                        db.add_(db_i)
            if need_Tc:
                dTc = _mix_grad(Zs, dY, W, Tc.shape[0])
        else:
            k.bdg_node_bwd(rows(Zs), Tc, W, dY.view(B * N, C, Ho), rows(dZ), dW, db, dTc)
    dval = torch.zeros_like(op.fwd_val) if need_val else None
    v3 = lambda t: t.view(B, N, F)
    dense = op.nnz == N * N                                        # learned dense Gs: the "pattern" is the whole matrix

    def values_grad(A, Bm, alpha):
        """dval[i, j] += alpha * sum_b <A[b, i, :], Bm[b, j, :]> (gradient of the 1-mode product w.r.t. the graph values)."""
        if dense:
            # on the full pattern this is ONE dense GEMM, (N, B*F) x (B*F, N): a plain library GEMM (rocBLAS through torch),
            # not a sampled product -- one wave per stored entry (stc_csr_sddmm_f32) took 524 us per call at the SF shape,
            # 62 % of the learned-graph train step
            a2 = A.transpose(0, 1).reshape(N, B * F)
            b2 = Bm.transpose(0, 1).reshape(N, B * F)
            dval.view(N, N).addmm_(a2, b2.t(), alpha=alpha)
        else:
            k.csr_sddmm(op.fwd_rowptr, op.fwd_colidx, N, N, A, Bm, dval, alpha, True)

    for order in range(Ks - 1, 1, -1):
        k.csr_spmm(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, N, N, v3(dZ[order]), v3(dZ[order - 1]),
                   v3(dZ[order - 1]), 2.0, 1.0, plan=op.bwd_plan)
        if dZ[order].dtype == torch.bfloat16:
            dZ[order - 2].sub_(dZ[order])                        # bf16 slabs, Ks >= 3 only: a torch stream op (no bf16 axpy entry point)
        else:
            k.axpy(-1.0, dZ[order], dZ[order - 2])
        if need_val:
            values_grad(v3(dZ[order]), v3(Zs[order - 1]), 2.0)
    if Ks > 1 and need_val:
        values_grad(v3(dZ[1]), v3(Zs[0]), 1.0)
    return dZ[:2], dW, db, dTc, dval


def _bdg_backward(dY, Zs, W, Tc, op: SpatialOperand, Ks: int, has_bias: bool, need_X: bool, need_Tc: bool, need_val: bool):
    """Launch sequence of one BDG_Dif backward; returns (dX | None, dW, db | None, dTc | None, dval | None)."""
    g, dW, db, dTc, dval = _bdg_backward_slabs(dY, Zs, W, Tc, op, Ks, has_bias, need_Tc, need_val)
    if Ks > 1 and need_X:
        B, N, C, L = g[0].shape
        v3 = lambda t: t.view(B, N, C * L)
        kernels().csr_spmm(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, N, N, v3(g[1]), v3(g[0]), v3(g[0]), 1.0, 1.0, plan=op.bwd_plan)
    return (g[0] if need_X else None), dW, db, dTc, dval


class _BdgDif(Function):
    @staticmethod
    def forward(ctx, X, W, b, Tc, fwd_val, op: SpatialOperand, Ks: int):
        X, W, b, Tc, fwd_val = _c(X), _c(W), _cn(b), _c(Tc), _c(fwd_val)
        Y, Zs = _bdg_forward(X, W, b, Tc, fwd_val, op, Ks)
        ctx.save_for_backward(W, Tc, *Zs)
        ctx.op = op
        ctx.has_bias = b is not None
        ctx.Ks = Ks
        return Y

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        W, Tc, *Zs = ctx.saved_tensors
        need_X, _, _, need_Tc, need_val = ctx.needs_input_grad[:5]
        dX, dW, db, dTc, dval = _bdg_backward(dY, Zs, W, Tc, ctx.op, ctx.Ks, ctx.has_bias, need_X, need_Tc, need_val)
        return dX, dW, db, dTc, dval, None, None


def bdg_dif(X: torch.Tensor, op: SpatialOperand, Tc: torch.Tensor, W: torch.Tensor,
            b: Optional[torch.Tensor], Ks: int, pad: int = 0) -> torch.Tensor:
    """Y (B,N,C,Ho) of one bi-dimensional graph diffusion; ``Tc`` from ``cheby_dense``.

    ``pad``: the last ``pad`` columns of X's feature axis are zero padding added by the caller
    (``concat2(..., pad)`` / ``gru_gates(..., pad)``) to make rows 16-byte aligned; W keeps its
    reference shape (Ks*Kc*(L-pad), Ho).
    """
    if X.dim() != 4:
        raise ValueError(f'BDG_Dif input must be (B,N,C,L), got {tuple(X.shape)}')
    B, N, C, L = X.shape
    Kc = Tc.shape[0]
    if N != op.n:
        raise ValueError(f'X has {N} nodes, the spatial graph {op.n}')
    if Tc.shape[1] != C:
        raise ValueError(f'X has {C} categories, the category graph {Tc.shape[1]}')
    if W.shape[0] != Ks * Kc * (L - pad):
        raise ValueError(f'W has {W.shape[0]} rows, expected Ks*Kc*L = {Ks * Kc * (L - pad)}')
    if X.dtype == torch.bfloat16:
        # bf16 feature rows (BASELINE configuration 5): fixed graphs only, shapes of the bf16 matrix-core kernels, no fallback
        if Tc.requires_grad or op.fwd_val.requires_grad:
            which = ' and '.join(n for n, t in (('Tc', Tc), ('op.fwd_val', op.fwd_val)) if t.requires_grad)
            raise ValueError(f'BDG_Dif on bfloat16 features needs fixed graphs (no gradient for Gs / Gc): {which} requires grad')
        if not kernels().node_bf16_supported(Ks, Kc, C, L, W.shape[1]):
            raise ValueError(f'BDG_Dif on bfloat16 features: Ks=Kc<=3, C in (32, 64), L in (16, 32), Ho in (16, 32); got Ks={Ks} Kc={Kc} C={C} L={L} Ho={W.shape[1]}')
    return _BdgDif.apply(X, W, b, Tc, op.fwd_val, op, Ks)


# ----------------------------------------------------------------------------- GRU gate math
class _GruGates(Function):
    @staticmethod
    def forward(ctx, G, Xt, H, pad):
        G, Xt, H = _c(G), _c(Xt), _c(H)
        U = torch.empty_like(H)
        Rg = torch.empty_like(H)
        CandIn = H.new_empty(H.shape[:-1] + (Xt.shape[-1] + H.shape[-1] + pad,))
        kernels().gru_gates_fwd(G, Xt, H, U, Rg, CandIn)
        ctx.save_for_backward(H, U, Rg)
        ctx.cin = Xt.shape[-1]
        ctx.pad = pad
        ctx.xshape = Xt.shape
        return U, CandIn

    @staticmethod
    @once_differentiable
    def backward(ctx, dU, dCandIn):
        H, U, Rg = ctx.saved_tensors
        dU = torch.zeros_like(U) if dU is None else _c(dU)
        dCandIn = H.new_zeros(H.shape[:-1] + (ctx.cin + H.shape[-1] + ctx.pad,)) if dCandIn is None else _c(dCandIn)
        dG = H.new_empty(H.shape[:-1] + (2 * H.shape[-1],))
        dXt = H.new_empty(ctx.xshape)
        dH = torch.empty_like(H)
        kernels().gru_gates_bwd(dCandIn, dU, H, U, Rg, dG, dXt, dH)
        return dG, dXt, dH, None


def gru_gates(G, Xt, H, pad: int = 0):
    """(update, cat[Xt, reset*H, zeros(pad)]) from the gate pre-activations G (.., 2h)."""
    return _GruGates.apply(G, Xt, H, pad)


class _GruBlend(Function):
    @staticmethod
    def forward(ctx, Cpre, U, H):
        Cpre, U, H = _c(Cpre), _c(U), _c(H)
        Cand = torch.empty_like(H)
        Hnew = torch.empty_like(H)
        kernels().gru_blend_fwd(Cpre, U, H, Cand, Hnew)
        ctx.save_for_backward(U, H, Cand)
        return Hnew

    @staticmethod
    @once_differentiable
    def backward(ctx, dHnew):
        U, H, Cand = ctx.saved_tensors
        dCpre, dU, dH = torch.empty_like(H), torch.empty_like(H), torch.empty_like(H)
        kernels().gru_blend_bwd(_c(dHnew), U, H, Cand, dCpre, dU, dH)
        return dCpre, dU, dH


def gru_blend(Cpre, U, H):
    """(1-U)*H + U*tanh(Cpre)."""
    return _GruBlend.apply(Cpre, U, H)


class _Concat2(Function):
    @staticmethod
    def forward(ctx, A, Bm, pad):
        A, Bm = _c(A), _c(Bm)
        out = A.new_empty(A.shape[:-1] + (A.shape[-1] + Bm.shape[-1] + pad,))
        kernels().concat2(A, Bm, out)
        ctx.shapes = (A.shape, Bm.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        sa, sb = ctx.shapes
        dA, dB = d.new_empty(sa), d.new_empty(sb)
        kernels().split2(_c(d), dA, dB)
        return dA, dB, None


def concat2(A, Bm, pad: int = 0):
    """cat([A, B, zeros(pad)], dim=-1) for tensors that agree on every leading dimension."""
    if A.shape[:-1] != Bm.shape[:-1]:
        raise ValueError(f'concat2: leading shapes differ: {tuple(A.shape)} vs {tuple(Bm.shape)}')
    return _Concat2.apply(A, Bm, pad)


# ----------------------------------------------------------------------------- output head
class _Head(Function):
    @staticmethod
    def forward(ctx, H, w, b):
        H, w, b = _c(H), _c(w), _c(b)
        y = H.new_empty(H.shape[:-1], dtype=torch.float32)          # bf16 state rows: the prediction stays fp32
        kernels().head_fwd(H, w, b, y)
        ctx.save_for_backward(H, w, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        H, w, y = ctx.saved_tensors
        dH = torch.empty_like(H)
        dwb = w.new_empty(w.numel() + 1)
        kernels().head_bwd(H, w, y, _c(dy), dH, dwb)
        return dH, dwb[:-1], dwb[-1:]


def head(H: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """sigmoid(<H[..., :], w> + b): the reference's Linear(h, h/2) -> Linear(h/2, 1) -> sigmoid with the two
    layers folded by the caller (no nonlinearity between them); returns H's shape without the last axis."""
    if w.shape != (H.shape[-1],) or b.shape != (1,):
        raise ValueError(f'head: w {tuple(w.shape)} / b {tuple(b.shape)} do not match feature width {H.shape[-1]}')
    return _Head.apply(H, w, b)


# ----------------------------------------------------------------------------- whole STC_Cell
class _StcCell(Function):
    """One STC_Cell step (reference STC_GNN.py:65-79) as a single autograd node.

    Same kernels as the composed path (concat2 -> bdg -> gru_gates -> bdg -> gru_blend); what it adds is
    the backward bookkeeping: the three gradients owed to H (blend, reset gate, concat) and the two owed
    to Xt are summed inside the gate / split kernels instead of by separate autograd accumulation passes,
    and nothing but the slabs the backward really needs is kept (Z of both convolutions, U, R, Cand, H).
    """

    @staticmethod
    def forward(ctx, Xt, H, Wg, bg, Wc, bc, Tc, fwd_val, op: SpatialOperand, Ks: int):
        k = kernels()
        Xt, H, Wg, Wc, Tc, fwd_val = _c(Xt), _c(H), _c(Wg), _c(Wc), _c(Tc), _c(fwd_val)
        bg, bc = _cn(bg), _cn(bc)
        cin, h = Xt.shape[-1], H.shape[-1]
        pad = -(cin + h) % 4                      # rows padded to 16 bytes (17 -> 20); W keeps its reference shape
        lead = H.shape[:-1]
        XH = H.new_empty(lead + (cin + h + pad,))
        k.concat2(Xt, H, XH)
        U, Rg, CandIn = torch.empty_like(H), torch.empty_like(H), torch.empty_like(XH)
        Cand, Hnew = torch.empty_like(H), torch.empty_like(H)
        B, N, C, L = XH.shape
        pack = _cell_pack(k, B * N, C, Ks, Tc.shape[0], L, h)
        if pack:
            # gate math in the node kernels' epilogues: the pre-activations never go to HBM (few categories: `pack` nodes per row tile)
            rows = lambda ts: [t.view(B * N // pack, pack * C, t.shape[-1]) for t in ts]
            Tcp = Tc if pack == 1 else _block_diag(Tc, pack)
            Zg = _spatial_slabs(XH, fwd_val, op, Ks)
            k.cell_gates_fwd(rows(Zg), Tcp, Wg, bg, *rows((H, U, Rg, CandIn)))
            Zc = _spatial_slabs(CandIn, fwd_val, op, Ks)
            k.cell_blend_fwd(rows(Zc), Tcp, Wc, bc, *rows((U, H, Cand, Hnew)))
        else:
            G, Zg = _bdg_forward(XH, Wg, bg, Tc, fwd_val, op, Ks)
            k.gru_gates_fwd(G, Xt, H, U, Rg, CandIn)
            del G
            Cpre, Zc = _bdg_forward(CandIn, Wc, bc, Tc, fwd_val, op, Ks)
            k.gru_blend_fwd(Cpre, U, H, Cand, Hnew)
        ctx.save_for_backward(H, U, Rg, Cand, Wg, Wc, Tc, *Zg, *Zc)
        ctx.op, ctx.Ks, ctx.cin = op, Ks, cin
        ctx.bias = (bg is not None, bc is not None)
        return Hnew

    @staticmethod
    @once_differentiable
    def backward(ctx, dHnew):
        k = kernels()
        H, U, Rg, Cand, Wg, Wc, Tc, *Z = ctx.saved_tensors
        Ks, op, cin = ctx.Ks, ctx.op, ctx.cin
        Zg, Zc = Z[:Ks], Z[Ks:]
        need_Xt, need_H = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_Tc, need_val = ctx.needs_input_grad[6], ctx.needs_input_grad[7]
        B, N, C, L = Zc[0].shape
        v3 = lambda t: t.view(B, N, C * L)
        bwd = (op.bwd_rowptr, op.bwd_colidx, op.bwd_val, op.bwd_plan)
        # the gate backward can run as the prologue of the gates convolution's node backward (dG is never stored); it then
        # also takes over two pure data movements: the state's (1 - U) share of the blend (read from dHnew in place) and
        # dXt = d[x part] (left in place, added by the final split straight from the candidate gradient's rows)
        pack = 0 if (need_Tc or need_val) else _cell_pack(k, B * N, C, Ks, Tc.shape[0], L, H.shape[-1])
        pro = pack > 0
        dHnew = _c(dHnew)
        dH = torch.empty_like(H)
        dXt = H.new_empty(H.shape[:-1] + (cin,))
        if pro:         # the blend backward (dCpre, dU, the state share) is formed inside the two node backward kernels
            dCpre = dU = dG = None
            g, dWc, dbc, dTc, dval = _bdg_backward_slabs(None, Zc, Wc, Tc, op, Ks, ctx.bias[1], False, False, cand=(dHnew, U, Cand), pack=pack)
        else:
            dCpre, dU = torch.empty_like(H), torch.empty_like(H)
            k.gru_blend_bwd(dHnew, U, H, Cand, dCpre, dU, dH)                     # dH = dHnew * (1 - U)
            dG = H.new_empty(H.shape[:-1] + (2 * H.shape[-1],))
            # candidate convolution: d[Xt | R*H] = g0 + Gs.g1, consumed by the gate backward
            g, dWc, dbc, dTc, dval = _bdg_backward_slabs(dCpre, Zc, Wc, Tc, op, Ks, ctx.bias[1], need_Tc, need_val)
        gates_pro, dci = None, g[0]
        if Ks > 1:
            k.csr_spmm(*bwd[:3], N, N, v3(g[1]), v3(g[0]), v3(g[0]), 1.0, 1.0, plan=op.bwd_plan)
        if pro:
            gates_pro = (dci, Cand, H, U, Rg, dHnew, dH)
        else:
            k.gru_gates_bwd(dci, dU, H, U, Rg, dG, dXt, dH, dH_in=dH)
        # gates convolution: d[Xt | H] = g0 + Gs.g1, split and added to what Xt and H are already owed
        g, dWg, dbg, dTc2, dval2 = _bdg_backward_slabs(dG, Zg, Wg, Tc, op, Ks, ctx.bias[0], need_Tc, need_val, gates=gates_pro, pack=max(1, pack))
        if need_Xt or need_H:
            if Ks > 1:
                k.csr_spmm(*bwd[:3], N, N, v3(g[1]), v3(g[0]), v3(g[0]), 1.0, 1.0, plan=op.bwd_plan)
            if pro:
                k.split2(g[0], dXt, dH, addA=dci, addB=dH, addA_ld=L)             # + d[x part] of the candidate, read in place
            else:
                k.split2(g[0], dXt, dH, addA=dXt, addB=dH)                        # + the concat's share, in place
        if need_Tc:
            dTc = dTc + dTc2
        if need_val:
            dval = dval + dval2
        return (dXt if need_Xt else None), (dH if need_H else None), dWg, dbg, dWc, dbc, dTc, dval, None, None


def stc_cell(Xt, H, op: SpatialOperand, Tc, Wg, bg, Wc, bc, Ks: int):
    """Ht of one STC_Cell step; gates / candidate BDG_Dif parameters in the reference's shapes."""
    if Xt.dim() != 4 or H.dim() != 4 or Xt.shape[:-1] != H.shape[:-1]:
        raise ValueError(f'stc_cell: Xt {tuple(Xt.shape)} and H {tuple(H.shape)} must be (B,N,C,*) with equal leading shape')
    B, N, C, h = H.shape
    L = Xt.shape[-1] + h
    Kc = Tc.shape[0]
    if N != op.n or Tc.shape[1] != C:
        raise ValueError(f'stc_cell: graphs are for N={op.n}, C={Tc.shape[1]}; got N={N}, C={C}')
    if Wg.shape != (Ks * Kc * L, 2 * h) or Wc.shape != (Ks * Kc * L, h):
        raise ValueError(f'stc_cell: W shapes {tuple(Wg.shape)}, {tuple(Wc.shape)} do not match Ks*Kc*L={Ks * Kc * L}, h={h}')
    return _StcCell.apply(Xt, H, Wg, bg, Wc, bc, Tc, op.fwd_val, op, Ks)


# ----------------------------------------------------------------------------- a whole schedule of cells as ONE autograd node
# Which kernels the cell-graph executor uses.  Module constants, looked up at every call (tests flip them to reach the forms other shapes still
# take -- C = 64 runs the two-launch backward, K = 3 the order-3 planar cells, other widths the interleaved rows); not environment switches.
_CELL_GRAPH = True       # encoder + decoder as ONE autograd node (False: one node per cell, ``_StcCell``)
_PLANAR = True           # cells with 16 + 16-column inputs read them as two planes (no concat, shared S.state)
_POST_AGG = True         # candidate convolution as Y = A + S.Bm (narrow SpMM after the node kernel)
_SMALL = True            # small graphs (N*C rows per sample fit the caches, C <= 16): one launch per cell step and direction
_RING2 = True            # state gradient + transpose aggregation of dY in one launch where the graph has a two-ring plan (no dY plane)
_RING2_FWD = True        # ... and the forward's blend + aggregation of the new state (stc_ring2_blend_f32)
_DTC = True              # a learned category graph on a fixed sparse spatial graph inside this executor: dT_c from the planar cells (``learn_Tc=``; False: one node per cell)
_DVAL = True             # a learned spatial graph on a sparse pattern inside this executor, where the caller asked (``op.sampled_grad``): its value gradient from the planar cells (False: one node per cell)
_FIRST_STEP = True       # cells on the zero initial state (a layer's first time step) in their first-step forms: no H, S.H, R planes, no dH, dS.H
_SUM_GATHERS, _CHAIN_FIRST_ADD = 2, 2     # kernel limits, not switches: planes that stc_spmm_sum_* / the two-ring launches gather through S (X, X2); first-ring addends of stc_ring2_chain_f32

_ZEROS = {}              # (device, dtype) -> one zero, never written: what ``zero_state`` views


def _first_step_kernels(k, dtype, C: int, h: int) -> bool:
    """The ONE test of whether kernel set ``k`` runs first-step forms on planes of ``dtype``: the switch, fp32 planes, the capability and the
    library's own shape predicate.  The model (``first_step_route``) and the executor (``_ForwardPass``) both ask here."""
    return bool(_FIRST_STEP and dtype == torch.float32 and getattr(k, 'first_step_cells', False) and k.cell_first_supported(C, h))


def first_step_route(op: SpatialOperand, Tc, Ks: int, C: int, h: int, x_widths, dtype=torch.float32, learn_Tc: bool = False) -> bool:
    """Whether ``stc_cell_graph`` runs the PLANAR_ONE_BWD cells of this problem whose state is a zero initial state in their first-step forms
    (fp32 planes, order 2, a kernel set with ``first_step_cells``, not the few-category executor): the caller then passes ``zero_state`` views
    instead of planes of zeros.  Never while the executor differentiates ``Tc`` (``learn_Tc``) or the spatial values (``_dval_route``): its cells are PLANAR, which has no such form."""
    k = kernels()
    if _learns_tc(learn_Tc, Tc) or _dval_route(k, op, Tc, Ks, C, h, x_widths, dtype):
        return False
    return Ks == 2 and _first_step_kernels(k, dtype, C, h) and not (_SMALL and small_graph_supported(k, op, Tc, Ks, C, h, x_widths, dtype))


def zero_state(ref: torch.Tensor, shape, dtype=None) -> torch.Tensor:
    """A zero initial state as a SHAPE: a stride-0 view of one cached zero on ``ref``'s device -- no plane is allocated or filled.  The executor
    recognises it (``_is_zero_state``), runs its consumers in their first-step forms and builds the plane only for a launch that reads one."""
    key = (ref.device, dtype or ref.dtype)
    if key not in _ZEROS:
        _ZEROS[key] = torch.zeros((), device=key[0], dtype=key[1])
    return _ZEROS[key].expand(*shape)


def _is_zero_state(t: torch.Tensor) -> bool:
    z = _ZEROS.get((t.device, t.dtype))
    return z is not None and t.dim() == 4 and not any(t.stride()) and t.untyped_storage().data_ptr() == z.untyped_storage().data_ptr()


def _learns_tc(learn_Tc: bool, Tc) -> bool:
    """Whether a call asks the general executor for the category graph's gradient: the caller's word, grad mode, a ``Tc`` that requires grad."""
    return bool(learn_Tc and torch.is_grad_enabled() and Tc.requires_grad)


def _dval_route(k, op: SpatialOperand, Tc, Ks: int, C: int, h: int, x_widths, dtype) -> bool:
    """Whether the general executor forms the value gradient of a learned spatial graph for this problem: the switch, the caller's word
    (``op.sampled_grad``: ``STCGNN(csr_cells='fused')``), values that require grad in grad mode, a sparse pattern (the full pattern is the dense
    learned graph), fp32 planes, Ks = Kc = 2, hidden 16, C in {32, 64}, every input 16 or 1..4 columns wide, a kernel set with
    ``cell_graph_vals``, every cell in ``_Form.PLANAR`` (the two-launch backward, in which dS.X, dS.H and dY exist as planes)."""
    widths = sorted(set(x_widths))
    return bool(_DVAL and op.sampled_grad and torch.is_grad_enabled() and op.fwd_val.requires_grad and op.nnz != op.n * op.n
                and dtype == torch.float32 and Ks == 2 and Tc.shape[0] == 2 and h == 16 and C in (32, 64)
                and all(w == h or 1 <= w <= 4 for w in widths) and getattr(k, 'cell_graph_vals', False)
                and all(f is _Form.PLANAR for f in _cell_forms(k, Ks, 2, C, h, widths, False, learn_Tc=True)))


def _dtc_route(k, op: SpatialOperand, Tc, Ks: int, C: int, h: int, x_widths, dtype) -> bool:
    """Whether the general executor can differentiate ``Tc`` for this problem (``stc_cell_graph(learn_Tc=True)``): the switch, fp32 planes,
    order 2, a kernel set with the planar cells' dT_c kernels that takes every input width, every cell in ``_Form.PLANAR`` (the two-launch
    backward, in which dY, dBm and dRH exist), a spatial graph that needs no gradient -- or whose value gradient the same backward forms
    (``_dval_route``)."""
    widths = sorted(set(x_widths))
    return bool(_DTC and dtype == torch.float32 and Ks == 2 and Tc.shape[0] == 2 and getattr(k, 'cell_dtc_planar', False)
                and (not op.fwd_val.requires_grad or _dval_route(k, op, Tc, Ks, C, h, x_widths, dtype)) and all(k.cell_dtc_planar_supported(C, w, h) for w in widths)
                and all(f is _Form.PLANAR for f in _cell_forms(k, Ks, 2, C, h, widths, False, learn_Tc=True)))


def cell_graph_supported(op: SpatialOperand, Tc, Ks: int, C: int, h: int, x_widths, dtype=torch.float32, learn_Tc: bool = False) -> bool:
    """Whether ``stc_cell_graph`` can run a schedule: matrix-core cell kernels for every row width that occurs, hidden 16,
    graphs that need no gradient (``csr-fixed`` mode).  ``dtype`` = storage type of the state tensors: bfloat16 runs the
    all-planar bf16 kernel set (Ks = Kc = 2; inputs 16 or 1..4 columns wide).  ``learn_Tc``: the caller wants the gradient of a ``Tc`` that
    requires grad from the general executor (``graph_mode='csr-category-learned'``); the answer is then ``_dtc_route``'s.  Spatial values that
    require grad are taken only on an operand with ``sampled_grad`` and only where ``_dval_route`` holds."""
    if not _CELL_GRAPH or h != 16:
        return False
    k = kernels()
    if _SMALL and small_graph_supported(k, op, Tc, Ks, C, h, x_widths, dtype):
        return True                                                   # small graphs, fixed or learned: one launch per cell step (stc_hip/small.py)
    if _learns_tc(learn_Tc, Tc):
        return _dtc_route(k, op, Tc, Ks, C, h, x_widths, dtype)
    if not Tc.requires_grad and _dval_route(k, op, Tc, Ks, C, h, x_widths, dtype):
        return True                                                   # a learned sparse spatial graph alone (``csr_cells='fused'``, frozen category generator)
    if Tc.requires_grad or op.fwd_val.requires_grad:
        return False
    if dtype == torch.bfloat16:
        return (_PLANAR and _POST_AGG and Ks == 2 and Tc.shape[0] == 2 and k.bf16.cell_planar_supported(Ks, 2, C, h)
                and all(w == h or 1 <= w <= 4 for w in x_widths))
    return all(k.cell_fused_supported(Ks, Tc.shape[0], C, w + h + (-(w + h)) % 4, h) for w in set(x_widths))


def _amplification(op: SpatialOperand, Ks: int) -> float:
    """What one BDG_Dif of order Ks can amplify a state by: the graph's largest absolute row sum to the power Ks - 1 (T_2(S) = 2 S^2 - I has
    row sums of up to 2 r^2 + 1; order 3 on a graph with row sums of 8 puts the reference's own fp32 noise at 3.5e-4 on the prediction)."""
    return float(op.row_sum_bound) ** max(1, Ks - 1)


class _Form(enum.Enum):
    """The form one cell of ``_StcCellGraph`` runs in, chosen once per cell before the forward's launches (``_cell_forms``).  Every form
    saves (H, U, R, Cand) for backward and then, in this order:"""
    PLANAR3 = 'order-3 planar'          # Zx[0..2], Zh[1..2], Zr[0..2]: gates and slab-planar candidate on three Chebyshev planes per side
    PLANAR_ONE_BWD = 'planar, one-launch backward'     # X, S.X, S.H: the backward re-forms R*H, which is never stored
    PLANAR = 'planar'                   # X, S.X, S.H, R*H[, Bm]: node_post backward of the candidate, then the planar gates backward (Bm: only while the spatial values are learned)
    ROWS_POST = 'rows, post-aggregation'   # Zg[0..Ks-1], CandIn: interleaved [Xt | H | 0] rows, candidate as Y = A + S.Bm (Ks = 2)
    ROWS_SLABS = 'rows, slabs'          # Zg[0..Ks-1], Zc[0..Ks-1]: interleaved rows, candidate convolution on its Chebyshev slabs

    def saved(self, Ks: int, vals: bool = False) -> int:            # vals: the value gradient is formed (``_dval_route``) -- PLANAR also keeps Bm
        return 4 + {'PLANAR3': 8, 'PLANAR_ONE_BWD': 3, 'PLANAR': 5 if vals else 4, 'ROWS_POST': Ks + 1, 'ROWS_SLABS': 2 * Ks}[self.name]

    @property
    def planar(self) -> bool:
        return self not in (_Form.ROWS_POST, _Form.ROWS_SLABS)


# form -> the methods of (``_ForwardPass``, ``_BackwardPass``) that hold its launches
_FORM_METHODS = {_Form.PLANAR3: ('planar3', 'planar3'), _Form.PLANAR_ONE_BWD: ('planar', 'planar_one_bwd'), _Form.PLANAR: ('planar', 'planar'),
                 _Form.ROWS_POST: ('rows_cell', 'rows_cell'), _Form.ROWS_SLABS: ('rows_cell', 'rows_cell')}

def _cell_forms(k, Ks: int, Kc: int, C: int, h: int, cin, bf16: bool, learn_Tc: bool = False):
    """The ``_Form`` of every cell from its input width ``cin[j]``: planar where the planar kernels take the shape -- 16 + 16 columns, or
    (layer 0) a narrow input plane of 1..4 columns beside the 16 state columns -- else interleaved rows.  ``learn_Tc``: the backward forms dT_c,
    from planes that only the two-launch backward holds -- PLANAR where it would be PLANAR_ONE_BWD."""
    planar2 = (_PLANAR and _POST_AGG and Ks == 2 and k.cell_planar_supported(Ks, Kc, C, h)
               and k.node_post_supported(Ks, Kc, C, 2 * h, h))
    post20 = bool(planar2) and k.node_post_supported(Ks, Kc, C, 20, h)
    # order 3 (BASELINE configuration 4): planar cells on the three Chebyshev planes of each side, candidate in slab-planar form
    planar3 = bool(_PLANAR and not bf16 and Ks == 3 and Kc == 3 and k.cell_planar_k_supported(Ks, C, h))
    forms = []
    for w in cin:
        if planar3 and (w == h or 1 <= w <= 4):
            forms.append(_Form.PLANAR3)
        elif planar2 and (w == h or (post20 and 1 <= w <= 4)):
            # the one-launch backward (stc_cell_bwd_planar_f32) forms R*H itself
            one_bwd = k.cell_bwd_planar_supported(C, h, w) if bf16 else k.cell_bwd_planar_supported(C, h)
            forms.append(_Form.PLANAR_ONE_BWD if one_bwd and not learn_Tc else _Form.PLANAR)
        else:                                                       # (Ks = 1 has no S.Bm term: slabs)
            post = Ks > 1 and _POST_AGG and k.node_post_supported(Ks, Kc, C, w + h + (-(w + h)) % 4, h)
            forms.append(_Form.ROWS_POST if post else _Form.ROWS_SLABS)
    return forms


class _Pass:
    """What the cells of one pass of ``_StcCellGraph`` share: kernel set, graph, shapes, forms and the activation-maximum slots (fp16 x 2
    operand format: every planar forward launch leaves the maxima of its input planes in a row of ``zmax_all``; the matching backward launch
    scales the activation operands of its dW products by them -- _lib.act_amax_buffer)."""

    def __init__(self, k, op: SpatialOperand, Ks: int, Tc, schedule, cin, forms, dims, bf16: bool, zmax_all, graph):
        self.k, self.op, self.Ks, self.Tc, self.schedule, self.cin, self.forms = k, op, Ks, Tc, schedule, cin, forms
        (self.B, self.N, self.C), self.h, self.bf16, self.zmax_all = dims, 16, bf16, zmax_all
        self.graph = graph                                          # (rowptr, colidx, val, plan) of S (forward) or S^T (backward)

    def spmm(self, X, Y0=None, Y=None, alpha=1.0, beta=0.0):        # Y = alpha S.X + beta Y0 on (B, N, C, w) tensors (S^T in the backward)
        Y = torch.empty_like(X) if Y is None else Y
        v3 = lambda t: None if t is None else t.view(self.B, self.N, -1)
        self.k.csr_spmm(*self.graph[:3], self.N, self.N, v3(X), v3(Y0), v3(Y), alpha, beta, plan=self.graph[3])
        return Y

    def rows(self, ts):
        return [None if t is None else t.view(self.B * self.N, self.C, t.shape[-1]) for t in ts]

    def act_slots(self, j, which=0):                                # which: 0 = the gates convolution's planes, 1 = the candidate's (order 3)
        return {} if self.zmax_all is None else dict(act_amax=self.zmax_all[j, which])


class _ForwardPass(_Pass):
    """... and, in the forward, the new states, the input rows of the interleaved cells and the aggregations of every source tensor (formed
    once for all the planar cells that consume it)."""

    def __init__(self, k, op: SpatialOperand, Ks: int, Tc, fwd_val, schedule, ext, cin, forms, bf16: bool, forward_only: bool = False, keep_bm: bool = False):
        # (forward only: no backward will read the maxima -- no buffer, and the launches get no slots to fill)
        zmax_all = k.act_amax_buffer(ext[0], len(schedule), 2, 2 * Ks) if (not forward_only and not bf16 and any(f.planar for f in forms)) else None   # (one zero fill)
        super().__init__(k, op, Ks, Tc, schedule, cin, forms, ext[0].shape[:3], bf16, zmax_all, (op.fwd_rowptr, op.fwd_colidx, fwd_val, op.fwd_plan))
        self.fwd_val, self.ext = fwd_val, ext
        self.keep_bm = keep_bm                                      # the backward forms the spatial values' gradient: PLANAR cells save the candidate's Bm plane
        self.state = [None] * len(schedule)                         # plain (B,N,C,h) new state of every cell
        self.XH, self.agg = {}, {}
        self.consumers = [[] for _ in schedule]
        for j, (_, x, hs) in enumerate(schedule):
            for src, role in ((hs, 'h'), (x, 'x')):
                if src[0] == 'cell':
                    self.consumers[src[1]].append((j, role))
        # two aggregations in one launch where the graph has a two-ring plan (stc_ring2_chain_f32 / stc_ring2_blend_f32; fp32 planes only)
        self.ring2 = _RING2_FWD and not bf16 and op.fwd_ring2 is not None and k.ring2_fits(self.B, self.N, self.C, self.h)
        # forward only, on a kernel set that takes None for them: the planes only a backward reads (R, Cand, R*H at order 2) are not stored
        self.lean = forward_only and bool(getattr(k, 'optional_gate_stores', False))
        # cells whose state is a zero initial state (``zero_state``), in the first-step forms where the cell's form and the kernel set have them
        zero = {('ext', i) for i, t in enumerate(ext) if _is_zero_state(t)}
        can = _first_step_kernels(k, ext[0].dtype, self.C, self.h)
        self.first = [can and hs in zero and f is _Form.PLANAR_ONE_BWD for (_, _, hs), f in zip(schedule, forms)]

    def source(self, src):
        if src[0] != 'ext':
            return self.state[src[1]]
        t = self.ext[src[1]]
        if not t.is_contiguous() and _is_zero_state(t):             # a zero initial state that some launch reads after all: its plane, at first touch
            t = self.ext[src[1]] = t.new_zeros(t.shape)
        return t

    def plane(self):                                                # an uninitialised state-sized plane
        return self.ext[0].new_empty(self.B, self.N, self.C, self.h)

    def rows_of(self, j):                                           # input rows of an interleaved cell, allocated at first touch
        if j not in self.XH:
            w = self.cin[j]
            self.XH[j] = self.ext[0].new_empty(self.B, self.N, self.C, w + self.h + (-(w + self.h)) % 4)
        return self.XH[j]

    def aggregated(self, src, planes=False):                        # S.source -- order 3: its Chebyshev planes -- once per source tensor,
        if src not in self.agg:                                     # shared by every cell that consumes it
            self.agg[src] = self.cheb_planes(self.source(src)) if planes else self.spmm(self.source(src))
        return self.agg[src]

    def cheb_planes(self, t):                                       # [t, S.t, 2 S.(S.t) - t]: the feature-side recurrence, order 3
        if not (self.ring2 and t.shape[-1] == self.h):
            s1 = self.spmm(t)
            return [t, s1, self.spmm(s1, t, alpha=2.0, beta=-1.0)]
        # both aggregations in one launch: S.t for a patch's first ring is formed in LDS and aggregated from there (stc_ring2_chain_f32)
        s1, s2 = torch.empty_like(t), torch.empty_like(t)
        self.k.ring2_chain(*self.graph[:3], self.op.fwd_ring2, t, None, 1.0, [], s1, 2.0, [(t, -1.0)], s2)
        return [t, s1, s2]

    def copy_plan(self, j):
        """Where else cell j's new state goes: straight into the input rows of the INTERLEAVED cells that consume it -- (copies, side) for the
        blend launch's epilogue, (late_copies, late_rows) for torch after it."""
        B, N, C, h, cin, schedule = self.B, self.N, self.C, self.h, self.cin, self.schedule
        copies, side, late_copies, late_rows = [], None, [], []
        for (d, role) in self.consumers[j]:
            if self.forms[d].planar:
                continue                                            # planar consumers read the state tensor itself
            Xd = self.rows_of(d)
            view = Xd.view(B * N, C, Xd.shape[-1])
            if role == 'x':
                copies.append((view, 0))
            elif schedule[d][1][0] == 'ext':                        # H part + the consumer's external X part and pad columns
                if side is None:
                    copies.insert(0, (view, cin[d]))
                    side = self.ext[schedule[d][1][1]].view(B * N, C, cin[d])
                else:
                    late_rows.append(d)
            elif Xd.shape[-1] > cin[d] + h:
                late_rows.append(d)                                 # pad columns to zero: not a case the kernel handles
            else:
                copies.append((view, cin[d]))
        first = 1 if side is not None else 0
        while len(copies) > 2:                                      # the kernel takes two destinations; the rest by torch
            late_copies.append(copies.pop(len(copies) - 1 if len(copies) - 1 >= first else first))
        return copies, side, late_copies, late_rows

    def finish(self, j, Hnew, late_copies, late_rows):
        for buf, off in late_copies:
            buf[..., off:off + self.h].copy_(Hnew.view(self.B * self.N, self.C, self.h))
        for d in late_rows:
            Xd, xs, w = self.rows_of(d), self.schedule[d][1], self.cin[d]
            if xs[0] == 'ext':
                self.k.concat2(self.ext[xs[1]], Hnew, Xd)
            else:
                Xd[..., w:w + self.h].copy_(Hnew)
                Xd[..., w + self.h:].zero_()
        self.state[j] = Hnew

    # ---- one function per form: the launches of cell j; returns what it saves after (H, U, R, Cand)
    def planar3(self, j, Wg, bg, Wc, bc, Hprev, U, Rg, Cand, Hnew, copies, side):
        k, rows, (_, x, hs) = self.k, self.rows, self.schedule[j]
        Zx, Zh, RH = self.aggregated(x, planes=True), self.aggregated(hs, planes=True), torch.empty_like(Hprev)
        k.cell_gates_fwd_planar_k(rows(Zx), rows(Zh), self.Tc, Wg, bg, *rows((U, Rg, RH)), **self.act_slots(j, 0))
        Zr = self.cheb_planes(RH)                                   # the candidate's H side: T_n(S) of R*H (its X side is Zx again)
        k.cell_cand_fwd_planar_k(rows(Zx), rows(Zr), self.Tc, Wc, bc, *rows((U, Hprev, Cand, Hnew)), **self.act_slots(j, 1))
        return [*Zx, *Zh[1:], *Zr]

    def planar(self, j, Wg, bg, Wc, bc, Hprev, U, Rg, Cand, Hnew, copies, side):
        """PLANAR_ONE_BWD and PLANAR: the candidate's projection rides in the gates launch; only PLANAR stores the R*H plane."""
        k, op, rows, (_, x, hs) = self.k, self.op, self.rows, self.schedule[j]
        first = Hprev is None                                       # the state is the zero initial state: the first-step forms (``cell``)
        Xp, SXp, SHp = self.source(x), self.aggregated(x), None if first else self.aggregated(hs)
        RH = None if (self.forms[j] is _Form.PLANAR_ONE_BWD or self.lean) else self.plane()
        A, Bm = self.plane(), self.plane()
        if first:                                                   # no H, S.H operands; the reset gate only ever multiplies H = 0
            k.cell_gates_fwd_first(*rows((Xp, SXp)), self.Tc, Wg, bg, *rows((U,)), (Wc, bc, *rows((A, Bm))), **self.act_slots(j))
        else:
            k.cell_gates_fwd_planar(*rows((Xp, Hprev, SXp, SHp)), self.Tc, Wg, bg, *rows((U, Rg, RH)), post=(Wc, bc, *rows((A, Bm))), **self.act_slots(j))
        # the blend and the aggregation of the new state in one launch where the graph has a two-ring plan and some planar cell will
        # ask for S.Hnew (stc_ring2_blend_f32: the new state is summed out of LDS instead of being read back by a launch of its own; on ring-bounded
        # clusters it measured 792 us against 548 + 203 for the two launches: tiles only)
        if (self.ring2 and not op.ring2_clusters and not copies and side is None
                and any(self.forms[d].planar for d, _ in self.consumers[j])):
            SHn = self.plane()
            if first:
                k.ring2_blend_first(*self.graph[:3], op.fwd_ring2, Bm, A, U, Cand, Hnew, SHn)
            else:
                k.ring2_blend(*self.graph[:3], op.fwd_ring2, Bm, A, U, Hprev, Cand, Hnew, SHn)
            self.agg[('cell', j)] = SHn
        else:                                                       # (the row-blocked blend reads a plane of zeros: built here only)
            k.spmm_blend_fwd(*self.graph, Bm, A, U, self.source(hs) if first else Hprev, Cand, Hnew, copies=copies, side=side)
        return [Xp, SXp, SHp] + ([] if RH is None else [RH]) + ([Bm] if self.keep_bm else [])

    def rows_cell(self, j, Wg, bg, Wc, bc, Hprev, U, Rg, Cand, Hnew, copies, side):
        """ROWS_POST and ROWS_SLABS: gates convolution on the Chebyshev slabs of the [Xt | H | 0] rows, gate math in its epilogue."""
        k, op, rows, Tc, (_, x, hs) = self.k, self.op, self.rows, self.Tc, self.schedule[j]
        Xj = self.rows_of(j)
        w = self.cin[j]
        if x[0] == 'ext' and hs[0] == 'ext':
            k.concat2(self.ext[x[1]], Hprev, Xj)
        elif x[0] == 'cell' and hs[0] == 'ext':                     # X part came from its producer; complete the row
            Xj[..., w:w + self.h].copy_(Hprev)
            if Xj.shape[-1] > w + self.h:
                Xj[..., w + self.h:].zero_()
        # (H part from a cell: its producer also wrote an external X part and the pad columns, see copy_plan)
        CandIn = torch.empty_like(Xj)
        Zg = _spatial_slabs(Xj, self.fwd_val, op, self.Ks)
        k.cell_gates_fwd(rows(Zg), Tc, Wg, bg, *rows((Hprev, U, Rg, CandIn)))
        if self.forms[j] is _Form.ROWS_POST:
            # candidate convolution as Y = A + S.Bm: project first, aggregate C*h-float rows, blend in the SpMM's epilogue
            A, Bm = torch.empty_like(Hprev), torch.empty_like(Hprev)
            k.node_post_fwd(*rows((CandIn,)), Tc, Wc, bc, *rows((A, Bm)))
            k.spmm_blend_fwd(*self.graph, Bm, A, U, Hprev, Cand, Hnew, copies=copies, side=side)
            return [*Zg, CandIn]
        Zc = _spatial_slabs(CandIn, self.fwd_val, op, self.Ks)
        k.cell_blend_fwd(rows(Zc), Tc, Wc, bc, *rows((U, Hprev, Cand, Hnew)), copies=copies, side=side)
        return [*Zg, *Zc]

    def cell(self, j, stack, out=None):
        """Every launch of cell j, in its form; the new state goes to ``out`` (a slot of the output stack) or to a tensor of its own.  Returns
        what the cell saves for backward: [H, U, R, Cand, *the form's planes]."""
        first = self.first[j]                                       # first-step forms: H and R are saved as None -- the planes do not exist
        Hprev = None if first else self.source(self.schedule[j][2])
        copies, side, late_copies, late_rows = self.copy_plan(j)
        form = self.forms[j]
        U = self.plane()
        Rg, Cand = (None, None) if (self.lean and form.planar) else (None if first else self.plane(), self.plane())
        Hnew = self.plane() if out is None else out
        more = getattr(self, _FORM_METHODS[form][0])(j, *stack, Hprev, U, Rg, Cand, Hnew, copies, side)
        self.finish(j, Hnew, late_copies, late_rows)
        return [Hprev, U, Rg, Cand, *more]

    def release(self, j, last, keep):
        """After cell j: its input rows, and every source it was the last consumer of -- the state (unless it is in ``keep``: the outputs live in
        the output stack) and its aggregation or Chebyshev planes; its own state at once if nothing consumes it."""
        self.XH.pop(j, None)
        for src in set(self.schedule[j][1:]) | {('cell', j)}:
            if last.get(src, j) == j:
                self.agg.pop(src, None)
                if src[0] == 'cell' and src[1] not in keep:
                    self.state[src[1]] = None


def _presum(ts, limit: int, tail: bool = False):
    """The list ``ts`` folded down to ``limit`` tensors for a kernel that takes no more: the last two into one (``tail``) or the first two, until it fits."""
    while len(ts) > limit:
        ts = ts[:-2] + [ts[-1] + ts[-2]] if tail else [ts[0] + ts[1]] + ts[2:]
    return ts


class _Ledger(dict):
    """cell -> what its state is still owed, for every state something downstream depends on: a record with the fields ``done``, a finished
    gradient tensor (from the outputs and interleaved consumers) or None; ``d`` = (d0, d1, d2), lists of planes owed to the state, to S.state
    and to T_2(S).state (from planar consumers); ``shared``, the (direct, aggregated) pair of ``claim`` or None (its planes are also in d0, d1).
    Aggregation being linear, the state's gradient is  done + sum d0 - sum d2 + S^T (sum d1 + 2 S^T sum d2)  (Clenshaw form of sum_n T_n(S)^T d_n):
    narrow SpMMs with the sums in their gather / epilogue instead of a wide transpose SpMM and a split pass per consuming cell.  An order-2
    consumer leaves no d2: its state's gradient is the same formula with d2 empty, done + sum d0 + S^T sum d1, ONE SpMM."""

    pending = dict.get                                              # the record of a state that is owed something, else None
    take = dict.pop                                                 # ... which leaves the ledger: its own cell runs

    def _rec(self, kid):
        return self.setdefault(kid, SimpleNamespace(done=None, d=([], [], []), shared=None))

    def finished(self, kid):
        return self[kid].done if kid in self else None

    def finish(self, kid, t):
        self._rec(kid).done = t

    def leave(self, kid, d0, d1, d2=()):
        for have, more in zip(self._rec(kid).d, (d0, d1, d2)):
            have += more

    def claim(self, src, claimed: set, new, share: bool):
        """(direct plane, aggregated plane, accumulate) of source ``src`` for a one-launch consumer.  The first consumer's fresh planes become
        the state's shared pair; a later consumer gets them back with accumulate = True and ADDS into them, so the state-gradient SpMM gathers
        one operand and reads one direct plane per state, not one per consumer.  ``share``: fp32 planes only (the bf16 kernels have no
        accumulate flags).  One claim per consuming cell per state: ``claimed`` is the set of states whose pair that cell holds, so a cell
        that reads one state on both sides takes the pair for its first side and fresh planes (``new()``) for the other."""
        if src[0] != 'cell':
            return new(), new(), False                              # an external tensor: gradients computed, nobody owed
        rec = self._rec(src[1])
        if share and rec.shared is not None and src[1] not in claimed:
            claimed.add(src[1])
            return (*rec.shared, True)
        d, a = new(), new()
        self.leave(src[1], [d], [a])
        if share and rec.shared is None:
            rec.shared = (d, a)
            claimed.add(src[1])
        return d, a, False


class _ParamGrads:
    """The parameter gradients of one backward.  Every planar cell writes its (dWg, dbg, dWc, dbc) into its own row of ONE buffer per parameter
    set (``next_row``), summed once at the end -- not four accumulation passes per cell (176 five-microsecond launches per metric step);
    the interleaved cells' gradients are accumulated as they come (``add``: reverse schedule order), the row sums after them."""

    def __init__(self, stacks, schedule):
        self.stacks, self.schedule, self.rows, self.acc = stacks, schedule, {}, [[None] * 4 for _ in stacks]   # rows: set -> (row buffer, its rows still to hand out)

    def _views(self, s_id, row):                                    # (dWg, dbg, dWc, dbc) as views of one row of the set's buffer
        st = self.stacks[s_id]
        parts = row.split([0 if t is None else t.numel() for t in st])
        return tuple(None if t is None else part.view_as(t) for t, part in zip(st, parts))

    def next_row(self, s_id):
        if s_id not in self.rows:
            st = self.stacks[s_id]
            buf = st[0].new_zeros(sum(1 for sc in self.schedule if sc[0] == s_id), sum(t.numel() for t in st if t is not None))
            self.rows[s_id] = (buf, iter(buf))
        return self._views(s_id, next(self.rows[s_id][1]))

    def add(self, s_id, grads):
        self.acc[s_id] = [a if t is None else t if a is None else a.add_(t) for a, t in zip(self.acc[s_id], grads)]

    def result(self):
        for s_id, (buf, _) in self.rows.items():
            self.add(s_id, self._views(s_id, buf[0] if buf.shape[0] == 1 else buf.sum(0)))
        return [None if prm is None else (g if g is not None else torch.zeros_like(prm)) for st, a in zip(self.stacks, self.acc) for prm, g in zip(st, a)]


class _BackwardPass(_Pass):
    """... and, in the backward, what every state is still owed (``owes``: one ``_Ledger`` record per state, filled by its consumers through ``finish`` /
    ``leave`` / ``claim``, emptied by ``owed`` / ``owed_ring2`` when its own cell runs) and the parameter gradients (``params``: ``_ParamGrads``)."""

    def __init__(self, k, op: SpatialOperand, Ks: int, Tc, schedule, stacks, cin, forms, dims, bf16: bool, zmax_all, learn_Tc: bool = False, learn_val: bool = False):
        super().__init__(k, op, Ks, Tc, schedule, cin, forms, dims, bf16, zmax_all, (op.bwd_rowptr, op.bwd_colidx, op.bwd_val, op.bwd_plan))
        # a learned category graph: every PLANAR cell's two dT_c launches ADD into one float64 buffer, zeroed here, folded once (``_dtc_fold``)
        self.dtc = torch.zeros(k.cell_dtc_slots(self.B * self.N), self.C, self.C, dtype=torch.float64, device=Tc.device) if learn_Tc else None
        # a learned sparse spatial graph: every PLANAR cell's launch ADDS its share of dval, in ``fwd_val``'s order, to one float64 buffer (stc_graph_grad_csr_pairs_f32)
        self.dval = torch.zeros(op.nnz, dtype=torch.float64, device=Tc.device) if learn_val else None
        # state gradient sums fused with a transpose aggregation where the graph has a two-ring plan (stc_ring2_sum_f32 / _chain_f32)
        self.ring2 = _RING2 and not bf16 and op.bwd_ring2 is not None and k.ring2_fits(self.B, self.N, self.C, self.h)
        self.owes, self.params = _Ledger(), _ParamGrads(stacks, schedule)

    def owed(self, kid, blend=None):
        """The gradient of state ``kid`` from its record; with ``blend`` = (U, Cand) of its cell also dY = gradient * U * (1 - Cand^2)."""
        rec = self.owes.take(kid)
        base, (d0, d1, d2) = rec.done, rec.d
        if not d1:                                                  # no planar consumer: the finished tensor is the gradient
            if blend is None:
                return base
            dY = torch.empty_like(base)
            self.k.gru_blend_bwd(base, blend[0], None, blend[1], dY, None, None)
            return base, dY
        d0 = d0 + ([base] if base is not None else [])
        if d2:                                                      # order-3 consumers (their states need no blend)
            return self.clenshaw(d0, d1, d2)
        # more consumers than the kernel takes addends for: pre-sum -- on fp32 planes too above the bf16 kernel's limit, below their own (SPMM_SUM_MAX_ADD)
        add = _presum(d0, SPMM_SUM_BF16_MAX_ADD, tail=True)
        aggs = _presum(d1, _SUM_GATHERS)
        out, dY = torch.empty_like(aggs[0]), torch.empty_like(aggs[0]) if blend is not None else None
        self.k.spmm_sum(*self.graph, aggs[0], aggs[1] if len(aggs) > 1 else None, [(t, 0) for t in add], out, blend=None if blend is None else (blend[0], blend[1], dY))
        return out if blend is None else (out, dY)

    def owed_ring2(self, kid, U_, Cand_):
        """(gradient of state ``kid``, S^T (gradient * U * (1 - Cand^2))) in one launch where the graph has a two-ring plan; None: the two
        launches (``owed`` with its blend epilogue, then the narrow aggregation) -- the record is then left as it is."""
        rec = self.owes.pending(kid)
        add = [] if rec is None else rec.d[0] + ([rec.done] if rec.done is not None else [])
        # (the forms that fit the register file: one aggregated plane, up to two addends -- 590 / 680 us for the 555 + 185 they replace; with a
        #  second aggregated plane the kernel spills and takes 840 - 1 150 us: the two launches stay)
        if not self.ring2 or rec is None or len(add) > 2 or len(rec.d[1]) != 1:
            return None
        agg = self.owes.take(kid).d[1][0]
        out, dBm_ = torch.empty_like(agg), torch.empty_like(agg)
        self.k.ring2_sum(*self.graph[:3], self.op.bwd_ring2, agg, None, add, U_, Cand_, out, dBm_)
        return out, dBm_

    def clenshaw(self, d0, d1, d2):
        """sum d0 - sum d2 + S^T (sum d1 + 2 S^T sum d2) from lists of planes (d2 non-empty): two narrow SpMMs with the sums in their gather /
        epilogue (alpha and signed addends of stc_spmm_sum_f32), each list pre-summed from its front to what the launch takes."""
        k, d2 = self.k, _presum(d2, _SUM_GATHERS)
        if self.ring2 and len(d1) <= _CHAIN_FIRST_ADD and 1 <= len(d0) + len(d2) <= k.RING2_MAX_ADD:
            # both transpose aggregations in one launch (stc_ring2_chain_f32): the inner sum d1 + 2 S^T d2 never leaves the chip
            out = torch.empty_like(d2[0])
            k.ring2_chain(*self.graph[:3], self.op.bwd_ring2, d2[0], d2[1] if len(d2) > 1 else None, 2.0, list(d1), None, 1.0,
                          [(a, 1.0) for a in d0] + [(a, -1.0) for a in d2], out)
            return out
        t = torch.empty_like(d2[0])
        k.spmm_sum(*self.graph, d2[0], d2[1] if len(d2) > 1 else None, [(a, 0) for a in _presum(d1, SPMM_SUM_MAX_ADD)], t, alpha=2.0)
        adds = [(a, 0) for a in _presum(d0, SPMM_SUM_MAX_ADD - len(d2))] + [(a, 0, -1.0) for a in d2]
        out = torch.empty_like(t)
        k.spmm_sum(*self.graph, t, None, adds, out, blend=None)
        return out

    # ---- one function per form: the launches of cell j's backward from what its forward saved (``_Form``)
    def planar3(self, j, Wg, bg, Wc, bc, saved):
        k, rows, Tc, (s_id, x, hs) = self.k, self.rows, self.Tc, self.schedule[j]
        Hprev, U, Rg, Cand, Zx0, Zx1, Zx2, Zh1, Zh2, *Zr = saved
        Zx, Zh = [Zx0, Zx1, Zx2], [Hprev, Zh1, Zh2]
        wide = self.cin[j] == self.h
        new = lambda: torch.empty_like(Hprev)
        dWg, dbg, dWc, dbc = self.params.next_row(s_id)             # (parameter gradients: rows of the set's buffer, summed at the end)
        dHnew = self.owed(j)
        dX, dR = ([new(), new(), new()] if wide else [None] * 3), [new(), new(), new()]
        k.cell_cand_bwd_planar_k(rows(Zx), rows(Zr), Tc, Wc, *rows((dHnew, U, Cand)), rows(dX), rows(dR), dWc, dbc, **self.act_slots(j, 1))
        dRH = self.clenshaw([dR[0]], [dR[1]], [dR[2]])              # gradient of the R*H plane from its three Chebyshev planes
        del dR
        # the kernel ADDS the gates' X-side gradients into the candidate's three planes (accumulate_x), so the source gets one plane per
        # order from this cell and its Clenshaw sums need no pre-sum; it adds the prologue's share into the H plane's gradient (dH = None)
        dHg = [new(), new(), new()]
        k.cell_gates_bwd_planar_k(rows(Zx), rows(Zh), Tc, Wg, *rows((dRH, Cand, U, Rg, dHnew)), rows(dX), rows(dHg), dWg, dbg, None,
                                  accumulate_x=wide, **self.act_slots(j, 0))
        if wide and x[0] == 'cell':
            self.owes.leave(x[1], dX[:1], dX[1:2], dX[2:])
        if hs[0] == 'cell':
            self.owes.leave(hs[1], dHg[:1], dHg[1:2], dHg[2:])

    def planar_one_bwd(self, j, Wg, bg, Wc, bc, saved):
        k, (s_id, x, hs) = self.k, self.schedule[j]
        Hprev, U, Rg, Cand, Xp, SXp, SHp = saved
        fused = self.owed_ring2(j, U, Cand)                         # state gradient + S^T dY in one launch, no dY plane (stc_ring2_sum_f32)
        if fused is not None:
            dHnew, dBm = fused
        else:
            dHnew, dY = self.owed(j, (U, Cand))
            dBm = self.spmm(dY)
            del dY                                                  # (the kernel re-forms dY from dHnew, U, Cand)
        dWg, dbg, dWc, dbc = self.params.next_row(s_id)
        # (a state's second consumer ADDS into the planes its first one wrote: ``_Ledger.claim``; claimed: the states whose planes this cell holds)
        new, claimed = (lambda: torch.empty_like(U)), set()
        dXd, dSX, acc_x = self.owes.claim(x, claimed, new, not self.bf16) if self.cin[j] == self.h else (None, None, False)
        if Hprev is None:                                           # the forward ran the first-step forms: no H, S.H, R; nobody is owed dH, dS.H
            k.cell_bwd_first(*self.rows((Xp, SXp)), self.Tc, Wg, Wc, *self.rows((U, Cand, dHnew, dBm)), self.rows((dXd, dSX)), dWg, dbg, dWc, dbc,
                             accumulate_x=acc_x, **self.act_slots(j))
            return
        dHd, dSH, acc_h = self.owes.claim(hs, claimed, new, not self.bf16)
        k.cell_bwd_planar(*self.rows((Xp, Hprev, SXp, SHp)), self.Tc, Wg, Wc, *self.rows((U, Rg, Cand, dHnew, dBm)),
                          self.rows((dXd, dSX, dHd, dSH)), dWg, dbg, dWc, dbc,
                          **(dict(accumulate_x=acc_x, accumulate_h=acc_h, **self.act_slots(j)) if not self.bf16 else {}))

    def planar(self, j, Wg, bg, Wc, bc, saved):
        k, rows, Tc, (s_id, x, hs) = self.k, self.rows, self.Tc, self.schedule[j]
        Hprev, U, Rg, Cand, Xp, SXp, SHp, RH, *Bm = saved            # (Bm: saved only while the spatial values are learned)
        dHnew, dY = self.owed(j, (U, Cand))
        wide = self.cin[j] == self.h                                # else: narrow input plane (layer 0), which needs no gradient
        # the candidate's input planes are (X, R*H): X's maximum as the gates forward left it, R*H rides on H's (|R*H| <= |H|).  Slot
        # rows of that launch: wide {X, S.X, H, S.H}, narrow {H, S.H, x, S.x}; the post kernel takes (16-wide plane, other plane).
        zr = None if self.zmax_all is None else self.zmax_all[j, 0]
        post_kw, gates_kw = ({}, {}) if zr is None else (dict(act_amax=(zr[0], zr[2])), dict(act_amax=zr))
        dBm = self.spmm(dY)
        dRH = torch.empty_like(Hprev)
        dWg, dbg, dWc, dbc = self.params.next_row(s_id)
        dHd, dSH = torch.empty_like(Hprev), torch.empty_like(Hprev)
        if wide:
            dXc, dXd, dSX = (torch.empty_like(Hprev) for _ in range(3))
            k.node_post_bwd(*rows((Xp,)), Tc, Wc, *rows((dY, dBm, dXc)), dWc, dbc, X2=RH.view(-1, self.C, self.h), dX2=dRH.view(-1, self.C, self.h),
                            **post_kw)
            planes = rows((dXd, dSX, dHd, dSH))
        else:
            k.node_post_bwd(*rows((RH,)), Tc, Wc, *rows((dY, dBm, dRH)), dWc, dbc, X2=Xp.view(-1, self.C, self.cin[j]), **post_kw)
            planes = [None, None] + rows((dHd, dSH))
        if self.dtc is not None:                                    # dT_c while the planes are alive: dY, dBm here, dRH as the launch above left it
            k.cell_dtc_cand(*rows((Xp, RH)), Wc, *rows((dY, dBm)), self.dtc)
            k.cell_dtc_gates(*rows((Xp, Hprev, SXp, SHp)), Wg, *rows((U, Rg, Cand, dHnew, dRH)), self.dtc)
        del dBm
        if self.dval is None:
            del dY
        # (dH = None: the kernel adds the prologue's share into the H plane's gradient)
        k.cell_gates_bwd_planar(*rows((Xp, Hprev, SXp, SHp)), Tc, Wg, *rows((dRH, Cand, U, Rg, dHnew)), planes, dWg, dbg, None, **gates_kw)
        if self.dval is not None:
            # the cell's three applications of S -- S.X, S.H, A + S.Bm -- in one launch: dval[e = (i, j)] += <dS.X[i], X[j]> + <dS.H[i], H[j]> + <dY[i], Bm[j]>
            if not wide:                                            # the gates backward forms no d(S.x) plane for a narrow input, which needs no gradient
                dSX = Xp.new_empty(Xp.shape)
                k.cell_dsx_narrow(*rows((Hprev,)), Wg, Tc, *rows((U, Rg, Cand, dHnew, dRH, dSX)))
            k.graph_grad_csr_pairs(self.op.fwd_rowptr, self.op.fwd_colidx, [(dSX, Xp), (dSH, Hprev), (dY, Bm[0])], self.N, self.dval)
        if wide and x[0] == 'cell':
            self.owes.leave(x[1], [dXd, dXc], [dSX])                # as the X plane: gates' and candidate's direct shares
        if hs[0] == 'cell':
            self.owes.leave(hs[1], [dHd], [dSH])                    # as the H plane, the gates prologue's share included

    def rows_cell(self, j, Wg, bg, Wc, bc, saved):
        """ROWS_POST and ROWS_SLABS; the sources get finished gradient tensors, the parameter gradients are added to their set's as they come."""
        k, op, Ks, h, Tc, (s_id, x, hs) = self.k, self.op, self.Ks, self.h, self.Tc, self.schedule[j]
        Hprev, U, Rg, Cand, *Z = saved
        Zg, Zc = Z[:Ks], Z[Ks:]
        post = self.forms[j] is _Form.ROWS_POST                     # candidate backward starts from dY = dHnew * U * (1 - Cand^2)
        dHnew, dY = self.owed(j, (U, Cand)) if post else (self.owed(j), None)
        dH = torch.empty_like(Hprev)
        if post:                                                    # the forward ran this convolution as Y = A + S.Bm (no Z_1 slab)
            dBm = self.spmm(dY)
            dci, dWc = torch.empty_like(Zc[0]), torch.empty_like(Wc)
            dbc = Wc.new_empty(h) if bc is not None else None
            k.node_post_bwd(*self.rows((Zc[0],)), Tc, Wc, *self.rows((dY, dBm, dci)), dWc, dbc)
        else:                                                       # slab form, blend backward in the node kernel's prologue
            g, dWc, dbc, _, _ = _bdg_backward_slabs(None, Zc, Wc, Tc, op, Ks, bc is not None, False, False, cand=(dHnew, U, Cand))
            if Ks > 1:
                self.spmm(g[1], g[0], g[0], 1.0, 1.0)
            dci = g[0]
        # gates convolution, gate + blend backward in its prologue
        g, dWg, dbg, _, _ = _bdg_backward_slabs(None, Zg, Wg, Tc, op, Ks, bg is not None, False, False, gates=(dci, Cand, Hprev, U, Rg, dHnew, dH))
        need_x, need_h = x[0] == 'cell', hs[0] == 'cell'
        if need_x or need_h:
            if Ks > 1:
                self.spmm(g[1], g[0], g[0], 1.0, 1.0)
            dXt = Hprev.new_empty(Hprev.shape[:-1] + (self.cin[j],))
            same = need_x and need_h and x[1] == hs[1]
            owedA = self.owes.finished(x[1]) if need_x else None
            owedB = self.owes.finished(hs[1]) if (need_h and not same) else None
            k.split2(g[0], dXt, dH, addA=dci, addB=dH, addA_ld=Zc[0].shape[-1], addA2=owedA, addB2=owedB)
            if need_h and not same:
                self.owes.finish(hs[1], dH)
            if need_x:
                self.owes.finish(x[1], dXt.add_(dH) if same else dXt)
        self.params.add(s_id, (dWg, dbg, dWc, dbc))


def _dtc_fold(partials, Tc):
    """dT_c (2, C, C) in ``Tc``'s type from the float64 slots the dT_c launches added into: dTc[1] = their sum, dTc[0] = 0 (T_0 = I is a constant)."""
    dTc = torch.zeros_like(Tc)
    dTc[1].copy_(partials.sum(0))
    return dTc


def _begin_forward(op: SpatialOperand, Ks: int, schedule, outputs, n_ext: int, Tc, fwd_val, tensors, forward_only: bool = False, learn_Tc: bool = False,
                   learn_val: bool = False):
    """What both routes of ``stc_cell_graph`` do before the first launch: kernel set, contiguous operands, one form per cell, the output stack.
    Returns (pass, parameter sets, output stack, output cell -> slot)."""
    k = kernels().for_graph(_amplification(op, Ks))              # (a heavy graph: the 24-bit operand format, _lib.HEAVY_ROW_SUM)
    _, stacks, Tc, fwd_val = _unpack(0, Tc, fwd_val, tensors[n_ext:])
    ext = [t if _is_zero_state(t) else _c(t) for t in tensors[:n_ext]]      # (zero initial states as shapes, ``zero_state``: not made contiguous)
    bf16 = ext[0].dtype == torch.bfloat16                       # bf16 state planes: the all-planar bf16 kernel set
    if bf16:
        k = k.bf16
    h = 16
    B, N, C = ext[0].shape[:3]
    cin = [ext[x[1]].shape[-1] if x[0] == 'ext' else h for _, x, _ in schedule]
    forms = _cell_forms(k, Ks, Tc.shape[0], C, h, cin, bf16, learn_Tc or learn_val)      # (the value gradient needs the planes of the two-launch backward as well)
    if bf16 and not all(f.planar for f in forms):
        raise ValueError('stc_cell_graph: bfloat16 states need an all-planar schedule (Ks = 2, inputs 16 or 1..4 columns wide)')
    p = _ForwardPass(k, op, Ks, Tc, fwd_val, schedule, ext, cin, forms, bf16, forward_only, keep_bm=learn_val)
    out_stack = ext[0].new_empty(len(outputs), B, N, C, h)      # the requested states are produced in place, stacked
    return p, stacks, out_stack, _out_slots(outputs)


def _forward_only(op: SpatialOperand, Ks: int, schedule, outputs, n_ext: int, Tc, fwd_val, tensors):
    """``_StcCellGraph.forward`` for a pass that no backward follows (evaluation, forecasting): the same launches per cell
    (``_ForwardPass.cell``), but nothing is saved -- every state, aggregation, input row and temporary goes back to the allocator after its
    last consumer has launched (``release``; the cells run by level, ``wavefront``), no activation maxima are collected, and on the fp32 kernel
    set the planes only a backward reads are not written: R and Cand of the planar cells, and R*H at order 2 whichever backward the form has
    (``_ForwardPass.lean``; stc_hip.h, ABI v34).  Interleaved cells, the bf16 set and kernel sets without ``optional_gate_stores`` get the
    liveness only.  The states are bit for bit those of the autograd node."""
    p, stacks, out_stack, out_slot = _begin_forward(op, Ks, schedule, outputs, n_ext, Tc, fwd_val, tensors, forward_only=True)
    order = wavefront(schedule)                                  # the cells by level, schedule order inside a level
    last = last_uses(schedule, order)                            # source -> the cell after whose launches nothing reads it any more
    for j in order:
        p.cell(j, stacks[schedule[j][0]], out_stack[out_slot[j]] if j in out_slot else None)
        p.release(j, last, out_slot)
    return out_stack


class _StcCellGraph(Function):
    """Encoder + decoder (any DAG of STC_Cells whose inputs are other cells' states) as one autograd node.
    Per cell the kernels are those of ``_StcCell``'s fused path.  What owning the whole schedule adds:
      * planar cells (inputs of 16 + 16 columns, i.e. every cell above layer 0): the [Xt | H] row of reference
        STC_GNN.py:68 is never built -- the kernels read the two state tensors as two planes, and the aggregation S.state is
        formed ONCE per state (narrow SpMM) for all the cells that consume it (``stc_cell_gates_fwd/bwd_planar_f32``);
      * interleaved cells (layer 0: 1 + 16 columns padded to 20): no concat pass either -- the producer's blend epilogue
        writes the new state straight into their input rows (state copies of ``stc_spmm_blend_fwd_f32`` / ``stc_cell_blend_fwd_f32``);
      * the candidate convolution in post-aggregation form where the kernels exist (``_POST_AGG``);
      * no autograd accumulation passes: what a state's consumers owe it is kept in ONE record per state (``_Ledger``) -- summed inside an
        interleaved consumer's final split (``stc_split2_f32`` addA2 / addB2), or inside the state's own narrow SpMM for planar consumers.
    Every cell runs in one of five forms (``_Form``), chosen once before the forward's launches: PLANAR3 (order 3), PLANAR_ONE_BWD and
    PLANAR (order 2: one-launch or two-launch backward), ROWS_POST and ROWS_SLABS (interleaved rows; candidate as Y = A + S.Bm or on slabs).
    The launches of each form are one method of ``_ForwardPass`` and one of ``_BackwardPass`` (``_FORM_METHODS``); the parameter gradients
    of a backward are one ``_ParamGrads``.  schedule[j] = (stack, Xt source, H source), a source being ('ext', i) or ('cell', k)."""

    @staticmethod
    def forward(ctx, op: SpatialOperand, Ks: int, schedule, outputs, n_ext: int, Tc, fwd_val, *tensors):
        learn_Tc = ctx.needs_input_grad[5]                           # (``stc_cell_graph`` lets a ``Tc`` that requires grad through only with ``learn_Tc``)
        learn_val = ctx.needs_input_grad[6]                          # (... and values that require grad only where ``_dval_route`` holds)
        p, stacks, out_stack, out_slot = _begin_forward(op, Ks, schedule, outputs, n_ext, Tc, fwd_val, tensors, learn_Tc=learn_Tc, learn_val=learn_val)
        saved = []
        for j, (s_id, _, _) in enumerate(schedule):
            saved += p.cell(j, stacks[s_id], _alias(out_stack, out_slot[j]) if j in out_slot else None)
        ctx.save_for_backward(p.Tc, *[t for st in stacks for t in st], *saved)
        ctx.meta = (op, Ks, schedule, tuple(outputs), p.cin, len(stacks), (p.B, p.N, p.C), p.forms)
        ctx.zmax_all = p.zmax_all
        _guard(ctx, out_stack)
        return out_stack

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_stack):
        k = kernels().for_graph(_amplification(ctx.meta[0], ctx.meta[1]))
        bf16 = grad_stack.dtype == torch.bfloat16
        if bf16:
            k = k.bf16
        op, Ks, schedule, outputs, cin, n_sets, dims, forms = ctx.meta
        _check_guard(ctx)
        Tc, *sv = ctx.saved_tensors
        stacks, sv = _stacks(sv[:4 * n_sets]), sv[4 * n_sets:]
        cells = []
        learn_Tc, learn_val = ctx.needs_input_grad[5], ctx.needs_input_grad[6]
        for f in forms:                                              # what each cell saved, by its form
            cells, sv = cells + [sv[:f.saved(Ks, learn_val)]], sv[f.saved(Ks, learn_val):]
        p = _BackwardPass(k, op, Ks, Tc, schedule, stacks, cin, forms, dims, bf16, ctx.zmax_all, learn_Tc, learn_val)
        grad_stack = _c(grad_stack)
        for i, j in enumerate(outputs):
            p.owes.finish(j, grad_stack[i])                          # read-only here: sums go to fresh buffers
        for j in range(len(schedule) - 1, -1, -1):
            if not p.owes.pending(j):
                continue                                             # nothing downstream depends on this cell
            getattr(p, _FORM_METHODS[forms[j]][1])(j, *stacks[schedule[j][0]], cells[j])
        flat = p.params.result()
        n_ext = len(ctx.needs_input_grad) - 7 - len(flat)
        dval = p.dval.to(op.fwd_val.dtype) if learn_val else None    # (in ``fwd_val``'s order: the pattern the launches walked is the forward CSR)
        return (None,) * 5 + (_dtc_fold(p.dtc, Tc) if learn_Tc else None, dval) + (None,) * n_ext + tuple(flat)


def stc_cell_graph(op: SpatialOperand, Tc, Ks: int, schedule, outputs, ext, stacks, learn_Tc: bool = False):
    """Run a schedule of STC_Cells (see ``_StcCellGraph``).  ``ext``: external (B,N,C,*) tensors (inputs, initial states;
    they get no gradient); ``stacks``: [(Wg, bg, Wc, bc)] parameter sets; returns the new states of the ``outputs`` cells
    stacked along a new leading axis, (len(outputs), B, N, C, h) -- written in place by the kernels, no stack pass.

    Only the parameter sets are differentiable on every route; the few-category executor (``small.stc_small_graph``) also differentiates
    the graphs.  In grad mode an external tensor that requires grad -- and, outside the few-category executor, ``Tc`` or ``op.fwd_val``
    that does -- raises ``ValueError`` naming the argument, before any launch: no gradient is ever dropped silently
    (``cell_graph_supported`` tells beforehand for the graphs; ``stc_cell`` differentiates every input).

    Which executor runs is decided per call, also by what requires grad: at Chebyshev order 3 a DENSE ``Gs`` takes the few-category executor
    only while it requires grad, or with grad mode off (``small.small_graph_supported``).  In grad mode with that graph frozen the call
    goes to the general executor, which has cell kernels for C in {16, 32, 64} only: on few categories it then fails in its first launch's
    host check (``StcError``: shape not on the fused path) -- loud, but without naming the graph.  Ask ``cell_graph_supported`` first, as
    the module does (it then runs one node per cell).

    ``learn_Tc=True`` (``graph_mode='csr-category-learned'``): a ``Tc`` that requires grad is differentiated by the general executor -- fp32
    planes, order 2, C in {32, 64}, every cell in ``_Form.PLANAR``, whose two-launch backward also adds the cell's share of dT_c[1] to one float64
    buffer (``stc_cell_dtc_gates_planar_f32`` / ``_cand_planar_f32``); ``cell_graph_supported(..., learn_Tc=True)`` tells beforehand, a problem
    outside it raises ``ValueError``.  ``op.fwd_val`` is refused as before.  With the default every answer and refusal is unchanged.

    A learned SPARSE spatial graph (``graph.learned_csr_operand(..., sampled_grad=True)``: ``STCGNN(graph_mode='csr-learned', csr_cells='fused')``)
    whose values require grad is differentiated here where ``_dval_route`` holds -- fp32 planes, Ks = Kc = 2, hidden 16, C in {32, 64}, inputs 16
    or 1..4 columns wide, a kernel set with ``cell_graph_vals``: every cell runs in ``_Form.PLANAR`` and also keeps its Bm plane; its backward
    adds < dS.X, X > + < dS.H, H > + < dY, Bm > at the stored entries to one float64 buffer (``stc_graph_grad_csr_pairs_f32``, one launch per cell;
    the d(S.x) plane of a narrow input from ``stc_cell_dsx_narrow_planar_f32``), returned in ``fwd_val``'s order.  With ``learn_Tc`` both graphs
    are learned in the one node; without ``sampled_grad`` values that require grad are refused as before."""
    ext = list(ext)
    _refuse_differentiable(ext=ext)
    k = kernels()
    if _SMALL and small_graph_supported(k, op, Tc, Ks, ext[0].shape[2], 16, {ext[x[1]].shape[-1] if x[0] == 'ext' else 16 for _, x, _ in schedule},
                                        ext[0].dtype):
        return stc_small_graph(k, op, Tc, Ks, schedule, outputs, ext, stacks)
    widths = {ext[x[1]].shape[-1] if x[0] == 'ext' else 16 for _, x, _ in schedule}
    kg = k.for_graph(_amplification(op, Ks))
    learn_val = _dval_route(kg, op, Tc, Ks, ext[0].shape[2], 16, widths, ext[0].dtype)
    if _learns_tc(learn_Tc, Tc):
        if not learn_val:
            _refuse_differentiable(fwd_val=op.fwd_val)
        if not _dtc_route(kg, op, Tc, Ks, ext[0].shape[2], 16, widths, ext[0].dtype):
            raise ValueError('stc_cell_graph: learn_Tc needs fp32 planes, Chebyshev order 2, C in (32, 64), inputs 16 or 1..4 columns wide and a kernel '
                             'set with the planar dT_c kernels (cell_graph_supported(..., learn_Tc=True) tells beforehand; stc_cell differentiates every input)')
    elif learn_val:
        _refuse_differentiable(Tc=Tc)                                # the value route alone
    else:
        _refuse_differentiable(Tc=Tc, fwd_val=op.fwd_val)
    flat = [p for st in stacks for p in st]
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (Tc, op.fwd_val, *ext, *flat)):
        with torch.no_grad():                                        # no backward will follow: nothing saved, nothing stored for one (``_forward_only``)
            return _forward_only(op, Ks, list(schedule), list(outputs), len(ext), Tc, op.fwd_val, (*ext, *flat))
    return _StcCellGraph.apply(op, Ks, list(schedule), list(outputs), len(ext), Tc, op.fwd_val, *ext, *flat)


# ---- the learned graph generator (MGP_Gen): dense MixedFusion and the front end; the rank-r MixedFusion is fusion.py ----------------------------
# What the three ``*_supported`` predicates share: float32 on a ROCm device; contiguous parameters, every tensor 16-byte aligned.
def _f32_on_gpu(ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


def _laid_out(ts, params) -> bool:
    return all(t.is_contiguous() for t in params) and all(t.data_ptr() % 16 == 0 for t in ts)      # (a view into a flat parameter buffer may not be)


class _MixedFusion(torch.autograd.Function):
    """G = gate * A + (1 - gate) * P with gate = sigmoid(lin_A(vec A) + lin_P(vec P)) (reference STC_GNN.py:253-260) in one streaming launch per
    direction (``stc_mixed_fusion_fwd/bwd_f32``): the two (n^2, n^2) weight matrices are read once forward and once backward, their
    gradients written once."""

    @staticmethod
    def forward(ctx, A, P, WA, bA, WP, bP):
        k = kernels()
        A_, P_ = A.detach().contiguous(), P.detach().contiguous()
        gate, G = k.mixed_fusion_fwd(WA.detach(), bA.detach(), WP.detach(), bP.detach(), A_, P_)
        ctx.save_for_backward(A_, P_, WA, WP, gate)
        return G

    @staticmethod
    @once_differentiable
    def backward(ctx, dG):
        A, P, WA, WP, gate = ctx.saved_tensors
        want_dA = ctx.needs_input_grad[0]
        need = ctx.needs_input_grad
        dWA, dWP, db, dP, dA = kernels().mixed_fusion_bwd(WA.detach(), WP.detach(), A, P, gate, dG.contiguous(), want_dA, want_dW=need[2] or need[4])
        return (dA if need[0] else None, dP if need[1] else None, dWA if need[2] else None, db if need[3] else None,
                dWP if need[4] else None, db if need[5] else None)


def mixed_fusion_supported(A: torch.Tensor, P: torch.Tensor, *params: torch.Tensor) -> bool:
    """Whether ``mixed_fusion`` takes these operands: float32 on a GPU, contiguous weights, 16-byte aligned, n^2 a multiple of 4."""
    ts = (A, P) + params
    return _f32_on_gpu(ts) and _laid_out(ts, params) and kernels().mixed_fusion_supported(A.numel())


def mixed_fusion(A, P, WA, bA, WP, bP):
    return _MixedFusion.apply(A, P, WA, bA, WP, bP)


# ---- front end of the learned graph generator --------------------------------------------------------------------------------------------
class _MgpUV(torch.autograd.Function):
    """U, V = tanh(alpha X Wu), tanh(alpha X Wv) (reference STC_GNN.py:229-230 / :237-238) in (rows, slices, hidden) layout, one launch; the data
    window X gets no gradient."""

    @staticmethod
    def forward(ctx, X, Wu, Wv, rows_axis, alpha):
        X_ = X.detach().contiguous()
        U, V = kernels().mgp_uv_fwd(X_, rows_axis, Wu.detach().contiguous(), Wv.detach().contiguous(), alpha)
        ctx.save_for_backward(X_, U, V)
        ctx.meta = (rows_axis, alpha)
        return U, V

    @staticmethod
    @once_differentiable
    def backward(ctx, dU, dV):
        X_, U, V = ctx.saved_tensors
        dWu, dWv = kernels().mgp_uv_bwd(X_, ctx.meta[0], U, V, dU.contiguous(), dV.contiguous(), ctx.meta[1])
        return None, dWu, dWv, None, None


class _MgpSoftmax(torch.autograd.Function):
    """softmax(relu(P - P^T), -1) (reference STC_GNN.py:231-232: the einsum pair is P - P^T) in one launch per direction."""

    @staticmethod
    def forward(ctx, P):
        P_ = P.detach().contiguous()
        Ps = kernels().mgp_softmax_fwd(P_)
        ctx.save_for_backward(P_, Ps)
        return Ps

    @staticmethod
    @once_differentiable
    def backward(ctx, dPs):
        P_, Ps = ctx.saved_tensors
        return kernels().mgp_softmax_bwd(P_, Ps, dPs.contiguous())


def mgp_front_supported(X: torch.Tensor, Wu: torch.Tensor, Wv: torch.Tensor) -> bool:
    """Whether ``mgp_front`` takes these operands: a float32 window (B, T, N, C) and float32 (F, h) parameters on a GPU, no gradient wanted for X."""
    return (X.dim() == 4 and _f32_on_gpu((X, Wu, Wv)) and not X.requires_grad
            and Wu.dim() == 2 and Wu.shape == Wv.shape and hasattr(kernels(), 'mgp_uv_fwd'))


def mgp_front(X, Wu, Wv, rows_axis: int, alpha: float, reduce=None):
    """The learned graph of one branch of ``MGP_Gen.forward``: softmax(relu(P - P^T)) with P = sum over (sample, time) of U V^T.  ``reduce``: applied
    to P before the softmax (the batch-sum all-reduce of a sharded batch).  The data window ``X`` gets no gradient: in grad mode an ``X`` that
    requires grad raises ``ValueError`` (``mgp_front_supported`` tells beforehand)."""
    if torch.is_grad_enabled() and X.requires_grad:
        raise ValueError('mgp_front: X requires grad, and this operator returns no gradient for X (detach the data window, or use torch ops)')
    U, V = _MgpUV.apply(X, Wu, Wv, rows_axis, alpha)
    P = U.flatten(1) @ V.flatten(1).t()                                # one plain GEMM over the (slice, hidden) axis; its autograd is two more
    if reduce is not None:
        P = reduce(P)
    return _MgpSoftmax.apply(P)
