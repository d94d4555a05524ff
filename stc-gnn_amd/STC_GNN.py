"""Drop-in for the reference's ``framework/STC_GNN.py``, computing on MI355X.

Put this directory on ``sys.path`` ahead of (or instead of) ``framework/`` and
``from STC_GNN import STCGNN`` (reference ``Model_Trainer.py:5``) resolves
here.  Class names, constructor arguments, ``forward`` signatures, parameter
creation order and ``state_dict`` keys are the reference's
(``STC_GNN.py:5-261``); the arithmetic of the message-passing path -- every
``BDG_Dif``, the gate math of ``STC_Cell`` -- is a sequence of hand-written
HIP kernels (``stc_hip.ops``), not torch ops.  Only the small-N graph
generator ``MGP_Gen`` / ``MixedFusion``, the 16->8->1 output head and the
``torch.stack`` bookkeeping stay on torch.

Beyond the reference:

* ``Gs`` may be a fixed sparse graph (``stc_hip.CsrGraph`` or a torch sparse
  tensor) anywhere a dense ``(N, N)`` tensor is accepted; the reference's dense
  learned ``Gs`` is handled as the full-pattern special case and stays
  differentiable.
* ``STCGNN(..., graph_mode='csr-fixed')`` skips ``MGP_Gen`` (whose
  ``MixedFusion`` holds 2*N^4 parameters and cannot exist beyond N ~ 300) and
  uses ``As`` / ``Ac`` directly as ``Gs`` / ``Gc``.
* ``STCGNN(..., graph_mode='csr-learned', spatial_graph=As, fusion_rank=r)`` learns
  ``Gs`` on the stored entries of the sparse prior graph (``MGP_Gen_Csr``: any N,
  rank-r fusion over nnz); in grad mode its cells run one autograd node per cell.
* ``STCGNN(..., graph_mode='csr-category-learned')`` treats ``As`` exactly as ``'csr-fixed'``
  does and learns the category graph alone (``MGP_Gen_Category``: the generator's category
  branch); at Chebyshev order 2, hidden 16, C in {32, 64} the cells stay in the cell-graph
  executor, whose planar backward forms the gradient of ``Gc``.

Inputs must live on a ROCm device; there is no CPU execution path.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch
from torch import nn

from stc_hip import fusion, learned, ops
from stc_hip.graph import CsrGraph, SpatialOperand, csr_operand, csr_pattern, dense_operand, learned_csr_operand

GraphLike = Union[torch.Tensor, CsrGraph, 'GraphPair']


class GraphPair:
    """The two graphs of one forward pass, prepared once for every BDG_Dif in it.

    ``spatial``: CSR operand of ``Gs`` (both orientations); ``Tc``: (Kc, C, C)
    Chebyshev stack of ``Gc`` (differentiable when ``Gc`` is).
    """

    def __init__(self, Gs, Gc: torch.Tensor, Ks: int, Kc: int):
        if isinstance(Gs, SpatialOperand):                               # prepared by the caller (csr-learned: learned values on a fixed pattern)
            self.spatial: SpatialOperand = Gs
        elif isinstance(Gs, CsrGraph):
            self.spatial = csr_operand(Gs, Gc.device)
        elif isinstance(Gs, torch.Tensor) and Gs.layout != torch.strided:
            self.spatial = csr_operand(_as_csr_graph(Gs), Gc.device)
        elif isinstance(Gs, torch.Tensor):
            self.spatial = dense_operand(Gs)
        else:
            raise TypeError(f'Gs must be a tensor or a CsrGraph, got {type(Gs).__name__}')
        self.Ks, self.Kc = Ks, Kc
        self.Tc = ops.cheby_dense(Gc, Kc)


def _as_csr_graph(Gs: torch.Tensor) -> CsrGraph:
    """The CsrGraph of a torch sparse tensor (COO / CSR), built once and cached on the tensor object."""
    cached = getattr(Gs, '_stc_csr', None)
    if cached is None:
        cached = CsrGraph.from_torch_sparse(Gs)
        try:
            Gs._stc_csr = cached
        except AttributeError:
            pass
    return cached


def _graphs(Gs: GraphLike, Gc: Optional[torch.Tensor], Ks: int, Kc: int) -> GraphPair:
    if isinstance(Gs, GraphPair):
        if (Gs.Ks, Gs.Kc) != (Ks, Kc):
            raise ValueError(f'GraphPair prepared for orders {(Gs.Ks, Gs.Kc)}, layer uses {(Ks, Kc)}')
        return Gs
    return GraphPair(Gs, Gc, Ks, Kc)


class BDG_Dif(nn.Module):
    """Bi-dimensional graph diffusion convolution (reference ``STC_GNN.py:5-47``)."""

    def __init__(self, Ks: int, Kc: int, input_dim: int, hidden_dim: int, use_bias=True, activation=None):
        super().__init__()
        self.Ks, self.Kc = Ks, Kc
        self.input_dim, self.hidden_dim = input_dim, hidden_dim
        self.use_bias = use_bias
        self.activation = None if activation is None else activation()
        self.W = nn.Parameter(torch.empty(input_dim * Ks * Kc, hidden_dim))
        nn.init.xavier_normal_(self.W)
        if use_bias:
            self.b = nn.Parameter(torch.zeros(hidden_dim))

    def forward(self, X: torch.Tensor, Gs: GraphLike, Gc: Optional[torch.Tensor] = None, _pad: int = 0):
        pair = _graphs(Gs, Gc, self.Ks, self.Kc)
        out = ops.bdg_dif(X, pair.spatial, pair.Tc, self.W, self.b if self.use_bias else None, self.Ks, _pad)
        return out if self.activation is None else self.activation(out)


class STC_Cell(nn.Module):
    """GRU-style co-evolution cell (reference ``STC_GNN.py:51-79``)."""

    def __init__(self, num_nodes: int, num_categories: int, Ks: int, Kc: int, input_dim: int, hidden_dim: int,
                 use_bias=True, activation=None):
        super().__init__()
        self.num_nodes, self.num_categories, self.hidden_dim = num_nodes, num_categories, hidden_dim
        self.gates = BDG_Dif(Ks, Kc, input_dim + hidden_dim, hidden_dim * 2, use_bias, activation)
        self.candi = BDG_Dif(Ks, Kc, input_dim + hidden_dim, hidden_dim, use_bias, activation)

    def init_hidden(self, batch_size: int):
        ref = self.gates.W
        return ref.new_zeros(batch_size, self.num_nodes, self.num_categories, self.hidden_dim)

    def forward(self, Gs: GraphLike, Gc: Optional[torch.Tensor], Xt: torch.Tensor, Ht_1: torch.Tensor):
        assert Xt.dim() == 4 and Ht_1.dim() == 4, 'STC-cell must take in 4D tensor as input [Xt, Ht-1]'
        pair = _graphs(Gs, Gc, self.gates.Ks, self.gates.Kc)
        if self.gates.activation is None and self.candi.activation is None:       # always, in the reference's use
            g, c = self.gates, self.candi
            return ops.stc_cell(Xt, Ht_1, pair.spatial, pair.Tc, g.W, g.b if g.use_bias else None,
                                c.W, c.b if c.use_bias else None, g.Ks)
        # a BDG_Dif activation sits between the convolution and the gate math: composed path
        # feature rows are padded with zeros to a multiple of 4 floats (in + hidden = 17 -> 20) so that every
        # (node, category) row is 16-byte aligned for the vector / MFMA kernels; W keeps its reference shape
        pad = -(Xt.shape[-1] + Ht_1.shape[-1]) % 4
        pre = self.gates(ops.concat2(Xt, Ht_1, pad), pair, None, pad)  # (B,N,C,2h) update|reset pre-activations
        update, cand_in = ops.gru_gates(pre, Xt, Ht_1, pad)           # sigmoid, reset*H and the second concat, fused
        cand_pre = self.candi(cand_in, pair, None, pad)
        return ops.gru_blend(cand_pre, update, Ht_1)                  # (1-u)*H + u*tanh(.)


def _per_layer(value, num_layers: int) -> list:
    return value if isinstance(value, list) else [value] * num_layers


class STC_Encoder(nn.Module):
    """Layer-major stack of cells over the observed sequence (reference ``STC_GNN.py:83-135``)."""

    def __init__(self, num_nodes: int, num_categories: int, Ks: int, Kc: int, input_dim: int, hidden_dim,
                 num_layers: int, use_bias=True, activation=None, return_all_layers=True):
        super().__init__()
        self.hidden_dim = _per_layer(hidden_dim, num_layers)
        self.num_layers = num_layers
        self.return_all_layers = return_all_layers
        assert len(self.hidden_dim) == num_layers, 'Input [hidden, layer] length must be consistent'
        self.cell_list = nn.ModuleList(
            STC_Cell(num_nodes, num_categories, Ks, Kc, input_dim if i == 0 else self.hidden_dim[i - 1],
                     self.hidden_dim[i], use_bias=use_bias, activation=activation)
            for i in range(num_layers))

    def _init_hidden(self, batch_size: int):
        return [cell.init_hidden(batch_size) for cell in self.cell_list]

    def forward(self, Gs: GraphLike, Gc: Optional[torch.Tensor], X_seq: torch.Tensor, H0_l=None):
        assert X_seq.dim() == 5, 'STC-encoder must take in 5D tensor as input X_seq'
        per_layer, last = self._run(Gs, Gc, X_seq, H0_l)
        seqs = [torch.stack(outs, dim=1) for outs in per_layer]        # (B, T, N, C, h) per layer, as the reference returns
        if not self.return_all_layers:
            return seqs[-1:], last[-1:]
        return seqs, last

    def _run(self, Gs, Gc, X_seq, H0_l=None):
        """Layer-major, then time.  Layer l reads layer l-1's per-step outputs directly: the reference stacks them
        and slices the stack again (STC_GNN.py:114-115, 111) -- same values, but every slice of a stacked
        tensor costs autograd a full-size zero-fill + add in backward."""
        first = self.cell_list[0].gates
        pair = _graphs(Gs, Gc, first.Ks, first.Kc)
        steps = X_seq.shape[1]
        states = self._init_hidden(X_seq.shape[0]) if H0_l is None else H0_l
        layer_in = [X_seq[:, t] for t in range(steps)]
        per_layer, last = [], []
        for cell, h in zip(self.cell_list, states):
            outs = []
            for x in layer_in:
                h = cell(pair, None, x, h)
                outs.append(h)
            layer_in = outs
            per_layer.append(outs)
            last.append(h)
        return per_layer, last


class STC_Decoder(nn.Module):
    """One autoregressive step through the layer stack (reference ``STC_GNN.py:139-172``)."""

    def __init__(self, num_nodes: int, num_categories: int, Ks: int, Kc: int, output_dim: int, hidden_dim,
                 num_layers: int, out_horizon: int, use_bias=True, activation=None):
        super().__init__()
        self.out_horizon = out_horizon
        self.hidden_dim = _per_layer(hidden_dim, num_layers)
        self.num_layers = num_layers
        assert len(self.hidden_dim) == num_layers, 'Input [hidden, layer] length must be consistent'
        self.cell_list = nn.ModuleList(
            STC_Cell(num_nodes, num_categories, Ks, Kc, output_dim if i == 0 else self.hidden_dim[i - 1],
                     self.hidden_dim[i], use_bias=use_bias, activation=activation)
            for i in range(num_layers))

    def forward(self, Gs: GraphLike, Gc: Optional[torch.Tensor], Xt: torch.Tensor, H0_l: Sequence[torch.Tensor]):
        assert Xt.dim() == 4, 'STC-decoder must take in 4D tensor as input Xt'
        first = self.cell_list[0].gates
        pair = _graphs(Gs, Gc, first.Ks, first.Kc)
        new_states: List[torch.Tensor] = []
        x = Xt
        for cell, h in zip(self.cell_list, H0_l):
            x = cell(pair, None, x, h)
            new_states.append(x)
        return x, new_states


class FactorisedLinear(nn.Module):
    """y = U (V^T x) + b: a rank-r stand-in for ``Linear(d, d)`` with 2 d r + d parameters instead of d^2 + d.

    Not in the reference: its ``MixedFusion`` gates every entry of an n x n graph with two dense
    ``Linear(n^2, n^2)`` layers -- 2 n^4 parameters, 2 x 10^8 at n = 100 and out of reach beyond n ~ 300.  With the
    factors, n = 1000 costs 2 x 32 M parameters at rank 16.  Initialised like ``nn.Linear`` would initialise the product.
    """

    def __init__(self, dim: int, rank: int):
        super().__init__()
        if rank < 1:
            raise ValueError(f'rank must be positive, got {rank}')
        self.dim, self.rank = dim, rank
        bound = (1.0 / dim) ** 0.5
        self.U = nn.Parameter(torch.empty(dim, rank).uniform_(-1, 1) * (bound / rank) ** 0.5)
        self.V = nn.Parameter(torch.empty(dim, rank).uniform_(-1, 1) * (bound / rank) ** 0.5)
        self.bias = nn.Parameter(torch.empty(dim).uniform_(-bound, bound))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.mv(self.U, torch.mv(self.V.t(), x)) + self.bias

    def dense_weight(self) -> torch.Tensor:
        """The (dim, dim) weight this layer stands for (small dims / tests only)."""
        return self.U @ self.V.t()


class MixedFusion(nn.Module):
    """Element-wise gated mix of a prior graph A and a learned graph P (reference ``STC_GNN.py:246-261``).

    Two ``Linear(n^2, n^2)`` layers: usable for small n only.  On the GPU (fp32, n^2 a multiple of 4) the gate's two matrix-vector
    products, the mix and their autograd are ``stc_mixed_fusion_fwd/bwd_f32`` -- the matrices are streamed once per direction; other
    shapes stay on torch.  ``rank`` (not in the reference) replaces the layers by rank-r factors so that a learned graph is affordable
    beyond n ~ 300; on the GPU (fp32, rank <= 64, any n) these run ``stc_mixed_fusion_lr_fwd/bwd_f32`` through ``stc_hip.fusion``, two
    launches per direction; other cases stay on torch.
    """

    def __init__(self, in_dim: int, rank: Optional[int] = None, dim: Optional[int] = None):
        super().__init__()
        self.in_dim = in_dim
        self.dim = dim          # csr-learned: A and P are the dim = nnz stored values of a sparse graph (1-D), gated by rank-r factors over nnz
        if dim is not None:
            if rank is None:
                raise ValueError('MixedFusion over the values of a sparse graph needs a rank (two Linear(nnz, nnz) layers are out of reach)')
            self.lin_A = FactorisedLinear(dim, rank)
            self.lin_P = FactorisedLinear(dim, rank)
        elif rank is None:
            self.lin_A = nn.Linear(in_dim ** 2, in_dim ** 2)
            self.lin_P = nn.Linear(in_dim ** 2, in_dim ** 2)
        else:
            self.lin_A = FactorisedLinear(in_dim ** 2, rank)
            self.lin_P = FactorisedLinear(in_dim ** 2, rank)

    def forward(self, A: torch.Tensor, P: torch.Tensor):
        if self.dim is not None:
            assert A.shape == (self.dim,) and P.shape == (self.dim,)
            params = (self.lin_A.U, self.lin_A.V, self.lin_A.bias, self.lin_P.U, self.lin_P.V, self.lin_P.bias)
            if A.is_cuda and fusion.mixed_fusion_lr_supported(A, P, *params):
                return fusion.mixed_fusion_lr(A, P, *params)
            gate = torch.sigmoid(self.lin_A(A) + self.lin_P(P))
            return gate * A + (1 - gate) * P
        assert A.dim() == 2 and P.dim() == 2
        n = self.in_dim
        if isinstance(self.lin_A, nn.Linear) and A.is_cuda:
            params = (self.lin_A.weight, self.lin_A.bias, self.lin_P.weight, self.lin_P.bias)
            if ops.mixed_fusion_supported(A, P, *params):                # both 2 x n^4-byte matrices streamed once per direction
                return ops.mixed_fusion(A, P, *params)
        elif isinstance(self.lin_A, FactorisedLinear) and A.is_cuda:
            params = (self.lin_A.U, self.lin_A.V, self.lin_A.bias, self.lin_P.U, self.lin_P.V, self.lin_P.bias)
            if fusion.mixed_fusion_lr_supported(A, P, *params):          # two launches per direction (stc_mixed_fusion_lr_fwd/bwd_f32)
                return fusion.mixed_fusion_lr(A, P, *params)
        gate = torch.sigmoid(self.lin_A(A.reshape(n * n)) + self.lin_P(P.reshape(n * n))).reshape(n, n)
        return gate * A + (1 - gate) * P


class MGP_Gen(nn.Module):
    """Learned mixed graph pair (Gs, Gc) from the input window (reference ``STC_GNN.py:210-243``)."""

    def __init__(self, num_nodes: int, num_categories: int, hidden_dim: int, alpha: int = 3, fusion_rank: Optional[int] = None):
        super().__init__()
        self.alpha = alpha
        self.batch_sharded = False      # True: the batch is split over ranks -> all-reduce the batch-summed pre-activation
        self.params_S = self.init_params(num_categories, hidden_dim)
        self.aggreg_S = MixedFusion(num_nodes, fusion_rank)         # only the N x N fusion is the 2 N^4 problem
        self.params_C = self.init_params(num_nodes, hidden_dim)
        self.aggreg_C = MixedFusion(num_categories)

    @staticmethod
    def init_params(in_dim: int, hidden_dim: int):
        params = nn.ParameterDict()
        for key in ('Wu', 'Wv'):
            params[key] = nn.Parameter(torch.randn(in_dim, hidden_dim))
        for p in params.values():
            nn.init.xavier_normal_(p)
        return params

    def _learned(self, X: torch.Tensor, params, rows_axis: int) -> torch.Tensor:
        reduce = None
        if self.batch_sharded:
            from stc_hip.dist import allreduce_sum
            reduce = allreduce_sum                                    # exact under batch sharding
        if ops.mgp_front_supported(X, params['Wu'], params['Wv']):    # three launches forward, six backward per branch instead of ~30
            return ops.mgp_front(X, params['Wu'], params['Wv'], rows_axis, float(self.alpha), reduce)
        if rows_axis == 3:
            X = X.transpose(2, 3)
        U = torch.tanh(self.alpha * torch.matmul(X, params['Wu']))
        V = torch.tanh(self.alpha * torch.matmul(X, params['Wv']))
        flat_u, flat_v = U.flatten(0, 1), V.flatten(0, 1)             # sum over batch and time
        P = torch.einsum('knh,kmh->nm', flat_u, flat_v)
        if reduce is not None:
            P = reduce(P)
        return torch.softmax(torch.relu(P - P.t()), dim=-1)

    def forward(self, X_seq: torch.Tensor, As: torch.Tensor, Ac: torch.Tensor):
        Gs = self.aggreg_S(As, self._learned(X_seq, self.params_S, 2))
        Gc = self.aggreg_C(Ac, self._learned(X_seq, self.params_C, 3))
        return Gs, Gc


class MGP_Gen_Csr(MGP_Gen):
    """``MGP_Gen`` with the spatial graph learned on the stored entries of a sparse prior graph (``graph_mode='csr-learned'``; not in the
    reference, whose learned ``Gs`` is a dense (N, N) matrix): the score ``<u_i, v_j> - <v_i, u_j>`` at the entries (i, j) of ``graph``, a
    softmax over every row's stored entries, and a rank-r ``MixedFusion`` over the nnz values (``stc_hip.learned``, ``stc_hip.fusion``).  The
    category branch is ``MGP_Gen``'s.  Same attribute and key names as ``MGP_Gen``; parameter order follows the entry order of ``graph``
    (CSR of Gs, rows ascending, columns ascending), so on the full pattern a ``state_dict`` of ``MGP_Gen(..., fusion_rank=r)`` loads unchanged
    and gives the same graphs.  ``forward`` returns (a ``SpatialOperand`` with the learned values, Gc)."""

    DEFAULT_RANK = 16

    def __init__(self, graph: CsrGraph, num_categories: int, hidden_dim: int, alpha: int = 3, fusion_rank: Optional[int] = None):
        nn.Module.__init__(self)
        if not isinstance(graph, CsrGraph) or graph.nnz == 0:
            raise ValueError('MGP_Gen_Csr needs the prior graph as a CsrGraph with at least one stored entry')
        self.alpha = alpha
        self.batch_sharded = False
        self.sampled_grad = False                                   # put on the operand ``forward`` returns (STCGNN sets it from ``csr_cells``)
        self.graph = graph                                          # the pattern (and the default prior values): not a parameter, not in the state_dict
        self.params_S = self.init_params(num_categories, hidden_dim)
        self.aggreg_S = MixedFusion(graph.n, self.DEFAULT_RANK if fusion_rank is None else fusion_rank, dim=graph.nnz)
        self.params_C = self.init_params(graph.n, hidden_dim)
        self.aggreg_C = MixedFusion(num_categories)

    def _same_pattern(self, As: CsrGraph) -> bool:
        if As is self.graph:
            return True
        if getattr(As, '_stc_same_pattern_as', None) is not self.graph:         # compared once per graph object
            a, b = As._host, self.graph._host
            if As.n != self.graph.n or As.nnz != self.graph.nnz or not ((a['bwd_rowptr'] == b['bwd_rowptr']).all() and (a['bwd_colidx'] == b['bwd_colidx']).all()):
                return False
            As._stc_same_pattern_as = self.graph
        return True

    def forward(self, X_seq: torch.Tensor, As: CsrGraph, Ac: torch.Tensor):
        if not isinstance(As, CsrGraph) or not self._same_pattern(As):
            raise ValueError('csr-learned: As must be a CsrGraph with the sparsity pattern the model was built on (the parameters are per stored entry)')
        pattern = csr_pattern(self.graph, X_seq.device)
        reduce = None
        if self.batch_sharded:
            from stc_hip.dist import allreduce_sum
            reduce = allreduce_sum
        Ps = learned.mgp_csr_front(X_seq, self.params_S['Wu'], self.params_S['Wv'], pattern, float(self.alpha), reduce)
        G = self.aggreg_S(As.on(X_seq.device)['bwd_val'].to(Ps.dtype), Ps)    # (fp32 on the device; a float64 module on the CPU in tests)
        Gc = self.aggreg_C(Ac, self._learned(X_seq, self.params_C, 3))
        return learned_csr_operand(self.graph, G, self.sampled_grad), Gc


class MGP_Gen_Category(MGP_Gen):
    """The category branch of ``MGP_Gen`` alone (``graph_mode='csr-category-learned'``; not in the reference): ``Gc = MixedFusion(C)(Ac, P_c)`` with
    ``P_c`` from the input window, for a spatial graph that stays fixed -- no N x N fusion exists.  Only ``params_C`` and ``aggreg_C``, under
    the reference's key names and created in the reference's relative order, so those entries of an ``MGP_Gen`` ``state_dict`` load unchanged.
    ``forward(X_seq, Ac)`` returns ``Gc``; ``X_seq`` in the node order the parameters were built for (``params_C`` has one row per node)."""

    def __init__(self, num_nodes: int, num_categories: int, hidden_dim: int, alpha: int = 3):
        nn.Module.__init__(self)
        self.alpha = alpha
        self.batch_sharded = False
        self.params_C = self.init_params(num_nodes, hidden_dim)
        self.aggreg_C = MixedFusion(num_categories)

    def forward(self, X_seq: torch.Tensor, Ac: torch.Tensor):
        return self.aggreg_C(Ac, self._learned(X_seq, self.params_C, 3))


class STCGNN(nn.Module):
    """Encoder-decoder STC-GNN (reference ``STC_GNN.py:175-207``); the drop-in boundary.

    ``graph_mode='csr-learned'`` (not in the reference): the spatial graph is learned on the stored entries of the sparse prior graph, which
    the CONSTRUCTOR takes as ``spatial_graph`` (a ``CsrGraph`` or a torch sparse tensor): the fusion's parameters are per stored entry, so nnz
    is needed before the first forward pass, and a ``state_dict`` must be loadable into a freshly built model.  ``forward`` is then given a
    graph with the same pattern (usually the same object) whose values are the prior.  ``fusion_rank`` defaults to 16; nodes are not
    renumbered (entry order defines parameter order); float32 storage only.  In grad mode the cells run one autograd node per cell (the
    general path: the graph values need a gradient); under ``no_grad`` they take whatever route the predicates give a fixed sparse graph.
    ``csr_cells='fused'`` (csr-learned only; default ``'per-cell'``) prefers the few-category cell executor in grad mode too, which forms the
    value gradient at the stored entries (``stc_graph_grad_csr_f32``): Chebyshev order 2, hidden 16, C <= 16 on the HIP kernel set.  At C in
    {32, 64} (order 2, hidden 16, fp32) ``'fused'`` runs the general cell-graph executor as ONE autograd node that forms both gradients: the
    spatial values' at the stored entries from its planar cells (``stc_graph_grad_csr_pairs_f32``, ``ops._dval_route``) and ``Gc``'s Chebyshev
    stack's (``learn_Tc=True``).  Where both executors decline, the per-cell path runs with the same bits as ``'per-cell'``.

    ``graph_mode='csr-category-learned'`` (not in the reference): ``As`` is handled exactly as in ``'csr-fixed'`` (``CsrGraph`` or torch sparse
    tensor, ``reorder_nodes``, plans); the category graph is ``MixedFusion(C)(Ac, P_c)`` from ``MGP_Gen_Category``, with ``P_c`` computed from
    the window in the caller's node order, before any renumbering.  In grad mode the cells ask the cell-graph executor for the gradient of
    ``Gc``'s Chebyshev stack (``ops.stc_cell_graph(learn_Tc=True)``: order 2, hidden 16, C in {32, 64}, fp32); other shapes run one autograd
    node per cell.  Under ``no_grad`` the route is ``'csr-fixed'``'s."""

    def __init__(self, num_nodes: int, num_categories: int, Ks: int, Kc: int, input_dim: int, hidden_dim: int,
                 num_layers: int, out_horizon: int, use_bias=True, activation=None,
                 graph_mode: str = 'dense-learned', reorder_nodes: bool = True, batch_sharded: bool = False,
                 fusion_rank: Optional[int] = None, storage_dtype: torch.dtype = torch.float32, spatial_graph=None,
                 csr_cells: str = 'per-cell'):
        super().__init__()
        if csr_cells not in ('per-cell', 'fused'):
            raise ValueError("csr_cells must be 'per-cell' (one autograd node per cell) or 'fused' (the few-category cell executor)")
        if csr_cells == 'fused' and graph_mode != 'csr-learned':
            raise ValueError("csr_cells='fused' needs graph_mode='csr-learned' (the other modes choose their cell route themselves)")
        self.csr_cells = csr_cells              # read at every forward
        if graph_mode not in ('dense-learned', 'csr-fixed', 'csr-learned', 'csr-category-learned'):
            raise ValueError("graph_mode must be 'dense-learned' (reference semantics), 'csr-fixed', 'csr-learned' or 'csr-category-learned'")
        if storage_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('storage_dtype must be torch.float32 (reference arithmetic) or torch.bfloat16')
        if storage_dtype == torch.bfloat16 and graph_mode != 'csr-fixed':
            raise ValueError("storage_dtype=torch.bfloat16 needs graph_mode='csr-fixed' (BASELINE configuration 5)")
        # bfloat16: states, gates and their gradients are stored in bf16 (fp32 parameters, fp32 sums inside every kernel);
        # not reference behaviour (the reference is fp32-only) -- the large-N configuration's memory / bandwidth option
        self.storage_dtype = storage_dtype
        self.graph_mode = graph_mode
        self.reorder_nodes = reorder_nodes      # csr-fixed + CsrGraph: renumber nodes internally when that restores locality
        self.Ks, self.Kc = Ks, Kc
        if graph_mode == 'dense-learned':
            self.mix_graph_pair = MGP_Gen(num_nodes, num_categories, hidden_dim, fusion_rank=fusion_rank)   # rank: SURVEY 8(f3)
            self.mix_graph_pair.batch_sharded = batch_sharded
        elif graph_mode == 'csr-learned':
            if isinstance(spatial_graph, torch.Tensor) and spatial_graph.layout != torch.strided:
                spatial_graph = _as_csr_graph(spatial_graph)
            if not isinstance(spatial_graph, CsrGraph):
                raise ValueError("graph_mode='csr-learned' needs spatial_graph=: the prior graph As as a CsrGraph or a torch sparse tensor "
                                 '(its stored entries are the pattern the graph is learned on)')
            if spatial_graph.n != num_nodes:
                raise ValueError(f'spatial_graph has {spatial_graph.n} nodes, the model {num_nodes}')
            self.mix_graph_pair = MGP_Gen_Csr(spatial_graph, num_categories, hidden_dim, fusion_rank=fusion_rank)
            self.mix_graph_pair.batch_sharded = batch_sharded
        elif graph_mode == 'csr-category-learned':
            self.mix_graph_pair = MGP_Gen_Category(num_nodes, num_categories, hidden_dim)
            self.mix_graph_pair.batch_sharded = batch_sharded
        self.encoder = STC_Encoder(num_nodes, num_categories, Ks, Kc, input_dim, hidden_dim, num_layers,
                                   use_bias, activation, return_all_layers=True)
        self.decoder = STC_Decoder(num_nodes, num_categories, Ks, Kc, hidden_dim, hidden_dim, num_layers,
                                   out_horizon, use_bias, activation)
        self.out_proj = nn.Sequential(nn.Linear(hidden_dim, hidden_dim // 2, bias=use_bias),
                                      nn.Linear(hidden_dim // 2, input_dim, bias=use_bias))

    def prepare_graph(self, graph: CsrGraph, device=None) -> CsrGraph:
        """Do at set-up time what ``forward`` would otherwise do on the first step for a ``CsrGraph`` in ``csr-fixed`` mode: the
        host-side locality analysis (reverse Cuthill-McKee, needs scipy; skipped with a warning without it), the renumbered
        copy when it pays, and the upload of the CSR / row-blocked arrays.  Returns ``graph`` (pass the same object to forward)."""
        g = graph.with_locality()[0] if self.reorder_nodes else graph
        if device is not None:
            g.on(torch.device(device))
        return graph

    def forward(self, X_seq: torch.Tensor, As: GraphLike, Ac: torch.Tensor):
        assert X_seq.dim() == 4, 'STC-GNN must take in 4D tensor as input X_seq'
        inv = None
        if self.graph_mode == 'dense-learned':
            Gs, Gc = self.mix_graph_pair(X_seq, As, Ac)
        elif self.graph_mode == 'csr-learned':
            if isinstance(As, torch.Tensor) and As.layout != torch.strided:
                As = _as_csr_graph(As)
            self.mix_graph_pair.sampled_grad = self.csr_cells == 'fused'
            Gs, Gc = self.mix_graph_pair(X_seq, As, Ac)                  # Gs: a SpatialOperand on the prior's pattern, in the given node order
        else:
            # csr-category-learned: Gc from the window as the caller gave it (the generator's parameters are per node, in the caller's order)
            Gs, Gc = As, (self.mix_graph_pair(X_seq, Ac) if self.graph_mode == 'csr-category-learned' else Ac)
            if isinstance(Gs, torch.Tensor) and Gs.layout != torch.strided:
                Gs = _as_csr_graph(Gs)                  # a torch sparse graph gets the same treatment as a CsrGraph (cached on the tensor)
            if self.reorder_nodes and isinstance(Gs, CsrGraph):
                # a graph given in a cache-hostile node order is renumbered once (reverse Cuthill-McKee); inputs are
                # gathered into that order here and the prediction scattered back, so callers never see it
                Gs, order = Gs.with_locality()
                if order is not None:
                    idx = getattr(Gs, '_order_dev', {}).get(X_seq.device)
                    if idx is None:
                        o = torch.from_numpy(order).to(X_seq.device)
                        idx = (o, torch.argsort(o))
                        Gs._order_dev = {**getattr(Gs, '_order_dev', {}), X_seq.device: idx}
                    X_seq = X_seq.index_select(2, idx[0])
                    inv = idx[1]
        pair = _graphs(Gs, Gc, self.Ks, self.Kc)
        stacked = self._run_cell_graph(pair, X_seq.unsqueeze(-1).to(self.storage_dtype))
        if stacked is None and self.storage_dtype != torch.float32:
            raise ValueError('storage_dtype=torch.bfloat16: shape outside the bf16 cell kernels (Ks = Kc = 2, hidden 16, C in {32, 64}, input_dim <= 4)')
        if stacked is not None:
            y = self._head(stacked).transpose(0, 1)                       # (horizon, B, N, C) -> (B, horizon, N, C), a view
        else:                                                             # general path: one autograd node per cell
            _, states = self.encoder._run(pair, None, X_seq.unsqueeze(-1))     # per-layer output stacks are not needed here
            step_in = states[-1]
            outs = []
            for _ in range(self.decoder.out_horizon):
                step_in, states = self.decoder(pair, None, step_in, states)
                outs.append(step_in)
            y = self._head(torch.stack(outs, dim=1))                     # (B, horizon, N, C)
        return y if inv is None else y.index_select(2, inv)

    def _run_cell_graph(self, pair: GraphPair, X: torch.Tensor):
        """Encoder and decoder as ONE autograd node (``ops.stc_cell_graph``) when the kernels allow it: fixed graphs,
        hidden 16 on the matrix-core shapes, no BDG_Dif activation.  Same cells, same order, same values as the general
        path; what changes is that no concat pass and no gradient-accumulation pass runs between the cells.
        Returns the decoder's top-layer states of all horizon steps, (horizon, B, N, C, h), or None when the general path
        must be used."""
        enc, dec = self.encoder.cell_list, self.decoder.cell_list
        cells = list(enc) + list(dec)
        hidden = {c.hidden_dim for c in cells}
        if len(hidden) != 1 or any(c.gates.activation is not None or c.candi.activation is not None for c in cells):
            return None
        h = hidden.pop()
        B, T, N, C, cin0 = X.shape
        # csr-category-learned: the executor is asked for Gc's gradient (it has none to give under no_grad); the other modes call as they always did
        # csr-learned with csr_cells='fused': both graphs are learned -- the executor is asked for Gc's gradient too (C in {32, 64}; ``ops._dval_route``)
        fused = self.graph_mode == 'csr-learned' and self.csr_cells == 'fused'
        learn = dict(learn_Tc=True) if self.graph_mode == 'csr-category-learned' or fused else {}
        if X.requires_grad or not ops.cell_graph_supported(pair.spatial, pair.Tc, self.Ks, C, h, [cin0, h], dtype=X.dtype, **learn):
            return None
        n_layers, horizon = len(enc), self.decoder.out_horizon
        # inputs, then the zero initial states -- as shapes only where the executor runs their cells in the first-step forms (no plane is read)
        if ops.first_step_route(pair.spatial, pair.Tc, self.Ks, C, h, [cin0, h], dtype=X.dtype, **learn):
            ext = [X[:, t] for t in range(T)] + [ops.zero_state(c.gates.W, (B, c.num_nodes, c.num_categories, c.hidden_dim), X.dtype) for c in enc]
        else:
            ext = [X[:, t] for t in range(T)] + [c.init_hidden(B).to(X.dtype) for c in enc]
        eid = lambda l, t: l * T + t                                                    # encoder: layer-major, then time
        did = lambda l, s_: n_layers * T + s_ * n_layers + l                            # decoder: step-major, then layer
        schedule = []
        for l in range(n_layers):
            for t in range(T):
                x = ('ext', t) if l == 0 else ('cell', eid(l - 1, t))
                hs = ('ext', T + l) if t == 0 else ('cell', eid(l, t - 1))
                schedule.append((l, x, hs))
        for s_ in range(horizon):
            for l in range(n_layers):
                top_prev = eid(n_layers - 1, T - 1) if s_ == 0 else did(n_layers - 1, s_ - 1)
                x = ('cell', top_prev) if l == 0 else ('cell', did(l - 1, s_))
                hs = ('cell', eid(l, T - 1) if s_ == 0 else did(l, s_ - 1))
                schedule.append((n_layers + l, x, hs))
        stacks = [(c.gates.W, c.gates.b if c.gates.use_bias else None, c.candi.W, c.candi.b if c.candi.use_bias else None) for c in cells]
        outputs = [did(n_layers - 1, s_) for s_ in range(horizon)]
        return ops.stc_cell_graph(pair.spatial, pair.Tc, self.Ks, schedule, outputs, ext, stacks, **learn)

    def _head(self, H: torch.Tensor) -> torch.Tensor:
        """sigmoid(out_proj(H)).squeeze(-1) (reference STC_GNN.py:206-207).  The two Linears have no nonlinearity
        between them, so they are folded into one h -> 1 map (two tiny matmuls, differentiable) and the
        streaming part runs in one fused HIP kernel instead of two skinny GEMMs."""
        lin1, lin2 = self.out_proj[0], self.out_proj[1]
        h = lin1.in_features
        if lin2.out_features != 1 or h % 4 or h > 64 or (H.dtype == torch.bfloat16 and h != 16):
            return torch.sigmoid(self.out_proj(H.float())).squeeze(dim=-1)
        w = (lin2.weight @ lin1.weight).reshape(h)
        if lin1.bias is not None:
            b = lin2.weight @ lin1.bias + lin2.bias
        else:
            b = w.new_zeros(1)
        return ops.head(H, w, b)
