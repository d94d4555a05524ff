"""A schedule of STC_Cells with FEW CATEGORIES (C <= 16: the SF-incidents shape and its relatives) as one autograd node.

The SF-incidents shape (N = 100, C = 5, hidden 16) is bound by the host's launch rate on the general path (~15 launches
per cell and direction).  ``stc_cell_small_fwd/bwd_f32`` run a whole cell step -- both aggregations, both convolutions, the gate math
and the blend (reference STC_GNN.py:65-79) -- in one launch with one workgroup per sample; this module is the bookkeeping around them,
with the same interface as ``ops.stc_cell_graph``:

  * states, gates and the saved aggregates of all cells live in a handful of stacked buffers (one allocation per kind and pass);
  * a state's gradient is ONE buffer that its consumer cells write / add to in place (``accumulate_x`` / ``accumulate_h`` of the
    backward kernel), in reverse schedule order -- no autograd accumulation passes;
  * parameter gradients are partial sums (one row per sample and wave) that every cell of a parameter set adds to; one sum over the
    rows per backward pass.
Learned graphs (the reference's own mode: dense Gs from MGP_Gen, Gc through its Chebyshev stack): the gradients of Gs and Gc are sums over
ALL cells of a step, so the launches only leave their operands (the slab [H | X | 0], the gradients of the two aggregated slabs, the gate
pre-activation gradients) and the backward forms  dGs^T = sum_cells dZ_1 x Z_0  and  dT_c = sum_cells V_c x dY  as a few stacked
products per parameter set at the end -- not per cell.  At Chebyshev order 3 the second matrix T_2 = 2 V V - I (V = Gs^T) is formed OUTSIDE the
node with differentiable torch ops and handed in as a second values tensor: the node returns  dT_2 = sum_cells dZ_2 x Z_0  beside d fwd_val,
and torch's autograd carries it through the N x N product to Gs.
A pass that no backward follows (``torch.no_grad()``, or nothing requires grad) skips the node: ``_forward_only`` runs the same launches on one
shared set of scratch planes, keeps no state beyond its last reader and leaves R / Cand unstored (``stc_small_graph`` picks the route).
"""
from __future__ import annotations

import weakref

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .graph import SpatialOperand

H16 = 16


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def small_graph_supported(k, op: SpatialOperand, Tc, Ks: int, C: int, h: int, x_widths, dtype=torch.float32) -> bool:
    """Fixed graphs, or the reference's learned ones: a learned spatial graph must be dense (values = the full N x N pattern, as
    ``graph.dense_operand`` builds it) -- its gradient is formed as a dense product.  A learned graph on a SPARSE pattern
    (``graph.learned_csr_operand``) is taken only where the caller asked for it (``op.sampled_grad``: ``STCGNN(csr_cells='fused')``), at
    Chebyshev order 2, by a kernel set with the sampled product (``graph_grad_csr``); its gradient is formed at the stored entries."""
    if dtype != torch.float32 or not hasattr(k, 'cell_small_supported'):
        return False
    if op.fwd_val.requires_grad and op.nnz != op.n * op.n and not (op.sampled_grad and Ks == 2 and hasattr(k, 'graph_grad_csr')):
        return False
    full = op.nnz == op.n * op.n
    # the graph as the learned mode hands it over: full pattern, requiring grad -- or, with grad mode off (evaluation: the generator's Gs does
    # not require grad there), the same graph as it arrives then
    as_learned = full and (op.fwd_val.requires_grad or (not torch.is_grad_enabled() and op.source is None))
    # rows per sample that a dense graph may have: what the LDS stages -- or, where the kernel set runs the split launches on global memory and
    # the blocked graph gradient (``small_dense_split``), its measured bound
    dense_rows = max(k.SMALL_STAGED_ROWS, k.SMALL_DENSE_ROWS) if as_learned and getattr(k, 'small_dense_split', False) else k.SMALL_STAGED_ROWS
    if Ks == 3:                                                     # order 3: T_2(S) as a second graph --
        # a learned full-pattern graph (T_2 dense, split launches) where the kernel set takes one; with grad mode off the same graph as it
        # arrives then -- in grad mode a dense graph that needs no gradient keeps the general path
        if op.fwd_val.requires_grad or (not torch.is_grad_enabled() and op.source is None and full):
            if not getattr(k, 'small_dense_order3', False) or op.n * C > dense_rows:
                return False
        elif op.source is None or full:                             # else fixed sparse graphs (CsrGraph.second_order)
            return False
    if full and op.n * C > dense_rows:
        return False                                                # a dense graph aggregates as a matrix product on the STAGED plane: the sample must fit the LDS
    if op.n * C > k.SMALL_PREFERRED_ROWS or (C == 16 and op.n * C > 4096):
        return False                                                # (16 categories on large graphs: the general path's fp32-MFMA node kernels win, 13.4 vs 18.3 ms)
    return all(k.cell_small_supported(Ks, Tc.shape[0], C, w, h, op.n) for w in set(x_widths))


# ---- what both cell-graph executors (this one and ``ops._StcCellGraph``) share
def _alias(base: torch.Tensor, i=None) -> torch.Tensor:
    """``base`` (or base[i]) as a tensor of its own that shares the storage WITHOUT being a view of ``base`` in autograd's books: saved for
    backward while ``base`` is the node's output, which view tracking forbids."""
    off, shape, stride = (0, base.shape, base.stride()) if i is None else (i * base.stride(0), base.shape[1:], base.stride()[1:])
    t = base.new_empty(0)
    t.set_(base.untyped_storage(), base.storage_offset() + off, shape, stride)
    return t


def _stacks(flat):
    """[(Wg, bg, Wc, bc)] per parameter set from their flat sequence (absent biases: None, saved for backward as such)."""
    return [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)]


def _unpack(n_ext: int, Tc, fwd_val, tensors):
    """(ext, stacks, Tc, fwd_val), contiguous, from an executor's arguments: the external tensors, then the parameter sets' flat sequence."""
    return [_c(t) for t in tensors[:n_ext]], _stacks([None if p is None else _c(p) for p in tensors[n_ext:]]), _c(Tc), _c(fwd_val)


def _out_slots(outputs):                                        # output cell -> its slot in the returned stack
    out_slot = {j: i for i, j in enumerate(outputs)}
    if len(out_slot) != len(outputs):
        raise ValueError('stc_cell_graph: duplicate output cells')
    return out_slot


def _guard(ctx, out_stack):
    """The saved states of the output cells ALIAS the returned stack's storage without sharing its autograd version counter: the stack is
    read-only for its consumers; ``_check_guard`` checks its version in backward (weak: no output -> ctx -> output cycle)."""
    ctx.out_stack_ref, ctx.out_stack_version = weakref.ref(out_stack), out_stack._version


def _check_guard(ctx):
    stack = ctx.out_stack_ref()
    if stack is not None and stack._version != ctx.out_stack_version:
        raise RuntimeError('stc_cell_graph: the returned state stack was modified in place after the forward pass; the states saved for '
                           'backward share its storage (treat the stack as read-only, or clone it before editing)')


def _refuse_differentiable(**named):
    """Both cell-graph executors return no gradient for some of their arguments (the external tensors; on the general executor the graphs
    too): in grad mode one of them that requires grad is refused here, before any launch, by name -- its gradient would otherwise be
    dropped without a word while the output still requires grad.  ``named``: argument name -> tensor or sequence of tensors."""
    if not torch.is_grad_enabled():
        return
    for name, value in named.items():
        for i, t in enumerate(value if isinstance(value, (list, tuple)) else [value]):
            if t is not None and t.requires_grad:
                which = f'{name}[{i}]' if isinstance(value, (list, tuple)) else name
                raise ValueError(f'stc_cell_graph: {which} requires grad, and this operator returns no gradient for {name} '
                                 '(detach it, or run the cells one by one through stc_cell, which differentiates every input)')


def wavefront(schedule):
    """The cells by level (longest path from the external tensors), schedule order inside a level: a topological order of the same graph in
    which a state's consumers follow it closely -- the encoder's schedule is layer-major, so in ITS order every state of a layer lives until
    the next layer has run (one state and one aggregation per observed step); by level, a constant number of them.  A cell's launches read
    the same operands in either order: same bits."""
    level = []
    for _, x, hs in schedule:
        level.append(1 + max([level[src[1]] for src in (x, hs) if src[0] == 'cell'], default=0))
    return sorted(range(len(schedule)), key=lambda j: (level[j], j))


def last_uses(schedule, order):
    """source -> the cell after whose launches nothing in ``order`` reads it any more."""
    last = {}
    for j in order:
        last[schedule[j][1]] = last[schedule[j][2]] = j
    return last


def _checked_shapes(op, Ks, schedule, ext, stacks, Tc):
    """((B, N, C), input width of every cell) of a few-category schedule, its operands checked (the per-cell launches skip the wrapper's checks)."""
    ref = ext[0]
    B, N, C = ref.shape[:3]
    cin = [ext[x[1]].shape[-1] if x[0] == 'ext' else H16 for _, x, _ in schedule]
    for t in ext:
        if t.shape[:3] != (B, N, C) or t.dtype != torch.float32 or t.device != ref.device:
            raise ValueError(f'stc_cell_graph: external tensors must be float32 (B, N, C, *) on one device, got {tuple(t.shape)} {t.dtype}')
    if N != op.n or Tc.shape[1:] != (C, C):
        raise ValueError(f'stc_cell_graph: graphs are for N={op.n}, C={Tc.shape[1]}; got N={N}, C={C}')
    for (s_id, _, hs), w in zip(schedule, cin):
        Wg, bg, Wc, bc = stacks[s_id]
        rows = Ks * Tc.shape[0] * (w + H16)
        if Wg.shape != (rows, 2 * H16) or Wc.shape != (rows, H16) or (hs[0] == 'ext' and ext[hs[1]].shape[-1] != H16):
            raise ValueError(f'stc_cell_graph: parameter set {s_id} does not fit an input of {w} + {H16} columns')
    return (B, N, C), cin


def _layout(schedule, cin, n_cells, outputs):
    """Where every cell's tensors live: slot in the output stack or the inner-state buffer, position inside its width group (cells whose
    input is 16 columns wide / 1..4 columns wide keep their aggregates in two buffers of different row widths)."""
    out_slot = _out_slots(outputs)
    pos, counts, inner_slot, nxt = [None] * n_cells, [0, 0], {}, 0
    # inside a width group the cells of ONE parameter set sit side by side (set by set, each in schedule order): the products over a set's
    # cells -- the learned graphs' dT_c through stc_mix_dt_f32 -- then take one contiguous run of planes (in schedule order the decoder's two
    # layers interleave)
    for j in sorted(range(n_cells), key=lambda j: (schedule[j][0], j)):
        wide = cin[j] == H16
        pos[j] = (wide, counts[wide])
        counts[wide] += 1
    for j in range(n_cells):
        if j not in out_slot:
            inner_slot[j] = nxt
            nxt += 1
    return out_slot, inner_slot, pos, counts


class _Buffers:
    """The stacked buffers of a pass, by name.  Of every cell, indexed [cell]: the planes U, R, Cand, RH, Zc (order 3: + Zc2 = T_2(S).(R*H)).  Per
    width group w (``_layout``), indexed [w][position]: the slabs Zg and -- learned graphs: what the graph-gradient products read -- Z0, Z0c, Z1c;
    at order 3 the third slabs Zg2 = T_2(S).[H | Xt | 0] and (learned) Z2c.  In the backward (``saved``: the forward's planes and slabs), for
    learned graphs, what its launches leave (zeros where a cell is never reached): the gradients of the aggregated slabs dZ1c, dZ1g (order 3:
    dZ2c, dZ2g) and the gate / candidate pre-activation gradients dYg, dYc.  A slot that the pass does not have is None."""
    def __init__(self, k, Ks, learned, counts, dims, n_cells, like, saved=None):
        B, N, C = self.dims = dims
        self.Ks, self.counts, o3, cells = Ks, counts, Ks == 3, [max(1, c) for c in counts]
        if saved is None:
            self.planes = like.new_empty(6 if o3 else 5, n_cells, B, N, C, H16)
            n_slabs = (4 if learned else 1) + o3 * (2 if learned else 1)
            self.slabs = [like.new_empty(n_slabs, cells[w], B, N * C, k.cell_small_zg_width((1, H16)[w])) for w in (0, 1)]
        else:
            self.planes, *self.slabs = saved
        per_slot = lambda stacked: iter(zip(*(st.unbind(0) for st in stacked)))      # slot by slot: (narrow group's, wide group's)
        slots = per_slot(self.slabs)
        self.Zg, self.Z0, self.Z0c, self.Z1c = (next(slots), next(slots), next(slots), next(slots)) if learned else (next(slots), None, None, None)
        self.Zg2 = next(slots) if o3 else None
        self.Z2c = next(slots) if o3 and learned else None
        self.dZ1c = self.dZ1g = self.dZ2c = self.dZ2g = self.dYg = self.dYc = None
        if saved is not None and learned:
            slots = per_slot([like.new_zeros(4 if o3 else 2, cells[w], B, N * C, self.slabs[w].shape[-1]) for w in (0, 1)])
            self.dZ1c, self.dZ1g, self.dZ2c, self.dZ2g = (*slots, None, None)[:4]
            self.dYg, self.dYc = ([like.new_zeros(cells[w], B, N * C, width) for w in (0, 1)] for width in (2 * H16, H16))
        self.U, self.R, self.Cand, self.RH, self.Zc, self.Zc2 = (*(p.unbind(0) for p in self.planes.unbind(0)), None)[:6]

    def _cell(self, j, pos, graph2, **learned):                      # learned: the learned graphs' share of a launch, by argument name
        (B, N, C), (w, i) = self.dims, pos
        order3 = dict(graph2=graph2, Zg2=self.Zg2[w][i], Zc2=self.Zc2[j].view(B, N * C, H16)) if self.Ks == 3 else {}
        return dict(U=self.U[j], R=self.R[j], Cand=self.Cand[j], RH=self.RH[j], Zg=self.Zg[w][i], Zc=self.Zc[j].view(B, N * C, H16),
                    **{name: s[w][i] for name, s in learned.items() if s is not None}, **order3)

    def fwd_args(self, j, pos, graph2):                              # cell j's buffers as keyword arguments of ``cell_small_fwd``
        return self._cell(j, pos, graph2, Z0=self.Z0, Z0c=self.Z0c, Z1c=self.Z1c, Z2c=self.Z2c)

    def bwd_args(self, j, pos, graph2):                              # ... of ``cell_small_bwd``
        return self._cell(j, pos, graph2, dZ1c=self.dZ1c, dZ1g=self.dZ1g, dZ2c=self.dZ2c, dZ2g=self.dZ2g, dYg=self.dYg, dYc=self.dYc)


def _graph2(op, Ks, t2, device, direction):
    """Order 3's T_2(S) for ``direction`` ('fwd' / 'bwd'): the full pattern with the dense ``t2``, else the fixed graph's own; order 2: None."""
    if Ks == 3 and t2 is not None:
        return getattr(op, direction + '_rowptr'), getattr(op, direction + '_colidx'), t2
    g2 = op.source.second_order(device) if Ks == 3 else None
    return g2 and tuple(g2[f'{direction}2_{part}'] for part in ('rowptr', 'colidx', 'val'))


def _slab_order(W, Ks, Kc, cw, LP):
    """W (..., Ks * Kc * (cw + 16), Ho) as (..., Ks, Kc, LP, Ho) with its rows in the slabs' column order [H (16) | X (cin) | 0]."""
    Wv = W.view(*W.shape[:-2], Ks, Kc, cw + H16, W.shape[-1])
    Wp = Wv.new_zeros(*Wv.shape[:-2], LP, W.shape[-1])
    Wp[..., :H16, :] = Wv[..., cw:, :]
    Wp[..., H16:H16 + cw, :] = Wv[..., :cw, :]
    return Wp


class _StcSmallGraph(Function):
    """schedule[j] = (stack, ('ext', i) | ('cell', k), ('ext', i) | ('cell', k)): parameter set, source of Xt, source of H."""

    @staticmethod
    def forward(ctx, k, op: SpatialOperand, Ks: int, schedule, outputs, n_ext: int, Tc, fwd_val, t2f, *tensors):
        # t2f (order 3 with a dense learned graph, else None): T_2 = 2 V V - I, V = fwd_val as (N, N), flattened -- formed by the caller with
        # differentiable ops; its gradient is this node's second graph output
        ext, stacks, Tc, fwd_val = _unpack(n_ext, Tc, fwd_val, tensors)
        n_cells = len(schedule)
        ref = ext[0]
        (B, N, C), cin = _checked_shapes(op, Ks, schedule, ext, stacks, Tc)
        out_slot, inner_slot, pos, counts = _layout(schedule, cin, n_cells, outputs)
        out_stack = ref.new_empty(len(outputs), B, N, C, H16)        # the requested states are produced in place, stacked
        inner = ref.new_empty(max(1, n_cells - len(outputs)), B, N, C, H16)
        learned = bool(ctx.needs_input_grad[6] or ctx.needs_input_grad[7])
        if Ks == 3 and learned and t2f is None:
            raise ValueError('stc_cell_graph: at Chebyshev order 3 the small-graph cell kernels take learned graphs as a dense Gs only')
        bufs = _Buffers(k, Ks, learned, counts, (B, N, C), n_cells, ref)
        t2f = _c(t2f.detach()) if Ks == 3 and t2f is not None else None
        ctx.t2b = None if t2f is None else t2f.view(N, N).t().contiguous().view(-1)      # T_2^T = 2 Gs^2 - I for the backward: once per forward, detached
        graph2 = _graph2(op, Ks, t2f, ref.device, 'fwd')
        out_alias = _alias(out_stack)
        state = [out_alias[out_slot[j]] if j in out_slot else inner[inner_slot[j]] for j in range(n_cells)]
        source = lambda src: ext[src[1]] if src[0] == 'ext' else state[src[1]]
        # Few samples: a cell step runs as a few launches over several workgroups per sample (each owning a contiguous range of row tiles)
        # instead of one launch with one workgroup per sample -- at the SF shape (batch 32) backward 79 -> ~45 us per cell in three
        # launches, forward 35 -> 24 us in two.  Dense learned graphs split alike: their aggregations are matrix products, in the forward over
        # the node tiles that cover a workgroup's own rows (so that the phase pairs still share a launch), in the backward over all workgroups.
        splits = k.cell_small_splits(B, N * C)
        for j, (s_id, x, hs) in enumerate(schedule):
            k.cell_small_fwd(op.fwd_rowptr, op.fwd_colidx, fwd_val, source(x), source(hs), Tc, *stacks[s_id], Hnew=state[j], checked=False,
                             splits=splits, **bufs.fwd_args(j, pos[j], graph2))
        ctx.save_for_backward(Tc, out_alias, inner, bufs.planes, *bufs.slabs, *ext, *[p for st in stacks for p in st])
        ctx.meta = (k, op, Ks, list(schedule), tuple(outputs), cin, (B, N, C), len(ext), splits)
        _guard(ctx, out_stack)
        return out_stack

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_stack):
        k, op, Ks, schedule, outputs, cin, (B, N, C), n_ext, splits = ctx.meta
        _check_guard(ctx)
        Tc, out_alias, inner, planes, slabs_n, slabs_w, *rest = ctx.saved_tensors
        need_Tc, need_val, need_t2 = ctx.needs_input_grad[6:9]
        learned = bool(need_Tc or need_val)
        ext, stacks = rest[:n_ext], _stacks(rest[n_ext:])
        n_cells = len(schedule)
        out_slot, inner_slot, pos, counts = _layout(schedule, cin, n_cells, outputs)
        state = [out_alias[out_slot[j]] if j in out_slot else inner[inner_slot[j]] for j in range(n_cells)]
        bufs = _Buffers(k, Ks, learned, counts, (B, N, C), n_cells, Tc, saved=(planes, slabs_n, slabs_w))
        source = lambda src: ext[src[1]] if src[0] == 'ext' else state[src[1]]
        Kc, graph2 = Tc.shape[0], _graph2(op, Ks, ctx.t2b, Tc.device, 'bwd')
        P = max(k.cell_small_params(Ks, Kc, w) for w in cin)
        dP = Tc.new_zeros(len(stacks), B * splits * k.cell_small_param_rows, P)   # parameter-gradient partials, every cell adds to its set's rows
        G = Tc.new_empty(n_cells, B, N, C, H16)                      # gradient owed to every cell's state
        owed = [False] * n_cells
        grad_stack = _c(grad_stack)
        for i, j in enumerate(outputs):
            G[j].copy_(grad_stack[i])
            owed[j] = True
        Gv, dPv = G.unbind(0), dP.unbind(0)
        for j in range(n_cells - 1, -1, -1):
            if not owed[j]:
                continue                                             # nothing downstream depends on this cell
            s_id, x, hs = schedule[j]
            Wg, bg, Wc, bc = stacks[s_id]
            dX = dH = late = None
            acc_x = acc_h = False
            if hs[0] == 'cell':
                dH, acc_h = Gv[hs[1]], owed[hs[1]]
                owed[hs[1]] = True
            if x[0] == 'cell':
                if hs[0] == 'cell' and hs[1] == x[1]:                # one state as both inputs: the kernel's two outputs must not alias
                    dX, late = torch.empty_like(Gv[x[1]]), x[1]
                else:
                    dX, acc_x = Gv[x[1]], owed[x[1]]
                    owed[x[1]] = True
            k.cell_small_bwd(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, source(x), source(hs), Tc, Wg, Wc, dHnew=Gv[j], dX=dX, accumulate_x=acc_x, dH=dH,
                             accumulate_h=acc_h, dparams=dPv[s_id], has_bg=bg is not None, has_bc=bc is not None, checked=False, splits=splits,
                             **bufs.bwd_args(j, pos[j], graph2))
            if late is not None:
                Gv[late].add_(dX)
        sums = dP.sum(1)                                             # (sets, P)
        flat = []
        for s_id, st in enumerate(stacks):
            w = next((cin[j] for j, sc in enumerate(schedule) if sc[0] == s_id), None)
            if w is None:
                flat += [None if p is None else torch.zeros_like(p) for p in st]
                continue
            nW, row = Ks * Kc * (w + H16), sums[s_id]
            dWg, dbg = row[:nW * 32].view(nW, 32), row[nW * 32:nW * 32 + 32]
            dWc, dbc = row[nW * 32 + 32:nW * 48 + 32].view(nW, H16), row[nW * 48 + 32:nW * 48 + 48]
            flat += [dWg, dbg if st[1] is not None else None, dWc, dbc if st[3] is not None else None]
        graph_grads = _graph_gradients(bufs, k, op, Tc, stacks, schedule, cin, pos, need_Tc, need_val, need_t2 and ctx.t2b is not None) if learned else (None,) * 3
        return (None,) * 6 + graph_grads + (None,) * n_ext + tuple(flat)


def _graph_gradients(bufs, k, op, Tc, stacks, schedule, cin, pos, need_Tc, need_val, need_t2=False):
    """(dT_c, d fwd_val, d T_2) of a learned-graph backward pass from what the cell launches left in ``bufs`` (module docstring), per width group
    (index 0: narrow inputs, 1: 16-column inputs), in the kernels' column order [H (16) | X (cin) | 0]; W's rows are re-ordered to match.  d T_2
    (order 3) is the same product as d fwd_val on the third slabs' gradients, its partials in the same buffer.  The sums over cells and samples
    run in ``graph_grad`` / ``mix_grad`` (stc_graph_grad_f32 / stc_mix_grad_f32: fp32 matrix products per plane, float64 accumulation):
      d fwd_val = sum_cells [dZ1g x Z0 + dZ1c x Z0c]                                      (every cell of a width at once)
                  on a sparse pattern (``op.nnz != N * N``, order 2): the same products at the stored entries only, in ``op.fwd_val``'s
                  order (``graph_grad_csr``: stc_graph_grad_csr_f32) -- (nnz,) instead of (N, N)
      dT_c[c, d] = < W[(ks, c)], Q_ks[c, :, d, :] >,  Q_ks = Z_ks^T . dY                  (per parameter set and convolution)."""
    (B, N, C), Ks, counts, Kc = bufs.dims, bufs.Ks, bufs.counts, Tc.shape[0]
    # every product of the pass leaves its float64 partials in ONE (chunks, total) buffer, side by side, and one sum adds them all: per
    # product that was an allocation, a reduction and -- for dT_c -- a stack, three weight copies and an einsum of its own (~100 launches of a
    # few microseconds per step at the SF shape)
    graph_jobs = []                                               # (A, B, cells): dGs^T pieces, then (order 3) as many d T_2 pieces
    for want, dZg, dZc in ((need_val, bufs.dZ1g, bufs.dZ1c), (need_t2, bufs.dZ2g, bufs.dZ2c)):
        for w in (w for w in (0, 1) if want and counts[w]):
            graph_jobs += [(dZg[w], bufs.Z0[w], counts[w]), (dZc[w], bufs.Z0c[w], counts[w])]
    classes = {}                                                  # (width group, convolution) -> [(slab 0, slab 1, W, dY, first cell, step, cells)]
    dT_direct = []                                                # dT_c pieces formed directly on the matrix cores (stc_mix_dt_f32)
    if need_Tc:
        for s_id, (Wg, bg, Wc, bc) in enumerate(stacks):
            cells = [j for j, sc in enumerate(schedule) if sc[0] == s_id]
            if not cells:
                continue
            w, first = pos[cells[0]]
            where = [pos[j][1] for j in cells]
            step = where[1] - where[0] if len(where) > 1 else 1
            # per convolution: (its Ks slabs, W, dY)
            operands = (((bufs.Z0[w], bufs.Zg[w]) + ((bufs.Zg2[w],) if Ks == 3 else ()), Wg, bufs.dYg[w]),
                        ((bufs.Z0c[w], bufs.Z1c[w]) + ((bufs.Z2c[w],) if Ks == 3 else ()), Wc, bufs.dYc[w]))
            if step < 1 or any(b_ - a_ != step for a_, b_ in zip(where, where[1:])):
                # (a schedule STCGNN never builds: the set's cells are not evenly spaced inside their width group -- gather them)
                pick = lambda t: torch.stack([t[i] for i in where])
                operands = tuple((tuple(pick(s) for s in ss), W, pick(dY)) for ss, W, dY in operands)
                first, step = 0, 1
            for conv, (ss, W, dY) in enumerate(operands):
                LP, Ho, cw = ss[0].shape[-1], W.shape[1], cin[cells[0]]
                if step == 1 and hasattr(k, 'mix_dT') and k.mix_dT_supported(Ks, Kc, C, LP, Ho):
                    # the set's cells are consecutive planes of their slabs: dT_c = sum over their rows of U_c . dY^T in ONE launch on tiles of
                    # floor(16 / C) nodes (U_c = [Z_0 | Z_1] . W_c re-formed inside) -- instead of Ks products Q = Z^T . dY with float64
                    # partials, their sum and a contraction with W per class (0.44 + ~0.2 ms of the 4.65 ms learned-graph SF step)
                    n, rows = len(cells), len(cells) * B * N
                    Wp = _slab_order(W, Ks, Kc, cw, LP)
                    piece = Tc.new_empty(Kc, C, C)
                    k.mix_dT([s[first:first + n].view(rows, C, LP) for s in ss], Wp.view(Ks * Kc * LP, Ho),
                             dY[first:first + n].view(rows, C, Ho), piece)
                    dT_direct.append(piece)
                    continue
                classes.setdefault((w, cin[cells[0]], conv), []).append((ss, W, dY, first, step, len(cells)))
    block = lambda s0, dY: C * s0.shape[-1] * C * dY.shape[-1]
    total = sum(Ks * block(e[0][0], e[2]) for es in classes.values() for e in es)
    dS = dT2 = None
    if need_val and op.nnz != N * N:                              # a sparse pattern: the products sampled at its entries, one shared partial buffer
        dS = torch.zeros(op.nnz, dtype=torch.float64, device=Tc.device)
        if graph_jobs:
            planes = min(n for _, _, n in graph_jobs) * B
            gpart = k.grad_partials(Tc, len(graph_jobs) * op.nnz, chunks=k.graph_grad_csr_chunks(planes, N, op.nnz, Tc.device))
            for i, (A, Bm, n_sel) in enumerate(graph_jobs):
                k.graph_grad_csr(op.fwd_rowptr, op.fwd_colidx, A, Bm, 0, 1, n_sel, N, into=(gpart, i * op.nnz))
            dS = gpart.view(-1, len(graph_jobs), op.nnz).sum((0, 1))                           # ONE sum for the partials of every job
    elif need_val or need_t2:                                     # (N x N blocks are small: more, shorter workgroups -- a buffer of their own)
        kinds = int(bool(need_val)) + int(bool(need_t2))
        both = torch.zeros(kinds, N, N, dtype=torch.float64, device=Tc.device)
        if graph_jobs:
            planes = min(n for _, _, n in graph_jobs) * B
            # (a kernel set without the rule: the one that every sample of up to SMALL_STAGED_ROWS rows keeps)
            chunks = k.graph_grad_chunks(planes, N, N * C, Tc.device) if hasattr(k, 'graph_grad_chunks') else max(1, min(256, planes))
            gpart = k.grad_partials(Tc, len(graph_jobs) * N * N, chunks=chunks)
            for i, (A, Bm, n_sel) in enumerate(graph_jobs):
                k.graph_grad(A, Bm, 0, 1, n_sel, N, into=(gpart, i * N * N))
            both = gpart.view(-1, kinds, len(graph_jobs) // kinds, N, N).sum((0, 2))       # ONE sum for the partials of both gradients
        dS = both[0] if need_val else None
        dT2 = both[kinds - 1] if need_t2 else None
    sums = None
    if total:
        part, off = k.grad_partials(Tc, total), 0
        for es in classes.values():
            for ss, W, dY, first, step, n_sel in es:
                for slab in ss:
                    k.mix_grad(slab, dY, first, step, n_sel, N, into=(part, off))
                    off += block(ss[0], dY)
        sums = part.sum(0)
    dT = torch.zeros(Tc.shape, dtype=torch.float64, device=Tc.device) if need_Tc else None
    if dT_direct:
        dT += torch.stack(dT_direct).sum(0)
    off = 0
    for (w, cw, conv), es in classes.items():
        LP, Ho = es[0][0][0].shape[-1], es[0][1].shape[1]
        size = len(es) * Ks * block(es[0][0][0], es[0][2])
        Q = sums[off:off + size].view(len(es), Ks, C, LP, C, Ho)
        off += size
        Wp = _slab_order(torch.stack([e[1] for e in es]), Ks, Kc, cw, LP)
        # sum_{p,s,l,o} Q[p,s,c,l,d,o] W[p,s,k,l,o] as a product and a sum (as an einsum: a float64 GEMM with a 50-element result, 190 us)
        dT += (Q[:, :, None] * Wp.double()[:, :, :, None, :, None, :]).sum((0, 1, 4, 6))
    flat32 = lambda g: None if g is None else g.to(Tc.dtype).reshape(-1)
    return (None if dT is None else dT.to(Tc.dtype)), flat32(dS), flat32(dT2)


def dense_second_order(op: SpatialOperand) -> torch.Tensor:
    """T_2 = 2 V V - I of a dense learned Gs in the forward's orientation (V = ``op.fwd_val`` as (N, N) = Gs^T), flattened like ``fwd_val``: formed
    by differentiable torch ops, so that autograd carries the node's d T_2 through the product back to Gs -- the node holds no hand-written
    chain (the reference forms T_2 on the matrix side too: cheby_poly, STC_GNN.py:24-29)."""
    V = op.fwd_val.view(op.n, op.n)
    return (2.0 * (V @ V) - torch.eye(op.n, dtype=V.dtype, device=V.device)).reshape(-1)


def _forward_only(k, op: SpatialOperand, Ks: int, schedule, outputs, n_ext: int, Tc, fwd_val, t2f, tensors):
    """``_StcSmallGraph.forward`` for a pass that no backward follows (evaluation, forecasting): the same launches per cell, in the same argument
    order, with the same ``splits`` -- but nothing is saved.  ONE set of the planes and slabs that carry a cell from phase to phase (U, RH, Zc and,
    per input-width group, Zg; order 3: Zc2, Zg2) serves every cell: the launches are stream-ordered and a cell's scratch is dead once its last
    launch has been issued.  No learned-graph slabs; R and Cand -- read by a backward only -- are not stored where the kernel set takes None for
    them (``small_optional_stores``; else one shared plane each).  The cells run by level (``wavefront``) and an inner state goes back to the
    allocator after the last cell that reads it has launched, so memory does not grow with the number of cells.  The requested states are
    written in place into the returned stack: bit for bit that of the autograd node."""
    ext, stacks, Tc, fwd_val = _unpack(n_ext, Tc, fwd_val, tensors)
    ref = ext[0]
    (B, N, C), cin = _checked_shapes(op, Ks, schedule, ext, stacks, Tc)
    out_slot = _out_slots(outputs)
    out_stack = ref.new_empty(len(outputs), B, N, C, H16)
    plane, rows = (lambda: ref.new_empty(B, N, C, H16)), (lambda width: ref.new_empty(B, N * C, width))
    o3 = Ks == 3
    shared = dict(U=plane(), RH=plane(), Zc=rows(H16), **(dict(Zc2=rows(H16)) if o3 else {}))
    shared.update(dict(R=None, Cand=None) if getattr(k, 'small_optional_stores', False) else dict(R=plane(), Cand=plane()))
    slabs = {w: dict(Zg=rows(k.cell_small_zg_width(w)), **(dict(Zg2=rows(k.cell_small_zg_width(w))) if o3 else {})) for w in set(cin)}
    if o3:
        shared['graph2'] = _graph2(op, Ks, None if t2f is None else _c(t2f), ref.device, 'fwd')
    splits = k.cell_small_splits(B, N * C)
    state = [None] * len(schedule)
    source = lambda src: ext[src[1]] if src[0] == 'ext' else state[src[1]]
    order = wavefront(schedule)
    last = last_uses(schedule, order)
    for j in order:
        s_id, x, hs = schedule[j]
        state[j] = out_stack[out_slot[j]] if j in out_slot else plane()
        k.cell_small_fwd(op.fwd_rowptr, op.fwd_colidx, fwd_val, source(x), source(hs), Tc, *stacks[s_id], Hnew=state[j], checked=False, splits=splits,
                         **shared, **slabs[cin[j]])
        for src in {x, hs, ('cell', j)}:                             # (an output lives in the stack; dropping its view frees nothing)
            if src[0] == 'cell' and last.get(src, j) == j:
                state[src[1]] = None
    return out_stack


def stc_small_graph(k, op: SpatialOperand, Tc, Ks: int, schedule, outputs, ext, stacks):
    """The schedule on the few-category cell kernels: the autograd node, or -- grad mode off, or nothing that requires grad (the predicate of
    ``ops.stc_cell_graph``) -- the forward-only route.  The graphs (``Tc``, ``op.fwd_val``) and the parameter sets are differentiable; the
    external tensors are not: in grad mode one that requires grad raises ``ValueError`` before any launch."""
    _refuse_differentiable(ext=list(ext))
    flat = [p for st in stacks for p in st]
    dense3 = Ks == 3 and op.nnz == op.n * op.n and op.source is None
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (Tc, op.fwd_val, *ext, *flat)):
        with torch.no_grad():
            return _forward_only(k, op, Ks, list(schedule), list(outputs), len(ext), Tc, op.fwd_val, dense_second_order(op) if dense3 else None,
                                 (*ext, *flat))
    t2f = dense_second_order(op) if dense3 else None
    return _StcSmallGraph.apply(k, op, Ks, list(schedule), list(outputs), len(ext), Tc, op.fwd_val, t2f, *ext, *flat)
