"""Helpers of tests/test_model_lattice.py: the STCGNN module and the cell-graph executors over depth, sequence length, horizon and bias on every
kernel route, against the float64 oracle (oracle/stc_oracle.py).

A case is (route, topology, use_bias).  ``ROUTES`` is closed: each entry fixes what selects a kernel route -- categories, Chebyshev order, hidden
width, graph mode, operand format, storage type -- and names, per mode (grad / ``torch.no_grad()``), the executor that must run and the entry
points of include/stc_hip.h that must and must not be launched.  ``TOPOLOGIES`` are (layers, T, horizon); inputs are
``bench_path_inputs`` on a 4 x 5 grid (N = 20: non-symmetric weighted queen grid, non-symmetric Gc, 0/1 windows), the model is built as
tests/test_scale_sweep._case builds it (global seed before the constructor, every bias 0.3 sigma from a private generator).

No tolerance is defined here: the fp32 routes go through ``tests/test_scale_sweep._check`` (1e-5 / 2e-5, or 3x / 10x the oracle's own float32
noise), the learned routes add the bounds of their own files (``LEARNED_GRAPH``), bf16 storage is held to the criterion of
tests/test_bf16_kernels.py::test_model_bf16_storage_tracks_fp32 (``BF16``) against float64.
"""
import dataclasses
import functools

import torch

import STC_GNN as M
from oracle import stc_oracle as O
from stc_hip import CsrGraph, ops
from stc_hip.graph import csr_operand
from tests.autograd_contract import MGP_NOISE, NOISE_FACTOR, SMALL_LEARNED, SMALL_LEARNED_K3
from tests.conftest import rel_err
from tests.golden.make_golden import bench_path_inputs
from tests.test_first_step_route import FirstStepTwin
from tests.test_scale_sweep import FWD_BOUND, FWD_NOISE_FACTOR, _check, rel_l2

GRID = (4, 5)                                                       # N = 20: the smallest size at which every route below is still selected
TOPOLOGIES = [(1, 1, 1), (1, 3, 2), (2, 1, 1), (2, 2, 1), (3, 2, 3), (3, 1, 2), (2, 3, 2)]      # (layers, T, horizon); the last: the goldens' (g11 - g13)
BIASES = (True, False)
MODES = ('grad', 'no_grad')

#: tests/test_bf16_kernels.py::test_model_bf16_storage_tracks_fp32: prediction (in (0, 1)) absolute, cosine and norm ratio of every gradient
BF16 = dict(pred=2e-2, cosine=0.995, norm=5e-2)
#: the learned graphs themselves, where the few-category executor differentiates them (dense-learned-small): the generator's output against
#: tests/test_mgp_front.py's bound (flat, MGP_NOISE x the oracle's fp32 noise), the gradient the executor hands back for Gs / Gc against
#: tests/test_small_cell.py's (order 2) or tests/test_small_dense_order3.py's (order 3) -- flat, or NOISE_FACTOR x that noise
LEARNED_GRAPH = {'forward': (FWD_BOUND, MGP_NOISE), 'grad': {2: (SMALL_LEARNED, NOISE_FACTOR), 3: (SMALL_LEARNED_K3, NOISE_FACTOR)}}

_FIRST = ('stc_cell_gates_fwd_first_f32', 'stc_cell_bwd_first_f32', 'stc_ring2_blend_first_f32')
_SMALL = ('stc_cell_small_fwd_f32', 'stc_cell_small_bwd_f32')
_PLANAR = ('stc_cell_gates_fwd_planar_f32', 'stc_cell_gates_bwd_planar_f32', 'stc_cell_bwd_planar_f32')
_PLANAR_K = ('stc_cell_gates_fwd_planar_k_f32', 'stc_cell_cand_fwd_planar_k_f32', 'stc_cell_gates_bwd_planar_k_f32', 'stc_cell_cand_bwd_planar_k_f32')
_ROWS = ('stc_cell_gates_fwd_f32', 'stc_cell_blend_fwd_f32', 'stc_cell_gates_bwd_f32', 'stc_cell_cand_bwd_f32')
_NODE = ('stc_bdg_node_fwd_f32', 'stc_bdg_node_bwd_f32', 'stc_gru_gates_fwd_f32', 'stc_gru_blend_fwd_f32')
_BF16 = ('stc_cell_gates_fwd_planar_bf16', 'stc_cell_gates_bwd_planar_bf16', 'stc_cell_bwd_planar_bf16', 'stc_spmm_blend_fwd_bf16', 'stc_head_fwd_bf16')
_RING2 = ('stc_ring2_sum_f32', 'stc_ring2_blend_f32', 'stc_ring2_blend_first_f32', 'stc_ring2_chain_f32')


@dataclasses.dataclass(frozen=True)
class Route:
    """One kernel route.  ``executor``: per mode 'graph' (``ops.stc_cell_graph``, not the few-category executor), 'small' (``ops.stc_small_graph``
    under it) or 'per-cell' (one ``ops.stc_cell`` per cell, no executor).  ``must`` / ``never``: entry points of include/stc_hip.h per mode, read
    off the dispatch (``ops._cell_forms``, ``ops._ForwardPass``, ``ops._BackwardPass``, ``small.small_graph_supported``, ``STCGNN.forward``);
    ``both`` are added to the two modes' ``must``.  ``twins``: the CPU kernel sets the route also runs on ('exact', 'first-step', 'f16x2')."""
    name: str
    C: int
    K: int
    hidden: int = 16
    graph_mode: str = 'csr-fixed'
    fmt: str = None                                                 # operand format of the split-operand kernels, set on the HIP kernel set
    storage: torch.dtype = torch.float32
    ctor: tuple = ()                                                # further constructor arguments, as (name, value) pairs
    queen: bool = False                                             # the unweighted normalised queen grid of ``ring2_grid()`` (two-ring plans)
    executor: tuple = ('graph', 'graph')                            # (grad, no_grad)
    executor_cpu: tuple = None                                      # ... on the CPU twins, where it differs (a kernel the twin does not have)
    both: tuple = ()
    must: tuple = ((), ())                                          # (grad, no_grad)
    never: tuple = ()
    twins: tuple = ('exact',)
    criterion: str = 'fp32'                                         # 'fp32' | 'learned' | 'bf16'


@functools.lru_cache(maxsize=None)
def ring2_grid():
    """The smallest normalised queen grid (by node count, then height; up to 16 x 16) whose operand carries two-ring plans for both
    orientations, or None."""
    for H, W in sorted(((H, W) for H in range(1, 17) for W in range(H, 17)), key=lambda g: (g[0] * g[1], g[0])):
        op = csr_operand(CsrGraph.queen_grid(H, W, normalize=True), torch.device('cpu'))
        if op.fwd_ring2 is not None and op.bwd_ring2 is not None:
            return H, W
    return None


_planar = dict(C=32, K=2, both=('stc_cell_gates_fwd_first_f32', 'stc_cell_gates_fwd_planar_f32', 'stc_spmm_blend_fwd_f32', 'stc_head_fwd_f32'),
               must=(('stc_cell_bwd_first_f32', 'stc_cell_bwd_planar_f32', 'stc_head_bwd_f32'), ()),
               never=_SMALL + _PLANAR_K + _ROWS + _NODE + _BF16 + ('stc_cell_gates_bwd_planar_f32', 'stc_bdg_node_post_bwd_f32'))
ROUTES = [
    # a, b: one-launch backward; the first-step forms for every encoder cell at t = 0 (both operand formats)
    Route('planar-f16x2', fmt='f16x2', twins=('first-step', 'f16x2'), **_planar),
    Route('planar-bf16x3', fmt='bf16x3', twins=('first-step',), **_planar),
    # c: two-launch backward (candidate through node_post, then the planar gates backward); no first-step forms at 64 categories
    Route('c64', 64, 2, twins=('exact', 'f16x2'), both=('stc_cell_gates_fwd_planar_f32', 'stc_spmm_blend_fwd_f32', 'stc_head_fwd_f32'),
          must=(('stc_bdg_node_post_bwd_f32', 'stc_cell_gates_bwd_planar_f32', 'stc_head_bwd_f32'), ()),
          never=_SMALL + _PLANAR_K + _ROWS + _NODE + _BF16 + _FIRST + ('stc_cell_bwd_planar_f32',)),
    # d: order 3 on the three Chebyshev planes of each side
    Route('order3', 32, 3, twins=('exact', 'f16x2'), both=('stc_cell_gates_fwd_planar_k_f32', 'stc_cell_cand_fwd_planar_k_f32', 'stc_head_fwd_f32'),
          must=(('stc_cell_gates_bwd_planar_k_f32', 'stc_cell_cand_bwd_planar_k_f32', 'stc_head_bwd_f32'), ()),
          never=_SMALL + _PLANAR + _ROWS + _NODE + _BF16 + _FIRST),
    # e: the few-category executor on fixed graphs
    Route('few-cat-k2', 5, 2, executor=('small', 'small'), both=('stc_cell_small_fwd_f32', 'stc_head_fwd_f32'),
          must=(('stc_cell_small_bwd_f32', 'stc_head_bwd_f32'), ()), never=_PLANAR + _PLANAR_K + _ROWS + _NODE + _BF16 + _FIRST),
    Route('few-cat-k3', 5, 3, executor=('small', 'small'), both=('stc_cell_small_fwd_f32', 'stc_head_fwd_f32'),
          must=(('stc_cell_small_bwd_f32', 'stc_head_bwd_f32'), ()), never=_PLANAR + _PLANAR_K + _ROWS + _NODE + _BF16 + _FIRST),
    # f: bf16 state planes
    Route('bf16-storage-c32', 32, 2, storage=torch.bfloat16, criterion='bf16',
          both=('stc_cell_gates_fwd_planar_bf16', 'stc_spmm_blend_fwd_bf16', 'stc_head_fwd_bf16'), must=(('stc_head_bwd_bf16',), ()),
          never=_SMALL + _PLANAR + _PLANAR_K + _ROWS + _NODE + _FIRST + ('stc_head_fwd_f32',)),
    Route('bf16-storage-c64', 64, 2, storage=torch.bfloat16, criterion='bf16',
          both=('stc_cell_gates_fwd_planar_bf16', 'stc_spmm_blend_fwd_bf16', 'stc_head_fwd_bf16'), must=(('stc_head_bwd_bf16',), ()),
          never=_SMALL + _PLANAR + _PLANAR_K + _ROWS + _NODE + _FIRST + ('stc_head_fwd_f32',)),
    # g: the reference's full model.  Few categories: the few-category executor differentiates both learned graphs (dT_c of a set's consecutive
    # cells on the matrix cores, stc_mix_dt_f32 -- every encoder layer has such a set; stc_mix_grad_f32 only for sets spaced apart).  32 categories: one autograd
    # node per cell in grad mode (dT_c, dGs per convolution); with grad mode off the graphs need no gradient and the general executor runs the
    # planar cells on the dense aggregation
    Route('dense-learned-small', 5, 2, graph_mode='dense-learned', criterion='learned', executor=('small', 'small'),
          both=('stc_mgp_uv_fwd_f32', 'stc_mgp_softmax_fwd_f32', 'stc_mixed_fusion_fwd_f32', 'stc_cheby_dense_fwd_f32', 'stc_cell_small_fwd_f32', 'stc_head_fwd_f32'),
          must=(('stc_cell_small_bwd_f32', 'stc_graph_grad_f32', 'stc_mix_dt_f32', 'stc_cheby_dense_bwd_f32', 'stc_mixed_fusion_bwd_f32',
                 'stc_mgp_softmax_bwd_f32', 'stc_mgp_uv_bwd_f32', 'stc_head_bwd_f32'), ()),
          never=_PLANAR + _PLANAR_K + _ROWS + _NODE + _BF16 + _FIRST),
    Route('dense-learned-general', 32, 2, graph_mode='dense-learned', criterion='learned', executor=('per-cell', 'graph'),
          both=('stc_mgp_uv_fwd_f32', 'stc_mgp_softmax_fwd_f32', 'stc_mixed_fusion_fwd_f32', 'stc_cheby_dense_fwd_f32', 'stc_dense_agg_f32', 'stc_head_fwd_f32'),
          # (grad mode: fused gate epilogues in the forward; the backward wants dT_c and dGs, which the node backward and stc_csr_sddmm_f32 form)
          must=(('stc_cell_gates_fwd_f32', 'stc_cell_blend_fwd_f32', 'stc_bdg_node_bwd_f32', 'stc_gru_gates_bwd_f32', 'stc_gru_blend_bwd_f32',
                 'stc_cheby_dense_bwd_f32', 'stc_mixed_fusion_bwd_f32', 'stc_mgp_uv_bwd_f32', 'stc_head_bwd_f32'),
                ('stc_cell_gates_fwd_planar_f32',)),
          never=_SMALL + _PLANAR_K + _BF16),
    # h: the spatial graph learned on the prior's pattern.  'per-cell': one autograd node per cell in grad mode (the sampled product per
    # convolution); 'fused': the few-category executor forms the value gradient at the stored entries.  Grad mode off: a fixed sparse graph
    Route('csr-learned-per-cell', 5, 2, graph_mode='csr-learned', criterion='learned', ctor=(('fusion_rank', 4), ('csr_cells', 'per-cell')),
          executor=('per-cell', 'small'), both=('stc_mgp_csr_score_f32', 'stc_mgp_csr_softmax_fwd_f32', 'stc_mixed_fusion_lr_fwd_f32', 'stc_head_fwd_f32'),
          must=(('stc_csr_sddmm_f32', 'stc_mgp_csr_softmax_bwd_f32', 'stc_mgp_csr_score_bwd_f32', 'stc_mixed_fusion_lr_bwd_f32', 'stc_head_bwd_f32'),
                ('stc_cell_small_fwd_f32',)),
          never=_PLANAR + _PLANAR_K + _BF16 + _FIRST + ('stc_cell_small_bwd_f32', 'stc_graph_grad_csr_f32')),
    Route('csr-learned-fused', 5, 2, graph_mode='csr-learned', criterion='learned', ctor=(('fusion_rank', 4), ('csr_cells', 'fused')),
          executor=('small', 'small'), executor_cpu=('per-cell', 'small'),         # (the twin has no sampled product, ``graph_grad_csr``)
          both=('stc_mgp_csr_score_f32', 'stc_mgp_csr_softmax_fwd_f32', 'stc_mixed_fusion_lr_fwd_f32', 'stc_cell_small_fwd_f32', 'stc_head_fwd_f32'),
          must=(('stc_cell_small_bwd_f32', 'stc_graph_grad_csr_f32', 'stc_mgp_csr_softmax_bwd_f32', 'stc_mgp_csr_score_bwd_f32', 'stc_mixed_fusion_lr_bwd_f32',
                 'stc_head_bwd_f32'), ()),
          never=_PLANAR + _PLANAR_K + _ROWS + _NODE + _BF16 + _FIRST + ('stc_csr_sddmm_f32',)),
    # i: hidden widths other than 16: no executor, the generic node kernels under one autograd node per cell
    Route('hidden8', 32, 2, hidden=8, executor=('per-cell', 'per-cell'), both=('stc_bdg_node_fwd_f32', 'stc_gru_gates_fwd_f32', 'stc_gru_blend_fwd_f32', 'stc_head_fwd_f32'),
          must=(('stc_bdg_node_bwd_f32', 'stc_gru_gates_bwd_f32', 'stc_gru_blend_bwd_f32', 'stc_head_bwd_f32'), ()),
          never=_SMALL + _PLANAR + _PLANAR_K + _ROWS + _BF16 + _FIRST),
    Route('hidden32', 5, 2, hidden=32, executor=('per-cell', 'per-cell'), both=('stc_bdg_node_fwd_f32', 'stc_gru_gates_fwd_f32', 'stc_gru_blend_fwd_f32', 'stc_head_fwd_f32'),
          must=(('stc_bdg_node_bwd_f32', 'stc_gru_gates_bwd_f32', 'stc_gru_blend_bwd_f32', 'stc_head_bwd_f32'), ()),
          never=_SMALL + _PLANAR + _PLANAR_K + _ROWS + _BF16 + _FIRST),
]
if ring2_grid() is not None:
    # j: route a on a graph with two-ring plans: the blend and the aggregation of the new state in one launch, the backward's sums through S^T
    ROUTES.append(Route('two-ring', fmt='f16x2', queen=True, twins=('first-step', 'f16x2'),
                        **{**_planar, 'both': ('stc_cell_gates_fwd_first_f32', 'stc_cell_gates_fwd_planar_f32', 'stc_head_fwd_f32')}))
BY_NAME = {r.name: r for r in ROUTES}
assert len(BY_NAME) == len(ROUTES)

#: constructor arguments of ``STCGNN`` that are neither an axis of the lattice nor fixed by a route -> why
NOT_SWEPT = {
    'num_nodes': 'every case runs the 4 x 5 grid (the two-ring route its own smallest grid): sizes belong to the kernel-level lattice, tests/test_shape_lattice.py',
    'input_dim': "forward asserts a 4-D X_seq, so the model's own input width is always 1",
    'activation': 'covered at layer level by tests/test_module_parity.py (the composed path of STC_Cell); with one the executor is never asked',
    'batch_sharded': 'covered by tests/test_dist_gloo.py (two ranks)',
    'reorder_nodes': 'covered by tests/test_module_parity.py::test_internal_node_reordering_is_invisible; a 4 x 5 grid in row order is never renumbered',
}
AXES = {'num_layers': 'TOPOLOGIES', 'out_horizon': 'TOPOLOGIES', 'use_bias': 'BIASES'}
BY_ROUTE = {'num_categories': 'C', 'Ks': 'K', 'Kc': 'K', 'hidden_dim': 'hidden', 'graph_mode': 'graph_mode', 'storage_dtype': 'storage',
            'fusion_rank': 'ctor', 'csr_cells': 'ctor', 'spatial_graph': 'graph_mode'}


def case_id(route, topo, bias):
    return f'{route.name}-L{topo[0]}T{topo[1]}H{topo[2]}-{"bias" if bias else "nobias"}'


CASES = [(r, t, b) for r in ROUTES for t in TOPOLOGIES for b in BIASES]


# ---- inputs, model, oracle ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(route, topo):
    layers, T, horizon = topo
    H, W = ring2_grid() if route.queen else GRID
    s = bench_path_inputs(route.C, route.K, H=H, W=W, h=route.hidden, layers=layers, horizon=horizon, B=2, T=T)
    if route.queen:
        s['graph'] = CsrGraph.queen_grid(H, W, normalize=True)
        s['Gs'] = s['graph'].to_dense()
    else:
        s['graph'] = CsrGraph.from_dense(s['Gs'])
    return s


def build(route, topo, bias):
    """(model on the CPU, its state dict, inputs): the global generator is seeded before the constructor; every bias is drawn from a private one
    (the initialisers leave them at zero, which would hide a dropped bias)."""
    s = _inputs(route, topo)
    layers, T, horizon = topo
    kw = dict(route.ctor)
    if route.graph_mode == 'csr-learned':
        kw['spatial_graph'] = s['graph']
    torch.manual_seed(977)
    model = M.STCGNN(num_nodes=s['N'], num_categories=route.C, Ks=route.K, Kc=route.K, input_dim=1, hidden_dim=route.hidden, num_layers=layers,
                     out_horizon=horizon, use_bias=bias, graph_mode=route.graph_mode, storage_dtype=route.storage, **kw)
    g = torch.Generator().manual_seed(4242)
    sd = {k: 0.3 * torch.randn(v.shape, generator=g) if k.endswith(('.b', '.bias')) else v.clone() for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    return model, sd, s


def _oracle_run(route, topo, sd, s, dtype):
    layers, T, horizon = topo
    leaves = {k: v.clone().to(dtype).requires_grad_() for k, v in sd.items()}
    X, Gs, Gc, K, h = s['X'].to(dtype), s['Gs'].to(dtype), s['Gc'].to(dtype), route.K, route.hidden
    graphs = {}
    if route.graph_mode == 'csr-fixed':
        yhat = O.encdec_forward(X, Gs, Gc, leaves, K, K, h, layers, horizon)
    elif route.graph_mode == 'dense-learned':                       # O.stcgnn_forward, with the learned graphs kept for LEARNED_GRAPH
        lGs, lGc = O.mgp_gen(X, Gs, Gc, leaves)
        lGs.retain_grad(), lGc.retain_grad()
        graphs = {'Gs': lGs, 'Gc': lGc}
        yhat = O.encdec_forward(X, lGs, lGc, leaves, K, K, h, layers, horizon)
    else:                                                           # the float64 expression tests/test_mgp_csr.py::_model_case is compared against
        from tests.test_mgp_csr import model_restatement
        yhat = model_restatement(X, s['graph'], Gc, leaves, K, h, layers, horizon)[0]
    O.combo_loss(yhat, s['Y'].to(dtype)).backward()
    return yhat.detach(), {k: v.grad for k, v in leaves.items()}, {k: (v.detach(), v.grad) for k, v in graphs.items()}


@functools.lru_cache(maxsize=None)
def _oracle_cached(model_of, topo, bias):
    _, sd, s = build(model_of, topo, bias)
    return _oracle_run(model_of, topo, sd, s, torch.float64), _oracle_run(model_of, topo, sd, s, torch.float32)


def oracle(route, topo, bias):
    """(float64 run, float32 run) of the oracle, each (yhat, {name: gradient}, {learned graph: (value, gradient)}): computed once per distinct
    model -- routes that differ only in operand format, storage type or in which executor forms the gradients share it -- and never modified."""
    ctor = tuple(kv for kv in route.ctor if kv[0] != 'csr_cells')
    model_of = Route('', route.C, route.K, route.hidden, route.graph_mode, ctor=ctor, queen=route.queen)
    return _oracle_cached(model_of, topo, bias)


# ---- running a case -------------------------------------------------------------------------------------------------------------------------------
class Spies:
    """Counts of the executors' calls (``ops.*``) and, on the GPU, the name of every C entry point launched (every ``HipKernels._launch``)."""

    def __init__(self, monkeypatch, dev):
        self.calls = {'stc_cell_graph': 0, 'stc_small_graph': 0, 'stc_cell': 0}
        self.launched = []
        for name in self.calls:
            monkeypatch.setattr(ops, name, self._counted(name, getattr(ops, name)))
        if dev == 'cuda':
            from stc_hip._lib import HipKernels
            real, log = HipKernels._launch, self.launched
            monkeypatch.setattr(HipKernels, '_launch', lambda k, name, *a, **kw: (log.append(name), real(k, name, *a, **kw))[1])

    def _counted(self, name, real):
        def call(*a, **kw):
            self.calls[name] += 1
            return real(*a, **kw)
        return call

    def reset(self):
        self.calls.update(dict.fromkeys(self.calls, 0))
        del self.launched[:]

    def executor(self):
        c = self.calls
        if c['stc_cell_graph'] and not c['stc_cell']:
            return 'small' if c['stc_small_graph'] else 'graph'
        return 'per-cell' if (c['stc_cell'] and not c['stc_cell_graph'] and not c['stc_small_graph']) else f'mixed {c}'


def route_findings(route, mode, spies, dev):
    """What the spies saw against the route's row of the table; on the CPU the executors only (the twin has no entry-point names)."""
    i = MODES.index(mode)
    found = []
    want = (route.executor if dev == 'cuda' or route.executor_cpu is None else route.executor_cpu)[i]
    if spies.executor() != want:
        found.append(f'{mode}: executor {spies.executor()}, the route names {want}')
    if dev == 'cuda':
        seen = set(spies.launched)
        missing, forbidden = sorted(set(route.both + route.must[i]) - seen), sorted(set(route.never) & seen)
        if missing or forbidden:
            found.append(f'{mode}: entry points missing {missing}, forbidden {forbidden}; launched {sorted(seen)}')
        if route.queen and not seen & set(_RING2):
            found.append(f'{mode}: no two-ring launch; launched {sorted(seen)}')
    return found


def run(model, route, s, dev, mode, capture=None):
    """One pass of the module on ``dev``: (prediction, {name: gradient}); ``capture``: filled with the learned graphs the generator returned."""
    model = model.to(dev)
    model.zero_grad(set_to_none=True)
    As = s['Gs'].to(dev) if route.graph_mode == 'dense-learned' else s['graph']
    hook = None
    if capture is not None and route.graph_mode == 'dense-learned':
        def keep(_, __, out):
            if mode == 'grad':
                out[0].retain_grad(), out[1].retain_grad()
            capture.update(Gs=out[0], Gc=out[1])
        hook = model.mix_graph_pair.register_forward_hook(keep)
    try:
        if mode == 'no_grad':
            with torch.no_grad():
                return model(X_seq=s['X'].to(dev), As=As, Ac=s['Gc'].to(dev)).detach(), {}
        yhat = model(X_seq=s['X'].to(dev), As=As, Ac=s['Gc'].to(dev))
        O.combo_loss(yhat, s['Y'].to(dev)).backward()
        return yhat.detach(), {k: p.grad for k, p in model.named_parameters()}
    finally:
        if hook is not None:
            hook.remove()


def _noise(b32, b64):
    return max(rel_err(b32, b64), rel_l2(b32, b64))


def value_findings(tag, route, mode, got, graphs, want64, want32, dev):
    """The values of one run against the float64 oracle, by the route's criterion.  Every measured error is recorded by ``_check``, the
    scale sweep's one writer of the parity record (on the GPU), with the case's tag."""
    (y, grads), (y64, g64, G64), (y32, g32, G32) = got, want64, want32
    found = []
    if mode == 'grad':
        # no gradient is missing: every parameter has one, and the set is the oracle's leaves
        if set(grads) != set(g64) or any(g is None for g in grads.values()):
            return [f'{tag}: gradients of {sorted(k for k, g in grads.items() if g is None)} missing; names differ by {sorted(set(grads) ^ set(g64))}']
    else:
        g64 = g32 = {}
    # nothing may be void: at these O(1) inputs the oracle's own fp32 run has digits on every tensor (``_check`` would skip one that has none)
    void = [k for k, a, b in [('yhat', y32, y64)] + [('d' + k, g32[k], g64[k]) for k in g64] if _noise(a, b) > 0.1]
    if void:
        found.append(f'{tag}: void tensors {void}')
    if route.criterion == 'bf16':
        _check(tag, (y, grads), (y64, g64), (y32, g32), dev)         # for the record only: the fp32 bounds are not this route's criterion
        e = float((y.detach().double().cpu() - y64).abs().max())
        if not torch.isfinite(y).all() or not e < BF16['pred']:
            found.append(f'{tag}: prediction off by {e:.3e}')
        for k in g64:
            a, b = grads[k].detach().double().cpu().flatten(), g64[k].flatten()
            cos, ratio = float((a @ b) / (a.norm() * b.norm() + 1e-30)), float(a.norm() / (b.norm() + 1e-30))
            if not cos > BF16['cosine'] or not abs(ratio - 1) < BF16['norm']:
                found.append(f'{tag}: d{k} cosine {cos:.5f}, norm ratio {ratio:.4f}')
        return found
    bad = _check(tag, (y, grads), (y64, g64), (y32, g32), dev)     # FWD_BOUND / GRAD_BOUND, or 3x / 10x the oracle's fp32 noise
    found += [f'{tag}: {name} max-norm {e_max:.3e} l2 {e_l2:.3e} (oracle fp32 noise {noise:.1e})' for name, e_max, e_l2, noise in bad]
    # the learned graphs and what the few-category executor hands back for them: the graph in the prediction's place, its gradient as the one
    # gradient, through the same ``_check`` with the bounds of LEARNED_GRAPH (its forward noise factor, 3, is MGP_NOISE)
    (fwd_flat, fwd_factor), (flat, factor) = LEARNED_GRAPH['forward'], LEARNED_GRAPH['grad'][route.K]
    assert fwd_factor == FWD_NOISE_FACTOR
    for k, t in graphs.items():
        pick = (lambda i, G: {k: G[k][i]}) if mode == 'grad' else (lambda i, G: {})
        bad = _check(f'{tag}[learned {k}]', (t.detach(), {k: t.grad} if mode == 'grad' else {}), (G64[k][0], pick(1, G64)), (G32[k][0], pick(1, G32)), dev,
                     fwd_bound=fwd_flat, grad_bound=flat, noise_factor=factor)
        found += [f'{tag}: learned {k}, {name} max-norm {e_max:.3e} l2 {e_l2:.3e} (oracle fp32 noise {noise:.1e})' for name, e_max, e_l2, noise in bad]
    return found


def check_case(route, topo, bias, dev, monkeypatch, twin='exact'):
    """Both modes of one case on ``dev`` (kernel set already behind ``ops.kernels()``): the list of findings, empty = pass."""
    model, sd, s = build(route, topo, bias)
    found = []
    keys = [k for k in sd if k.endswith('.b') or (k.startswith('out_proj.') and k.endswith('.bias'))]
    if bool(keys) != bias:
        found.append(f'use_bias={bias}: state dict has {keys}')
    if route.queen:
        k = ops.kernels()
        op = csr_operand(s['graph'], torch.device(dev))
        assert op.fwd_ring2 is not None and op.bwd_ring2 is not None and k.ring2_fits(2, s['N'], route.C, route.hidden)
    want64, want32 = oracle(route, topo, bias)
    spies = Spies(monkeypatch, dev)
    for mode in MODES:
        spies.reset()
        graphs = {}
        got = run(model, route, s, dev, mode, graphs if route.name == 'dense-learned-small' else None)
        if dev == 'cuda':
            torch.cuda.synchronize()
        tag = f'model_lattice[{case_id(route, topo, bias)}-{mode}{"" if dev == "cuda" else "-" + twin}]'
        found += [f'{tag}: {f}' for f in route_findings(route, mode, spies, dev)]
        found += value_findings(tag, route, mode, got, graphs, want64, want32, dev)
    return found


# ---- CPU kernel sets --------------------------------------------------------------------------------------------------------------------------------
def twin_of(kind):
    from oracle.kernel_emul import EmulatedKernels
    return {'exact': EmulatedKernels, 'first-step': FirstStepTwin, 'f16x2': lambda: EmulatedKernels(operand_format='f16x2')}[kind]()


class BiaslessFirstStep(FirstStepTwin):
    """Negative control: a first-step gates launch that loses its bias."""

    def cell_gates_fwd_first(self, X, SX, Tc, W, bias, U, post, act_amax=None):
        return super().cell_gates_fwd_first(X, SX, Tc, W, None, U, post, act_amax=act_amax)


def wrong_decoder_edge(real):
    """Negative control: ``ops.stc_cell_graph`` with one wrong edge -- the decoder's first step takes layer l's state from encoder layer
    (l + 1) % layers.  (The module's schedule: encoder cells layer-major then time, then the decoder step-major; T inputs + one state per layer.)"""
    def call(op, Tc, Ks, schedule, outputs, ext, stacks):
        layers = len(stacks) // 2
        T = len(ext) - layers
        schedule = list(schedule)
        for l in range(layers):
            j = layers * T + l
            s_id, x, hs = schedule[j]
            assert hs == ('cell', l * T + T - 1)
            schedule[j] = (s_id, x, ('cell', ((l + 1) % layers) * T + T - 1))
        return real(op, Tc, Ks, schedule, outputs, ext, stacks)
    return call
