"""``STCGNN(graph_mode='csr-learned', csr_cells='fused')`` at C in {32, 64}: both learned graphs inside the general cell-graph executor
(``ops._StcCellGraph``, one autograd node).  Every cell runs in ``_Form.PLANAR`` and keeps its Bm plane; its backward adds the cell's share of the
spatial values' gradient at the stored entries (``stc_graph_grad_csr_pairs_f32``: < dS.X, X > + < dS.H, H > + < dY, Bm >, the d(S.x) plane of a
narrow input from ``stc_cell_dsx_narrow_planar_f32``) and of dT_c[1] (``stc_cell_dtc_*_planar_f32``) -- instead of one autograd node per cell with
``stc_csr_sddmm_f32``.  Opt-in through ``SpatialOperand.sampled_grad``; ``ops._dval_route`` is the predicate.

CPU: the predicate as a conjunction on stub kernel sets (one clause flipped at a time; values that require grad without ``sampled_grad`` are
refused as before); the forms and what they save; ``first_step_route`` off in the mode; on the emulated kernels ``'fused'`` and ``'per-cell'`` give
equal bits at C = 32.

GPU (-m gpu): K = 2, hidden 16, rank 4 on a 4 x 4 queen grid (2 samples, C = 32, with and without bias), a 6 x 7 grid (3 samples, C = 64) and the
``ragged`` case of tests/graph_cases.py (C = 32), each at (layers, T, horizon) = (2, 2, 2), (1, 1, 1) -- a zero state feeds every encoder cell --
and (1, 3, 2) -- the first decoder cell reads one state both as x and as hs.  ``_model_case`` / ``_restated`` / ``_check_model`` and the ``routed``
fixture of tests/test_mgp_csr.py: the route, parity with the float64 restatement at that file's bounds (forward <= max(1e-5, 3 x noise),
gradients <= max(2e-5, 10 x noise)), the generator's gradients against the per-cell route, run-to-run bits, eager against replayed training,
and the fallbacks.  The seeds keep every score of the float64 run off relu's edge (``_restated`` asserts it on the CPU, before any launch)."""
import os

import pytest
import torch

import STC_GNN as M
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, _lib, ops
from stc_hip.graph import csr_operand, learned_csr_operand
from tests import graph_cases
from tests.conftest import rel_err
from tests.test_csr_cells_fused import _bits_equal, _run
from tests.test_gc_learned import _PlanarStub, _ask, _tc
from tests.test_mgp_csr import _check_model, _log, _model_case, _restated, hip, routed      # noqa: F401 (fixtures)

K, HIDDEN, RANK = 2, 16, 4
PAIRS, DSX, SPARSE, SMALL = 'stc_graph_grad_csr_pairs_f32', 'stc_cell_dsx_narrow_planar_f32', 'stc_csr_sddmm_f32', 'stc_cell_small_fwd_f32'
DTC_GATES, DTC_CAND = 'stc_cell_dtc_gates_planar_f32', 'stc_cell_dtc_cand_planar_f32'


# ============================================================================================================== CPU
class _ValsStub(_PlanarStub):
    """A kernel set of the general executor that says yes to every planar shape and carries both capabilities."""
    cell_graph_vals = True


def _learned(graph, sampled=True, grad=True):
    vals = torch.from_numpy(graph._host['bwd_val']).clone().requires_grad_(grad)
    return learned_csr_operand(graph, vals, sampled_grad=sampled)


def test_the_predicate_is_a_conjunction(monkeypatch):
    graph = CsrGraph.queen_grid(4, 4)
    op = _learned(graph)
    monkeypatch.setattr(ops, '_kernels', _ValsStub())
    assert _ask(op, _tc(), learn_Tc=True)                                          # every clause holds: both graphs learned
    assert _ask(op, _tc(grad=False)) and _ask(op, _tc(grad=False), learn_Tc=True)  # a Tc that needs no gradient: the value route alone
    assert not _ask(op, _tc()) and not _ask(op, _tc(), learn_Tc=False)             # a Tc that requires grad without the caller's word for it
    # values that require grad but no ``sampled_grad``: refused as before, whatever else holds
    for flag in (False, True):
        assert not _ask(_learned(graph, sampled=False), _tc(), learn_Tc=flag) and not _ask(_learned(graph, sampled=False), _tc(grad=False), learn_Tc=flag)
    # values that need no gradient: the field changes nothing -- the dT_c route, or a fixed graph
    assert _ask(_learned(graph, grad=False), _tc(), learn_Tc=True) and _ask(_learned(graph, grad=False), _tc(grad=False))
    monkeypatch.setattr(ops, '_DVAL', False)
    assert not _ask(op, _tc(), learn_Tc=True) and not _ask(op, _tc(grad=False))    # the switch
    monkeypatch.setattr(ops, '_DVAL', True)
    with torch.no_grad():                                                          # grad mode (a leaf that requires grad is refused as today)
        assert not _ask(op, _tc(grad=False)) and not ops._dval_route(_ValsStub(), op, _tc(), 2, 32, 16, [1, 16], torch.float32)
    full = _learned(CsrGraph.from_dense(torch.rand(6, 6) + 0.1))
    assert not _ask(full, _tc(grad=False)) and not _ask(full, _tc(), learn_Tc=True)                 # the full pattern is the dense learned graph
    assert not _ask(op, _tc(grad=False), dtype=torch.bfloat16)                     # fp32 planes
    assert not _ask(op, _tc(Kc=3, grad=False), Ks=3) and not _ask(op, _tc(Kc=3), Ks=3, learn_Tc=True)       # Ks = Kc = 2
    assert not _ask(op, _tc(grad=False), h=8) and not _ask(op, _tc(grad=False), h=32)               # hidden 16
    for C in (16, 48, 128):
        assert not _ask(op, _tc(C=C, grad=False), C=C), C                          # C in {32, 64}
    assert _ask(op, _tc(C=64, grad=False), C=64)
    assert not _ask(op, _tc(grad=False), widths=(5, 16)) and not _ask(op, _tc(grad=False), widths=(1, 8))          # every input 16 or 1..4 columns wide
    assert all(_ask(op, _tc(grad=False), widths=(w, 16)) for w in (1, 2, 3, 4))
    monkeypatch.setattr(ops, '_kernels', type('NoVals', (_ValsStub,), dict(cell_graph_vals=False))())
    assert not _ask(op, _tc(grad=False)) and not _ask(op, _tc(), learn_Tc=True)    # the capability
    monkeypatch.setattr(ops, '_kernels', _PlanarStub())
    assert not _ask(op, _tc(grad=False)) and not hasattr(_PlanarStub, 'cell_graph_vals')
    monkeypatch.setattr(ops, '_kernels', type('NoDtc', (_ValsStub,), dict(cell_dtc_planar=False))())
    assert not _ask(op, _tc(), learn_Tc=True) and _ask(op, _tc(grad=False))        # without the dT_c kernels: the value route alone still
    monkeypatch.setattr(ops, '_kernels', type('NoPost20', (_ValsStub,), dict(node_post_supported=lambda self, Ks, Kc, C, L, h: L != 20))())
    assert not _ask(op, _tc(grad=False)) and _ask(op, _tc(grad=False), widths=(16,))                # every cell in _Form.PLANAR
    # the CPU twin has neither capability: the per-cell route
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    assert not hasattr(EmulatedKernels, 'cell_graph_vals') and not _ask(op, _tc(), learn_Tc=True) and not _ask(op, _tc(grad=False))
    assert _lib.HipKernels.cell_graph_vals is True                                 # on the class: ``for_graph`` views have it


def test_the_forms_what_they_save_and_the_first_step_route(monkeypatch):
    k = _ValsStub()
    F = ops._Form
    assert ops._cell_forms(k, 2, 2, 32, 16, [1, 16, 16], False) == [F.PLANAR_ONE_BWD] * 3          # the default: unchanged
    assert ops._cell_forms(k, 2, 2, 32, 16, [1, 16, 16], False, learn_Tc=True) == [F.PLANAR] * 3   # what the value gradient forces as well
    assert F.PLANAR.saved(2) == 8 and F.PLANAR.saved(2, True) == 9                  # ... and Bm among the cell's saved planes in the mode only
    for f in F:
        assert f is F.PLANAR or f.saved(2, True) == f.saved(2)
    monkeypatch.setattr(ops, '_kernels', k)
    graph = CsrGraph.queen_grid(4, 4)
    fixed, op = csr_operand(graph, 'cpu'), _learned(graph)
    assert ops.first_step_route(fixed, _tc(grad=False), 2, 32, 16, [1, 16])
    assert not ops.first_step_route(op, _tc(), 2, 32, 16, [1, 16], learn_Tc=True) and not ops.first_step_route(op, _tc(grad=False), 2, 32, 16, [1, 16])
    with torch.no_grad():
        assert ops.first_step_route(op, _tc(), 2, 32, 16, [1, 16], learn_Tc=True)                  # nothing to learn: the forward-only route


def test_the_executor_refuses_by_name_what_it_cannot_learn(monkeypatch):
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    graph = CsrGraph.queen_grid(4, 4)
    ext = [torch.zeros(1, graph.n, 32, 1), torch.zeros(1, graph.n, 32, 16)]
    stacks = [(torch.zeros(4 * 17, 32), None, torch.zeros(4 * 17, 16), None)]
    for sampled in (False, True):                                                  # (the twin lacks the capability: the field alone opens nothing)
        with pytest.raises(ValueError, match='fwd_val requires grad'):
            ops.stc_cell_graph(_learned(graph, sampled=sampled), _tc(grad=False), 2, [(0, ('ext', 0), ('ext', 1))], [0], ext, stacks)
        with pytest.raises(ValueError, match='fwd_val requires grad'):
            ops.stc_cell_graph(_learned(graph, sampled=sampled), _tc(), 2, [(0, ('ext', 0), ('ext', 1))], [0], ext, stacks, learn_Tc=True)


def test_no_new_autograd_function():
    from torch.autograd import Function
    names = [n for n, v in vars(ops).items() if isinstance(v, type) and issubclass(v, Function) and v is not Function and v.__module__ == ops.__name__]
    assert '_StcCellGraph' in names and not [n for n in names if 'dval' in n.lower() or 'pairs' in n.lower()]


def test_on_the_emulated_kernels_fused_is_per_cell_bit_for_bit(monkeypatch):
    """The CPU twin has neither kernel nor capability: ``'fused'`` at C = 32 declines in both executors and runs one autograd node per cell."""
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    graph = CsrGraph.queen_grid(4, 4)
    model, X, Ac, Rw = _model_case(graph, 32, K, HIDDEN, seed=3, layers=2, T=2, horizon=2, B=2, rank=RANK)
    calls = []
    real = ops.stc_cell
    monkeypatch.setattr(ops, 'stc_cell', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    out = {}
    for cells in ('fused', 'per-cell'):
        model.csr_cells = cells
        model.zero_grad(set_to_none=True)
        y = model(X_seq=X, As=graph, Ac=Ac)
        (y * Rw).sum().backward()
        out[cells] = (y.detach(), {k: p.grad.clone() for k, p in model.named_parameters()})
    assert len(calls) == 2 * 2 * (2 + 2)
    assert _bits_equal(out['fused'], out['per-cell']) and all(bool(g.abs().sum() > 0) for g in out['fused'][1].values())


# ============================================================================================================== GPU
def _graph(name):
    return {'grid4x4': lambda: CsrGraph.queen_grid(4, 4), 'grid6x7': lambda: CsrGraph.queen_grid(6, 7), 'ragged': lambda: graph_cases.case('ragged')[0]}[name]()


GRAPHS = [('grid4x4', 32, 2, True), ('grid4x4', 32, 2, False), ('grid6x7', 64, 3, True), ('ragged', 32, 2, True)]
TOPOLOGIES = [(2, 2, 2), (1, 1, 1), (1, 3, 2)]                     # (layers, T, horizon)
CASES = [(*g, *t) for g in GRAPHS for t in TOPOLOGIES]
_IDS = [f'{n}-C{c}-B{b}-{"bias" if bias else "nobias"}-L{l}T{t}H{h}' for n, c, b, bias, l, t, h in CASES]
_REF = {}


def _seed(name, C, B, bias, layers, T, horizon):
    """At these seeds no score of the float64 run sits within the margin of relu's edge (checked on the CPU for all twelve; ``_restated`` asserts it)."""
    return 100 + C + B + 10 * layers + T + horizon


def _case(name, C, B, bias, layers, T, horizon):
    """(graph, model on the CPU, X, Ac, Rw) of one case; without bias the same construction with ``use_bias=False``."""
    graph, seed = _graph(name), _seed(name, C, B, bias, layers, T, horizon)
    model, X, Ac, Rw = _model_case(graph, C, K, HIDDEN, seed=seed, layers=layers, T=T, horizon=horizon, B=B, rank=RANK)
    if not bias:
        torch.manual_seed(seed)
        model = M.STCGNN(graph.n, C, K, K, 1, HIDDEN, layers, horizon, use_bias=False, graph_mode='csr-learned', fusion_rank=RANK, spatial_graph=graph)
    return graph, model, X, Ac, Rw


def _reference(*case):
    """The case and its float64 truth, computed once and shared (never modified)."""
    if case not in _REF:
        graph, model, X, Ac, Rw = _case(*case)
        layers, horizon = case[4], case[6]
        _REF[case] = (graph, model.state_dict(), X, Ac, Rw, _restated(model, graph, X, Ac, Rw, K, HIDDEN, layers=layers, horizon=horizon))
    return _REF[case]


def _fresh(*case):
    graph, sd, X, Ac, Rw, ref = _reference(*case)
    name, C, B, bias, layers, T, horizon = case
    model = M.STCGNN(graph.n, C, K, K, 1, HIDDEN, layers, horizon, use_bias=bias, graph_mode='csr-learned', fusion_rank=RANK, spatial_graph=graph, csr_cells='fused')
    model.load_state_dict(sd)
    return graph, model.cuda(), [t.cuda() for t in (X, Ac, Rw)], ref


@pytest.mark.gpu
@pytest.mark.parametrize('name,C,B,bias,layers,T,horizon', CASES, ids=_IDS)
def test_the_fused_route_and_its_parity(routed, name, C, B, bias, layers, T, horizon):
    graph, model, dev, (y64, g64, noise, _) = _fresh(name, C, B, bias, layers, T, horizon)
    y, grads = _run(model, graph, *dev, 'fused')
    cells = layers * (T + horizon)            # every cell is owed a gradient: the last decoder step's top layer is an output, everything else feeds it
    # the route: one pairs launch per cell, one d(S.x) launch per cell with a narrow input (the encoder's layer 0), no per-cell value gradient
    assert routed.count(PAIRS) == cells and routed.count(DSX) == T, (routed.count(PAIRS), routed.count(DSX))
    assert SPARSE not in routed and SMALL not in routed and 'stc_graph_grad_csr_f32' not in routed, sorted(set(routed))
    assert routed.count(DTC_GATES) == cells and routed.count(DTC_CAND) == cells     # both graphs are learned in the one node
    assert 'stc_cell_gates_bwd_planar_f32' in routed and 'stc_bdg_node_bwd_f32' not in routed and 'stc_cell_bwd_planar_f32' not in routed
    assert all(g is not None and bool(torch.isfinite(g).all()) and bool(g.abs().sum() > 0) for g in grads.values()), [k for k, g in grads.items() if g is None]
    # parity with the float64 restatement
    _check_model(f'csr-learned cell graph {name} C={C} B={B} bias={bias} L{layers} T{T} H{horizon}', y, grads, y64, g64, noise)
    # two runs: the same bits
    assert _bits_equal((y, grads), _run(model, graph, *dev, 'fused'))
    # the generator's gradients against the per-cell route: two fp32 paths against one truth
    del routed[:]
    y_cell, cell = _run(model, graph, *dev, 'per-cell')
    assert SPARSE in routed and PAIRS not in routed and DSX not in routed and DTC_GATES not in routed
    failures = []
    for k in (k for k in g64 if k.startswith('mix_graph_pair.')):
        err, own = rel_err(grads[k], cell[k]), rel_err(cell[k], g64[k])
        _log(f'csr-learned cell graph {name} L{layers} T{T} H{horizon} d{k} vs per-cell', err, own, max(1e-5, own))
        print(name, k, f'fused vs per-cell {err:.2e}, per-cell vs float64 {own:.2e}')
        if not err < max(1e-5, own):
            failures.append((k, err, max(1e-5, own)))
    assert not failures, failures
    assert rel_err(y, y_cell) < 1e-5


@pytest.mark.gpu
def test_with_the_switch_off_fused_is_per_cell_bit_for_bit(routed, monkeypatch):
    graph, model, dev, _ = _fresh(*CASES[0])
    monkeypatch.setattr(ops, '_DVAL', False)
    fused = _run(model, graph, *dev, 'fused')
    assert SPARSE in routed and PAIRS not in routed and DSX not in routed and DTC_GATES not in routed
    assert _bits_equal(fused, _run(model, graph, *dev, 'per-cell'))


@pytest.mark.gpu
@pytest.mark.parametrize('Ks,hidden', [(3, 16), (2, 4)])
def test_where_the_predicate_declines_fused_is_per_cell_bit_for_bit(routed, Ks, hidden):
    graph = _graph('grid4x4')
    model, X, Ac, Rw = _model_case(graph, 32, Ks, hidden, seed=10 * Ks + hidden, layers=2, T=2, horizon=2, B=2, rank=RANK)
    model, dev = model.cuda(), [t.cuda() for t in (X, Ac, Rw)]
    fused = _run(model, graph, *dev, 'fused')
    assert SPARSE in routed and PAIRS not in routed and DSX not in routed and SMALL not in routed
    assert _bits_equal(fused, _run(model, graph, *dev, 'per-cell'))


@pytest.mark.gpu
def test_a_frozen_category_generator_is_the_value_route_alone(routed):
    """``Gc`` needs no gradient, the spatial values do: the pairs launches without the dT_c launches; frozen altogether: a fixed graph's route."""
    case = CASES[0]
    graph, model, dev, _ = _fresh(*case)
    gen = model.mix_graph_pair
    frozen = [p for n, p in gen.named_parameters() if n.startswith(('params_C', 'aggreg_C'))]
    assert frozen
    for p in frozen:
        p.requires_grad_(False)
    y, grads = _run(model, graph, *dev, 'fused')
    cells = case[4] * (case[5] + case[6])
    assert routed.count(PAIRS) == cells and DTC_GATES not in routed and DTC_CAND not in routed and SPARSE not in routed
    del routed[:]
    y_cell, cell = _run(model, graph, *dev, 'per-cell')
    assert SPARSE in routed and rel_err(y, y_cell) < 1e-5
    for k, g in grads.items():
        assert (g is None) == (cell[k] is None), k
        if g is not None and k.startswith('mix_graph_pair.'):
            assert rel_err(g, cell[k]) < 1e-4, (k, rel_err(g, cell[k]))
    for p in gen.parameters():
        p.requires_grad_(False)
    del routed[:]
    _run(model, graph, *dev, 'fused')
    assert PAIRS not in routed and DSX not in routed and SPARSE not in routed and 'stc_cell_bwd_planar_f32' in routed       # nothing learned: the one-launch backward


@pytest.mark.gpu
def test_one_trainer_epoch_fused_eager_and_replayed(tmp_path, monkeypatch):
    """The shape of tests/test_csr_cells_fused.py::test_one_trainer_epoch_fused_eager_and_replayed at C = 32: bitwise equal parameters after one
    epoch eager and one replayed from the same seed, and the route in both."""
    from stc_hip import data as sdata
    from stc_hip.trainer import Trainer
    monkeypatch.setattr(ops, '_kernels', None)
    launched = []
    inner = _lib.HipKernels._launch
    monkeypatch.setattr(_lib.HipKernels, '_launch', lambda self, name, *a, **kw: (launched.append(name), inner(self, name, *a, **kw))[1])
    data = sdata.synthetic_incidents(6, 8, 32, 40, sparse_graph=True)
    params = dict(device='cuda:0', H=6, W=8, C=32, batch_size=4, obs_len=3, pred_len=2, split_ratio=[6, 1, 1], model='STC-GNN', cheby_order=2,
                  hidden_dim=16, nn_layers=1, learn_rate=2e-3, decay_rate=1e-4, num_epochs=1, time_slice=4, city='SYN', fusion_rank=4, csr_cells='fused')
    flat = {}
    for graphed in (False, True):
        out = tmp_path / str(graphed)
        os.makedirs(out)
        del launched[:]
        loaders = sdata.get_data_loader(params, data, params['obs_len'], params['pred_len'], params['split_ratio'])
        torch.manual_seed(123)
        trainer = Trainer(dict(params, output_dir=str(out)), data, graph_mode='csr-learned', hip_graph=graphed)
        assert trainer.model.csr_cells == 'fused'
        trainer.train(loaders, verbose=False)
        flat[graphed] = {k: p.detach().clone() for k, p in trainer.model.named_parameters()}
        assert PAIRS in launched and DSX in launched and SPARSE not in launched, sorted(set(launched))
        if graphed:
            assert any(slot[1] is not None for slot in trainer._captured.values()), 'no step was captured'
    differ = {k: float((flat[True][k] - v).abs().max()) for k, v in flat[False].items() if not torch.equal(flat[True][k].view(torch.int32), v.view(torch.int32))}
    assert not differ, differ
