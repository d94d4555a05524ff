"""``STCGNN(graph_mode='csr-learned', csr_cells='fused')``: the learned graph on a sparse pattern through the few-category cell executor
(``small._StcSmallGraph``), whose backward forms the value gradient at the stored entries (``stc_graph_grad_csr_f32``) -- instead of one
autograd node per cell with ``stc_csr_sddmm_f32``.  Opt-in: ``SpatialOperand.sampled_grad`` (``learned_csr_operand(..., sampled_grad=True)``),
Chebyshev order 2, a kernel set with ``graph_grad_csr``; everything else answers as before.

CPU: the predicate's truth table on stub kernel sets (as tests/test_small_dense_split.py builds them); constructor, generator, Trainer and CLI plumbing.
GPU (-m gpu): ``_model_case`` / ``_restated`` / ``_check_model`` and the ``routed`` fixture of tests/test_mgp_csr.py at K = 2, hidden 16, on ``ragged``
(N = 240, C = 3: 720 rows per sample -- the split launches, aggregating from global memory) and ``one_side`` (6 x 6, C = 3) with
``STC_SMALL_SPLITS=1`` (whole-cell launches on the staged graph): the route, parity with the float64 restatement at that file's bounds, the
generator's gradients against the per-cell route, run-to-run and eager-against-replayed bits, and the fallbacks."""
import os

import pytest
import torch

import STC_GNN as M
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, _lib, ops, small
from stc_hip.graph import csr_operand, learned_csr_operand
from tests import graph_cases
from tests.conftest import REPO, rel_err
from tests.test_mgp_csr import LAUNCHED, _check_model, _log, _model_case, _restated, hip, routed      # noqa: F401 (fixtures)
from tests.test_small_dense_order3 import _StubKernels

K, HIDDEN, C = 2, 16, 3
SEED = 10 * K + HIDDEN                 # that of test_the_model_against_the_float64_restatement; on one_side it keeps every score off relu's edge too
SPARSE, CSR_GRAD = 'stc_csr_sddmm_f32', 'stc_graph_grad_csr_f32'


# ============================================================================================================== CPU
def _sampled_stub():
    return type('SampledStub', (_StubKernels,), dict(graph_grad_csr=lambda *a, **kw: None))()


def _operand(graph, sampled, learned=True):
    vals = torch.from_numpy(graph._host['bwd_val']).clone().requires_grad_(learned)
    return learned_csr_operand(graph, vals) if sampled is None else learned_csr_operand(graph, vals, sampled_grad=sampled)


def _supported(k, op, Ks=2, Cc=C):
    return small.small_graph_supported(k, op, torch.zeros(Ks, Cc, Cc), Ks, Cc, 16, {1, 16})


def test_the_predicate_takes_a_sparse_learned_graph_only_when_asked():
    graph = graph_cases.case('one_side')[0]
    stub, bare = _sampled_stub(), _StubKernels()
    assert _supported(stub, _operand(graph, True))                                  # the conjunction: sampled_grad, order 2, the attribute
    assert not _supported(stub, _operand(graph, None)) and not _supported(stub, _operand(graph, False))        # the default operand
    assert not _supported(stub, _operand(graph, True), Ks=3)                        # order 3 keeps the general path
    assert not _supported(bare, _operand(graph, True)) and not hasattr(bare, 'graph_grad_csr')                  # a kernel set without the product
    assert not _supported(EmulatedKernels(), _operand(graph, True)) and not hasattr(EmulatedKernels, 'graph_grad_csr')
    assert hasattr(_lib.HipKernels, 'graph_grad_csr')                              # on the class: ``for_graph`` views have it
    # the rows rules stay: 16 categories above 4 096 rows per sample
    big = CsrGraph.queen_grid(17, 16)
    assert _supported(stub, _operand(big, True), Cc=8) and not _supported(stub, _operand(big, True), Cc=16)
    small_rows = type('Few', (_StubKernels,), dict(graph_grad_csr=None, SMALL_PREFERRED_ROWS=100))()
    assert not _supported(small_rows, _operand(graph, True))                        # 108 rows against SMALL_PREFERRED_ROWS = 100
    # a graph that needs no gradient is answered as a fixed sparse graph, whatever the field says
    for k in (stub, bare):
        assert _supported(k, _operand(graph, True, learned=False)) == _supported(k, _operand(graph, None, learned=False)) == _supported(k, csr_operand(graph, 'cpu'))
    # the full pattern requiring grad is the dense learned graph, as before
    full = CsrGraph.from_dense(torch.rand(6, 6) + 0.1)
    assert _supported(bare, _operand(full, None)) and _supported(stub, _operand(full, True), Ks=3)


def test_the_operand_carries_the_field_last():
    graph = graph_cases.case('one_side')[0]
    import dataclasses
    assert [f.name for f in dataclasses.fields(type(csr_operand(graph, 'cpu')))][-1] == 'sampled_grad'
    assert csr_operand(graph, 'cpu').sampled_grad is False and _operand(graph, None).sampled_grad is False and _operand(graph, True).sampled_grad is True


def test_the_constructor_and_the_generator():
    graph = graph_cases.case('one_side')[0]
    make = lambda **kw: M.STCGNN(graph.n, C, K, K, 1, HIDDEN, 1, 2, fusion_rank=2, **kw)
    assert make(graph_mode='csr-learned', spatial_graph=graph).csr_cells == 'per-cell'
    model = make(graph_mode='csr-learned', spatial_graph=graph, csr_cells='fused')
    assert model.csr_cells == 'fused'
    with pytest.raises(ValueError, match='csr_cells'):
        make(graph_mode='csr-learned', spatial_graph=graph, csr_cells='both')
    for mode in ('dense-learned', 'csr-fixed'):
        with pytest.raises(ValueError, match="csr_cells='fused'"):
            make(graph_mode=mode, csr_cells='fused')
        assert make(graph_mode=mode).csr_cells == 'per-cell'
    # the generator puts its attribute on the operand it returns
    gen = model.mix_graph_pair
    X, Ac = torch.rand(2, 3, graph.n, C), torch.softmax(torch.randn(C, C), -1)
    assert gen.sampled_grad is False and gen(X, graph, Ac)[0].sampled_grad is False
    gen.sampled_grad = True
    assert gen(X, graph, Ac)[0].sampled_grad is True


def test_the_attribute_is_read_at_every_forward(monkeypatch):
    graph = graph_cases.case('one_side')[0]
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    model = M.STCGNN(graph.n, C, K, K, 1, 4, 1, 1, graph_mode='csr-learned', fusion_rank=2, spatial_graph=graph, csr_cells='fused')
    seen = []
    real = M.learned_csr_operand
    monkeypatch.setattr(M, 'learned_csr_operand', lambda g, v, s=False: (seen.append(s), real(g, v, s))[1])
    X, Ac = torch.rand(1, 2, graph.n, C), torch.softmax(torch.randn(C, C), -1)
    y_fused = model(X_seq=X, As=graph, Ac=Ac)
    model.csr_cells = 'per-cell'
    y_cell = model(X_seq=X, As=graph, Ac=Ac)
    assert seen == [True, False] and torch.equal(y_fused, y_cell)                  # the twin declines: the same per-cell path, the same bits


def test_the_trainer_and_the_command_line(tmp_path, monkeypatch):
    from stc_hip import data as sdata
    from stc_hip.trainer import Trainer
    from tests.golden.make_golden import pipeline_inputs
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    _, params = pipeline_inputs()
    params = dict(params, H=6, W=8, C=3, output_dir=str(tmp_path), _allow_cpu_for_tests=True, fusion_rank=3)
    data = sdata.synthetic_incidents(6, 8, 3, 40, sparse_graph=True)
    assert Trainer(params, data, graph_mode='csr-learned').model.csr_cells == 'per-cell'
    assert Trainer(dict(params, csr_cells='fused'), data, graph_mode='csr-learned').model.csr_cells == 'fused'
    with pytest.raises(ValueError, match='csr_cells'):
        Trainer(dict(params, csr_cells='fast'), data, graph_mode='csr-learned')
    fixed = {k: v for k, v in params.items() if k != 'fusion_rank'}
    with pytest.raises(ValueError, match="csr_cells='fused'"):
        Trainer(dict(fixed, csr_cells='fused'), data, graph_mode='csr-fixed')
    src = open(os.path.join(REPO, 'tools', 'train.py')).read()
    assert "'-cells', '--csr_cells'" in src and "choices=['per-cell', 'fused']" in src and "for key in ('fusion_rank', 'csr_cells'):" in src


def test_no_new_autograd_function():
    """The gradient lives inside ``_StcSmallGraph`` (tests/test_autograd_contract.py counts the package's Functions)."""
    from torch.autograd import Function
    assert [n for n, v in vars(small).items() if isinstance(v, type) and issubclass(v, Function) and v is not Function] == ['_StcSmallGraph']


# ============================================================================================================== GPU
def _graph(name):
    return graph_cases.case(name)[0]


def _setup(name, monkeypatch):
    if name == 'one_side':
        monkeypatch.setenv('STC_SMALL_SPLITS', '1')                  # whole-cell launches: the staged graph
    return _graph(name)


def _run(model, graph, X, Ac, Rw, cells):
    """One forward + backward with ``csr_cells`` = ``cells``: (prediction, {parameter: gradient})."""
    model.csr_cells = cells
    model.zero_grad(set_to_none=True)
    y = model(X_seq=X, As=graph, Ac=Ac)
    (y * Rw).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def _bits_equal(a, b):
    (ya, ga), (yb, gb) = a, b
    same = lambda x, y: (x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32))
    return same(ya, yb) and ga.keys() == gb.keys() and all(same(ga[k], gb[k]) for k in ga)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['ragged', 'one_side'])
def test_the_fused_route_and_its_parity(routed, monkeypatch, name):
    graph = _setup(name, monkeypatch)
    model, X, Ac, Rw = _model_case(graph, C, K, HIDDEN, seed=SEED)
    y64, g64, noise, _ = _restated(model, graph, X, Ac, Rw, K, HIDDEN)
    model, dev = model.cuda(), [t.cuda() for t in (X, Ac, Rw)]
    y, grads = _run(model, graph, *dev, 'fused')
    # the route
    assert 'stc_cell_small_fwd_f32' in routed and SPARSE not in routed, sorted(set(routed))
    assert routed.count(CSR_GRAD) == 4, routed.count(CSR_GRAD)                      # two layers: 2 jobs per input-width group
    assert 'stc_graph_grad_f32' not in routed
    for entry in LAUNCHED:
        assert routed.count(entry) == 1, (entry, routed.count(entry))
    print(f'{name}: {routed.count("stc_cell_small_fwd_f32")} forward and {routed.count("stc_cell_small_bwd_f32")} backward cell launches')
    # parity with the float64 restatement, at the bounds of test_the_model_against_the_float64_restatement
    _check_model(f'csr-learned fused {name} K={K} h={HIDDEN}', y, grads, y64, g64, noise)
    # two fused runs: the same bits
    assert _bits_equal((y, grads), _run(model, graph, *dev, 'fused'))
    # the generator's gradients against the per-cell route: two fp32 paths against one truth
    del routed[:]
    y_cell, cell = _run(model, graph, *dev, 'per-cell')
    assert SPARSE in routed and CSR_GRAD not in routed and 'stc_cell_small_fwd_f32' not in routed
    failures = []
    for k in (k for k in g64 if k.startswith('mix_graph_pair.')):
        err, own = rel_err(grads[k], cell[k]), rel_err(cell[k], g64[k])
        _log(f'csr-learned fused {name} d{k} vs per-cell', err, own, max(1e-5, own))
        print(name, k, f'fused vs per-cell {err:.2e}, per-cell vs float64 {own:.2e}')
        if not err < max(1e-5, own):
            failures.append((k, err, max(1e-5, own)))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize('Ks,hidden', [(3, 16), (2, 4)])
def test_where_the_predicate_declines_fused_is_per_cell_bit_for_bit(routed, Ks, hidden):
    graph = _graph('one_side')
    model, X, Ac, Rw = _model_case(graph, C, Ks, hidden, seed=SEED)
    model, dev = model.cuda(), [t.cuda() for t in (X, Ac, Rw)]
    fused = _run(model, graph, *dev, 'fused')
    assert SPARSE in routed and CSR_GRAD not in routed and 'stc_cell_small_fwd_f32' not in routed
    assert _bits_equal(fused, _run(model, graph, *dev, 'per-cell'))


@pytest.mark.gpu
def test_a_frozen_generator_takes_the_route_of_a_fixed_graph(routed):
    graph = _graph('one_side')
    model, X, Ac, Rw = _model_case(graph, C, K, HIDDEN, seed=SEED)
    model, dev = model.cuda(), [t.cuda() for t in (X, Ac, Rw)]
    for p in model.mix_graph_pair.parameters():
        p.requires_grad_(False)
    fused = _run(model, graph, *dev, 'fused')
    assert 'stc_cell_small_fwd_f32' in routed and SPARSE not in routed and CSR_GRAD not in routed          # nothing learned: no graph gradient at all
    first = list(routed)
    del routed[:]
    assert _bits_equal(fused, _run(model, graph, *dev, 'per-cell')) and routed == first
    assert all(g is None for k, g in fused[1].items() if k.startswith('mix_graph_pair.'))


@pytest.mark.gpu
def test_one_trainer_epoch_fused_eager_and_replayed(tmp_path, monkeypatch):
    """The shape of tests/test_mgp_csr.py::test_one_trainer_epoch_eager_and_replayed with ``csr_cells='fused'``: bitwise equal parameters, a
    falling loss, and the fused route in both."""
    from stc_hip import data as sdata
    from stc_hip.trainer import Trainer
    monkeypatch.setattr(ops, '_kernels', None)
    launched = []
    inner = _lib.HipKernels._launch
    monkeypatch.setattr(_lib.HipKernels, '_launch', lambda self, name, *a, **kw: (launched.append(name), inner(self, name, *a, **kw))[1])
    data = sdata.synthetic_incidents(6, 8, 3, 40, sparse_graph=True)
    params = dict(device='cuda:0', H=6, W=8, C=3, batch_size=4, obs_len=3, pred_len=2, split_ratio=[6, 1, 1], model='STC-GNN', cheby_order=2,
                  hidden_dim=16, nn_layers=1, learn_rate=2e-3, decay_rate=1e-4, num_epochs=2, time_slice=4, city='SYN', fusion_rank=4, csr_cells='fused')
    flat, hist = {}, {}
    for graphed in (False, True):
        out = tmp_path / str(graphed)
        os.makedirs(out)
        del launched[:]
        loaders = sdata.get_data_loader(params, data, params['obs_len'], params['pred_len'], params['split_ratio'])
        torch.manual_seed(123)
        trainer = Trainer(dict(params, output_dir=str(out)), data, graph_mode='csr-learned', hip_graph=graphed)
        assert trainer.model.csr_cells == 'fused'
        hist[graphed] = trainer.train(loaders, verbose=False)['loss']
        flat[graphed] = {k: p.detach().clone() for k, p in trainer.model.named_parameters()}
        assert CSR_GRAD in launched and SPARSE not in launched, sorted(set(launched))
        if graphed:
            assert any(slot[1] is not None for slot in trainer._captured.values()), 'no step was captured'
    assert hist[False]['train'][1] < hist[False]['train'][0], hist                # the loss falls
    differ = {k: float((flat[True][k] - v).abs().max()) for k, v in flat[False].items() if not torch.equal(flat[True][k].view(torch.int32), v.view(torch.int32))}
    print('parameters that differ between eager and replayed training:', differ)
    assert not differ, differ
