"""``STCGNN(graph_mode='csr-category-learned')``: the spatial graph as in ``'csr-fixed'``, the category graph learned by ``MGP_Gen_Category``, and
in grad mode the cell-graph executor asked for the gradient of ``Gc``'s Chebyshev stack (``ops.stc_cell_graph(learn_Tc=True)``: every cell in
``_Form.PLANAR``, whose backward adds the cell's share of dT_c[1] through ``stc_cell_dtc_gates_planar_f32`` / ``stc_cell_dtc_cand_planar_f32``).

CPU: the predicate as a conjunction on stub kernel sets (as tests/test_csr_cells_fused.py builds them) with every default unchanged; the forms and
``first_step_route`` in the mode; constructor, ``state_dict`` keys and their loading from an ``MGP_Gen`` dict; Trainer refusals and the ``-graph``
choice; on the emulated kernels the mode runs the per-cell path and matches a float64 restatement.

GPU (-m gpu): K = 2, hidden 16, 2 layers, T = 2, horizon 2 on a 4 x 4 queen grid (2 samples, C = 32, with and without bias), a 6 x 7 grid
(3 samples, C = 64) and the ``ragged`` case of tests/graph_cases.py (C = 32).  Truth: the same generator in float64 on the CPU with the cells of
oracle/stc_oracle.py.  Route through the ``routed`` fixture of tests/test_mgp_csr.py; prediction and every parameter gradient at that file's
``_check_model`` bounds (forward <= max(1e-5, 3 x noise), gradients <= max(2e-5, 10 x noise))."""
import os

import pytest
import torch

import STC_GNN as M
from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, _lib, ops
from stc_hip.graph import csr_operand
from tests import graph_cases
from tests.conftest import REPO, rel_err
from tests.test_mgp_csr import _check_model, hip, routed      # noqa: F401 (fixtures)

MODE = 'csr-category-learned'
K, HIDDEN, LAYERS, T, HORIZON = 2, 16, 2, 2, 2
GATES, CAND = 'stc_cell_dtc_gates_planar_f32', 'stc_cell_dtc_cand_planar_f32'
MARGIN = 1e-5                         # relu's edge in the generator: no score of the float64 run within this of 0, but the diagonal's exact zeros


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def gc_restatement(X, Ac, sd, alpha=3.0, p='mix_graph_pair'):
    """(Gc, antisymmetric score) of ``MGP_Gen_Category.forward`` from a state dict, in the operands' precision (reference STC_GNN.py:236-243)."""
    Xc = X.transpose(2, 3)
    Uc = torch.tanh(alpha * torch.matmul(Xc, sd[f'{p}.params_C.Wu']))
    Vc = torch.tanh(alpha * torch.matmul(Xc, sd[f'{p}.params_C.Wv']))
    D = torch.einsum('btnh,btmh->nm', Uc, Vc) - torch.einsum('btmh,btnh->mn', Vc, Uc)
    Gc = O.mixed_fusion(Ac, O._antisym_softmax(Uc, Vc), sd[f'{p}.aggreg_C.lin_A.weight'], sd[f'{p}.aggreg_C.lin_A.bias'],
                        sd[f'{p}.aggreg_C.lin_P.weight'], sd[f'{p}.aggreg_C.lin_P.bias'])
    return Gc, D


def model_restatement(X, graph, Ac, sd, layers=LAYERS, horizon=HORIZON):
    Gc, D = gc_restatement(X, Ac, sd)
    return O.encdec_forward(X, graph.to_dense().to(X.dtype), Gc, sd, K, K, HIDDEN, layers, horizon), D


def _model_case(graph, C, seed, B=2, bias=True, layers=LAYERS, horizon=HORIZON):
    torch.manual_seed(seed)
    model = M.STCGNN(graph.n, C, K, K, 1, HIDDEN, layers, horizon, use_bias=bias, graph_mode=MODE)
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(B, T, graph.n, C, generator=g)
    Ac = torch.softmax(torch.randn(C, C, generator=g), -1)
    Rw = torch.randn(B, horizon, graph.n, C, generator=g)
    return model, X, Ac, Rw


def _restated(model, graph, X, Ac, Rw, **kw):
    """Prediction and parameter gradients of the restatement in float64, and the fp32 run's distance from them (the noise)."""
    out = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in model.state_dict().items()}
        y, D = model_restatement(X.to(dt), graph, Ac.to(dt), sd, **kw)
        (y * Rw.to(dt)).sum().backward()
        out[dt] = (y.detach(), {k: v.grad for k, v in sd.items()}, D.detach())
    D = out[torch.float64][2].abs()
    off = ~torch.eye(D.shape[0], dtype=torch.bool)
    assert bool((D[off] >= MARGIN * D.max()).all()) and bool((D[~off] == 0).all()), 'a score of the window sits on the edge of relu'
    y64, g64, _ = out[torch.float64]
    y32, g32, _ = out[torch.float32]
    return y64, g64, {k: rel_err(g32[k], g64[k]) for k in g64}, rel_err(y32, y64)


# ============================================================================================================== CPU
class _PlanarStub:
    """A kernel set of the general executor that says yes to every planar shape and carries the dT_c capability."""
    cell_dtc_planar = True

    def cell_planar_supported(self, *a):
        return True

    node_post_supported = cell_bwd_planar_supported = cell_fused_supported = cell_first_supported = cell_planar_supported
    first_step_cells = True

    def cell_dtc_planar_supported(self, C, cin, h):
        return C in (32, 64) and h == 16 and (cin == 16 or 1 <= cin <= 4)


def _tc(C=32, Kc=2, grad=True):
    return torch.zeros(Kc, C, C).requires_grad_(grad)


def _ask(op, Tc, Ks=2, C=32, h=16, widths=(1, 16), dtype=torch.float32, **kw):
    return ops.cell_graph_supported(op, Tc, Ks, C, h, list(widths), dtype=dtype, **kw)


def test_the_predicate_is_a_conjunction(monkeypatch):
    graph = CsrGraph.queen_grid(4, 4)
    op = csr_operand(graph, 'cpu')
    monkeypatch.setattr(ops, '_kernels', _PlanarStub())
    assert _ask(op, _tc(), learn_Tc=True)                                          # every clause holds
    assert not _ask(op, _tc()) and not _ask(op, _tc(), learn_Tc=False)             # the caller's word
    bare = type('Bare', (_PlanarStub,), dict(cell_dtc_planar=False))()
    monkeypatch.setattr(ops, '_kernels', bare)
    assert not _ask(op, _tc(), learn_Tc=True)                                      # the capability
    monkeypatch.setattr(ops, '_kernels', _PlanarStub())
    assert not _ask(op, _tc(Kc=3), Ks=3, learn_Tc=True)                            # order 2
    assert not _ask(op, _tc(), dtype=torch.bfloat16, learn_Tc=True)                # fp32 planes
    assert not _ask(op, _tc(), widths=(5, 16), learn_Tc=True) and not _ask(op, _tc(C=16), C=16, learn_Tc=True)       # the widths, the categories
    assert not _ask(op, _tc(), h=8, learn_Tc=True)
    learned_op = csr_operand(graph, 'cpu')
    learned_op.fwd_val = learned_op.fwd_val.clone().requires_grad_()
    assert not _ask(learned_op, _tc(), learn_Tc=True)                              # no gradient for the spatial values
    one_launch_only = type('NoPost20', (_PlanarStub,), dict(node_post_supported=lambda self, Ks, Kc, C, L, h: L != 20))()
    monkeypatch.setattr(ops, '_kernels', one_launch_only)
    assert not _ask(op, _tc(), learn_Tc=True) and _ask(op, _tc(), widths=(16,), learn_Tc=True)     # every cell in _Form.PLANAR
    monkeypatch.setattr(ops, '_kernels', _PlanarStub())
    monkeypatch.setattr(ops, '_DTC', False)
    assert not _ask(op, _tc(), learn_Tc=True)                                      # the switch
    monkeypatch.setattr(ops, '_DTC', True)
    # a Tc that needs no gradient, or grad mode off: today's answer, whatever the flag says
    for flag in (False, True):
        assert _ask(op, _tc(grad=False), learn_Tc=flag)
        with torch.no_grad():
            assert _ask(op, _tc(grad=False), learn_Tc=flag) and not _ask(op, _tc(), learn_Tc=flag)     # (a leaf that requires grad is refused as today)
    # the CPU twin has no capability: the per-cell route
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    assert not hasattr(EmulatedKernels, 'cell_dtc_planar') and not _ask(op, _tc(), learn_Tc=True) and _ask(op, _tc(grad=False), learn_Tc=True)


def test_the_forms_and_the_first_step_route(monkeypatch):
    k = _PlanarStub()
    F = ops._Form
    assert ops._cell_forms(k, 2, 2, 32, 16, [1, 16, 16], False) == [F.PLANAR_ONE_BWD] * 3          # the default: unchanged
    assert ops._cell_forms(k, 2, 2, 32, 16, [1, 16, 16], False, learn_Tc=True) == [F.PLANAR] * 3
    assert ops._cell_forms(k, 2, 2, 32, 16, [7, 16], False, learn_Tc=True)[0] is F.ROWS_POST       # (a width the planar kernels do not take)
    monkeypatch.setattr(ops, '_kernels', k)
    op = csr_operand(CsrGraph.queen_grid(4, 4), 'cpu')
    assert ops.first_step_route(op, _tc(), 2, 32, 16, [1, 16]) and ops.first_step_route(op, _tc(grad=False), 2, 32, 16, [1, 16], learn_Tc=True)
    assert not ops.first_step_route(op, _tc(), 2, 32, 16, [1, 16], learn_Tc=True)
    with torch.no_grad():
        assert ops.first_step_route(op, _tc(), 2, 32, 16, [1, 16], learn_Tc=True)                  # nothing to learn: the forward-only route


def test_the_executor_refuses_by_name_what_it_cannot_learn(monkeypatch):
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    graph = CsrGraph.queen_grid(4, 4)
    op = csr_operand(graph, 'cpu')
    ext = [torch.zeros(1, graph.n, 32, 1), torch.zeros(1, graph.n, 32, 16)]
    stacks = [(torch.zeros(4 * 17, 32), None, torch.zeros(4 * 17, 16), None)]
    with pytest.raises(ValueError, match='Tc requires grad'):                      # the default refusal, unchanged
        ops.stc_cell_graph(op, _tc(), 2, [(0, ('ext', 0), ('ext', 1))], [0], ext, stacks)
    with pytest.raises(ValueError, match='learn_Tc needs'):                        # asked, on a kernel set without the kernels
        ops.stc_cell_graph(op, _tc(), 2, [(0, ('ext', 0), ('ext', 1))], [0], ext, stacks, learn_Tc=True)


def test_the_constructor_the_keys_and_loading_from_the_reference_generator():
    N, C = 12, 5
    torch.manual_seed(0)
    model = M.STCGNN(N, C, K, K, 1, HIDDEN, 1, 2, graph_mode=MODE)
    gen = model.mix_graph_pair
    assert isinstance(gen, M.MGP_Gen_Category) and isinstance(gen, M.MGP_Gen) and gen.batch_sharded is False
    keys = [k for k in model.state_dict() if k.startswith('mix_graph_pair.')]
    assert keys == ['mix_graph_pair.params_C.Wu', 'mix_graph_pair.params_C.Wv', 'mix_graph_pair.aggreg_C.lin_A.weight', 'mix_graph_pair.aggreg_C.lin_A.bias',
                    'mix_graph_pair.aggreg_C.lin_P.weight', 'mix_graph_pair.aggreg_C.lin_P.bias']
    assert tuple(gen.params_C['Wu'].shape) == (N, HIDDEN) and gen.aggreg_C.lin_A.weight.shape == (C * C, C * C)
    assert M.STCGNN(N, C, K, K, 1, HIDDEN, 1, 2, graph_mode=MODE, batch_sharded=True).mix_graph_pair.batch_sharded is True
    full = M.MGP_Gen(N, C, HIDDEN).state_dict()
    mine = {k: v for k, v in full.items() if k.startswith(('params_C', 'aggreg_C'))}
    assert sorted('mix_graph_pair.' + k for k in mine) == sorted(keys)
    assert gen.load_state_dict(mine).missing_keys == []
    # ... and gives the reference generator's category graph
    X, Ac = torch.rand(2, 3, N, C), torch.softmax(torch.randn(C, C), -1)
    ref = M.MGP_Gen(N, C, HIDDEN)
    ref.load_state_dict(full)
    assert torch.equal(gen(X, Ac), ref(X, torch.rand(N, N), Ac)[1])
    with pytest.raises(ValueError, match='csr-category-learned'):
        M.STCGNN(N, C, K, K, 1, HIDDEN, 1, 2, graph_mode='category-learned')
    with pytest.raises(ValueError, match='bfloat16'):
        M.STCGNN(N, C, K, K, 1, HIDDEN, 1, 2, graph_mode=MODE, storage_dtype=torch.bfloat16)


def test_the_trainer_and_the_command_line(tmp_path, monkeypatch):
    from stc_hip import data as sdata
    from stc_hip.trainer import Trainer
    from tests.golden.make_golden import pipeline_inputs
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    _, params = pipeline_inputs()
    params = dict(params, H=6, W=8, C=3, output_dir=str(tmp_path), _allow_cpu_for_tests=True)
    data = sdata.synthetic_incidents(6, 8, 3, 40, sparse_graph=True)
    trainer = Trainer(params, data, graph_mode=MODE)
    assert isinstance(trainer.prior_graph[0], CsrGraph) and isinstance(trainer.model.mix_graph_pair, M.MGP_Gen_Category)
    with pytest.raises(ValueError, match='fusion_rank'):
        Trainer(dict(params, fusion_rank=3), data, graph_mode=MODE)
    with pytest.raises(ValueError, match='csr_cells'):
        Trainer(dict(params, csr_cells='fused'), data, graph_mode=MODE)
    src = open(os.path.join(REPO, 'tools', 'train.py')).read()
    assert "choices=['dense-learned', 'csr-fixed', 'csr-learned', 'csr-category-learned']" in src
    assert "'-cells', '--csr_cells'" in src and "choices=['per-cell', 'fused']" in src              # the -cells line: untouched


@pytest.mark.parametrize('reorder', [True, False])
def test_on_the_emulated_kernels_the_mode_runs_per_cell_and_matches_float64(monkeypatch, reorder):
    """The CPU twin lacks the capability: one autograd node per cell (``_StcCell`` differentiates ``Tc``), every gradient present; the graph is
    given in a shuffled node order, so with ``reorder_nodes`` the generator must have seen the window before the renumbering."""
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    graph = CsrGraph.queen_grid(4, 5, permute_seed=3)
    model, X, Ac, Rw = _model_case(graph, 32, seed=7)
    model.reorder_nodes = reorder
    calls = []
    real = ops.stc_cell
    monkeypatch.setattr(ops, 'stc_cell', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    y64, g64, noise, _ = _restated(model, graph, X, Ac, Rw)
    y = model(X_seq=X, As=graph, Ac=Ac)
    (y * Rw).sum().backward()
    assert len(calls) == LAYERS * (T + HORIZON)
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(g is not None and bool(g.abs().sum() > 0) for g in grads.values())
    _check_model(f'{MODE} emulated reorder={reorder}', y, grads, y64, g64, noise)


def test_no_new_autograd_function():
    from torch.autograd import Function
    names = [n for n, v in vars(ops).items() if isinstance(v, type) and issubclass(v, Function) and v is not Function and v.__module__ == ops.__name__]
    assert '_StcCellGraph' in names and not [n for n in names if 'dtc' in n.lower() or 'Dtc' in n]


# ============================================================================================================== GPU
def _graph(name):
    return {'grid4x4': lambda: CsrGraph.queen_grid(4, 4), 'grid6x7': lambda: CsrGraph.queen_grid(6, 7), 'ragged': lambda: graph_cases.case('ragged')[0]}[name]()


CASES = [('grid4x4', 32, 2, True), ('grid4x4', 32, 2, False), ('grid6x7', 64, 3, True), ('ragged', 32, 2, True)]
_IDS = [f'{n}-C{c}-B{b}-{"bias" if bias else "nobias"}' for n, c, b, bias in CASES]
_REF = {}


def _reference(name, C, B, bias):
    """The case and its float64 truth, computed once and shared (never modified)."""
    key = (name, C, B, bias)
    if key not in _REF:
        graph = _graph(name)
        model, X, Ac, Rw = _model_case(graph, C, seed=100 + C + B, B=B, bias=bias)
        _REF[key] = (graph, model.state_dict(), X, Ac, Rw, _restated(model, graph, X, Ac, Rw))
    return _REF[key]


def _fresh(name, C, B, bias, mode=MODE):
    graph, sd, X, Ac, Rw, ref = _reference(name, C, B, bias)
    model = M.STCGNN(graph.n, C, K, K, 1, HIDDEN, LAYERS, HORIZON, use_bias=bias, graph_mode=mode)
    model.load_state_dict(sd if mode == MODE else {k: v for k, v in sd.items() if not k.startswith('mix_graph_pair.')})
    return graph, model.cuda(), X.cuda(), Ac.cuda(), Rw.cuda(), ref


def _step(model, graph, X, Ac, Rw):
    model.zero_grad(set_to_none=True)
    y = model(X_seq=X, As=graph, Ac=Ac)
    (y * Rw).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), {k: p.grad.clone() if p.grad is not None else None for k, p in model.named_parameters()}


CELLS = LAYERS * (T + HORIZON)        # every cell is owed a gradient: the last decoder step's top layer is an output, everything else feeds it


@pytest.mark.gpu
@pytest.mark.parametrize('name,C,B,bias', CASES, ids=_IDS)
def test_the_model_against_the_float64_restatement(routed, name, C, B, bias):
    graph, model, X, Ac, Rw, (y64, g64, noise, _) = _fresh(name, C, B, bias)
    y, grads = _step(model, graph, X, Ac, Rw)
    assert routed.count(GATES) == CELLS and routed.count(CAND) == CELLS, (routed.count(GATES), routed.count(CAND))
    assert 'stc_cell_gates_bwd_planar_f32' in routed and 'stc_bdg_node_bwd_f32' not in routed and 'stc_cell_bwd_planar_f32' not in routed
    assert all(g is not None and bool(torch.isfinite(g).all()) and bool(g.abs().sum() > 0) for g in grads.values()), [k for k, g in grads.items() if g is None]
    _check_model(f'{MODE} {name} C={C} B={B} bias={bias}', y, grads, y64, g64, noise)
    y2, grads2 = _step(model, graph, X, Ac, Rw)                                     # two runs: equal bits
    assert torch.equal(y, y2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


@pytest.mark.gpu
def test_with_the_switch_off_the_per_cell_route_agrees(routed, monkeypatch):
    name, C, B, bias = CASES[0]
    graph, model, X, Ac, Rw, (y64, g64, noise, _) = _fresh(name, C, B, bias)
    y, grads = _step(model, graph, X, Ac, Rw)
    del routed[:]
    monkeypatch.setattr(ops, '_DTC', False)
    y_cell, grads_cell = _step(model, graph, X, Ac, Rw)
    assert GATES not in routed and CAND not in routed and 'stc_bdg_node_bwd_f32' in routed          # one node per cell, dT_c from the node backward
    for k in grads:
        if k.startswith('mix_graph_pair.'):
            bound = max(1e-5, rel_err(grads_cell[k], g64[k]))
            assert rel_err(grads[k], grads_cell[k]) <= bound, (k, rel_err(grads[k], grads_cell[k]), bound)
    assert rel_err(y, y_cell) < 1e-5


@pytest.mark.gpu
def test_no_grad_and_a_frozen_generator_are_the_fixed_graph_route(routed):
    name, C, B, bias = CASES[0]
    graph, model, X, Ac, Rw, _ = _fresh(name, C, B, bias)
    _, fixed, *_ = _fresh(name, C, B, bias, mode='csr-fixed')
    with torch.no_grad():
        Gc = model.mix_graph_pair(X, Ac)
        del routed[:]
        y = model(X_seq=X, As=graph, Ac=Ac)
        assert GATES not in routed and CAND not in routed
        assert torch.equal(y, fixed(X_seq=X, As=graph, Ac=Gc))                     # bit for bit the fixed-graph model given the generator's Gc
    for p in model.mix_graph_pair.parameters():
        p.requires_grad_(False)
    del routed[:]
    y, grads = _step(model, graph, X, Ac, Rw)
    assert GATES not in routed and CAND not in routed and 'stc_cell_bwd_planar_f32' in routed       # nothing to learn: the one-launch backward
    y_fixed = fixed(X_seq=X, As=graph, Ac=Gc)
    (y_fixed * Rw).sum().backward()
    assert torch.equal(y, y_fixed.detach())
    named = dict(fixed.named_parameters())
    assert all(torch.equal(grads[k], named[k].grad) for k in named)


@pytest.mark.gpu
def test_one_trainer_epoch_eager_and_replayed_ends_in_equal_parameters(tmp_path, monkeypatch):
    """A synthetic 6 x 8 x 32 set, one epoch eager and one with ``hip_graph=True`` from the same seed: the capturable Adam in both, equal bits."""
    from stc_hip import data as sdata
    from stc_hip.trainer import Trainer
    launched = []
    inner = _lib.HipKernels._launch
    monkeypatch.setattr(_lib.HipKernels, '_launch', lambda self, name, *a, **kw: (launched.append(name), inner(self, name, *a, **kw))[1])
    data = sdata.synthetic_incidents(6, 8, 32, 40, sparse_graph=True)
    params = dict(device='cuda:0', H=6, W=8, C=32, batch_size=4, obs_len=3, pred_len=2, split_ratio=[6, 1, 1], model='STC-GNN', cheby_order=2,
                  hidden_dim=16, nn_layers=1, learn_rate=2e-3, decay_rate=1e-4, num_epochs=1, time_slice=4, city='SYN')
    flat = {}
    for graphed in (False, True):
        out = tmp_path / str(graphed)
        os.makedirs(out)
        del launched[:]
        loaders = sdata.get_data_loader(params, data, params['obs_len'], params['pred_len'], params['split_ratio'])
        torch.manual_seed(123)
        trainer = Trainer(dict(params, output_dir=str(out)), data, graph_mode=MODE, hip_graph=graphed)
        trainer.train(loaders, verbose=False)
        flat[graphed] = {k: p.detach().clone() for k, p in trainer.model.named_parameters()}
        assert GATES in launched and CAND in launched and 'stc_bdg_node_bwd_f32' not in launched, sorted(set(launched))
        if graphed:
            assert any(slot[1] is not None for slot in trainer._captured.values()), 'no step was captured'
    differ = {k: float((flat[True][k] - v).abs().max()) for k, v in flat[False].items() if not torch.equal(flat[True][k].view(torch.int32), v.view(torch.int32))}
    assert not differ, differ
