"""The first-step route of ``ops.stc_cell_graph``: the cells whose state is a zero initial state -- (layer, t = 0) of the encoder -- run the
first-step forms (``cell_gates_fwd_first``, ``ring2_blend_first``, ``cell_bwd_first``) on a kernel set that has them (``first_step_cells``), the
model passes the zero states as shapes (``ops.zero_state``) and no plane of zeros, R, dH or dS.H exists for those cells.

CPU: the CPU twin wrapped into a kernel set with the capability -- its three methods call the twin's general ones on explicit zeros -- under the
model of golden g11 (the bench path's widths), route on against route off and against the golden.  GPU: an 8 x 8 grid, route on against off, bit
for bit, in grad mode and under ``torch.no_grad()``.
"""
import pytest
import torch

import STC_GNN as M
from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, ops
from tests.conftest import load_golden, rel_err, sub_dict
from tests.golden.make_golden import bench_path_inputs

FWD, GRAD, LOSS = 2e-6, 5e-6, 5e-6          # the bounds of tests/test_module_parity.py for the CPU twin against the reference's goldens


class FirstStepTwin(EmulatedKernels):
    """The CPU twin with the first-step capability: each first-step method is the twin's general method on explicit planes of zeros (and, the
    backward, an arbitrary R).  ``log``: the executor's own calls -- (name, what the test looks at)."""

    first_step_cells = True
    LOGGED = ('csr_spmm', 'cell_gates_fwd_planar', 'cell_bwd_planar', 'ring2_blend', 'spmm_blend_fwd')

    def __init__(self):
        super().__init__()
        self.log, self.depth = [], 0

    def __getattribute__(self, name):
        attr = super().__getattribute__(name)
        if name not in FirstStepTwin.LOGGED:
            return attr

        def call(*a, **kw):
            if self.depth == 0:
                zero_operand = name == 'csr_spmm' and not bool(a[5].any())          # (rowptr, colidx, val, n_rows, n_cols, X, ...)
                self.log.append((name, zero_operand))
            self.depth += 1
            try:
                return attr(*a, **kw)
            finally:
                self.depth -= 1
        return call

    def _inner(self, name, fn, *a, **kw):
        self.log.append((name, False))
        self.depth += 1
        try:
            return fn(self, *a, **kw)
        finally:
            self.depth -= 1

    def cell_first_supported(self, Cc, h) -> bool:
        return self.cell_bwd_planar_supported(Cc, h)

    def cell_gates_fwd_first(self, X, SX, Tc, W, bias, U, post, act_amax=None):
        zero = torch.zeros_like(U)
        self._inner('cell_gates_fwd_first', EmulatedKernels.cell_gates_fwd_planar, X, zero, SX, zero, Tc, W, bias, U, torch.empty_like(U), None, post=post,
                    act_amax=act_amax)

    def ring2_blend_first(self, rowptr, colidx, val, ring2, Bm, A, U, Cand, Hnew, SHnew):
        self._inner('ring2_blend_first', EmulatedKernels.ring2_blend, rowptr, colidx, val, ring2, Bm, A, U, torch.zeros_like(U),
                    torch.empty_like(U) if Cand is None else Cand, Hnew, SHnew)

    def cell_bwd_first(self, X, SX, Tc, Wg, Wc, U, Cand, dHnew, dBm, dXs, dWg, dbg, dWc, dbc, accumulate_x=False, act_amax=None):
        zero = torch.zeros_like(U)
        self._inner('cell_bwd_first', EmulatedKernels.cell_bwd_planar, X, zero, SX, zero, Tc, Wg, Wc, U, torch.rand_like(U), Cand, dHnew, dBm,
                    [*dXs, torch.empty_like(U), torch.empty_like(U)], dWg, dbg, dWc, dbc, accumulate_x=accumulate_x, act_amax=act_amax)


def _g11_model(dev):
    g = load_golden('g11_bench_c32')
    model = M.STCGNN(num_nodes=int(g['N']), num_categories=int(g['C']), Ks=int(g['K']), Kc=int(g['K']), input_dim=1, hidden_dim=int(g['h']),
                     num_layers=int(g['layers']), out_horizon=int(g['horizon']), graph_mode='csr-fixed').to(dev)
    model.load_state_dict({k: v.to(dev) for k, v in sub_dict(g, 'sd/').items()})
    return g, model


def _step(model, X, graph, Gc, Y):
    model.zero_grad(set_to_none=True)
    yhat = model(X_seq=X, As=graph, Ac=Gc)
    loss = O.combo_loss(yhat, Y)
    loss.backward()
    return yhat.detach(), loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}


def test_route_on_the_cpu_twin_against_route_off_and_the_golden(monkeypatch):
    g, model = _g11_model('cpu')
    s = bench_path_inputs(32, 2)
    graph = CsrGraph.from_dense(s['Gs'])
    layers, T, horizon = int(g['layers']), s['X'].shape[1], int(g['horizon'])
    runs = {}
    real = ops.zero_state
    for on in (True, False):
        twin = FirstStepTwin()
        monkeypatch.setattr(ops, '_kernels', twin)
        monkeypatch.setattr(ops, '_FIRST_STEP', on)
        states = []
        monkeypatch.setattr(ops, 'zero_state', lambda *a, **k: (states.append(real(*a, **k)), states[-1])[1])
        out = _step(model, s['X'], graph, s['Gc'], s['Y'])
        with torch.no_grad():                                       # the forward-only route takes the same two forward forms
            quiet = model(X_seq=s['X'], As=graph, Ac=s['Gc'])
        assert torch.equal(quiet, out[0])
        runs[on] = (*out, [n for n, _ in twin.log], sum(z for _, z in twin.log), states)
    (y1, l1, g1, log1, zeros1, states1), (y0, l0, g0, log0, zeros0, states0) = runs[True], runs[False]
    # the same prediction, loss and gradients (the twin's first-step methods ARE its general ones on zeros) ...
    assert torch.equal(y1, y0) and torch.equal(l1, l0) and all(torch.equal(g1[k], g0[k]) for k in g0)
    # ... within the golden's bounds
    assert rel_err(y1, g['yhat']) < FWD and abs(float(l1) - float(g['loss'])) < LOSS
    for k, v in sub_dict(g, 'grad/').items():
        assert rel_err(g1[k], v) < GRAD, k
    # the route was taken: one first-step launch of each kind per layer, in the place of the general ones
    n = lambda log, name: log.count(name)
    cells = layers * (T + horizon)
    assert n(log0, 'cell_gates_fwd_first') == n(log0, 'cell_bwd_first') == n(log0, 'ring2_blend_first') == 0
    assert n(log0, 'cell_gates_fwd_planar') == 2 * cells and n(log0, 'cell_bwd_planar') == cells          # (grad mode + no_grad forward)
    assert n(log1, 'cell_gates_fwd_first') == 2 * layers and n(log1, 'cell_bwd_first') == layers
    assert n(log1, 'cell_gates_fwd_planar') == 2 * (cells - layers) and n(log1, 'cell_bwd_planar') == cells - layers
    assert n(log1, 'ring2_blend_first') + n(log1, 'spmm_blend_fwd') + n(log1, 'ring2_blend') == 2 * cells
    assert n(log1, 'ring2_blend_first') == (2 * layers if n(log0, 'ring2_blend') else 0)
    # no aggregation of a plane of zeros (off: one per layer and forward), and the zero states were shapes, never planes
    assert zeros0 == 2 * layers and zeros1 == 0 and n(log1, 'csr_spmm') == n(log0, 'csr_spmm') - 2 * layers
    assert not states0 and len(states1) == 2 * layers
    assert all(z.untyped_storage().nbytes() == z.element_size() and not any(z.stride()) for z in states1)


def test_first_step_cells_save_no_state_side_planes(monkeypatch):
    """What a first-step cell keeps for backward: None in the slots of H, R and S.H (the counts of ``_Form.saved`` stand), so neither those
    planes nor the gradient planes of the external state exist; the general cells keep theirs."""
    g, model = _g11_model('cpu')
    s = bench_path_inputs(32, 2)
    monkeypatch.setattr(ops, '_kernels', FirstStepTwin())
    saved = []
    real = ops._ForwardPass.cell
    monkeypatch.setattr(ops._ForwardPass, 'cell', lambda self, j, *a, **k: (saved.append((j, real(self, j, *a, **k))), saved[-1][1])[1])
    yhat = model(X_seq=s['X'], As=CsrGraph.from_dense(s['Gs']), Ac=s['Gc'])
    T = s['X'].shape[1]
    first = {l * T for l in range(int(g['layers']))}
    assert {j for j, _ in saved} >= first
    for j, sv in saved:
        assert len(sv) == ops._Form.PLANAR_ONE_BWD.saved(2)
        Hprev, U, Rg, Cand, Xp, SXp, SHp = sv
        assert (Hprev is None and Rg is None and SHp is None) == (j in first)
        assert all(t is not None for t in (U, Cand, Xp, SXp))
    O.combo_loss(yhat, s['Y']).backward()          # ... and the backward takes them as they are
    assert all(p.grad is not None for p in model.parameters())


@pytest.mark.gpu
def test_route_on_against_route_off_on_the_gpu(monkeypatch):
    """8 x 8 grid, C = 32, 3 + 2 steps, 2 layers, 2 samples, csr-fixed: prediction, loss and every parameter gradient bit for bit, and the
    forward-only prediction."""
    from stc_hip._lib import HipKernels
    monkeypatch.setattr(ops, '_kernels', None)
    torch.manual_seed(11)
    Hg = Wg = 8
    C, h, K, B, T, horizon, layers = 32, 16, 2, 2, 3, 2, 2
    graph = CsrGraph.queen_grid(Hg, Wg, normalize=True)
    model = M.STCGNN(Hg * Wg, C, K, K, 1, h, layers, horizon, graph_mode='csr-fixed').cuda()
    Gc = torch.softmax(torch.randn(C, C), -1).cuda()
    X = (torch.rand(B, T, Hg * Wg, C) < 0.3).float().cuda()
    Y = (torch.rand(B, horizon, Hg * Wg, C) < 0.3).float().cuda()
    calls = []
    for name in ('cell_gates_fwd_first', 'ring2_blend_first', 'cell_bwd_first'):
        real = getattr(HipKernels, name)
        monkeypatch.setattr(HipKernels, name, lambda self, *a, _real=real, _name=name, **kw: (calls.append(_name), _real(self, *a, **kw))[1])
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(ops, '_FIRST_STEP', on)
        del calls[:]
        out = _step(model, X, graph, Gc, Y)
        with torch.no_grad():
            quiet = model(X_seq=X, As=graph, Ac=Gc)
        torch.cuda.synchronize()
        runs[on] = (*out, quiet, list(calls))
    (y1, l1, g1, q1, c1), (y0, l0, g0, q0, c0) = runs[True], runs[False]
    assert not c0 and c1.count('cell_gates_fwd_first') == 2 * layers and c1.count('cell_bwd_first') == layers
    assert torch.equal(y1, y0) and torch.equal(l1, l0) and torch.equal(q1, q0) and torch.equal(q1, y1)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), (k, rel_err(g1[k], g0[k]))
