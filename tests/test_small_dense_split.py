"""Dense graphs (learned, or evaluated with grad mode off) on samples of MORE than ``SMALL_STAGED_ROWS`` rows on the few-category cell kernels:
the routing rule (``small.small_graph_supported`` with ``small_dense_split`` / ``SMALL_DENSE_ROWS``), the executor on the split launches (never
phase 0 there: ``HipKernels._small_head``), the chunk rule of the graph-gradient partials, and the module.

CPU: routing on stub kernel sets; the chunk rule of samples up to ``SMALL_STAGED_ROWS`` rows.
GPU (-m gpu): a schedule of two layers x two steps at N = 129, C = 5 (645 rows) through ``small.stc_small_graph`` against the float64 oracle with
autograd (states, parameter gradients, dGs, dGc) at K = 2 and 3; the same with one workgroup per sample (``STC_SMALL_SPLITS=1``): no phase-0
launch; the module at N = 41, C = 16 and N = 65, C = 10 against the float64 oracle, its ``no_grad`` route, and a HIP-graph capture.
"""
import os
import tempfile
import types

import pytest
import torch

import STC_GNN as M
from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib, ops, small
from stc_hip.graph import dense_operand
from tests.conftest import rel_err
from tests.test_module_parity import FWD, GPU
from tests.test_small_dense_order3 import FWD_CELL, GRAD_CELL, _close, _dense_gs, _learned_operand, _StubKernels

H16 = 16
MODULE_GRAD = 2e-5      # tests/test_module_parity.py::test_learned_graphs_on_the_small_graph_kernels on the GPU: max(1e-5, gpu_tol = 2e-5)


# ------------------------------------------------------------------------------------------------------------------------------ CPU: routing
def _split_stub(rows):
    return type('SplitStub', (_StubKernels,), dict(small_dense_split=True, SMALL_DENSE_ROWS=rows))()


def _supported(k, op, K, C=5):
    return small.small_graph_supported(k, op, torch.zeros(K, C, C), K, C, 16, {1, 16})


@pytest.mark.parametrize('K', [2, 3])
def test_routing_of_dense_graphs_above_the_staged_size(K):
    stub, bare = _split_stub(645), _StubKernels()
    assert _supported(stub, _learned_operand(129), K)                               # 645 rows: above SMALL_STAGED_ROWS, the bound itself
    assert _supported(stub, _learned_operand(128), K)                               # 640 rows: as before
    assert not _supported(stub, _learned_operand(323), K, C=2)                      # 646 rows: R + 1
    big = _split_stub(8000)
    assert _supported(big, _learned_operand(256), K, C=16) and not _supported(big, _learned_operand(257), K, C=16)      # C = 16 above 4 096 rows
    op = _learned_operand(129)
    op.nnz -= 1
    assert not _supported(stub, op, K)                                              # not the full pattern
    # the graph as it arrives with grad mode off (validation): the same bound; in grad mode a dense graph that needs no gradient keeps the general path
    frozen = lambda N: dense_operand(_dense_gs(N, seed=N))
    with torch.no_grad():
        assert _supported(stub, frozen(129), K) and not _supported(stub, frozen(323), K, C=2)
        assert not _supported(bare, frozen(129), K)
    assert not _supported(stub, frozen(129), K)
    # a kernel set without the attribute keeps every answer: the stub of tests/test_small_dense_order3.py, the CPU twin
    for k in (bare, EmulatedKernels()):
        assert not hasattr(k, 'small_dense_split')
        assert not _supported(k, _learned_operand(129), K) and not _supported(k, _learned_operand(323), K, C=2)
    assert _supported(bare, _learned_operand(128), K)
    off = type('Off', (_StubKernels,), dict(small_dense_split=False, SMALL_DENSE_ROWS=645))()
    assert not _supported(off, _learned_operand(129), K)


def test_the_hip_kernel_set_carries_the_route():
    assert _lib.HipKernels.small_dense_split is True
    assert _lib.HipKernels.SMALL_STAGED_ROWS == 640 < _lib.HipKernels.SMALL_DENSE_ROWS <= _lib.HipKernels.SMALL_PREFERRED_ROWS


def test_chunk_rule_of_samples_up_to_the_staged_size_is_unchanged():
    """Up to 640 rows per sample the float64 fold order of every run so far must not move: min(256, planes), whatever N."""
    k = types.SimpleNamespace(SMALL_STAGED_ROWS=640)
    for planes, N, rows in ((9 * 32, 100, 500), (3, 100, 500), (0, 7, 35), (1000, 128, 640), (288, 40, 640)):
        assert _lib.HipKernels.graph_grad_chunks(k, planes, N, rows) == max(1, min(256, planes))


# ------------------------------------------------------------------------------------------------------------------------------ GPU: executor
N_EX, C_EX, B_EX = 129, 5, 2
SCHEDULE = [(0, ('ext', 0), ('ext', 2)), (0, ('ext', 1), ('cell', 0)),             # layer 0: inputs of 1 column, two steps
            (1, ('cell', 0), ('ext', 3)), (1, ('cell', 1), ('cell', 2))]           # layer 1: inputs of 16 columns
OUTPUTS = [0, 1, 2, 3]
_REFERENCE = {}


def _problem(K):
    g = torch.Generator().manual_seed(100 + K)
    rnd = lambda *s: torch.randn(*s, generator=g)
    N, C, B = N_EX, C_EX, B_EX
    ext = [(torch.rand(B, N, C, 1, generator=g) < 0.3).float() for _ in range(2)] + [torch.tanh(rnd(B, N, C, H16)) for _ in range(2)]
    stacks = []
    for cin in (1, H16):
        L = K * K * (cin + H16)
        stacks.append((rnd(L, 2 * H16) / L ** 0.5, rnd(2 * H16) * 0.1, rnd(L, H16) / L ** 0.5, rnd(H16) * 0.1))
    return dict(Gs=_dense_gs(N, seed=N + K), Gc=torch.softmax(rnd(C, C), -1), ext=ext, stacks=stacks, Rw=rnd(len(OUTPUTS), B, N, C, H16))


def _tc(Gc, K):
    return torch.stack([torch.eye(Gc.shape[0], dtype=Gc.dtype, device=Gc.device), Gc, 2 * Gc @ Gc - torch.eye(Gc.shape[0], dtype=Gc.dtype, device=Gc.device)][:K])


def _oracle_run(p, K, dtype):
    """The schedule through the oracle's cell with autograd in ``dtype``: (states, {name: gradient})."""
    to = lambda t: t.detach().clone().to(dtype)                     # (float32: a copy too -- the shared problem stays free of autograd state)
    Gs, Gc = to(p['Gs']).requires_grad_(), to(p['Gc']).requires_grad_()
    stacks = [tuple(to(w).requires_grad_() for w in st) for st in p['stacks']]
    ext, states = [to(t) for t in p['ext']], []
    src = lambda s: ext[s[1]] if s[0] == 'ext' else states[s[1]]
    for s_id, x, hs in SCHEDULE:
        states.append(O.stc_cell(Gs, Gc, src(x), src(hs), *stacks[s_id], K, K))
    out = torch.stack(states)
    (out * to(p['Rw'])).sum().backward()
    grads = dict(dGs=Gs.grad, dGc=Gc.grad)
    grads.update({f'd{n}{i}': w.grad for i, st in enumerate(stacks) for n, w in zip(('Wg', 'bg', 'Wc', 'bc'), st)})
    return out.detach(), grads


def _reference(K):
    """Problem and float64 oracle: computed once per K, shared, never modified."""
    if K not in _REFERENCE:
        p = _problem(K)
        _REFERENCE[K] = (p, *_oracle_run(p, K, torch.float64))
    return _REFERENCE[K]


def _executor_run(hip, p, K):
    dev = torch.device('cuda')
    Gs, Gc = p['Gs'].detach().to(dev).requires_grad_(), p['Gc'].detach().to(dev).requires_grad_()
    stacks = [tuple(w.detach().to(dev).requires_grad_() for w in st) for st in p['stacks']]
    out = small.stc_small_graph(hip, dense_operand(Gs), _tc(Gc, K), K, SCHEDULE, OUTPUTS, [t.to(dev) for t in p['ext']], stacks)
    (out * p['Rw'].to(dev)).sum().backward()
    grads = dict(dGs=Gs.grad, dGc=Gc.grad)
    grads.update({f'd{n}{i}': w.grad for i, st in enumerate(stacks) for n, w in zip(('Wg', 'bg', 'Wc', 'bc'), st)})
    return out.detach().cpu(), {n: g.cpu() for n, g in grads.items()}


def _dgs_bound(K, err, p, grads):
    """GRAD_CELL -- and where that does not hold on dGs (a sum over every cell, sample and category of N x N outer products): the project's 10 x the
    reference's own fp32 distance from float64 on the same inputs (the oracle in float32), if that is larger; error, noise and factor then go to
    parity_errors.tsv."""
    if err < GRAD_CELL:
        return GRAD_CELL
    noise = rel_err(_oracle_run(p, K, torch.float32)[1]['dGs'], grads['dGs'])
    bound = max(GRAD_CELL, 10 * noise)
    line = f'test_small_dense_split\tK={K} N={N_EX} C={C_EX} dGs\terror {err:.3e}\tfp32 oracle noise {noise:.3e}\tfactor 10\tbound {bound:.3e}\n'
    out = os.environ.get('STC_PARITY_DIR') or tempfile.gettempdir()       # (where a job keeps its records, else the temporary directory)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'parity_errors.tsv'), 'a') as f:
        f.write(line)
    print(line, end='')
    return bound


def _record_phases(hip, monkeypatch):
    """(entry point, phase code) of every stc_cell_small_* launch made through ``hip`` from here on."""
    seen, real = [], hip._launch

    def launch(name, on, *args, **kw):
        if name.startswith('stc_cell_small_'):
            seen.append((name, args[-4]))                           # ..., phase, splits, batch, C
        return real(name, on, *args, **kw)
    monkeypatch.setattr(hip, '_launch', launch)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize('K', [2, 3])
def test_schedule_on_a_dense_graph_of_645_rows_against_the_float64_oracle(monkeypatch, K):
    hip = _lib.HipKernels()
    p, states, grads = _reference(K)
    assert small.small_graph_supported(hip, dense_operand(p['Gs'].clone().requires_grad_()), _tc(p['Gc'], K), K, C_EX, H16, {1, H16})
    monkeypatch.delenv('STC_SMALL_SPLITS', raising=False)
    assert hip.cell_small_splits(B_EX, N_EX * C_EX) == 8
    seen = _record_phases(hip, monkeypatch)
    got, ggot = _executor_run(hip, p, K)
    assert seen and all(phase != 0 for _, phase in seen)
    _close(got, states, FWD_CELL, f'645 rows K={K} states')
    for n, want in grads.items():
        if n == 'dGs':
            err = rel_err(ggot[n], want)
            print(f'645 rows K={K} dGs: {err:.3e} (bound {GRAD_CELL:.1e}, or 10 x the error of the oracle in float32)')
            assert err < _dgs_bound(K, err, p, grads), f'dGs: {err:.3e}'
        else:
            _close(ggot[n], want, GRAD_CELL, f'645 rows K={K} {n}')
    # one workgroup per sample (what batches of 256 and more get): the split phases all the same, never the whole-cell launch
    monkeypatch.setenv('STC_SMALL_SPLITS', '1')
    assert hip.cell_small_splits(B_EX, N_EX * C_EX) == 1
    del seen[:]
    one, gone = _executor_run(hip, p, K)
    fwd = [ph for name, ph in seen if name == 'stc_cell_small_fwd_f32']
    bwd = [ph for name, ph in seen if name == 'stc_cell_small_bwd_f32']
    assert fwd == list(hip.SMALL_FWD_PHASES) * len(SCHEDULE) and bwd == list(hip.SMALL_BWD_PHASES) * len(SCHEDULE)
    _close(one, got, FWD_CELL, f'645 rows K={K} states, splits 1 vs 8')
    for n in grads:
        _close(gone[n], ggot[n], GRAD_CELL, f'645 rows K={K} {n}, splits 1 vs 8')
    with torch.no_grad():                                           # the forward-only route: the same launches, the node's bits
        del seen[:]
        dev = torch.device('cuda')
        quiet = small.stc_small_graph(hip, dense_operand(p['Gs'].to(dev)), _tc(p['Gc'].to(dev), K), K, SCHEDULE, OUTPUTS, [t.to(dev) for t in p['ext']],
                                      [tuple(w.to(dev) for w in st) for st in p['stacks']])
    assert [ph for _, ph in seen] == list(hip.SMALL_FWD_PHASES) * len(SCHEDULE) and torch.equal(quiet.cpu(), one)


# ------------------------------------------------------------------------------------------------------------------------------ GPU: module
# Seed: on the CPU, of the seeds 0 .. 5 (41, 16) / 0 .. 7 (65, 10), the one on which the reference's OWN fp32 backward (the oracle in float32) is
# closest to float64 on every parameter: 2 for both (2.1e-6 / 2.2e-6; seed 0: 1.1e-4 / 1.2e-5 -- MGP_Gen's conditioning, as
# tests/test_module_parity.py::test_learned_graphs_on_the_small_graph_kernels notes for its own draws)
MODULE = [(41, 16, 2), (65, 10, 2)]


def _module_step(N, C, seed, dev):
    layers, T, horizon = 1, 3, 2
    torch.manual_seed(seed)
    model = M.STCGNN(N, C, 2, 2, 1, 16, layers, horizon, graph_mode='dense-learned')
    X = (torch.rand(2, T, N, C) < 0.3).float()
    As, Ac = torch.rand(N, N), torch.rand(C, C)
    Y = (torch.rand(2, horizon, N, C) < 0.3).float()
    return model.to(dev), X, As, Ac, Y, (layers, horizon)


def _count_calls(monkeypatch, owner, name):
    calls, real = [], getattr(owner, name)
    monkeypatch.setattr(owner, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,seed', MODULE)
def test_learned_dense_module_above_the_staged_size_runs_on_the_small_graph_kernels(monkeypatch, N, C, seed):
    monkeypatch.setattr(ops, '_kernels', None)
    dev = torch.device('cuda')
    assert N * C > _lib.HipKernels.SMALL_STAGED_ROWS
    forward_only = _count_calls(monkeypatch, small, '_forward_only')
    calls = _count_calls(monkeypatch, ops, 'stc_small_graph')
    model, X, As, Ac, Y, (layers, horizon) = _module_step(N, C, seed, dev)
    y = model(X_seq=X.to(dev), As=As.to(dev), Ac=Ac.to(dev))
    assert calls and not forward_only, 'the small-graph path was not taken'
    loss = O.combo_loss(y, Y.to(dev))
    loss.backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    want = O.stcgnn_forward(X.double(), As.double(), Ac.double(), sd, 2, 2, 16, layers, horizon)
    want_loss = O.combo_loss(want, Y.double())
    want_loss.backward()
    _close(y, want.detach(), max(FWD, GPU), f'N={N} C={C} yhat')
    _close(loss, want_loss.detach(), max(FWD, GPU), f'N={N} C={C} loss')
    for n, prm in model.named_parameters():
        _close(prm.grad, sd[n].grad, MODULE_GRAD, f'N={N} C={C} d{n}')
    del calls[:]
    with torch.no_grad():
        quiet = model(X_seq=X.to(dev), As=As.to(dev), Ac=Ac.to(dev))
    assert calls and forward_only, 'the forward-only route was not taken'
    assert torch.equal(quiet, y.detach())


@pytest.mark.gpu
def test_hip_graph_capture_of_the_learned_step_above_the_staged_size(monkeypatch):
    """One captured forward + backward at N = 41, C = 16 replays to the gradients of an eager step (as
    tests/test_small_dense_order3.py::test_hip_graph_capture_of_the_order_3_learned_step)."""
    monkeypatch.setattr(ops, '_kernels', None)
    dev = torch.device('cuda')
    N, C, seed = MODULE[0]
    model, X, As, Ac, Y, _ = _module_step(N, C, seed, dev)
    X, As, Ac, Y = X.to(dev), As.to(dev), Ac.to(dev), Y.to(dev)
    calls = _count_calls(monkeypatch, ops, 'stc_small_graph')

    def step():
        model.zero_grad(set_to_none=True)
        O.combo_loss(model(X_seq=X, As=As, Ac=Ac), Y).backward()

    step()
    assert calls
    torch.cuda.synchronize()
    eager = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert rel_err(p.grad, eager[n]) < 1e-6, n
