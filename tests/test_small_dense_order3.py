"""Chebyshev order 3 with a LEARNED DENSE spatial graph on the few-category cell kernels (stc_cell_small_fwd/bwd_f32, Ks = Kc = 3, MODE 3: the
split launches 5, 6 / 1, 7, 4 with T_2(S) = 2 S^2 - I as a second dense matrix; ABI v35) and the executor around them (stc_hip/small.py).

GPU (-m gpu): one cell step against the float64 oracle cell and against the order-3 CSR form of the same kernels; the refusals; the reference's
full model with learned graphs on this path against the float64 oracle and the general path; a HIP-graph capture.
CPU: the routing rule (``small.small_graph_supported``) and the T_2 wiring outside the autograd node (``small.dense_second_order``).
"""
import pytest
import torch

import STC_GNN as M
from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, ops, small
from stc_hip.graph import csr_operand, dense_operand
from tests.conftest import rel_err
from tests.test_module_parity import FWD
from tests.test_small_cell import _buffers, _inputs, _split_params

FWD_CELL, GRAD_CELL, VS_CSR = 1e-5, 2e-5, 5e-6        # one cell step: forward / gradients against float64; forward against the CSR form


def _close(got, want, bound, what):
    err = rel_err(got, want)
    print(f'{what}: {err:.3e} (bound {bound:.1e})')
    assert err < bound, f'{what}: relative error {err:.3e} >= {bound:.1e}'


def _dense_gs(N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(N, N, generator=g), -1)


def _t2(G):
    return 2.0 * G @ G - torch.eye(G.shape[0], dtype=G.dtype)


def _dense_graphs(Gs, dev):
    """(op, forward graph2, backward graph2) of a dense Gs: the full pattern, with T_2 formed in float64 and rounded once."""
    op = dense_operand(Gs.to(dev))
    T2 = _t2(Gs.double())
    f2 = (op.fwd_rowptr, op.fwd_colidx, T2.t().contiguous().float().reshape(-1).to(dev))       # 2 (Gs^T)^2 - I
    b2 = (op.bwd_rowptr, op.bwd_colidx, T2.contiguous().float().reshape(-1).to(dev))           # 2 Gs^2 - I
    return op, f2, b2


def _step(hip, op, f2, b2, t, buf, P, splits, dev, dumps=False):
    """Forward + backward of one cell step at order 3 through ``hip``; plain CPU tensors."""
    to = lambda v: v.to(dev)
    d = {n: (None if v is None else to(v)) for n, v in t.items()}
    b = {n: to(v) for n, v in buf.items()}
    B = d['H'].shape[0]
    nan = lambda: to(torch.full_like(buf['Zg'], float('nan')))
    fd = dict(Z0=nan(), Z0c=nan(), Z1c=nan(), Z2c=nan()) if dumps else {}
    hip.cell_small_fwd(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, d['X'], d['H'], d['Tc'], d['Wg'], d['bg'], d['Wc'], d['bc'], b['U'], b['R'], b['Cand'],
                       b['Hnew'], b['RH'], b['Zg'], b['Zc'], splits=splits, graph2=f2, Zg2=b['Zg2'], Zc2=b['Zc2'], **fd)
    dX, dH = to(torch.full(t['X'].shape, float('nan'))), to(torch.full(t['H'].shape, float('nan')))
    dP = to(torch.zeros(B * splits * hip.cell_small_param_rows, P))
    bd = dict(dZ1c=nan(), dZ1g=nan(), dZ2c=nan(), dZ2g=nan(), dYg=to(torch.full((B, buf['Zg'].shape[1], 32), float('nan'))),
              dYc=to(torch.full((B, buf['Zg'].shape[1], 16), float('nan')))) if dumps else {}
    hip.cell_small_bwd(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, d['X'], d['H'], d['Tc'], d['Wg'], d['Wc'], b['U'], b['R'], b['Cand'], b['RH'], b['Zg'],
                       b['Zc'], d['dHnew'], dX, False, dH, False, dP, t['bg'] is not None, t['bc'] is not None, splits=splits, graph2=b2, Zg2=b['Zg2'],
                       Zc2=b['Zc2'], **bd)
    return {n: v.detach().cpu() for n, v in dict(b, dX=dX, dH=dH, dP=dP, **fd, **bd).items()}


_ORACLE = {}


def _oracle_cell(N, C, cin, B, bias):
    """The float64 oracle cell (dense Gs, K = 3) and its autograd for a case: computed once, shared, never modified."""
    key = (N, C, cin, B, bias)
    if key not in _ORACLE:
        Gs = _dense_gs(N, seed=N + cin)
        t = _inputs(B, N, C, cin, seed=3 * N + C + cin, bias=bias, K=3)
        leaves = {n: t[n].double().requires_grad_(True) for n in ('X', 'H', 'Wg', 'Wc') + (('bg', 'bc') if bias else ())}
        gates = {}

        def conv(X, Gs_, Gc_, W, b, Ks, Kc):               # (the oracle's own convolution, its pre-activations kept: gates first, candidate second)
            y = O.bdg_dif(X, Gs_, Gc_, W, b, Ks, Kc)
            gates.setdefault('pre', []).append(y.detach())
            return y
        Hnew = O.stc_cell(Gs.double(), t['Gc'].double(), leaves['X'], leaves['H'], leaves['Wg'], leaves.get('bg'), leaves['Wc'], leaves.get('bc'), 3, 3,
                          conv=conv)
        Hnew.backward(t['dHnew'].double())
        u, r = torch.sigmoid(gates['pre'][0]).split(16, -1)
        _ORACLE[key] = (Gs, t, dict(Hnew=Hnew.detach(), U=u, R=r, Cand=torch.tanh(gates['pre'][1]), **{'d' + n: v.grad for n, v in leaves.items()}))
    return _ORACLE[key]


CASES = [(7, 5, 1, 2, 1, True),       # three nodes per tile, ragged last tile
         (7, 5, 1, 2, 1, False),      # ... without biases
         (7, 5, 16, 1, 2, True),
         (10, 8, 4, 2, 8, True),      # a boundary node tile shared by two workgroups; more splits than row tiles
         (9, 3, 16, 2, 2, True),
         (6, 16, 1, 1, 2, True),      # one node per tile
         (33, 7, 16, 1, 4, True),     # two nodes per tile, N neither a multiple of 16 nor of 4
         (20, 5, 1, 2, 2, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,cin,B,splits,bias', CASES)
def test_one_cell_step_with_a_dense_graph_at_order_3(N, C, cin, B, splits, bias):
    """cell_small_fwd / cell_small_bwd with a dense Gs at Ks = Kc = 3 against the float64 oracle cell and its autograd (U, R, Cand, Hnew to 1e-5;
    dX, dH and the summed parameter-gradient rows to 2e-5), and against the order-3 CSR form of the same kernels on the same matrix (a CSR
    whose column array is not the cached full pattern: row gathers) to 5e-6 on the forward."""
    from stc_hip._lib import HipKernels
    hip = HipKernels()
    dev = torch.device('cuda')
    Gs, t, want = _oracle_cell(N, C, cin, B, bias)
    buf, P = _buffers(B, N, C, cin, torch.float32, hip, K=3)
    op, f2, b2 = _dense_graphs(Gs, dev)
    got = _step(hip, op, f2, b2, t, buf, P, splits, dev, dumps=True)
    for name in ('U', 'R', 'Cand', 'Hnew'):
        _close(got[name], want[name], FWD_CELL, f'dense K=3 {name}')
    dWg, dbg, dWc, dbc, rest = _split_params(got['dP'], cin, K=3)
    assert float(rest.abs().max()) == 0.0                           # columns beyond the parameters: untouched
    for name, g in (('dX', got['dX']), ('dH', got['dH']), ('dWg', dWg), ('dWc', dWc)) + ((('dbg', dbg), ('dbc', dbc)) if bias else ()):
        _close(g, want[name], GRAD_CELL, f'dense K=3 {name}')
    if not bias:
        assert float(dbg.abs().max()) == 0.0 and float(dbc.abs().max()) == 0.0
    # the slabs left for the learned-graph gradients: complete (no NaN left), the third slabs as the planes hold them
    for name in ('Z0', 'Z0c', 'Z1c', 'Z2c', 'dZ1c', 'dZ1g', 'dZ2c', 'dZ2g', 'dYg', 'dYc'):
        assert bool(torch.isfinite(got[name]).all()), name
    assert torch.equal(got['Z2c'][..., :16], got['Zc2']) and torch.equal(got['Z2c'][..., 16:], got['Zg2'][..., 16:])
    # the CSR form of order 3 on the same dense matrix
    graph = CsrGraph.from_dense(Gs)
    cop = csr_operand(graph, dev)
    g2 = graph.second_order(dev)
    csr = _step(hip, cop, tuple(g2[f'fwd2_{n}'] for n in ('rowptr', 'colidx', 'val')), tuple(g2[f'bwd2_{n}'] for n in ('rowptr', 'colidx', 'val')),
                t, buf, P, splits, dev)
    for name in ('U', 'R', 'Cand', 'Hnew', 'Zg', 'Zg2', 'Zc', 'Zc2'):
        _close(got[name], csr[name], VS_CSR, f'dense vs CSR K=3 {name}')
    for name in ('dX', 'dH'):
        _close(got[name], csr[name], GRAD_CELL, f'dense vs CSR K=3 {name}')


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,cin', [(37, 8, 3), (100, 5, 16)])
def test_the_two_matrix_streams_of_the_dense_product_are_order_identical(N, C, cin):
    """The dense aggregation runs both matrices through ONE tile product (same tile geometry, same masks, one accumulator chain per matrix in
    the same order): with ``graph2`` carrying the first matrix's own values, the forward's split form leaves Zg2 bitwise equal to Zg and Zc2
    to Zc (N neither a multiple of 16 nor of 4 with a narrow input; the SF shape with the wide one)."""
    from stc_hip._lib import HipKernels
    hip = HipKernels()
    dev = torch.device('cuda')
    B, splits = 2, 2
    t = _inputs(B, N, C, cin, seed=N + C + cin, bias=True, K=3)
    buf, _ = _buffers(B, N, C, cin, torch.float32, hip, K=3)
    op = dense_operand(_dense_gs(N, seed=N).to(dev))
    d = {n: v.to(dev) for n, v in t.items()}
    b = {n: torch.full_like(v, float('nan')).to(dev) for n, v in buf.items()}
    hip.cell_small_fwd(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, d['X'], d['H'], d['Tc'], d['Wg'], d['bg'], d['Wc'], d['bc'], b['U'], b['R'], b['Cand'],
                       b['Hnew'], b['RH'], b['Zg'], b['Zc'], splits=splits, graph2=(op.fwd_rowptr, op.fwd_colidx, op.fwd_val), Zg2=b['Zg2'], Zc2=b['Zc2'])
    for name in ('Zg', 'Zc'):
        assert bool(torch.isfinite(b[name]).all()), name
        assert torch.equal(b[name + '2'], b[name]), f'{name}2 differs from {name} in {int((b[name + "2"] != b[name]).sum())} elements'


@pytest.mark.gpu
def test_refusals_of_the_dense_form_at_order_3():
    """Phase 0 (one workgroup per sample) with a dense graph at Ks = 3: STC_EUNSUPPORTED; a second graph of other than n * n values beside a dense
    first one: STC_EINVAL -- and nothing is launched (the NaN-filled outputs keep their bits)."""
    from stc_hip._lib import HipKernels, StcError
    hip = HipKernels()
    dev = torch.device('cuda')
    N, C, cin, B = 7, 5, 1, 2
    Gs, t, _ = _oracle_cell(N, C, cin, B, True)
    buf, P = _buffers(B, N, C, cin, torch.float32, hip, K=3)
    op, f2, b2 = _dense_graphs(Gs, dev)
    d = {n: v.to(dev) for n, v in t.items()}
    b = {n: v.to(dev) for n, v in buf.items()}
    ws = torch.empty(hip.lib.stc_cell_small_workspace_bytes(N, C, cin, B, 3) // 4, device=dev)
    dP = torch.zeros(B * hip.cell_small_param_rows, P, device=dev)
    dX, dH = torch.full_like(d['X'], float('nan')), torch.full_like(d['H'], float('nan'))
    p = lambda v: None if v is None else v.data_ptr()

    def fwd(graph2, phase):
        return hip.lib.stc_cell_small_fwd_f32(p(op.fwd_rowptr), p(op.fwd_colidx), p(op.fwd_val), N, N * N, 1, p(graph2[0]), p(graph2[1]), p(graph2[2]),
                                              graph2[2].numel(), p(d['X']), cin, p(d['H']), p(d['Tc']), 3, 3, p(d['Wg']), p(d['bg']), p(d['Wc']), p(d['bc']),
                                              p(b['U']), p(b['R']), p(b['Cand']), p(b['Hnew']), p(b['RH']), p(b['Zg']), p(b['Zc']), p(b['Zg2']), p(b['Zc2']),
                                              None, None, None, None, phase, 1, B, C, torch.cuda.current_stream().cuda_stream)

    def bwd(graph2, phase):
        return hip.lib.stc_cell_small_bwd_f32(p(op.bwd_rowptr), p(op.bwd_colidx), p(op.bwd_val), N, N * N, 1, p(graph2[0]), p(graph2[1]), p(graph2[2]),
                                              graph2[2].numel(), p(d['X']), cin, p(d['H']), p(d['Tc']), 3, 3, p(d['Wg']), p(d['Wc']), p(b['U']), p(b['R']),
                                              p(b['Cand']), p(b['RH']), p(b['Zg']), p(b['Zc']), p(b['Zg2']), p(b['Zc2']), p(d['dHnew']), p(dX), 0, p(dH), 0,
                                              p(dP), P, 1, 1, None, None, None, None, None, None, p(ws), ws.numel() * 4, phase, 1, B, C,
                                              torch.cuda.current_stream().cuda_stream)

    short = lambda g: (g[0], g[1], g[2][:N * N - 1])
    EINVAL, EUNSUPPORTED = -1, -4
    assert fwd(f2, 0) == EUNSUPPORTED and 'split form' in hip.lib.stc_last_error().decode()
    assert bwd(b2, 0) == EUNSUPPORTED and 'split form' in hip.lib.stc_last_error().decode()
    assert fwd(short(f2), 5) == EINVAL and bwd(short(b2), 1) == EINVAL
    torch.cuda.synchronize()
    for name, v in dict(b, dX=dX, dH=dH).items():
        assert bool(torch.isnan(v).all()), name                     # nothing ran
    assert float(dP.abs().max()) == 0.0
    # the tensor-level front refuses a second graph that is not the full pattern beside a dense first one
    g2 = CsrGraph.from_dense(Gs).second_order(dev)
    with pytest.raises(StcError, match='dense'):
        hip.cell_small_fwd(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, d['X'], d['H'], d['Tc'], d['Wg'], d['bg'], d['Wc'], d['bc'], b['U'], b['R'], b['Cand'],
                           b['Hnew'], b['RH'], b['Zg'], b['Zc'], splits=2, graph2=tuple(g2[f'fwd2_{n}'] for n in ('rowptr', 'colidx', 'val')),
                           Zg2=b['Zg2'], Zc2=b['Zc2'])


# Seeds: those of tests/test_module_parity.py::test_learned_graphs_on_the_small_graph_kernels (7, 25) are, at order 3, draws on which the
# reference's own float32 arithmetic is 4.1e-4 / 9.1e-5 off on MGP_Gen's parameters (T_2 = 2 G^2 - I amplifies rounding).  Chosen instead, on
# the CPU: the nearest seeds for which MGP_Gen's own fp32 backward -- the oracle in float32, torch ops -- is within 1e-5 of float64 on every
# ``mix_graph_pair`` parameter at K = 3.  (12, 3): seed 196 (7.0e-6; the only one of 0 .. 199 -- next best 1.9e-5 at 181 and 97);
# (20, 5): seed 33 (7.9e-6; 34: 7.1e-6; every seed of 17 .. 32 is above 4e-5).
FULL_MODEL = [(12, 3, 2, 4, 2, 196), (20, 5, 1, 3, 3, 33)]


def _full_model_step(N, C, layers, T, horizon, seed, dev):
    torch.manual_seed(seed)
    model = M.STCGNN(N, C, 3, 3, 1, 16, layers, horizon).to(dev)
    X = (torch.rand(2, T, N, C) < 0.3).float()
    As, Ac, Rw = torch.rand(N, N), torch.rand(C, C), torch.randn(2, horizon, N, C)
    return model, X, As, Ac, Rw


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,layers,T,horizon,seed', FULL_MODEL)
def test_learned_graphs_at_order_3_on_the_small_graph_kernels(monkeypatch, N, C, layers, T, horizon, seed):
    """The reference's FULL model at K = 3 with learned graphs (MGP_Gen's dense Gs and Gc: ``Main.py -K 3``) runs its cells on the few-category
    kernels (asserted); the prediction and EVERY parameter gradient -- those that reach MGP_Gen through Gs, through T_2(Gs) and through Gc
    included -- against the float64 oracle of the same model.  Gradient bound: max(2e-5, 10 x the reference's own fp32 noise on that tensor),
    the clause of test_learned_graphs_on_the_general_path_with_packed_node_kernels; and, on MGP_Gen's parameters, against the general path
    within the larger of 1e-5 and the general path's own distance from float64 (two fp32 paths against one truth)."""
    monkeypatch.setattr(ops, '_kernels', None)
    dev = torch.device('cuda')
    calls = []
    real_small = ops.stc_small_graph
    monkeypatch.setattr(ops, 'stc_small_graph', lambda *a, **k: (calls.append(1), real_small(*a, **k))[1])
    model, X, As, Ac, Rw = _full_model_step(N, C, layers, T, horizon, seed, dev)
    y = model(X_seq=X.to(dev), As=As.to(dev), Ac=Ac.to(dev))
    assert calls, 'the small-graph path was not taken'
    (y * Rw.to(dev)).sum().backward()
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    monkeypatch.setattr(ops, '_SMALL', False)                       # the general path: one autograd node per cell
    model.zero_grad(set_to_none=True)
    (model(X_seq=X.to(dev), As=As.to(dev), Ac=Ac.to(dev)) * Rw.to(dev)).sum().backward()
    general = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    want = O.stcgnn_forward(X.double(), As.double(), Ac.double(), sd, 3, 3, 16, layers, horizon)
    (want * Rw.double()).sum().backward()
    sd32 = {k: v.detach().cpu().float().requires_grad_(True) for k, v in model.state_dict().items()}
    (O.stcgnn_forward(X, As, Ac, sd32, 3, 3, 16, layers, horizon) * Rw).sum().backward()
    _close(y, want.detach().float(), FWD, 'learned K=3 small-graph yhat')
    for n in got:
        noise = rel_err(sd32[n].grad, sd[n].grad)
        print(f'd{n}: reference fp32 noise {noise:.3e}')
        _close(got[n], sd[n].grad, max(2e-5, 10 * noise), f'learned K=3 small-graph d{n}')
        if n.startswith('mix_graph_pair'):
            _close(got[n], general[n], max(1e-5, rel_err(general[n], sd[n].grad)), f'learned K=3 small-graph d{n} vs the general path')


@pytest.mark.gpu
def test_hip_graph_capture_of_the_order_3_learned_step(monkeypatch):
    """One captured forward + backward of the (12, 3) model replays to the gradients of an eager step (the same launches in the same order;
    1e-6 leaves room only for the order of atomic adds inside torch's own kernels)."""
    monkeypatch.setattr(ops, '_kernels', None)
    dev = torch.device('cuda')
    N, C, layers, T, horizon, seed = FULL_MODEL[0]
    model, X, As, Ac, Rw = _full_model_step(N, C, layers, T, horizon, seed, dev)
    X, As, Ac, Rw = X.to(dev), As.to(dev), Ac.to(dev), Rw.to(dev)
    calls = []
    real_small = ops.stc_small_graph
    monkeypatch.setattr(ops, 'stc_small_graph', lambda *a, **k: (calls.append(1), real_small(*a, **k))[1])

    def step():
        model.zero_grad(set_to_none=True)
        (model(X_seq=X, As=As, Ac=Ac) * Rw).sum().backward()

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


# ------------------------------------------------------------------------------------------------------------------------------ CPU: routing
class _StubKernels:
    """A kernel set that says yes to every few-category shape and carries the order-3 dense form."""
    SMALL_STAGED_ROWS, SMALL_PREFERRED_ROWS = 640, 65535
    small_dense_order3 = True

    def cell_small_supported(self, *a):
        return True


def _learned_operand(N):
    return dense_operand(torch.softmax(torch.randn(N, N), -1).requires_grad_())


def test_routing_of_learned_graphs_at_order_3():
    Tc = torch.zeros(3, 5, 5)
    supported = lambda k, op, C=5: small.small_graph_supported(k, op, Tc[:, :C, :C], 3, C, 16, {1, 16})
    # the CPU twin (and any kernel set without the attribute): K = 3 with learned graphs stays on the general path
    assert not hasattr(EmulatedKernels, 'small_dense_order3') and not supported(EmulatedKernels(), _learned_operand(20))
    stub = _StubKernels()
    assert supported(stub, _learned_operand(20))                                    # 100 rows
    assert supported(stub, _learned_operand(128))                                   # 640 rows: the bound itself
    assert not supported(stub, _learned_operand(129))                               # above SMALL_STAGED_ROWS
    assert supported(stub, _learned_operand(40), C=16) and not supported(stub, _learned_operand(41), C=16)
    # a learned graph that is not the full pattern: refused as at order 2
    op = _learned_operand(20)
    op.nnz -= 1
    assert not supported(stub, op)
    # fixed graphs at order 3 are routed as before: sparse yes, dense no
    g = CsrGraph.queen_grid(4, 5)
    assert supported(stub, csr_operand(g, torch.device('cpu'))) and not supported(stub, dense_operand(torch.rand(20, 20)))
    from stc_hip._lib import HipKernels
    assert HipKernels.small_dense_order3 is True


def test_second_order_matrix_is_wired_through_autograd():
    """``small.dense_second_order``: T_2 in the forward's orientation from ``op.fwd_val`` by differentiable ops.  With a stand-in for the node
    (a linear functional of fwd_val and T_2 -- what the node's two graph gradients are the derivative of) the gradient that reaches Gs equals
    the one through the oracle's matrix-side ``cheby_poly``, in float64 on a 6 x 6 matrix."""
    torch.manual_seed(3)
    n = 6
    A, Bw = torch.randn(n, n, dtype=torch.float64), torch.randn(n, n, dtype=torch.float64)
    Gs = torch.softmax(torch.randn(n, n, dtype=torch.float64), -1).requires_grad_()
    op = dense_operand(Gs)
    t2f = small.dense_second_order(op)
    assert t2f.shape == (n * n,) and t2f.requires_grad
    ((op.fwd_val.view(n, n) * A).sum() + (t2f.view(n, n) * Bw).sum()).backward()
    Gr = Gs.detach().clone().requires_grad_()
    T = O.cheby_poly(Gr, 3)
    assert float((t2f.detach().view(n, n) - T[2].detach().t()).abs().max()) < 1e-14         # the forward aggregates with the transposes
    ((T[1].t() * A).sum() + (T[2].t() * Bw).sum()).backward()
    assert rel_err(Gs.grad, Gr.grad) < 1e-13
    assert torch.autograd.gradcheck(lambda G: small.dense_second_order(dense_operand(G)), (Gs.detach().clone().requires_grad_(),))
