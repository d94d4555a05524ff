"""The forward-only route of the few-category cell path (``small.stc_small_graph`` under ``torch.no_grad()`` or when nothing requires grad).

It saves nothing, shares ONE set of phase-to-phase scratch among all cells, releases an inner state after its last reader and, on the HIP kernel
set, passes ``None`` for R and Cand -- planes only a backward reads --, which ``stc_cell_small_fwd_f32`` then does not store (ABI v36).  With grad
mode off a dense graph at Chebyshev order 3 reaches these kernels as well (``small.small_graph_supported``).

CPU: the route on the CPU twin (a subclass that takes ``None`` planes and watches what it is handed): same states as the autograd node, routing,
scratch and live states independent of the number of cells; the C front's refusals.
GPU (-m gpu): the launch with and without the two planes, bit for bit and against the float64 oracle cell; the executor on the HIP kernels; the
module against the reference's goldens and the float64 oracle; peak memory; ``Trainer.test``.
"""
import gc
import os
import weakref

import numpy as np
import pytest
import torch

import STC_GNN as M
from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, _lib, ops, small
from stc_hip import data as sdata
from stc_hip.graph import csr_operand, dense_operand
from tests.abi_refusal_table import EINVAL, MIS, OK, P, check_refusal
from tests.conftest import REPO, load_golden, rel_err, sub_dict
from tests.golden.make_golden import SF_SHAPE, bench_path_inputs
from tests.test_forward_only import SENT, Arena, _encdec
from tests.test_small_cell import _graph, _inputs
from tests.test_small_dense_order3 import _dense_gs, _full_model_step, _StubKernels

H16 = 16
TOL = 1e-5           # max-norm relative, against float64: the bound of tests/test_small_cell.py and of the goldens
SCRATCH = ('U', 'RH', 'Zg', 'Zc', 'Zg2', 'Zc2')


# ----------------------------------------------------------------------------------------------------------------- the twin, watching
class PlainTwin(EmulatedKernels):
    """The CPU twin as it is (no ``small_optional_stores``), remembering per ``cell_small_fwd`` launch which of R / Cand arrived as None, which
    tensors it got as scratch -- (name, input width) -> data pointers -- and, weakly, every state-sized tensor: ``alive`` is how many of them
    still existed at each launch."""

    def __init__(self, state_numel=0):
        super().__init__()
        self.state_numel, self.nones, self.scratch, self.refs, self.alive = state_numel, [], {}, {}, []

    def _see(self, t):
        if isinstance(t, torch.Tensor):
            base = t if t._base is None else t._base
            if base.numel() == self.state_numel and (id(base) not in self.refs or self.refs[id(base)]() is not base):      # (ids are reused)
                self.refs[id(base)] = weakref.ref(base)

    def cell_small_fwd(self, rowptr, colidx, val, X, H, Tc, Wg, bg, Wc, bc, U, R, Cand, Hnew, RH, Zg, Zc, **kw):
        self.nones.append((R is None, Cand is None))
        for name, t in dict(U=U, RH=RH, Zg=Zg, Zc=Zc, Zg2=kw.get('Zg2'), Zc2=kw.get('Zc2')).items():
            if t is not None:
                self.scratch.setdefault((name, X.shape[-1]), set()).add(t.data_ptr())
        for t in (X, H, U, R, Cand, Hnew, RH):
            self._see(t)
        self.refs = {i: r for i, r in self.refs.items() if r() is not None}
        self.alive.append(len(self.refs))
        self.launch(rowptr, colidx, val, X, H, Tc, Wg, bg, Wc, bc, U, R, Cand, Hnew, RH, Zg, Zc, **kw)

    def launch(self, *a, **kw):
        EmulatedKernels.cell_small_fwd(self, *a, **kw)


class LeanTwin(PlainTwin):
    """... as a kernel set that takes None for R / Cand (the twin itself writes both: a scratch tensor stands in)."""
    small_optional_stores = True

    def __init__(self, state_numel=0, dense_order3=False):
        super().__init__(state_numel)
        if dense_order3:
            self.small_dense_order3 = True

    def launch(self, rowptr, colidx, val, X, H, Tc, Wg, bg, Wc, bc, U, R, Cand, *a, **kw):
        EmulatedKernels.cell_small_fwd(self, rowptr, colidx, val, X, H, Tc, Wg, bg, Wc, bc, U, torch.empty_like(U) if R is None else R,
                                       torch.empty_like(U) if Cand is None else Cand, *a, **kw)


def _problem(K, dense, T=3, layers=2, horizon=2, B=2, Hg=4, Wg=5, C=5, seed=0, dev='cpu'):
    """A two-layer encoder-decoder (layer 0 narrow with cin = 1, above it wide) on a queen grid, or on a dense graph of as many nodes."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s_: torch.randn(*s_, generator=g)
    N, h, cin = Hg * Wg, H16, 1
    Gc = torch.softmax(rnd(C, C), -1)
    Tc = torch.stack([torch.eye(C), Gc, 2 * Gc @ Gc - torch.eye(C)][:K]).contiguous().to(dev)
    Gs = torch.softmax(rnd(N, N), -1)
    op = dense_operand(Gs.to(dev)) if dense else csr_operand(CsrGraph.queen_grid(Hg, Wg, normalize=True), torch.device(dev))
    ext = [(torch.rand(B, N, C, cin, generator=g) < 0.3).float().to(dev) for _ in range(T)] + [torch.zeros(B, N, C, h, device=dev) for _ in range(layers)]
    stacks = []
    for i in range(2 * layers):                                      # encoder sets, then the decoder's (its layer 0 reads the top state: wide)
        L = (cin if i == 0 else h) + h
        stacks.append(tuple(p.to(dev) for p in (rnd(K * K * L, 2 * h) / (K * K * L) ** 0.5, rnd(2 * h) * 0.1, rnd(K * K * L, h) / (K * K * L) ** 0.5,
                                                rnd(h) * 0.1)))
    schedule, outputs = _encdec(T, layers, horizon)
    return op, Tc, schedule, outputs, ext, stacks, B * N * C * h


def _leaves(stacks):
    return [tuple(p.clone().requires_grad_() for p in st) for st in stacks]


GRAPHS = [(2, False), (3, False), (2, True), (3, True)]          # (K, dense)
IDS = ['csr-K2', 'csr-K3', 'dense-K2', 'dense-K3']


# ----------------------------------------------------------------------------------------------------------------- CPU: equality, route
@pytest.mark.parametrize('every_cell', [False, True])
@pytest.mark.parametrize('K,dense', GRAPHS, ids=IDS)
def test_forward_only_route_gives_the_stack_of_the_autograd_node(K, dense, every_cell):
    """Under no_grad, and in grad mode with everything frozen: the stack of the grad-mode node, bit for bit (the decoder's top states -- inner
    states are released on the way -- and every cell's state)."""
    op, Tc, schedule, outputs, ext, stacks, numel = _problem(K, dense)
    if every_cell:
        outputs = list(range(len(schedule)))
    em = LeanTwin(numel, dense_order3=dense and K == 3)
    want = small.stc_small_graph(em, op, Tc, K, schedule, outputs, ext, _leaves(stacks))
    assert want.requires_grad and want.shape == (len(outputs), *ext[-1].shape) and not any(r or c for r, c in em.nones)
    del em.nones[:]
    with torch.no_grad():
        got = small.stc_small_graph(em, op, Tc, K, schedule, outputs, ext, _leaves(stacks))
    assert torch.equal(got, want.detach()) and not got.requires_grad
    frozen = small.stc_small_graph(em, op, Tc, K, schedule, outputs, ext, stacks)
    assert torch.equal(frozen, want.detach()) and not frozen.requires_grad
    assert len(em.nones) == 2 * len(schedule) and all(r and c for r, c in em.nones)


def test_routing_between_the_autograd_node_and_the_forward_only_route(monkeypatch):
    op, Tc, schedule, outputs, ext, stacks, numel = _problem(2, False)
    em = LeanTwin(numel)
    node, plain = [], []
    real_apply, real_plain = small._StcSmallGraph.apply, small._forward_only
    monkeypatch.setattr(small._StcSmallGraph, 'apply', staticmethod(lambda *a: (node.append(1), real_apply(*a))[1]))
    monkeypatch.setattr(small, '_forward_only', lambda *a, **k: (plain.append(1), real_plain(*a, **k))[1])
    leaf = _leaves(stacks)
    out = small.stc_small_graph(em, op, Tc, 2, schedule, outputs, ext, leaf)           # a parameter wants a gradient, grad mode on: the node
    assert out.requires_grad and node == [1] and not plain
    assert len(em.nones) == len(schedule) and not any(r or c for r, c in em.nones)     # every launch with its R and Cand buffers
    out.sum().backward()
    assert all(p.grad is not None for st in leaf for p in st)
    del em.nones[:]
    with torch.no_grad():                                                              # no_grad: the plain function, whatever the parameters want
        quiet = small.stc_small_graph(em, op, Tc, 2, schedule, outputs, ext, leaf)
    assert node == [1] and plain == [1] and not quiet.requires_grad and torch.equal(quiet, out.detach())
    frozen = small.stc_small_graph(em, op, Tc, 2, schedule, outputs, ext, stacks)      # grad mode on, everything frozen: the plain function
    assert node == [1] and plain == [1, 1] and not frozen.requires_grad and torch.equal(frozen, quiet)
    assert len(em.nones) == 2 * len(schedule) and all(r and c for r, c in em.nones)
    learned = small.stc_small_graph(em, op, Tc.clone().requires_grad_(), 2, schedule, outputs, ext, stacks)       # only the category graph learns: the node
    assert node == [1, 1] and learned.requires_grad
    # a kernel set without the attribute: None never reaches cell_small_fwd (the unwrapped twin would fail on it), same states
    assert not hasattr(EmulatedKernels, 'small_optional_stores')
    twin = PlainTwin(numel)
    with torch.no_grad():
        plain_out = small.stc_small_graph(twin, op, Tc, 2, schedule, outputs, ext, leaf)
    assert len(twin.nones) == len(schedule) and not any(r or c for r, c in twin.nones) and torch.equal(plain_out, quiet)
    with torch.no_grad():                                                              # ... and through ops.stc_cell_graph, which hands the schedule over
        monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
        assert torch.equal(ops.stc_cell_graph(op, Tc, 2, schedule, outputs, ext, leaf), quiet) and plain == [1, 1, 1, 1]


@pytest.mark.parametrize('K,dense', GRAPHS, ids=IDS)
def test_scratch_and_live_states_do_not_grow_with_the_observed_length(K, dense):
    """The distinct tensors handed over as U / RH / Zg / Zc (Zg2 / Zc2) across a pass: at most one per input-width group and name, for 3 and for 9
    observed steps alike; and the largest number of state-sized tensors alive at a launch is the same for both lengths.  (On the autograd node both
    grow with every cell: one set per cell, everything saved.)"""
    counts, most = {}, {}
    for T in (3, 9):
        op, Tc, schedule, outputs, ext, stacks, numel = _problem(K, dense, T=T)
        em = LeanTwin(numel, dense_order3=dense and K == 3)
        with torch.no_grad():
            out = small.stc_small_graph(em, op, Tc, K, schedule, outputs, ext, stacks)
        assert len(em.alive) == len(schedule)
        counts[T], most[T] = {key: len(ptrs) for key, ptrs in em.scratch.items()}, max(em.alive)
        assert set(counts[T]) == {(name, w) for name in SCRATCH[:4 if K == 2 else 6] for w in (1, H16)}
        del out, em
        gc.collect()
    print(counts, most)
    assert counts[3] == counts[9] and set(counts[3].values()) == {1}
    assert most[3] == most[9], most
    node = LeanTwin(numel)                                                             # the node, for contrast: a set per cell
    small.stc_small_graph(node, op, Tc, K, schedule, outputs, ext, _leaves(stacks))
    assert sum(len(p) for p in node.scratch.values()) == (4 if K == 2 else 6) * len(schedule)


def test_routing_of_dense_graphs_at_order_3_under_no_grad():
    """``small.small_graph_supported``: with grad mode OFF a dense full-pattern graph that does not require grad is accepted at order 3 under the
    learned graph's conditions; in grad mode it is refused as before; the learned answers do not depend on the mode."""
    Tc = torch.zeros(3, 5, 5)
    supported = lambda k, op, C=5: small.small_graph_supported(k, op, Tc[:, :C, :C], 3, C, 16, {1, 16})
    fixed = lambda N: dense_operand(torch.softmax(torch.randn(N, N), -1))
    learned = lambda N: dense_operand(torch.softmax(torch.randn(N, N), -1).requires_grad_())
    stub = _StubKernels()
    bare = type('NoOrder3', (), dict(SMALL_STAGED_ROWS=640, SMALL_PREFERRED_ROWS=65535, cell_small_supported=lambda self, *a: True))()
    with torch.no_grad():
        assert supported(stub, fixed(20)) and supported(stub, fixed(128))              # 100 rows; 640 rows: the bound itself
        assert not supported(stub, fixed(129))                                         # 645 rows
        assert not supported(bare, fixed(20)) and not supported(EmulatedKernels(), fixed(20))
        sparse = csr_operand(CsrGraph.queen_grid(4, 5), torch.device('cpu'))
        assert supported(stub, sparse) and supported(bare, sparse)                     # fixed sparse graphs: as in grad mode
        assert not supported(stub, csr_operand(CsrGraph.from_dense(torch.rand(20, 20)), torch.device('cpu')))      # a full CSR that is no dense operand
        quiet = [supported(stub, learned(n)) for n in (20, 128, 129)] + [supported(bare, learned(20))]
    assert not supported(stub, fixed(20)) and not supported(stub, fixed(128))          # grad mode: unchanged
    assert [supported(stub, learned(n)) for n in (20, 128, 129)] + [supported(bare, learned(20))] == quiet == [True, True, False, False]
    # both callers in ops ask in the same call, in the same mode: the same answer
    for mode in (torch.no_grad, torch.enable_grad):
        with mode():
            op = fixed(20)
            assert small.small_graph_supported(stub, op, Tc, 3, 5, 16, {1, 16}) == (mode is torch.no_grad)


# ----------------------------------------------------------------------------------------------------------------- CPU: the C front
GOOD = {'stc_cell_small_fwd_f32': dict(rowptr=P(), colidx=P(), val=P(), n_nodes=8, nnz=8, graph_is_dense=0, rowptr2=None, colidx2=None, val2=None, nnz2=0,
                                       X=P(), cin=16, H=P(), Tc=P(), Ks=2, Kc=2, Wg=P(), bg=P(), Wc=P(), bc=P(), U=P(), R=P(), Cand=P(), Hnew=P(), RH=P(),
                                       Zg=P(), Zc=P(), Zg2=None, Zc2=None, Z0=None, Z0c=None, Z1c=None, Z2c=None, phase=0, splits=1, batch=2, C=5,
                                       stream=None)}
ORDER3 = dict(rowptr2=P(), colidx2=P(), val2=P(), nnz2=8, Ks=3, Kc=3, Zg2=P(), Zc2=P())


@pytest.fixture(scope='module')
def lib():
    return _lib.load_library()


@pytest.mark.parametrize('order3', [False, True])
def test_refusals_of_the_forward_entry_point(lib, order3):
    """Before any HIP call (no device needed): the planes later phases read stay required, R / Cand are held to the alignment rule when given, and
    neither is missed where nothing is launched."""
    fn = 'stc_cell_small_fwd_f32'
    assert len(GOOD[fn]) == len(_lib._ABI[fn][1])
    more = ORDER3 if order3 else {}
    for name in ('U', 'Hnew', 'RH', 'Zg', 'Zc'):
        check_refusal(lib, GOOD, fn, {**more, name: None}, EINVAL, ('null operand',))
    if order3:
        for name in ('Zg2', 'Zc2'):
            check_refusal(lib, GOOD, fn, {**more, name: None}, EINVAL, ('Zg2, Zc2',))
    for name in ('R', 'Cand'):
        check_refusal(lib, GOOD, fn, {**more, name: MIS}, EINVAL, ('16-byte aligned',))
        check_refusal(lib, GOOD, fn, {**more, name: MIS, 'Cand' if name == 'R' else 'R': None}, EINVAL, ('16-byte aligned',))
    check_refusal(lib, GOOD, fn, {**more, 'R': None, 'Cand': None, 'batch': 0}, OK, ())
    check_refusal(lib, GOOD, fn, {**more, 'R': None, 'Cand': None, 'U': None}, EINVAL, ('null operand',))


def test_binding_says_that_it_takes_the_optional_stores():
    from stc_hip._lib import HipKernels
    assert HipKernels.small_optional_stores is True and _lib.ABI_VERSION >= 36


# ----------------------------------------------------------------------------------------------------------------- GPU: the launch
def _hip():
    from stc_hip._lib import HipKernels
    return HipKernels()


# (B, N, C, cin, splits), graph kinds, orders -- (2, 35, 8, 3, 2) on a 5 x 7 grid: two nodes per row tile, the last tile half full; a narrow input
# that is no multiple of 4; every MODE: 0 (CSR, split; order 3), 1 (CSR staged), 2 (dense staged), 3 (dense, split); the last line adds the wide
# input to the staged forms
LAUNCHES = [((2, 35, 8, 3, 2), ('csr', 'dense'), (2, 3)),
            ((3, 20, 5, 16, 4), ('csr', 'dense'), (2, 3)),
            ((1, 10, 16, 4, 1), ('csr',), (2, 3)),
            ((2, 20, 5, 1, 1), ('dense',), (2,)),
            ((2, 20, 5, 16, 1), ('csr', 'dense'), (2,))]
LAUNCH_CASES = [(*shape, kind, K, bias) for shape, kinds, orders in LAUNCHES for kind in kinds for K in orders for bias in (True, False)]
_ORACLE = {}


def _launch_case(B, N, C, cin, kind, K, bias):
    """(dense float64 Gs, inputs, the float64 oracle's Hnew) of a case: computed once, shared, never modified."""
    key = (B, N, C, cin, kind, K, bias)
    if key not in _ORACLE:
        if kind == 'dense':
            Gs = _dense_gs(N, seed=N + cin)
        else:
            Gs = (CsrGraph.queen_grid(5, 7, normalize=True) if N == 35 else _graph(N, seed=N + cin)).to_dense()
        t = _inputs(B, N, C, cin, seed=3 * N + C + cin + K, bias=bias, K=K)
        d = lambda v: None if v is None else v.double()
        with torch.no_grad():
            want = O.stc_cell(Gs.double(), t['Gc'].double(), d(t['X']), d(t['H']), d(t['Wg']), d(t['bg']), d(t['Wc']), d(t['bc']), K, K)
        _ORACLE[key] = (Gs, t, want)
    return _ORACLE[key]


@pytest.mark.gpu
@pytest.mark.parametrize('B,N,C,cin,splits,kind,K,bias', LAUNCH_CASES)
def test_launch_without_R_and_Cand_is_bit_identical(B, N, C, cin, splits, kind, K, bias):
    """cell_small_fwd with both planes, with neither, and with only one of them: every other output bit for bit, Hnew within 1e-5 of the float64
    oracle cell; every output sits between sentinel margins, an absent plane's stand-in keeps its sentinel."""
    hip, dev = _hip(), torch.device('cuda')
    Gs, t, want = _launch_case(B, N, C, cin, kind, K, bias)
    if kind == 'dense':
        op = dense_operand(Gs.to(dev))
        T2 = (2.0 * Gs.double() @ Gs.double() - torch.eye(N, dtype=torch.float64)).t().contiguous().float().reshape(-1).to(dev)
        graph2 = (op.fwd_rowptr, op.fwd_colidx, T2) if K == 3 else None
    else:
        graph = CsrGraph.from_dense(Gs)
        op = csr_operand(graph, dev)
        g2 = graph.second_order(dev) if K == 3 else None
        graph2 = g2 and tuple(g2[f'fwd2_{n}'] for n in ('rowptr', 'colidx', 'val'))
    d = {n: (None if v is None else v.to(dev)) for n, v in t.items()}
    plane, zgw = (B, N, C, H16), hip.cell_small_zg_width(cin)
    kept = ('U', 'Hnew', 'RH', 'Zg', 'Zc') + (('Zg2', 'Zc2') if K == 3 else ())
    runs = []
    for with_r, with_cand in ((True, True), (False, False), (False, True), (True, False)):
        ar = Arena(dev, U=plane, R=plane, Cand=plane, Hnew=plane, RH=plane, Zg=(B, N * C, zgw), Zc=(B, N * C, H16),
                   **(dict(Zg2=(B, N * C, zgw), Zc2=(B, N * C, H16)) if K == 3 else {}))
        third = dict(graph2=graph2, Zg2=ar['Zg2'], Zc2=ar['Zc2']) if K == 3 else {}
        hip.cell_small_fwd(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, d['X'], d['H'], d['Tc'], d['Wg'], d['bg'], d['Wc'], d['bc'], ar['U'],
                           ar['R'] if with_r else None, ar['Cand'] if with_cand else None, ar['Hnew'], ar['RH'], ar['Zg'], ar['Zc'], splits=splits, **third)
        torch.cuda.synchronize()
        assert ar.gaps_clean(), 'a launch wrote outside its outputs'
        assert ar.untouched('R') == (not with_r) and ar.untouched('Cand') == (not with_cand)
        assert all(bool(torch.isfinite(ar[n]).all()) and not bool((ar[n] == SENT).any()) for n in kept)
        runs.append(ar)
    full = runs[0]
    for ar in runs[1:]:
        for n in kept:
            assert torch.equal(ar[n], full[n]), f'{n} differs in {int((ar[n] != full[n]).sum())} elements'
    assert torch.equal(runs[2]['Cand'], full['Cand']) and torch.equal(runs[3]['R'], full['R'])
    assert torch.equal(full['RH'], full['R'] * d['H'])
    err = rel_err(runs[1]['Hnew'], want)
    print(f'lean Hnew against float64: {err:.3e}')
    assert err < TOL


# ----------------------------------------------------------------------------------------------------------------- GPU: executor
def _spy_small_fwd(monkeypatch, log):
    from stc_hip._lib import HipKernels
    real = HipKernels.cell_small_fwd

    def spy(self, rowptr, colidx, val, X, H, Tc, Wg, bg, Wc, bc, U, R, Cand, *a, **kw):
        log.append((R is None, Cand is None))
        return real(self, rowptr, colidx, val, X, H, Tc, Wg, bg, Wc, bc, U, R, Cand, *a, **kw)
    monkeypatch.setattr(HipKernels, 'cell_small_fwd', spy)


@pytest.mark.gpu
@pytest.mark.parametrize('K,dense', GRAPHS, ids=IDS)
def test_forward_only_executor_on_the_hip_kernels(monkeypatch, K, dense):
    hip = _hip()
    op, Tc, schedule, outputs, ext, stacks, _ = _problem(K, dense, dev='cuda')
    outputs = list(range(len(schedule)))
    log = []
    _spy_small_fwd(monkeypatch, log)
    want = small.stc_small_graph(hip, op, Tc, K, schedule, outputs, ext, _leaves(stacks))
    assert want.requires_grad and len(log) == len(schedule) and not any(r or c for r, c in log)
    del log[:]
    with torch.no_grad():
        got = small.stc_small_graph(hip, op, Tc, K, schedule, outputs, ext, _leaves(stacks))
    torch.cuda.synchronize()
    assert torch.equal(got, want.detach()) and not got.requires_grad
    assert len(log) == len(schedule) and all(r and c for r, c in log)
    with torch.no_grad():                                            # the decoder's top states alone: inner states are released on the way
        top = small.stc_small_graph(hip, op, Tc, K, schedule, outputs[-3::2], ext, stacks)
    assert torch.equal(top, want.detach()[-3::2])


# ----------------------------------------------------------------------------------------------------------------- GPU: model
def _count_small_graph_calls(monkeypatch):
    calls, plain = [], []
    real_small, real_plain = ops.stc_small_graph, small._forward_only
    monkeypatch.setattr(ops, 'stc_small_graph', lambda *a, **k: (calls.append(1), real_small(*a, **k))[1])
    monkeypatch.setattr(small, '_forward_only', lambda *a, **k: (plain.append(1), real_plain(*a, **k))[1])
    return calls, plain


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['g14_sf_shape', 'g15_sf_shape_k3', 'g5_sf_shape'])
def test_no_grad_prediction_against_reference_goldens(monkeypatch, name):
    """The SF shape through STCGNN under no_grad -- fixed CSR graph at K = 2 (g14) and K = 3 (g15), the reference's own dense graphs at K = 2 (g5):
    within 1e-5 of the reference's prediction, on the few-category kernels' forward-only route (one call per forward, every launch without R / Cand)."""
    monkeypatch.setattr(ops, '_kernels', None)
    g = load_golden(name)
    model = M.STCGNN(num_nodes=int(g['N']), num_categories=int(g['C']), Ks=int(g['K']), Kc=int(g['K']), input_dim=1, hidden_dim=int(g['h']),
                     num_layers=int(g['layers']), out_horizon=int(g['horizon']), graph_mode='csr-fixed').to('cuda')
    model.load_state_dict({k: v.cuda() for k, v in sub_dict(g, 'sd/').items()})
    if name == 'g5_sf_shape':
        X, As, Ac = g['X'].float().cuda(), g['Gs'].cuda(), g['Gc'].cuda()
    else:
        s = bench_path_inputs(int(g['C']), int(g['K']), **SF_SHAPE)
        X, As, Ac = s['X'].cuda(), CsrGraph.from_dense(s['Gs']), s['Gc'].cuda()
    calls, plain = _count_small_graph_calls(monkeypatch)
    log = []
    _spy_small_fwd(monkeypatch, log)
    with torch.no_grad():
        y = model(X_seq=X, As=As, Ac=Ac)
    err = rel_err(y, g['yhat'])
    print(f'{name}: no_grad yhat relative error {err:.3e}')
    assert err < TOL and not y.requires_grad
    assert calls == [1] and plain == [1] and log and all(r and c for r, c in log)
    y_grad = model(X_seq=X, As=As, Ac=Ac)
    assert y_grad.requires_grad and plain == [1] and torch.equal(y, y_grad.detach())


@pytest.mark.gpu
def test_learned_graphs_at_order_3_under_no_grad_run_on_the_small_graph_kernels(monkeypatch):
    """The reference's full model with learned graphs at K = 3 (N = 20, C = 5, two layers, 3 + 2 steps, B = 3) under no_grad: its cells on
    ``stc_small_graph`` (the routing of a dense graph that does not require grad, grad mode off), the prediction within 1e-5 of the float64
    oracle of the full model."""
    monkeypatch.setattr(ops, '_kernels', None)
    dev = torch.device('cuda')
    N, C, layers, T, horizon, seed = 20, 5, 2, 3, 2, 33
    model, X, As, Ac, _ = _full_model_step(N, C, layers, T, horizon, seed, dev)
    X = (torch.rand(3, T, N, C, generator=torch.Generator().manual_seed(seed)) < 0.3).float()
    calls, plain = _count_small_graph_calls(monkeypatch)
    with torch.no_grad():
        y = model(X_seq=X.to(dev), As=As.to(dev), Ac=Ac.to(dev))
    assert calls == [1] and plain == [1], 'the cells did not run on the few-category kernels'
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want = O.stcgnn_forward(X.double(), As.double(), Ac.double(), sd, 3, 3, 16, layers, horizon)
    err = rel_err(y, want)
    print(f'learned K=3 no_grad yhat relative error {err:.3e}')
    assert err < TOL and y.shape == (3, horizon, N, C) and not y.requires_grad


@pytest.mark.gpu
def test_no_grad_peak_memory_does_not_grow_with_the_observed_length(monkeypatch):
    """Peak allocation of a no_grad forward (above what is allocated before the call) for 3 and for 9 observed steps on the few-category route: the
    six more steps may cost their two narrow planes each and one state plane of slack -- nothing per cell."""
    monkeypatch.setattr(ops, '_kernels', None)
    Hg, Wg, C, B, h = 5, 6, 5, 4, 16
    N = Hg * Wg
    torch.manual_seed(11)
    model = M.STCGNN(N, C, 2, 2, 1, h, 2, 2, graph_mode='csr-fixed').to('cuda').eval()
    graph = CsrGraph.queen_grid(Hg, Wg, normalize=True)
    Gc = torch.softmax(torch.randn(C, C), -1).cuda()
    calls, plain = _count_small_graph_calls(monkeypatch)
    peaks = {}
    for T in (3, 9):
        X = (torch.rand(B, T, N, C) < 0.3).float().cuda()
        with torch.no_grad():
            model(X_seq=X, As=graph, Ac=Gc)                           # (warm-up: graph operands, workspaces)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            y = model(X_seq=X, As=graph, Ac=Gc)
            torch.cuda.synchronize()
        peaks[T] = torch.cuda.max_memory_allocated() - before
        del y
    assert len(plain) == len(calls) == 4
    state_plane = B * N * C * h * 4
    narrow_plane = state_plane // 16
    print(f'peak above the inputs: T=3 {peaks[3]} B, T=9 {peaks[9]} B = {peaks[3] / state_plane:.2f} / {peaks[9] / state_plane:.2f} state planes')
    assert peaks[9] - peaks[3] <= 6 * 2 * narrow_plane + state_plane


@pytest.mark.gpu
def test_trainer_test_gives_the_grad_mode_forecast(monkeypatch, tmp_path):
    """Trainer.test() (no_grad) on a 6 x 7 corner of the SF incidents with its own five categories, csr-fixed: the forecast array of a grad-enabled
    forward of the same checkpoint, through the few-category forward-only route (once per test batch)."""
    from stc_hip.trainer import Trainer
    monkeypatch.setattr(ops, '_kernels', None)
    sf = sdata.load_incidents(os.path.join(REPO, 'tests', 'golden', 'sf_incidents_4h.npz'))
    Hg, Wg, C = 6, 7, 5
    data = dict(inc=np.ascontiguousarray(sf['inc'][:48, :Hg, :Wg]), s_adj=CsrGraph.queen_grid(Hg, Wg, normalize=True), c_cor=np.asarray(sf['c_cor']))
    assert data['inc'].shape[-1] == C and data['c_cor'].shape == (C, C)
    params = dict(device='cuda:0', H=Hg, W=Wg, C=C, batch_size=4, obs_len=4, pred_len=2, split_ratio=[6, 1, 1], model='STC-GNN', cheby_order=2,
                  hidden_dim=16, nn_layers=2, learn_rate=2e-3, decay_rate=1e-4, num_epochs=1, time_slice=4, city='SF', output_dir=str(tmp_path))
    loaders = sdata.get_data_loader(params, data, params['obs_len'], params['pred_len'], params['split_ratio'])
    torch.manual_seed(7)
    trainer = Trainer(params, data, graph_mode='csr-fixed')
    torch.save({'epoch': 0, 'train_loss': 0.0, 'val_loss': 0.0, 'state_dict': trainer.model.state_dict()}, trainer.checkpoint_path)
    calls, plain = _count_small_graph_calls(monkeypatch)
    res = trainer.test(loaders)
    assert len(plain) == len(calls) == len(loaders['test']) > 0
    del plain[:]
    with torch.enable_grad():
        want = torch.cat([trainer._forward(x) for x, _ in loaders['test']], 0)
    assert want.requires_grad and not plain
    assert res['test']['forecast'].shape == (loaders['test'].length, 2, Hg * Wg, C)
    assert np.array_equal(res['test']['forecast'], want.detach().cpu().numpy())
