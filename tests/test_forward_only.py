"""The forward-only route of ``ops.stc_cell_graph`` (``ops._forward_only``): what runs under ``torch.no_grad()`` or when nothing requires grad.

It keeps nothing for a backward -- states, aggregations, input rows and temporaries are released after their last consumer -- and on the fp32 HIP
kernel set it passes ``None`` for the planes only a backward reads (``Rg``, ``Cand``, ``RH``), which the kernels then do not store (ABI v34).

GPU (-m gpu): the five entry points with and without the optional plane, bit for bit; the module against the reference's goldens; peak
memory independent of the observed length; ``Trainer.test``.  CPU: the route on the CPU twin (a subclass that takes ``None`` planes and watches
what it is handed): same states as the autograd node, liveness, routing.
"""
import gc
import inspect
import os
import weakref

import numpy as np
import pytest
import torch

import STC_GNN as M
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, ops
from stc_hip import data as sdata
from stc_hip.graph import csr_operand
from tests.conftest import REPO, load_golden, rel_err, sub_dict
from tests.golden.make_golden import bench_path_inputs

SENT = -7.25          # the sentinel: not NaN, not a value the kernels produce in these tests (gates in (0, 1), states in (-1, 1), A / Bm small)
H16 = 16


# ----------------------------------------------------------------------------------------------------------------- helpers
class Arena:
    """Tensors carved out of ONE sentinel-filled buffer with 64-float gaps before, between and after them (every tensor 16-byte aligned): what a
    launch wrote outside its results shows in the gaps or in a tensor it was not given."""

    GAP = 64

    def __init__(self, dev, **shapes):
        sizes = {k: int(np.prod(s)) for k, s in shapes.items()}
        total = self.GAP + sum(-(-n // 4) * 4 + self.GAP for n in sizes.values())
        self.buf = torch.full((total,), SENT, dtype=torch.float32, device=dev)
        self.inside = torch.zeros(total, dtype=torch.bool, device=dev)
        self.t, at = {}, self.GAP
        for k, s in shapes.items():
            self.t[k] = self.buf[at:at + sizes[k]].view(*s)
            self.inside[at:at + sizes[k]] = True
            at += -(-sizes[k] // 4) * 4 + self.GAP

    def __getitem__(self, k):
        return self.t[k]

    def fill(self, k, value):
        self.t[k].copy_(value)
        return self.t[k]

    def gaps_clean(self):
        return bool((self.buf[~self.inside] == SENT).all())

    def untouched(self, k):
        return bool((self.t[k] == SENT).all())


def _hip():
    from stc_hip._lib import HipKernels
    return HipKernels()


def _formats(hip):
    """The kernel set on both operand formats: the default one and the 24-bit view heavy graphs get (the same object if that is the default)."""
    other = hip.for_graph(float('inf'))
    return [hip] if other is hip else [hip, other]


def _blend_operands(n, B, C, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.randn(B, n, C, H16, generator=g)
    return dict(Bm=rnd() * 0.5, A=rnd() * 0.5, U=torch.sigmoid(rnd()), H=torch.tanh(rnd()))


# ----------------------------------------------------------------------------------------------------------------- 1. kernels, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize('H,W,B', [(12, 20, 2), (9, 33, 1), (31, 8, 3)])
def test_ring2_blend_without_the_candidate_plane_is_bit_identical(H, W, B):
    hip, C, n = _hip(), 32, H * W
    op = csr_operand(CsrGraph.queen_grid(H, W, normalize=True), torch.device('cuda'))
    assert op.fwd_ring2 is not None
    src = _blend_operands(n, B, C, H * W)
    runs = []
    for with_cand in (True, False):
        shape = (B, n, C, H16)
        ar = Arena('cuda', **{k: shape for k in ('Bm', 'A', 'U', 'H', 'Cand', 'Hnew', 'SHnew')})
        for k, v in src.items():
            ar.fill(k, v.cuda())
        hip.ring2_blend(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, op.fwd_ring2, ar['Bm'], ar['A'], ar['U'], ar['H'],
                        ar['Cand'] if with_cand else None, ar['Hnew'], ar['SHnew'])
        torch.cuda.synchronize()
        assert ar.gaps_clean() and all(torch.equal(ar[k].cpu(), v) for k, v in src.items())
        assert not ar.untouched('Hnew') and not ar.untouched('SHnew') and ar.untouched('Cand') == (not with_cand)
        runs.append(ar)
    assert torch.equal(runs[0]['Hnew'], runs[1]['Hnew']) and torch.equal(runs[0]['SHnew'], runs[1]['SHnew'])


@pytest.mark.gpu
@pytest.mark.parametrize('H,W,B,copies', [(12, 20, 2, False), (9, 33, 1, False), (31, 8, 3, False), (7, 5, 2, True)])
def test_spmm_blend_without_the_candidate_plane_is_bit_identical(H, W, B, copies):
    """... also with two state copies and a side source (the producer of an interleaved cell's input rows)."""
    hip, C, n, cin = _hip(), 32, H * W, 1
    op = csr_operand(CsrGraph.queen_grid(H, W, normalize=True), torch.device('cuda'))
    src = _blend_operands(n, B, C, H * W + 1)
    side = torch.randn(B * n, C, cin, generator=torch.Generator().manual_seed(3))
    runs = []
    for with_cand in (True, False):
        shape = (B, n, C, H16)
        extra = dict(copy0=(B * n, C, 20), copy1=(B * n, C, 32), side=(B * n, C, cin)) if copies else {}
        ar = Arena('cuda', **{k: shape for k in ('Bm', 'A', 'U', 'H', 'Cand', 'Hnew')}, **extra)
        for k, v in src.items():
            ar.fill(k, v.cuda())
        kw = {}
        if copies:                                    # copy 0: [side | state | zero pad] rows of 20, copy 1: the state in columns 16..31 of rows of 32
            ar.fill('side', side.cuda())
            kw = dict(copies=[(ar['copy0'], cin), (ar['copy1'], 16)], side=ar['side'])
        hip.spmm_blend_fwd(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, op.fwd_plan, ar['Bm'], ar['A'], ar['U'], ar['H'],
                           ar['Cand'] if with_cand else None, ar['Hnew'], **kw)
        torch.cuda.synchronize()
        assert ar.gaps_clean() and all(torch.equal(ar[k].cpu(), v) for k, v in src.items())
        assert not ar.untouched('Hnew') and ar.untouched('Cand') == (not with_cand)
        runs.append(ar)
    assert torch.equal(runs[0]['Hnew'], runs[1]['Hnew'])
    if copies:
        a, b = runs
        assert torch.equal(a['copy0'], b['copy0']) and torch.equal(a['copy1'], b['copy1'])
        Hn = a['Hnew'].view(B * n, C, H16)
        assert torch.equal(a['copy0'][..., cin:cin + 16], Hn) and torch.equal(a['copy0'][..., :cin], a['side']) and bool((a['copy0'][..., cin + 16:] == 0).all())
        assert torch.equal(a['copy1'][..., 16:], Hn) and bool((a['copy1'][..., :16] == SENT).all())


def _gate_operands(nodes, C, cin, K, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s_: torch.randn(*s_, generator=g)
    Lw = cin + H16
    Tc = rnd(K, C, C) / C ** 0.5
    Tc[0] = torch.eye(C)
    return dict(Tc=Tc, Wg=rnd(K * K * Lw, 2 * H16) / (2 * K * Lw) ** 0.5, bg=rnd(2 * H16), Wc=rnd(K * K * Lw, H16) / (2 * K * Lw) ** 0.5, bc=rnd(H16),
                Zx=[rnd(nodes, C, cin) for _ in range(K)], Zh=[torch.tanh(rnd(nodes, C, H16)) for _ in range(K)], U=torch.sigmoid(rnd(nodes, C, H16)))


@pytest.mark.gpu
@pytest.mark.parametrize('C', [32, 64])
@pytest.mark.parametrize('cin', [16, 1, 4])
def test_planar_gates_without_the_reset_gate_plane_are_bit_identical(C, cin):
    """stc_cell_gates_fwd_planar_f32 with the fused candidate projection: Rg given / None (and RH None as well); 35 nodes: a ragged last wave."""
    nodes = 35
    s = _gate_operands(nodes, C, cin, 2, 100 + C + cin)
    cu = lambda t: t.cuda()
    for hip in _formats(_hip()):
        runs = []
        for rg, rh in ((True, True), (False, True), (False, False)):
            plane = (nodes, C, H16)
            ar = Arena('cuda', X=(nodes, C, cin), SX=(nodes, C, cin), H=plane, SH=plane, U=plane, Rg=plane, RH=plane, A=plane, Bm=plane)
            for k, v in (('X', s['Zx'][0]), ('SX', s['Zx'][1]), ('H', s['Zh'][0]), ('SH', s['Zh'][1])):
                ar.fill(k, cu(v))
            amax = hip.act_amax_buffer(ar['H'], 4)
            hip.cell_gates_fwd_planar(ar['X'], ar['H'], ar['SX'], ar['SH'], cu(s['Tc']), cu(s['Wg']), cu(s['bg']), ar['U'], ar['Rg'] if rg else None,
                                      ar['RH'] if rh else None, post=(cu(s['Wc']), cu(s['bc']), ar['A'], ar['Bm']), act_amax=amax)
            torch.cuda.synchronize()
            assert ar.gaps_clean() and torch.equal(ar['H'].cpu(), s['Zh'][0]) and torch.equal(ar['X'].cpu(), s['Zx'][0])
            assert ar.untouched('Rg') == (not rg) and ar.untouched('RH') == (not rh) and not any(ar.untouched(k) for k in ('U', 'A', 'Bm'))
            runs.append((ar, amax))
        (a, am), rest = runs[0], runs[1:]
        for b, bm in rest:
            assert all(torch.equal(a[k], b[k]) for k in ('U', 'A', 'Bm'))
            assert (am is None and bm is None) or torch.equal(am, bm)
        assert torch.equal(a['RH'], runs[1][0]['RH'])
        with pytest.raises(Exception, match='optional only with the fused candidate projection'):
            hip.cell_gates_fwd_planar(a['X'], a['H'], a['SX'], a['SH'], cu(s['Tc']), cu(s['Wg']), cu(s['bg']), a['U'], None, a['RH'])


@pytest.mark.gpu
@pytest.mark.parametrize('C', [32, 64])
@pytest.mark.parametrize('cin', [16, 1, 4])
def test_order3_planar_kernels_without_the_backward_planes_are_bit_identical(C, cin):
    """stc_cell_gates_fwd_planar_k_f32 with Rg = None and stc_cell_cand_fwd_planar_k_f32 with Cand = None, where the order-3 planar kernels are
    built for the category count (C = 32)."""
    nodes, K = 35, 3
    base = _hip()
    if not base.cell_planar_k_supported(K, C, H16):
        assert C == 64                                 # (not a skip: the order-3 planar kernels exist for 32 categories; nothing to compare at 64)
        return
    s = _gate_operands(nodes, C, cin, K, 200 + C + cin)
    cu = lambda t: t.cuda()
    for hip in _formats(base):
        gates, cands = [], []
        for given in (True, False):
            plane = (nodes, C, H16)
            ar = Arena('cuda', **{f'Zx{n}': (nodes, C, cin) for n in range(K)}, **{f'Zh{n}': plane for n in range(K)},
                       U=plane, Rg=plane, RH=plane, Uin=plane, Cand=plane, Hnew=plane)
            Zx = [ar.fill(f'Zx{n}', cu(s['Zx'][n])) for n in range(K)]
            Zh = [ar.fill(f'Zh{n}', cu(s['Zh'][n])) for n in range(K)]
            ar.fill('Uin', cu(s['U']))
            am_g, am_c = hip.act_amax_buffer(ar['U'], 2 * K), hip.act_amax_buffer(ar['U'], 2 * K)
            hip.cell_gates_fwd_planar_k(Zx, Zh, cu(s['Tc']), cu(s['Wg']), cu(s['bg']), ar['U'], ar['Rg'] if given else None, ar['RH'], act_amax=am_g)
            torch.cuda.synchronize()
            assert ar.gaps_clean() and ar.untouched('Rg') == (not given) and ar.untouched('Cand') and ar.untouched('Hnew')
            gates.append((ar['U'].clone(), ar['RH'].clone(), am_g))
            # (Zh doubles as the planes of R*H here: any planes do for a bit-for-bit comparison)
            hip.cell_cand_fwd_planar_k(Zx, Zh, cu(s['Tc']), cu(s['Wc']), cu(s['bc']), ar['Uin'], Zh[0], ar['Cand'] if given else None, ar['Hnew'], act_amax=am_c)
            torch.cuda.synchronize()
            assert ar.gaps_clean() and ar.untouched('Cand') == (not given) and not ar.untouched('Hnew')
            assert all(torch.equal(ar[f'Zh{n}'].cpu(), s['Zh'][n]) and torch.equal(ar[f'Zx{n}'].cpu(), s['Zx'][n]) for n in range(K))
            cands.append((ar['Hnew'].clone(), am_c))
        assert torch.equal(gates[0][0], gates[1][0]) and torch.equal(gates[0][1], gates[1][1])
        assert torch.equal(cands[0][0], cands[1][0])
        for a, b in ((gates[0][2], gates[1][2]), (cands[0][1], cands[1][1])):
            assert (a is None and b is None) or torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------- 2. module, against the reference
PLANAR_LAUNCHES = ('cell_gates_fwd_planar', 'spmm_blend_fwd', 'ring2_blend', 'cell_gates_fwd_planar_k', 'cell_cand_fwd_planar_k')


def _spy_on(monkeypatch, cls, log):
    """Record, for every planar forward launch through ``cls``, which of its optional planes arrived as None."""
    for name in PLANAR_LAUNCHES:
        real = getattr(cls, name)
        params = list(inspect.signature(real).parameters)

        def spy(self, *a, _real=real, _params=params, _name=name, **kw):
            bound = dict(zip(_params[1:], a), **kw)
            log.append((_name, {p: bound.get(p) is None for p in ('Rg', 'RH', 'Cand') if p in _params}))
            return _real(self, *a, **kw)
        monkeypatch.setattr(cls, name, spy)


@pytest.mark.gpu
@pytest.mark.parametrize('name,C,K', [('g11_bench_c32', 32, 2), ('g12_bench_c64', 64, 2), ('g13_bench_c32_k3', 32, 3)])
def test_no_grad_prediction_against_reference_goldens(monkeypatch, name, C, K):
    """The bench path under no_grad: within 1e-5 (max-norm, relative) of the reference's yhat, bit for bit the grad-mode prediction of the same
    model, and through the forward-only route with every Rg / RH / Cand of the planar launches passed as None."""
    from stc_hip._lib import HipKernels
    monkeypatch.setattr(ops, '_kernels', None)
    g = load_golden(name)
    s = bench_path_inputs(C, K)
    model = M.STCGNN(num_nodes=int(g['N']), num_categories=int(g['C']), Ks=int(g['K']), Kc=int(g['K']), input_dim=1, hidden_dim=int(g['h']),
                     num_layers=int(g['layers']), out_horizon=int(g['horizon']), graph_mode='csr-fixed').to('cuda')
    model.load_state_dict({k: v.cuda() for k, v in sub_dict(g, 'sd/').items()})
    graph = CsrGraph.from_dense(s['Gs'])
    log = []
    _spy_on(monkeypatch, HipKernels, log)
    y_grad = model(X_seq=s['X'].cuda(), As=graph, Ac=s['Gc'].cuda())
    assert y_grad.requires_grad and log and not any(v for _, nones in log for p, v in nones.items() if p != 'RH')      # the autograd node: every plane stored
    del log[:]
    with torch.no_grad():
        y = model(X_seq=s['X'].cuda(), As=graph, Ac=s['Gc'].cuda())
    err = rel_err(y, g['yhat'])
    print(f'{name}: no_grad yhat relative error {err:.3e}')
    assert err < 1e-5
    assert torch.equal(y, y_grad.detach())
    want = {'cell_gates_fwd_planar', 'spmm_blend_fwd', 'ring2_blend'} if K == 2 else {'cell_gates_fwd_planar_k', 'cell_cand_fwd_planar_k'}
    seen = {n for n, _ in log}
    assert seen and seen <= want and ({'cell_gates_fwd_planar'} <= seen if K == 2 else seen == want)
    for n, nones in log:
        assert all(nones[p] for p in nones if not (p == 'RH' and K == 3)), (n, nones)
    assert not y.requires_grad


# ----------------------------------------------------------------------------------------------------------------- 3. memory
@pytest.mark.gpu
def test_no_grad_peak_memory_does_not_grow_with_the_observed_length(monkeypatch):
    """Peak allocation of a no_grad forward (above what is allocated before the call) for 3 and for 9 observed steps: the six more steps may cost
    their two narrow planes each (an input and its aggregation: cin / 16 of a state plane) and one state plane of slack -- nothing per cell."""
    monkeypatch.setattr(ops, '_kernels', None)
    Hg, Wg, C, B, h = 12, 20, 32, 2, 16
    N = Hg * Wg
    torch.manual_seed(11)
    model = M.STCGNN(N, C, 2, 2, 1, h, 2, 2, graph_mode='csr-fixed').to('cuda').eval()
    graph = CsrGraph.queen_grid(Hg, Wg, normalize=True)
    Gc = torch.softmax(torch.randn(C, C), -1).cuda()
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
    state_plane = B * N * C * h * 4
    narrow_plane = state_plane // 16
    print(f'peak above the inputs: T=3 {peaks[3]} B, T=9 {peaks[9]} B = {peaks[3] / state_plane:.2f} / {peaks[9] / state_plane:.2f} state planes')
    assert peaks[9] - peaks[3] <= 6 * 2 * narrow_plane + state_plane


# ----------------------------------------------------------------------------------------------------------------- 4. trainer
@pytest.mark.gpu
def test_trainer_test_gives_the_grad_mode_forecast(monkeypatch, tmp_path):
    """Trainer.test() (no_grad) on a 6 x 7 corner of the SF incidents, its five categories repeated to 32, csr-fixed: the forecast array of a
    grad-enabled forward of the same checkpoint, and through the forward-only route."""
    from stc_hip.trainer import Trainer
    monkeypatch.setattr(ops, '_kernels', None)
    sf = sdata.load_incidents(os.path.join(REPO, 'tests', 'golden', 'sf_incidents_4h.npz'))
    Hg, Wg, C = 6, 7, 32
    cat = np.arange(C) % 5
    data = dict(inc=np.ascontiguousarray(sf['inc'][:48, :Hg, :Wg][..., cat]), s_adj=CsrGraph.queen_grid(Hg, Wg, normalize=True),
                c_cor=np.asarray(sf['c_cor'])[cat][:, cat])
    params = dict(device='cuda:0', H=Hg, W=Wg, C=C, batch_size=4, obs_len=4, pred_len=2, split_ratio=[6, 1, 1], model='STC-GNN', cheby_order=2,
                  hidden_dim=16, nn_layers=2, learn_rate=2e-3, decay_rate=1e-4, num_epochs=1, time_slice=4, city='SF', output_dir=str(tmp_path))
    loaders = sdata.get_data_loader(params, data, params['obs_len'], params['pred_len'], params['split_ratio'])
    torch.manual_seed(7)
    trainer = Trainer(params, data, graph_mode='csr-fixed')
    torch.save({'epoch': 0, 'train_loss': 0.0, 'val_loss': 0.0, 'state_dict': trainer.model.state_dict()}, trainer.checkpoint_path)
    routed = []
    real = ops._forward_only
    monkeypatch.setattr(ops, '_forward_only', lambda *a, **k: (routed.append(1), real(*a, **k))[1])
    res = trainer.test(loaders)
    assert len(routed) == len(loaders['test']) > 0
    del routed[:]
    with torch.enable_grad():
        want = torch.cat([trainer._forward(x) for x, _ in loaders['test']], 0)
    assert want.requires_grad and not routed
    assert res['test']['forecast'].shape == (loaders['test'].length, 2, Hg * Wg, C)
    assert np.array_equal(res['test']['forecast'], want.detach().cpu().numpy())


# ----------------------------------------------------------------------------------------------------------------- CPU: the route on the twin
class WatchfulTwin(EmulatedKernels):
    """The CPU twin as a kernel set that may take None for the planes only a backward reads (``optional_gate_stores``; the twin itself writes
    every plane: a scratch tensor stands in), and that remembers -- weakly -- every state-sized tensor it is handed: ``alive_at_blend`` is how
    many of them still existed at each blend launch, ``nones`` which optional planes of each planar launch arrived as None.  Only the executor's
    own calls count (``inner``: the twin builds some of its methods from others)."""

    WATCHED = PLANAR_LAUNCHES + ('csr_spmm', 'ring2_chain', 'cell_gates_fwd', 'cell_blend_fwd', 'node_post_fwd', 'concat2')
    BLENDS = ('spmm_blend_fwd', 'ring2_blend', 'cell_cand_fwd_planar_k', 'cell_blend_fwd')

    def __init__(self, optional=True, state_numel=0):
        super().__init__()
        self.optional_gate_stores = bool(optional)
        self.state_numel, self.refs, self.alive_at_blend, self.nones, self.inner = state_numel, {}, [], [], 0

    def _see(self, obj):
        if isinstance(obj, torch.Tensor):
            base = obj if obj._base is None else obj._base
            if base.numel() == self.state_numel and (id(base) not in self.refs or self.refs[id(base)]() is not base):      # (ids are reused)
                self.refs[id(base)] = weakref.ref(base)
        elif isinstance(obj, (list, tuple)):
            for o in obj:
                self._see(o)

    def __getattribute__(self, name):
        attr = super().__getattribute__(name)
        if name not in WatchfulTwin.WATCHED or super().__getattribute__('inner'):
            return attr

        def call(*a, **kw):
            self._see(a)
            self._see(list(kw.values()))
            if name in PLANAR_LAUNCHES:
                params = list(inspect.signature(attr).parameters)
                bound = dict(zip(params, a), **kw)
                self.nones.append((name, {p: bound.get(p) is None for p in ('Rg', 'RH', 'Cand') if p in params}))
            if name in self.BLENDS:
                self.refs = {i: r for i, r in self.refs.items() if r() is not None}
                self.alive_at_blend.append(len(self.refs))
            self.inner += 1
            try:
                return attr(*a, **kw)
            finally:
                self.inner -= 1
        return call

    # ---- the five methods with an optional plane: a scratch tensor stands in for None
    def cell_gates_fwd_planar(self, X, H, SX, SH, Tc, W, bias, U, Rg, RH, post=None, act_amax=None):
        super().cell_gates_fwd_planar(X, H, SX, SH, Tc, W, bias, U, torch.empty_like(U) if Rg is None else Rg, RH, post=post, act_amax=act_amax)

    def spmm_blend_fwd(self, rowptr, colidx, val, plan, Bm, A, U, H, Cand, Hnew, copies=(), side=None):
        super().spmm_blend_fwd(rowptr, colidx, val, plan, Bm, A, U, H, torch.empty_like(H) if Cand is None else Cand, Hnew, copies=copies, side=side)

    def ring2_blend(self, rowptr, colidx, val, ring2, Bm, A, U, H, Cand, Hnew, SHnew):
        super().ring2_blend(rowptr, colidx, val, ring2, Bm, A, U, H, torch.empty_like(H) if Cand is None else Cand, Hnew, SHnew)

    def cell_gates_fwd_planar_k(self, Zx, Zh, Tc, W, bias, U, Rg, RH, act_amax=None):
        super().cell_gates_fwd_planar_k(Zx, Zh, Tc, W, bias, U, torch.empty_like(U) if Rg is None else Rg, RH, act_amax=act_amax)

    def cell_cand_fwd_planar_k(self, Zx, Zh, Tc, W, bias, U, H, Cand, Hnew, act_amax=None):
        super().cell_cand_fwd_planar_k(Zx, Zh, Tc, W, bias, U, H, torch.empty_like(H) if Cand is None else Cand, Hnew, act_amax=act_amax)


def _encdec(T, layers, horizon):
    """The schedule STCGNN builds: encoder layer-major then time, decoder step-major; outputs = the decoder's top states."""
    eid = lambda l, t: l * T + t
    did = lambda l, s_: layers * T + s_ * layers + l
    schedule = []
    for l in range(layers):
        for t in range(T):
            schedule.append((l, ('ext', t) if l == 0 else ('cell', eid(l - 1, t)), ('ext', T + l) if t == 0 else ('cell', eid(l, t - 1))))
    for s_ in range(horizon):
        for l in range(layers):
            top_prev = eid(layers - 1, T - 1) if s_ == 0 else did(layers - 1, s_ - 1)
            schedule.append((layers + l, ('cell', top_prev) if l == 0 else ('cell', did(l - 1, s_)), ('cell', eid(l, T - 1) if s_ == 0 else did(l, s_ - 1))))
    return schedule, [did(layers - 1, s_) for s_ in range(horizon)]


def _problem(K, cin, T=3, layers=2, horizon=2, B=2, Hg=4, Wg=5, C=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s_: torch.randn(*s_, generator=g)
    N, h = Hg * Wg, H16
    op = csr_operand(CsrGraph.queen_grid(Hg, Wg, normalize=True), torch.device('cpu'))
    Gc = torch.softmax(rnd(C, C), -1)
    T_list = [torch.eye(C), Gc] + ([2 * Gc @ Gc - torch.eye(C)] if K == 3 else [])
    Tc = torch.stack(T_list[:K]).contiguous()
    ext = [(torch.rand(B, N, C, cin, generator=g) < 0.3).float() for _ in range(T)] + [torch.zeros(B, N, C, h) for _ in range(layers)]
    stacks = []
    for l in list(range(layers)) * 2:
        L = (cin if l == 0 else h) + h
        stacks.append((rnd(K * K * L, 2 * h) / (K * K * L) ** 0.5, rnd(2 * h) * 0.1, rnd(K * K * L, h) / (K * K * L) ** 0.5, rnd(h) * 0.1))
    schedule, outputs = _encdec(T, layers, horizon)
    return op, Tc, schedule, outputs, ext, stacks, B * N * C * h


@pytest.mark.parametrize('optional', [True, False])
@pytest.mark.parametrize('K,cin,forms', [(2, 1, {'PLANAR_ONE_BWD', 'PLANAR'}), (3, 1, {'PLANAR3'}), (2, 5, {'ROWS_POST', 'ROWS_SLABS', 'PLANAR_ONE_BWD', 'PLANAR'})])
def test_forward_only_route_gives_the_states_of_the_autograd_node(monkeypatch, K, cin, forms, optional):
    """Encoder + decoder at K = 2, at K = 3, and with interleaved layer-0 cells (an input 5 columns wide): EVERY cell's state, bit for bit."""
    op, Tc, schedule, _, ext, stacks, numel = _problem(K, cin)
    outputs = list(range(len(schedule)))
    em = WatchfulTwin(optional, numel)
    monkeypatch.setattr(ops, '_kernels', em)
    seen_forms = []
    real_forms = ops._cell_forms
    monkeypatch.setattr(ops, '_cell_forms', lambda *a: (seen_forms.append(real_forms(*a)), seen_forms[-1])[1])
    leaf = [tuple(p.clone().requires_grad_() for p in st) for st in stacks]
    want = ops._StcCellGraph.apply(op, K, schedule, outputs, len(ext), Tc, op.fwd_val, *ext, *[p for st in leaf for p in st])
    assert want.requires_grad and not any(v for _, nones in em.nones for k, v in nones.items() if k != 'RH')
    del em.nones[:]
    with torch.no_grad():
        got = ops.stc_cell_graph(op, Tc, K, schedule, outputs, ext, stacks)
    assert torch.equal(got, want.detach()) and not got.requires_grad
    names = {f.name for f in seen_forms[-1]}
    assert names <= forms and (cin != 5 or names & {'ROWS_POST', 'ROWS_SLABS'}) and seen_forms[0] == seen_forms[-1]
    planar_launches = [(n, nones) for n, nones in em.nones if n != 'spmm_blend_fwd']
    assert planar_launches
    if optional:      # every planar launch without its backward-only planes (order 3 keeps R*H: it is aggregated); an interleaved cell's blend keeps its Cand
        assert all(v for n, nones in planar_launches for p, v in nones.items() if not (p == 'RH' and n == 'cell_gates_fwd_planar_k'))
    else:
        assert not any(nones[k] for n, nones in em.nones for k in nones if k != 'RH')


@pytest.mark.parametrize('optional', [True, False])
@pytest.mark.parametrize('K', [2, 3])
def test_live_state_planes_do_not_depend_on_the_observed_length(monkeypatch, K, optional):
    """The twin watches the state-sized tensors it is handed; at every blend launch it counts those still alive.  Under no_grad the largest count
    is the same for 3 and for 9 observed steps (on the autograd node it grows with every cell: everything is saved)."""
    most = {}
    for T in (3, 9):
        op, Tc, schedule, outputs, ext, stacks, numel = _problem(K, 1, T=T)
        em = WatchfulTwin(optional, numel)
        monkeypatch.setattr(ops, '_kernels', em)
        with torch.no_grad():
            out = ops.stc_cell_graph(op, Tc, K, schedule, outputs, ext, stacks)
        assert len(em.alive_at_blend) == len(schedule)
        most[T] = max(em.alive_at_blend)
        del out, em
        gc.collect()
    print(most)
    assert most[3] == most[9], most


def test_routing_between_the_autograd_node_and_the_forward_only_route(monkeypatch):
    op, Tc, schedule, outputs, ext, stacks, numel = _problem(2, 1)
    em = WatchfulTwin(True, numel)
    monkeypatch.setattr(ops, '_kernels', em)
    routed = []
    real = ops._forward_only
    monkeypatch.setattr(ops, '_forward_only', lambda *a, **k: (routed.append(1), real(*a, **k))[1])
    leaf = [tuple(p.clone().requires_grad_() for p in st) for st in stacks]
    out = ops.stc_cell_graph(op, Tc, 2, schedule, outputs, ext, leaf)                  # a parameter wants a gradient, grad mode on: the node
    assert out.requires_grad and not routed and not any(v for _, nones in em.nones for k, v in nones.items() if k != 'RH')
    out.sum().backward()
    assert all(p.grad is not None for st in leaf for p in st)
    del em.nones[:]
    with torch.no_grad():                                                              # no_grad: the route, whatever the parameters want
        quiet = ops.stc_cell_graph(op, Tc, 2, schedule, outputs, ext, leaf)
    assert len(routed) == 1 and not quiet.requires_grad and torch.equal(quiet, out.detach())
    assert em.nones and all(all(nones.values()) for n, nones in em.nones)
    del em.nones[:]
    frozen = ops.stc_cell_graph(op, Tc, 2, schedule, outputs, ext, stacks)             # grad mode on, everything frozen: the route
    assert len(routed) == 2 and not frozen.requires_grad and torch.equal(frozen, quiet)
    assert em.nones and all(all(nones.values()) for n, nones in em.nones)
