"""Helpers of tests/test_autograd_contract.py: the case table of every ``torch.autograd.Function`` of ``stc_hip.ops`` / ``stc_hip.small`` and the
checkers of the autograd contract ("Autograd contract").

A ``Case`` names an operator, the Function classes it reaches, and

    make(dev, seed) -> {name: value}     named inputs, built on the CPU from ``seed`` and moved to ``dev``; ``diff`` lists the tensor inputs a caller
                                         may want a gradient for, ``params`` the subset that P3 freezes (weights, biases, learned graphs)
    call(x)         -> tuple of outputs  the operator on those inputs
    reference(x)    -> tuple of outputs  the same expression from oracle/stc_oracle.py or plain torch; run in float64 (the reference) and in
                                         float32 (its own noise), differentiated by torch autograd
    tol                                  which of the project's existing bounds applies (``bound``): no new numbers
    setup(mp, dev)  -> verify()          switches and spies; ``verify`` asserts the route / form taken after a call

The properties P1..P11 are functions ``pN(case, dev, ...)`` that raise ``ContractFailure(property, message)``; the three closed exception tables are
``REFUSALS`` (P2: who may raise instead of returning a gradient), ``NOT_BITWISE_WHEN_FROZEN`` (P3) and ``NOT_APPLICABLE`` (property, case) -> reason.
Everything compared "bitwise" is compared with ``torch.equal``.
"""
import dataclasses

import torch

import STC_GNN as M
from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, ops, small
from stc_hip.graph import csr_operand, dense_operand
from tests.conftest import rel_err
from tests.test_bf16_kernels import BTOL
from tests.test_hip_kernels import TOL
from tests import test_module_parity as parity
from tests.test_small_cell import TOL as SMALL_LEARNED      # the few-category executor's learned-graph gradients at order 2
from tests.test_module_parity import FWD, GENERAL_OUTPUTS, GENERAL_SCHEDULE, GPU, GRAD

N_GRID = (4, 5)
N, H16 = 20, 16
GRAPH = CsrGraph.queen_grid(*N_GRID, normalize=True)
NOISE_FACTOR = 10.0          # the margin of tests/test_scale_sweep.py over the reference's own float32 noise
SMALL_LEARNED_K3 = 2e-5      # tests/test_small_dense_order3.py: max(2e-5, 10 x noise) at order 3
FUSION_GRAD = 2e-5           # test_mixed_fusion's gradient bound (tests/test_hip_kernels.py)
MGP_NOISE = 3.0              # tests/test_mgp_front.py: max(1e-5 / 2e-5, 3 x the reference's float32 noise)


class ContractFailure(AssertionError):
    def __init__(self, prop, msg):
        super().__init__(f'{prop}: {msg}')
        self.prop = prop


# ---- the three exception tables -----------------------------------------------------------------------------------------------------------------
#: P2: (operator[route], argument) pairs that may refuse -- raise ValueError / StcError / RuntimeError naming the argument -- instead of returning a
#: gradient.  Closed: anything else must produce the gradient.
REFUSALS = {
    ('stc_cell_graph[general]', 'ext'): 'the executor forms no gradient for external tensors (only states owed to cells); out of scope to build',
    ('stc_cell_graph[general]', 'Tc'): 'the general executor runs fixed graphs only: its cell kernels leave no operands for dT_c',
    ('stc_cell_graph[general]', 'fwd_val'): 'the general executor runs fixed graphs only: no product with the aggregated slabs is kept for dGs',
    ('stc_small_graph', 'ext'): 'the few-category executor writes state gradients for cells only, none for external tensors',
    ('mgp_front', 'X'): 'the data window is data: stc_mgp_uv_bwd_f32 forms dWu / dWv only',
    ('bdg_dif[bf16]', 'Tc'): 'the bf16 node kernels have no dT_c output (fixed graphs only, BASELINE configuration 5)',
    ('bdg_dif[bf16]', 'fwd_val'): 'no bf16 sampled product for the graph values (fixed graphs only)',
}

#: P3: (case id, gradient) pairs compared within the case's tolerance instead of bitwise when something is frozen, because fewer wanted gradients
#: legitimately select another kernel instantiation.  ``'*'``: every gradient of the case.
NOT_BITWISE_WHEN_FROZEN = {}
#: ... and, where only some frozen inputs cause it, which: with none of them frozen the pair is held bitwise like any other
NOT_BITWISE_CAUSES = {}

#: (property, case id) or (property, case id, input) -> why the property cannot apply.
NOT_APPLICABLE = {}

#: Functions of ``stc_hip`` without a case here -> the test file that holds their contract properties instead (no P1..P11 cases yet).  Closed: the
#: coverage walk of tests/test_autograd_contract.py goes over every module of the package and takes nothing else without a case.
CONTRACT_ELSEWHERE = {
    'stc_hip.fusion._MixedFusionLR': 'tests/test_mixed_fusion_lr.py',
    'stc_hip.loss._ComboLossFused': 'tests/test_combo_loss.py',
    'stc_hip.dist._AllReduceSum': 'tests/test_dist_gloo.py',      # a collective, no kernel: its gradient is held by the two-rank learned-graph tests
}


def _loose(case_id, names, reason):
    for n in names:
        NOT_BITWISE_WHEN_FROZEN[(case_id, n)] = reason


# ---- small helpers ----------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rnd(g, *shape):
    return torch.randn(*shape, generator=g)


def _w(g, rows, cols):
    return _rnd(g, rows, cols) / rows ** 0.5


def _to(d, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def _spatial(x, dev):
    """The spatial operand of a case: the dense learned ``Gs`` where the inputs hold one, else the fixed grid graph -- with ``val`` (a copy of its
    forward values, a leaf) in place of its own values where the case wants to ask for their gradient."""
    if 'Gs' in x:
        return dense_operand(x['Gs'])
    op = csr_operand(x.get('graph', GRAPH), torch.device(dev))
    return dataclasses.replace(op, fwd_val=x['val']) if 'val' in x else op


def _dense_gs(x):
    return x['Gs'] if 'Gs' in x else x.get('graph', GRAPH).to_dense().to(next(v for v in x.values() if isinstance(v, torch.Tensor) and v.is_floating_point()).dtype)


def _device_of(x):
    return next(v for v in x.values() if isinstance(v, torch.Tensor)).device


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _span(t):
    """[first byte, one past the last byte) that ``t`` can touch."""
    if t.numel() == 0:
        return (t.data_ptr(), t.data_ptr())
    last = sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    return (t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size())


def overlap(a, b):
    (a0, a1), (b0, b1) = _span(a), _span(b)
    return a0 < b1 and b0 < a1


def _detached(v):
    if isinstance(v, torch.Tensor):
        return v.detach()
    if isinstance(v, (list, tuple)):
        return type(v)(_detached(t) for t in v)
    return v


class KernelTwin(EmulatedKernels):
    """The CPU twin as a kernel sees its operands: memory, without autograd flags.  ``torch.matmul`` on the CPU picks its algorithm by whether an
    operand ``requires_grad`` (also under ``no_grad``: whether to fold a batched product into one matrix product), so the plain twin's sums
    differ in the last bit between a run with a weight frozen and one without -- an artefact of the stand-in that no HIP kernel can have, and
    that would drown the bitwise properties."""

    _called = None                                         # a list: the names of the kernels called, in order

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if callable(v) and not name.startswith('_') and not isinstance(v, type):
            def kernel(*a, **kw):
                log = object.__getattribute__(self, '_called')
                if log is not None:
                    log.append(name)
                return v(*_detached(a), **{k: _detached(t) for k, t in kw.items()})
            return kernel
        return v


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, id, op, functions, make, call, reference, diff, params=(), tol='single', argument_of=None, refusal_key=None, gpu_only=None,
                 setup=None, noise_only=(), noise_floor=None, layouts=None, out_tol=None):
        self.id, self.op, self.functions, self.make, self.call, self.reference = id, op, tuple(functions), make, call, reference
        self.diff, self.params, self.tol = tuple(diff), tuple(params), tol
        self.argument_of = argument_of or {}          # input name -> the operator's argument it is (where the names differ)
        self.refusal_key = refusal_key or op
        self.gpu_only = gpu_only                       # reason why the CPU twin cannot run it
        self.setup = setup or (lambda mp, dev: (lambda: None))
        self.noise_only = frozenset(noise_only)        # gradients without a bound in the project: NOISE_FACTOR x the reference's float32 noise
        self.noise_floor = noise_floor or {}           # gradient -> (flat bound, factor): max(flat, factor x noise), as the operator's own test has it
        self.layouts = self.diff if layouts is None else tuple(layouts)      # the inputs P8 hands over in other layouts
        self.out_tol = out_tol
        self.p11_on = None                             # what requires grad in P11's grad-mode run (default: everything differentiable)

    def argument(self, name):
        return self.argument_of.get(name, name)

    def refused(self, name):
        return (self.refusal_key, self.argument(name)) in REFUSALS

    @property
    def on_all(self):
        return tuple(n for n in self.diff if not self.refused(n))

    def bound(self, dev, name, kind, noise):
        """The bound on max |got - want| / max |want| of output or gradient ``name`` (``kind``: 'out' / 'grad'), from the project's own numbers."""
        if kind == 'grad' and name in self.noise_only:
            return NOISE_FACTOR * noise
        if kind == 'grad' and name in self.noise_floor:
            flat, factor = self.noise_floor[name]
            return max(flat, factor * noise)
        if kind == 'out' and self.out_tol is not None:
            return max(self.out_tol[0], self.out_tol[1] * noise)
        if self.tol == 'bf16':
            return BTOL
        if self.tol == 'single':
            return TOL
        assert self.tol == 'cell'
        return GPU if dev == 'cuda' else (FWD if kind == 'out' else GRAD)


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))
    return CASES[-1]


def _spy(mp, obj, name, log, pick=lambda out, a, kw: out):
    real = getattr(obj, name)
    def wrapped(*a, **kw):
        out = real(*a, **kw)
        log.append(pick(out, a, kw))
        return out
    mp.setattr(obj, name, wrapped)


# -- cheby_dense
def _cheby():
    n, K = 5, 3
    make = lambda dev, seed: _to(dict(G=torch.softmax(_rnd(_gen(seed), n, n), -1)), dev)
    case('cheby_dense-n5-K3', 'cheby_dense', [ops._ChebyDense], make, lambda x: (ops.cheby_dense(x['G'], K),),
         lambda x: (torch.stack(O.cheby_poly(x['G'], K)[:K]),), diff=['G'], params=['G'])


# -- bdg_dif
def _bdg(C, L, B, learned, K=2, Ho=16, bf16=False):
    pad = -L % 4
    cid = f'bdg_dif-{"bf16-" if bf16 else ""}{"learned" if learned else "fixed"}-C{C}-L{L}-K{K}'

    def make(dev, seed):
        g = _gen(seed)
        d = dict(X=_rnd(g, B, N, C, L), W=_w(g, K * K * L, Ho), b=0.1 * _rnd(g, Ho), Gc=torch.softmax(_rnd(g, C, C), -1))
        if learned:
            d['Gs'] = torch.softmax(_rnd(g, N, N), -1)
        if bf16:
            d['X'] = d['X'].to(torch.bfloat16)
        d = _to(d, dev)
        if bf16:
            d['val'] = csr_operand(GRAPH, torch.device(dev)).fwd_val.detach().clone()
        return d

    def call(x):
        X = x['X'] if not pad else torch.cat([x['X'], x['X'].new_zeros(*x['X'].shape[:-1], pad)], -1)      # rows padded to 16 bytes by the caller
        return (ops.bdg_dif(X, _spatial(x, X.device), ops.cheby_dense(x['Gc'], K), x['W'], x['b'], K, pad),)

    def reference(x):
        return (O.bdg_dif(x['X'], _dense_gs(x), x['Gc'], x['W'], x['b'], K, K),)

    def setup(mp, dev):
        packs = []
        _spy(mp, ops, '_node_pack', packs)
        def verify():
            want = 0 if (C > 16 or (L + pad) not in (20, 32) or bf16) else (16 // C if (B * N) % (16 // C) == 0 else 1)
            assert packs and set(packs) == {want}, (cid, packs, want)
        return verify

    graphs = ('Gs', 'Gc') if learned else ()
    c = case(cid, 'bdg_dif', [ops._BdgDif] + ([ops._ChebyDense] if learned else []), make, call, reference,
             diff=('X', 'W', 'b') + graphs + (('Gc', 'val') if bf16 else ()), params=('W', 'b') + graphs, tol='bf16' if bf16 else 'single',
             argument_of=dict(Gc='Tc', Gs='fwd_val', val='fwd_val'), refusal_key='bdg_dif[bf16]' if bf16 else 'bdg_dif', setup=setup)
    if learned and not (C <= 16 and (L + pad) in (20, 32)):
        _loose(cid, ('X', 'W', 'b', 'Gs'), 'Gc frozen: stc_bdg_node_bwd runs without its dTc output, another instantiation of the kernel')
    return c


# -- gate math, concat, head
def _gru_gates(cin, pad, C=5):
    def make(dev, seed):
        g = _gen(seed)
        return _to(dict(G=_rnd(g, 2, N, C, 2 * H16), Xt=_rnd(g, 2, N, C, cin), H=torch.tanh(_rnd(g, 2, N, C, H16))), dev)

    def reference(x):
        U, R = torch.sigmoid(x['G'][..., :H16]), torch.sigmoid(x['G'][..., H16:])
        return U, torch.cat([x['Xt'], R * x['H'], x['H'].new_zeros(*x['H'].shape[:-1], pad)], -1)
    case(f'gru_gates-cin{cin}-pad{pad}', 'gru_gates', [ops._GruGates], make, lambda x: tuple(ops.gru_gates(x['G'], x['Xt'], x['H'], pad)), reference,
         diff=('G', 'Xt', 'H'), noise_only=('G', 'Xt', 'H'))


def _gru_blend(C=5):
    def make(dev, seed):
        g = _gen(seed)
        return _to(dict(Cpre=_rnd(g, 2, N, C, H16), U=torch.sigmoid(_rnd(g, 2, N, C, H16)), H=torch.tanh(_rnd(g, 2, N, C, H16))), dev)
    case('gru_blend', 'gru_blend', [ops._GruBlend], make, lambda x: (ops.gru_blend(x['Cpre'], x['U'], x['H']),),
         lambda x: ((1 - x['U']) * x['H'] + x['U'] * torch.tanh(x['Cpre']),), diff=('Cpre', 'U', 'H'), noise_only=('Cpre', 'U', 'H'))


def _concat2(C=5, pad=3):
    def make(dev, seed):
        g = _gen(seed)
        return _to(dict(A=_rnd(g, 2, N, C, 1), Bm=_rnd(g, 2, N, C, H16)), dev)
    case('concat2-pad3', 'concat2', [ops._Concat2], make, lambda x: (ops.concat2(x['A'], x['Bm'], pad),),
         lambda x: (torch.cat([x['A'], x['Bm'], x['A'].new_zeros(*x['A'].shape[:-1], pad)], -1),), diff=('A', 'Bm'))


def _head(C=5):
    def make(dev, seed):
        g = _gen(seed)
        return _to(dict(H=torch.tanh(_rnd(g, 2, 2, N, C, H16)), w=_rnd(g, H16) / 4, b=0.1 * _rnd(g, 1)), dev)
    case('head-h16', 'head', [ops._Head], make, lambda x: (ops.head(x['H'], x['w'], x['b']),),
         lambda x: (torch.sigmoid(x['H'] @ x['w'] + x['b']),), diff=('H', 'w', 'b'), params=('w', 'b'))


# -- one cell
def _cell_inputs(g, C, K, cin, B=2):
    rows = K * K * (cin + H16)
    return dict(Xt=_rnd(g, B, N, C, cin), H=torch.tanh(_rnd(g, B, N, C, H16)), Wg=_w(g, rows, 2 * H16), bg=0.1 * _rnd(g, 2 * H16),
                Wc=_w(g, rows, H16), bc=0.1 * _rnd(g, H16), Gc=torch.softmax(_rnd(g, C, C), -1))


def _stc_cell(C, K, cin, learned):
    cid = f'stc_cell-{"learned" if learned else "fixed"}-C{C}-K{K}-cin{cin}'
    B = 2

    def make(dev, seed):
        g = _gen(seed)
        d = _cell_inputs(g, C, K, cin, B)
        if learned:
            d['Gs'] = torch.softmax(_rnd(g, N, N), -1)
        return _to(d, dev)

    def call(x):
        return (ops.stc_cell(x['Xt'], x['H'], _spatial(x, x['H'].device), ops.cheby_dense(x['Gc'], K), x['Wg'], x['bg'], x['Wc'], x['bc'], K),)

    def reference(x):
        return (O.stc_cell(_dense_gs(x), x['Gc'], x['Xt'], x['H'], x['Wg'], x['bg'], x['Wc'], x['bc'], K, K),)

    def setup(mp, dev):
        packs = []
        _spy(mp, ops, '_cell_pack', packs)
        def verify():
            L = cin + H16 + (-(cin + H16)) % 4
            fused = ops.kernels().cell_fused_supported       # (the CPU twin fuses at any C; the library at C in {16, 32, 64})
            want = 1 if fused(K, K, C, L, H16) else (16 // C if (16 % C == 0 and (B * N) % (16 // C) == 0 and fused(K, K, 16, L, H16)) else 0)
            assert packs and set(packs) == {want}, (cid, packs, want)
            if dev == 'cuda':                                # fused (C = 32), packed (C = 8: two nodes per tile), composed (C = 5)
                assert want == {32: 1, 8: 2, 5: 0}[C], (cid, want)
        return verify

    graphs = ('Gs', 'Gc') if learned else ()
    case(cid, 'stc_cell', [ops._StcCell] + ([ops._ChebyDense] if learned else []), make, call, reference,
         diff=('Xt', 'H', 'Wg', 'bg', 'Wc', 'bc') + graphs, params=('Wg', 'bg', 'Wc', 'bc') + graphs, tol='cell',
         argument_of=dict(Gc='Tc', Gs='fwd_val'), setup=setup,
         noise_floor={n: (GPU, NOISE_FACTOR) for n in graphs} if (learned and K == 3) else None)
    if learned:
        _loose(cid, ('*',), '_StcCell.backward picks the fused prologue kernels (pack > 0) only when neither dTc nor d fwd_val is wanted; '
                            'with a graph gradient wanted it runs the composed sequence, and stc_bdg_node_bwd with or without dTc')


# -- a schedule of cells
def _schedule_inputs(g, C, K, B=2, N=N):
    wide, narrow = K * K * (H16 + H16), K * K * (1 + H16)
    d = dict(x0=torch.rand(B, N, C, 1, generator=g), xw=torch.rand(B, N, C, H16, generator=g), h0=torch.rand(B, N, C, H16, generator=g),
             Gc=torch.softmax(_rnd(g, C, C), -1))
    for s, rows in ((0, wide), (1, narrow)):
        d.update({f's{s}.Wg': _w(g, rows, 2 * H16), f's{s}.bg': 0.1 * _rnd(g, 2 * H16), f's{s}.Wc': _w(g, rows, H16), f's{s}.bc': 0.1 * _rnd(g, H16)})
    return d


_SET_NAMES = tuple(f's{s}.{p}' for s in (0, 1) for p in ('Wg', 'bg', 'Wc', 'bc'))


def _schedule_reference(K):
    def reference(x):
        ext, state = [x['x0'], x['xw'], x.get('h0', None)], []
        if ext[2] is None:
            ext[2] = torch.zeros_like(x['xw'])
        Gs = _dense_gs(x)
        for s_id, xs, hs in GENERAL_SCHEDULE:
            src = lambda t: ext[t[1]] if t[0] == 'ext' else state[t[1]]
            state.append(O.stc_cell(Gs, x['Gc'], src(xs), src(hs), *(x[f's{s_id}.{p}'] for p in ('Wg', 'bg', 'Wc', 'bc')), K, K))
        return (torch.stack([state[j] for j in GENERAL_OUTPUTS]),)
    return reference


def _schedule_call(K):
    def call(x):
        dev = x['x0'].device
        h0 = x['h0'] if 'h0' in x else ops.zero_state(x['xw'], x['xw'].shape)
        stacks = [tuple(x[f's{s}.{p}'] for p in ('Wg', 'bg', 'Wc', 'bc')) for s in (0, 1)]
        return (ops.stc_cell_graph(_spatial(x, dev), ops.cheby_dense(x['Gc'], K), K, GENERAL_SCHEDULE, GENERAL_OUTPUTS, [x['x0'], x['xw'], h0], stacks),)
    return call


#: P3, module cases: gradient -> why it is not bitwise when something is frozen (the frozen input that causes it is named in the reason)
MODULE_NOT_BITWISE = {
    'STCGNN-dense-learned-C5': {
        '*': (('p:mix_graph_pair.params_C.Wu', 'p:mix_graph_pair.params_C.Wv'),
              'mix_graph_pair.params_C.Wu or .Wv frozen (alone, or in an all-but-one run): with X_seq differentiable MGP_Gen runs its torch expression, '
              'and torch.matmul(X.transpose(2, 3), W) on the strided window folds the batch into one matrix product only when W does not require '
              'grad -- another library GEMM, whose last bits differ already in the FORWARD (measured on the GPU: the prediction itself changes, '
              'and with it every gradient; on the CPU only dX_seq moves).  Torch operations, no kernel of this project.  Every run that '
              'freezes neither of the two is held bitwise')},
}
WIDE_CELLS = [j for j, (s, _, _) in enumerate(GENERAL_SCHEDULE) if s == 0]


RING2_GRID = (4, 8)          # the smallest queen grid with a two-ring plan: one 4 x 8 tile (graph.GRID_TILE)


def _cell_graph(form, K=2, C=32, zero=False, bf16=False, switches=None, ring2=False):
    cid = f'stc_cell_graph-{form}-C{C}-K{K}' + ('-zero_state' if zero else '') + ('-bf16' if bf16 else '') + ('-ring2' if ring2 else '')
    graph = CsrGraph.queen_grid(*RING2_GRID, normalize=True) if ring2 else GRAPH

    def make(dev, seed):
        d = _schedule_inputs(_gen(seed), C, K, N=graph.n)
        d['graph'] = graph
        if zero:
            del d['h0']
        if bf16:
            for n in ('x0', 'xw', 'h0'):
                d[n] = d[n].to(torch.bfloat16)
        d = _to(d, dev)
        d['val'] = csr_operand(graph, torch.device(dev)).fwd_val.detach().clone()
        return d

    def setup(mp, dev):
        mp.setattr(ops, '_SMALL', False)
        launched = []
        if zero and dev == 'cuda':                           # (the twin has no first-step forms: it builds the plane of zeros)
            k = ops.kernels()
            real_first = k._launch
            mp.setattr(k, '_launch', lambda name, *a, **kw: (launched.append(name), real_first(name, *a, **kw))[1])
        if ring2:                                            # the names of the launches: the library's on the GPU, the twin's methods on the CPU
            k = ops.kernels()
            op = csr_operand(graph, torch.device(dev))
            assert op.bwd_ring2 is not None and op.fwd_ring2 is not None and k.ring2_fits(2, graph.n, C, H16)
            if dev == 'cuda':
                real_launch = k._launch
                mp.setattr(k, '_launch', lambda name, *a, **kw: (launched.append(name), real_launch(name, *a, **kw))[1])
            else:
                mp.setattr(k, '_called', launched)
        for name, value in (switches or {}).items():
            mp.setattr(ops, name, value)
        if form == 'PLANAR' and C == 32:         # the two-launch backward is what C = 64 runs: force it, as test_two_launch_cell_backward_option does
            mp.setattr(type(ops.kernels()), 'cell_bwd_planar_supported', lambda self, Cc, hh, *w: False)
        forms, small, bwd_expected = [], [], [False]
        real_bwd = ops._StcCellGraph.backward
        mp.setattr(ops._StcCellGraph, 'backward', staticmethod(lambda ctx, *g: (bwd_expected.__setitem__(0, True), real_bwd(ctx, *g))[1]))
        _spy(mp, ops, '_cell_forms', forms)
        _spy(mp, ops, 'stc_small_graph', small)
        def verify():
            assert forms and not small, (cid, 'the general executor was not taken')
            for fs in forms:
                assert {fs[j].name for j in WIDE_CELLS} == {form}, (cid, [f.name for f in fs])
            if zero and dev == 'cuda':                       # cell 0 sits on the zero state: its first-step forms ran, forward and backward
                assert 'stc_cell_gates_fwd_first_f32' in launched and (not bwd_expected[0] or 'stc_cell_bwd_first_f32' in launched), (cid, sorted(set(launched)))
            if ring2:
                assert any(n.startswith(('stc_ring2_', 'ring2_')) and not n.endswith('fits') for n in launched), (cid, sorted(set(launched)))
        return verify

    ext = ('x0', 'xw') + (() if zero else ('h0',))
    case(cid, 'stc_cell_graph', [ops._StcCellGraph], make, _schedule_call(K), _schedule_reference(K),
         diff=_SET_NAMES + ext + ('Gc', 'val'), params=_SET_NAMES, tol='bf16' if bf16 else 'cell',
         argument_of=dict(x0='ext', xw='ext', h0='ext', Gc='Tc', val='fwd_val'), refusal_key='stc_cell_graph[general]', setup=setup,
         gpu_only=None)


def _small_graph(K, learned, C=5):
    cid = f'stc_small_graph-{"learned" if learned else "fixed"}-C{C}-K{K}'

    def make(dev, seed):
        g = _gen(seed)
        d = _schedule_inputs(g, C, K)
        if learned:
            d['Gs'] = torch.softmax(_rnd(g, N, N), -1)
        return _to(d, dev)

    def setup(mp, dev):
        small = []
        _spy(mp, ops, 'stc_small_graph', small)
        def verify():
            assert small, (cid, 'the few-category executor was not taken')
        return verify

    graphs = ('Gs', 'Gc') if learned else ()
    flat = SMALL_LEARNED_K3 if K == 3 else SMALL_LEARNED
    case(cid, 'stc_small_graph', [small._StcSmallGraph] + ([ops._ChebyDense] if learned else []), make, _schedule_call(K), _schedule_reference(K),
         diff=_SET_NAMES + ('x0', 'xw', 'h0') + graphs, params=_SET_NAMES + graphs, tol='cell',
         argument_of=dict(x0='ext', xw='ext', h0='ext', Gc='Tc', Gs='fwd_val'), refusal_key='stc_small_graph', setup=setup,
         noise_floor={n: (flat, NOISE_FACTOR if K == 3 else 0.0) for n in graphs},
         gpu_only='the CPU twin has no dense order-3 few-category kernels (small_dense_order3)' if (learned and K == 3) else None)


# -- learned graph generator (GPU only: the twin has no such kernels)
def _mixed_fusion(n=10):
    D = n * n

    def make(dev, seed):
        g = _gen(seed)
        return _to(dict(A=torch.rand(n, n, generator=g), P=torch.softmax(_rnd(g, n, n), -1), WA=_rnd(g, D, D) / D ** 0.5, bA=0.1 * _rnd(g, D),
                        WP=_rnd(g, D, D) / D ** 0.5, bP=0.1 * _rnd(g, D)), dev)

    def call(x):
        args = tuple(x[n_] for n_ in ('A', 'P', 'WA', 'bA', 'WP', 'bP'))
        assert ops.mixed_fusion_supported(*args)
        return (ops.mixed_fusion(*args),)

    def reference(x):
        a = torch.sigmoid(x['WA'] @ x['A'].reshape(D) + x['bA'] + x['WP'] @ x['P'].reshape(D) + x['bP']).reshape(n, n)
        return (a * x['A'] + (1 - a) * x['P'],)
    names = ('A', 'P', 'WA', 'bA', 'WP', 'bP')
    case(f'mixed_fusion-n{n}', 'mixed_fusion', [ops._MixedFusion], make, call, reference, diff=names, params=names[2:],
         noise_floor={n_: (FUSION_GRAD, 0.0) for n_ in names}, gpu_only='the CPU twin has no mixed-fusion kernels', layouts=('A', 'P'))


def _mgp_front(rows_axis, B=2, T=3, C=5, h=16):
    F, R = (C, N) if rows_axis == 2 else (N, C)
    cid = f'mgp_front-rows_axis{rows_axis}'

    def make(dev, seed):
        g = _gen(seed)
        return _to(dict(X=(torch.rand(B, T, N, C, generator=g) < 0.3).float(), Wu=_rnd(g, F, h) * (2.0 / (F + h)) ** 0.5,
                        Wv=_rnd(g, F, h) * (2.0 / (F + h)) ** 0.5), dev)

    def reference(x):
        X = x['X'].transpose(2, 3) if rows_axis == 3 else x['X']
        U, V = torch.tanh(3 * torch.matmul(X, x['Wu'])), torch.tanh(3 * torch.matmul(X, x['Wv']))
        P = torch.einsum('btnh,btmh->nm', U, V)
        return (torch.softmax(torch.relu(P - P.t()), dim=-1),)
    case(cid, 'mgp_front', [ops._MgpUV, ops._MgpSoftmax], make, lambda x: (ops.mgp_front(x['X'], x['Wu'], x['Wv'], rows_axis, 3.0),), reference,
         diff=('X', 'Wu', 'Wv'), params=('Wu', 'Wv'), noise_floor={n_: (2e-5, MGP_NOISE) for n_ in ('Wu', 'Wv')}, out_tol=(1e-5, MGP_NOISE),
         gpu_only='the CPU twin has no MGP front kernels')


def _mgp_uv(rows_axis=2, B=2, T=3, C=5, h=16):
    """``_MgpUV`` by itself, both outputs returned (under ``mgp_front`` the softmax node sits in front of it): U, V in (rows, slices, hidden)
    layout; the data window is a constant here -- the Function is internal, ``mgp_front`` is where a differentiable X is refused."""
    F, R = (C, N) if rows_axis == 2 else (N, C)

    def make(dev, seed):
        g = _gen(seed)
        return _to(dict(X=(torch.rand(B, T, N, C, generator=g) < 0.3).float(), Wu=_rnd(g, F, h) * (2.0 / (F + h)) ** 0.5,
                        Wv=_rnd(g, F, h) * (2.0 / (F + h)) ** 0.5), dev)

    def reference(x):
        X = x['X'].transpose(2, 3) if rows_axis == 3 else x['X']
        rows = lambda t: t.permute(2, 0, 1, 3).reshape(R, B * T, h)
        return rows(torch.tanh(3 * torch.matmul(X, x['Wu']))), rows(torch.tanh(3 * torch.matmul(X, x['Wv'])))
    case(f'mgp_uv-rows_axis{rows_axis}', 'mgp_uv', [ops._MgpUV], make, lambda x: tuple(ops._MgpUV.apply(x['X'], x['Wu'], x['Wv'], rows_axis, 3.0)), reference,
         diff=('Wu', 'Wv'), params=('Wu', 'Wv'), noise_floor={n_: (2e-5, MGP_NOISE) for n_ in ('Wu', 'Wv')}, out_tol=(1e-5, MGP_NOISE),
         gpu_only='the CPU twin has no MGP front kernels')


# -- the module
def _module(mode, C, K=2, T=2, horizon=2, B=2):
    cid = f'STCGNN-{mode}-C{C}'
    learned = mode == 'dense-learned'

    def make(dev, seed):
        torch.manual_seed(seed)
        model = M.STCGNN(N, C, K, K, 1, H16, 1, horizon, graph_mode=mode)
        g = _gen(seed)
        d = dict(X_seq=(torch.rand(B, T, N, C, generator=g) < 0.3).float() + 0.1 * torch.rand(B, T, N, C, generator=g),
                 Ac=torch.softmax(_rnd(g, C, C), -1) if not learned else torch.rand(C, C, generator=g))
        if learned:
            d['As'] = torch.rand(N, N, generator=g)
        d.update({'p:' + n_: p.detach().clone() for n_, p in model.named_parameters()})
        d = _to(d, dev)
        d['model'] = model.to(dev)
        return d

    def call(x):
        params = {n_[2:]: v for n_, v in x.items() if n_.startswith('p:')}
        As = x['As'] if learned else GRAPH
        return (torch.func.functional_call(x['model'], params, kwargs=dict(X_seq=x['X_seq'], As=As, Ac=x['Ac'])),)

    def reference(x):
        sd = {n_[2:]: v for n_, v in x.items() if n_.startswith('p:')}
        if learned:
            return (O.stcgnn_forward(x['X_seq'], x['As'], x['Ac'], sd, K, K, H16, 1, horizon),)
        return (O.encdec_forward(x['X_seq'], GRAPH.to_dense().to(x['X_seq'].dtype), x['Ac'], sd, K, K, H16, 1, horizon),)

    def setup(mp, dev):
        graph_calls, cell_calls = [], []
        _spy(mp, ops, 'stc_cell_graph', graph_calls)
        _spy(mp, ops, 'stc_cell', cell_calls)
        def verify():                                        # the path taken, recorded and returned -- not forced (``module_path``: what is expected)
            assert bool(graph_calls) != bool(cell_calls), (cid, len(graph_calls), len(cell_calls))
            return 'cell-graph' if graph_calls else 'per-cell'
        return verify

    probe = M.STCGNN(N, C, K, K, 1, H16, 1, horizon, graph_mode=mode)
    pnames = tuple('p:' + n_ for n_, _ in probe.named_parameters())
    case(cid, 'STCGNN', [ops._StcCell, ops._Head, ops._ChebyDense], make, call, reference, diff=('X_seq', 'Ac') + (('As',) if learned else ()) + pnames,
         params=pnames, tol='cell', setup=setup, layouts=('X_seq', 'Ac') + (('As',) if learned else ()),
         # parameters: GPU / GRAD / FWD of tests/test_module_parity.py on fixed graphs, max(2e-5, 10 x noise) with learned graphs (as that file's
         # learned-graph module tests); the data inputs, which no test differentiated before: 10 x the reference's noise
         noise_only=('X_seq', 'Ac', 'As'), noise_floor={n_: (2e-5, NOISE_FACTOR) for n_ in pnames} if learned else None)
    CASES[-1].p11_on = pnames                                 # (with X_seq or Ac differentiable the module takes its per-cell path: other kernels)
    CASES[-1].C = C
    for n_, (causes, why) in MODULE_NOT_BITWISE.get(cid, {}).items():
        _loose(cid, (n_,), why)
        NOT_BITWISE_CAUSES[(cid, n_)] = frozenset(causes)


def module_path(c, on):
    """The path ``STCGNN.forward`` is expected to take with ``on`` requiring grad: one node per cell when X_seq is differentiable
    (``_run_cell_graph`` returns None), or when the category graph is on shapes outside the few-category executor (the general executor runs
    fixed graphs only); else the cell graph."""
    return 'per-cell' if ('X_seq' in on or (c.C > 16 and 'Ac' in on)) else 'cell-graph'


_cheby()
for _C, _L, _B in ((5, 17, 3), (32, 32, 2), (3, 5, 2)):
    for _learned in (False, True):
        _bdg(_C, _L, _B, _learned)
_bdg(32, 32, 2, False, bf16=True)
_gru_gates(1, 3)
_gru_gates(16, 0)
_gru_blend()
_concat2()
_head()
for _C, _K, _cin, _learned in ((32, 2, 1, False), (32, 3, 16, False), (8, 2, 16, False), (8, 3, 1, False), (5, 2, 1, False), (5, 3, 16, False),
                               (8, 2, 1, True), (5, 3, 16, True), (32, 2, 16, True)):
    _stc_cell(_C, _K, _cin, _learned)
_cell_graph('PLANAR_ONE_BWD')
_cell_graph('PLANAR_ONE_BWD', zero=True)
_cell_graph('PLANAR')
_cell_graph('PLANAR3', K=3)
_cell_graph('ROWS_POST', switches=dict(_PLANAR=False))
_cell_graph('ROWS_SLABS', switches=dict(_PLANAR=False, _POST_AGG=False))
_cell_graph('PLANAR_ONE_BWD', bf16=True)
_cell_graph('PLANAR_ONE_BWD', ring2=True)
for _K in (2, 3):
    for _learned in (False, True):
        _small_graph(_K, _learned)
_mixed_fusion()
_mgp_front(2)
_mgp_front(3)
_mgp_uv(2)
_module('csr-fixed', 32)
_module('csr-fixed', 5)
_module('dense-learned', 5)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# properties that cannot apply to a case
for _c in CASES:
    if not _c.params:
        NOT_APPLICABLE[('P3', _c.id)] = 'no parameter to freeze: every input is data (P2 runs each alone)'
    if _c.id == 'stc_small_graph-learned-C5-K3':
        _why = ('at order 3 a dense Gs that needs no gradient keeps the general executor in grad mode (small.small_graph_supported), which has no '
                'kernels for C = 5 and says so (StcError; the module asks cell_graph_supported first): every run with Gs frozen is outside the operator')
        NOT_APPLICABLE[('P3', _c.id)] = NOT_APPLICABLE[('P11', _c.id)] = _why
        for _n in _c.diff:
            if _n != 'Gs' and not _c.refused(_n):
                NOT_APPLICABLE[('P2', _c.id, _n)] = _why


# ---- running a case ---------------------------------------------------------------------------------------------------------------------------------------
def leaves(c, inp, on):
    """The inputs with every differentiable tensor replaced by a fresh leaf clone that requires grad iff it is in ``on``."""
    x = dict(inp)
    for n in c.diff:
        x[n] = inp[n].detach().clone().requires_grad_(n in on)
    return x


def cotangents(outs, seed=0):
    g = _gen(1000 + seed)
    # (values that bfloat16 holds exactly: the reference and a bf16 case see the same numbers)
    return [_rnd(g, *o.shape).to(torch.bfloat16).float().to(device=o.device, dtype=o.dtype) for o in outs]


def sync(dev):
    if dev == 'cuda':
        torch.cuda.synchronize()


def grads_of(outs, x, on, gs, **kw):
    need = [o for o in outs if o.requires_grad]
    got = torch.autograd.grad(need, [x[n] for n in on], [g for o, g in zip(outs, gs) if o.requires_grad], allow_unused=True, **kw)
    return dict(zip(on, got))


def run(c, inp, on, gs=None, seed=0, **kw):
    x = leaves(c, inp, on)
    outs = c.call(x)
    gs = cotangents(outs, seed) if gs is None else gs
    return outs, (grads_of(outs, x, on, gs, **kw) if on else {}), x, gs


_REFERENCE = {}


def reference_of(c, seed):
    """(outputs, gradients, output noise, gradient noise) of the float64 reference for ``make(., seed)``, computed once: the float32 run of the same
    expression gives the noise."""
    key = (c.id, seed)
    if key not in _REFERENCE:
        inp = c.make('cpu', seed)
        res = {}
        for dt in (torch.float64, torch.float32):
            x = {k: (v.detach().to(dt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in inp.items()}
            for n in c.diff:
                x[n] = x[n].clone().requires_grad_()
            outs = c.reference(x)
            gs = [g.to(dt) for g in cotangents([o.detach().float() for o in outs])]
            grads = torch.autograd.grad(outs, [x[n] for n in c.diff], gs, allow_unused=True)
            res[dt] = ([o.detach() for o in outs], dict(zip(c.diff, grads)))
        o64, g64 = res[torch.float64]
        o32, g32 = res[torch.float32]
        _REFERENCE[key] = (o64, g64, [rel_err(a, b) for a, b in zip(o32, o64)],
                           {n: (rel_err(g32[n], g64[n]) if g64[n] is not None else 0.0) for n in c.diff})
    return _REFERENCE[key]


def _log(dev, what, got, want, noise, bound):
    """On the GPU, the measured error beside the reference's noise and the bound, in the file where ``test_module_parity._close`` keeps its
    errors -- written by ``_close`` itself (with an infinite bound of its own: the assertion is the caller's)."""
    if dev == 'cuda':
        keep, parity.DEV = parity.DEV, 'cuda'
        try:
            parity._close(got, want, float('inf'), f'{what} (noise {noise:.3e}, bound {bound:.3e} = {bound / noise if noise else float("nan"):.1f} x noise)')
        finally:
            parity.DEV = keep


def check_parity(c, dev, prop, outs, grads, seed=0, outputs=True):
    o64, g64, on_, gn_ = reference_of(c, seed)
    if outputs:
        for i, (o, w) in enumerate(zip(outs, o64)):
            err, bound = rel_err(o.float(), w), c.bound(dev, f'out{i}', 'out', on_[i])
            _log(dev, f'{c.id} out{i}', o.float(), w, on_[i], bound)
            if not err <= bound:
                raise ContractFailure(prop, f'{c.id} output {i}: {err:.3e} > {bound:.1e} (reference noise {on_[i]:.1e})')
    for n, g in grads.items():
        want = g64[n]
        if want is None or float(want.abs().max()) == 0.0:
            continue
        if g is None:
            raise ContractFailure(prop, f'{c.id}: no gradient for {n}, the reference has one (max {float(want.abs().max()):.3g})')
        err, bound = rel_err(g.float(), want), c.bound(dev, n, 'grad', gn_[n])
        _log(dev, f'{c.id} d{n}', g.float(), want, gn_[n], bound)
        if not err <= bound:
            raise ContractFailure(prop, f'{c.id} d{n}: {err:.3e} > {bound:.1e} (reference noise {gn_[n]:.1e})')


def _same(prop, c, what, a, b):
    for n in b:
        if (a[n] is None) != (b[n] is None) or (a[n] is not None and not bits_equal(a[n], b[n])):
            err = 'None' if a[n] is None or b[n] is None else f'rel {rel_err(a[n].float(), b[n].float()):.2e}'
            raise ContractFailure(prop, f'{c.id}: {what}: d{n} differs ({err})')


def _same_outs(prop, c, what, a, b):
    for i, (p, q) in enumerate(zip(a, b)):
        if not bits_equal(p.detach(), q.detach()):
            raise ContractFailure(prop, f'{c.id}: {what}: output {i} differs (rel {rel_err(p.float(), q.float()):.2e})')


# ---- the properties -------------------------------------------------------------------------------------------------------------------------------------------
def p1(c, dev, inp):
    """Parity of the outputs and of every differentiable input's gradient with the float64 reference."""
    outs, grads, _, _ = run(c, inp, c.on_all)
    sync(dev)
    check_parity(c, dev, 'P1', outs, grads)


def p2(c, dev, inp, name):
    """With only ``name`` requiring grad: its gradient matches the reference, or -- for the pairs of ``REFUSALS`` only -- the call or the backward
    raises naming the argument.  Never a None, missing or zero gradient where the reference's is not zero."""
    from stc_hip._lib import StcError
    try:
        outs, grads, _, _ = run(c, inp, (name,))
    except (ValueError, StcError, RuntimeError) as e:
        if not c.refused(name):
            raise ContractFailure('P2', f'{c.id}: {name} alone requiring grad raised {type(e).__name__}: {e}') from e
        if c.argument(name) not in str(e):
            raise ContractFailure('P2', f'{c.id}: the refusal does not name the argument {c.argument(name)!r}: {e}') from e
        return 'refused'
    sync(dev)
    if c.refused(name):
        raise ContractFailure('P2', f'{c.id}: {name} is listed as refused ({c.refusal_key}, {c.argument(name)}) but nothing was raised')
    want = reference_of(c, 0)[1][name]
    if want is not None and float(want.abs().max()) > 0 and (grads[name] is None or not outs[0].requires_grad):
        raise ContractFailure('P2', f'{c.id}: silent: no gradient for {name} (reference max {float(want.abs().max()):.3g})')
    check_parity(c, dev, 'P2', outs, grads, outputs=False)
    return 'gradient'


def _backward_into_leaves(c, inp, on, gs=None, seed=0):
    x = leaves(c, inp, on)
    outs = c.call(x)
    gs = cotangents(outs, seed) if gs is None else gs
    torch.autograd.backward([o for o in outs if o.requires_grad], [g for o, g in zip(outs, gs) if o.requires_grad])
    return outs, x, gs


def p3(c, dev, inp):
    """Freeze each parameter alone, then all parameters but one: a frozen input gets None, every other gradient equals the all-on run bitwise
    (or, for the pairs of ``NOT_BITWISE_WHEN_FROZEN``, within the case's tolerance)."""
    on_all = c.on_all
    params = [p for p in c.params if p in on_all]
    _, xa, _ = _backward_into_leaves(c, inp, on_all)
    full = {n: xa[n].grad for n in on_all}
    sync(dev)
    runs = [[n for n in on_all if n != p] for p in params] + ([[n for n in on_all if n not in params or n == p] for p in params] if len(params) > 1 else [])
    for on in runs:
        outs, x, _ = _backward_into_leaves(c, inp, on)
        sync(dev)
        for n in c.diff:
            g = x[n].grad
            if n not in on:
                if g is not None:
                    raise ContractFailure('P3', f'{c.id}: frozen {n} got a gradient')
                continue
            if full[n] is None and g is None:
                continue
            if g is None or full[n] is None:
                raise ContractFailure('P3', f'{c.id}: d{n} is {"None" if g is None else "set"} with {sorted(set(on_all) - set(on))} frozen')
            key = (c.id, n) if (c.id, n) in NOT_BITWISE_WHEN_FROZEN else (c.id, '*')
            if key in NOT_BITWISE_WHEN_FROZEN and (key not in NOT_BITWISE_CAUSES or NOT_BITWISE_CAUSES[key] & (set(on_all) - set(on))):
                noise = reference_of(c, 0)[3][n]
                err, bound = rel_err(g.float(), full[n].float()), c.bound(dev, n, 'grad', noise)
                if not err <= bound:
                    raise ContractFailure('P3', f'{c.id}: d{n} with {sorted(set(on_all) - set(on))} frozen: {err:.3e} > {bound:.1e}')
            elif not bits_equal(g, full[n]):
                raise ContractFailure('P3', f'{c.id}: d{n} with {sorted(set(on_all) - set(on))} frozen differs from the all-on run '
                                            f'(rel {rel_err(g.float(), full[n].float()):.2e})')


def _tensors(x):
    out = {}
    for k, v in x.items():
        if isinstance(v, torch.Tensor):
            out[k] = v
        elif isinstance(v, torch.nn.Module):
            out.update({f'{k}.{n}': p for n, p in v.state_dict().items()})
    return out


def p4(c, dev, inp, call=None):
    """Nothing handed in is modified: after ``torch.autograd.grad(out, inputs, g)``, g, every input and every parameter keep their bits."""
    x = leaves(c, inp, c.on_all)
    before = {k: v.detach().clone() for k, v in _tensors(x).items()}
    outs = (call or c.call)(x)
    gs = cotangents(outs)
    gs_before = [g.clone() for g in gs]
    grads_of(outs, x, c.on_all, gs)
    sync(dev)
    for i, (g, b) in enumerate(zip(gs, gs_before)):
        if not bits_equal(g, b):
            raise ContractFailure('P4', f'{c.id}: the incoming gradient of output {i} was modified')
    for k, v in _tensors(x).items():
        if not bits_equal(v.detach(), before[k]):
            raise ContractFailure('P4', f'{c.id}: input {k} was modified')


def p5(c, dev, inp, call=None):
    """Two backward passes over one graph (retain_graph=True) give bitwise equal gradients: saved state is not consumed."""
    x = leaves(c, inp, c.on_all)
    outs = (call or c.call)(x)
    gs = cotangents(outs)
    first = grads_of(outs, x, c.on_all, gs, retain_graph=True)
    first = {n: (None if g is None else g.clone()) for n, g in first.items()}
    second = grads_of(outs, x, c.on_all, gs, retain_graph=True)
    sync(dev)
    _same('P5', c, 'second backward over the same graph', second, first)


def p6(c, dev, inp, inp_b):
    """Two live graphs and a no_grad call in between: outputs and gradients equal two independent runs, bitwise."""
    ya, ga, _, _ = run(c, inp, c.on_all, seed=1)
    yb, gb, _, _ = run(c, inp_b, c.on_all, seed=2)
    xa, xb = leaves(c, inp, c.on_all), leaves(c, inp_b, c.on_all)
    y1 = c.call(xa)
    y2 = c.call(xb)
    with torch.no_grad():
        c.call(leaves(c, inp, ()))
    g1 = grads_of(y1, xa, c.on_all, cotangents(y1, 1))
    g2 = grads_of(y2, xb, c.on_all, cotangents(y2, 2))
    sync(dev)
    _same_outs('P6', c, 'first of two live graphs', y1, ya)
    _same_outs('P6', c, 'second of two live graphs', y2, yb)
    _same('P6', c, 'first of two live graphs', g1, ga)
    _same('P6', c, 'second of two live graphs', g2, gb)


def p7(c, dev, inp):
    """Layouts of the incoming gradient -- stride-0 expanded, non-contiguous, non-zero on one slice only, one of two outputs unused -- give the
    gradients of the same gradient materialised contiguous, bitwise."""
    on = c.on_all
    def both(what, loss_of, gs_of):
        x = leaves(c, inp, on)
        outs = c.call(x)
        got = dict(zip(on, torch.autograd.grad(loss_of(outs), [x[n] for n in on], allow_unused=True)))
        x2 = leaves(c, inp, on)
        outs2 = c.call(x2)
        want = grads_of(outs2, x2, on, gs_of(outs2))
        sync(dev)
        _same('P7', c, what, got, want)
    both('expanded gradient (out.sum())', lambda outs: sum(o.sum() for o in outs), lambda outs: [torch.ones_like(o) for o in outs])
    def weights(outs):                                       # one weight per output, stored with its axes reversed
        g = _gen(7)
        return [_rnd(g, *reversed(o.shape)).to(device=o.device, dtype=o.dtype) for o in outs]
    both('non-contiguous gradient (permute, weight, sum)',
         lambda outs: sum((o.permute(*reversed(range(o.dim()))) * w).sum() for o, w in zip(outs, weights(outs))),
         lambda outs: [w.permute(*reversed(range(w.dim()))).contiguous() for w in weights(outs)])
    def pick(o):
        return o[o.shape[0] - 1:] if o.shape[0] > 1 else o[..., -1:]
    def sliced(outs):
        gs = []
        for o, g in zip(outs, cotangents(outs, 3)):
            z = torch.zeros_like(o)
            pick(z).copy_(pick(g))
            gs.append(z)
        return gs
    both('gradient on one slice of the output', lambda outs: sum((pick(o) * pick(g)).sum() for o, g in zip(outs, cotangents(outs, 3))), sliced)
    x = leaves(c, inp, on)
    n_out = len(c.call(x))
    for used in range(n_out if n_out > 1 else 0):            # two-output Functions: an unused output equals zeros for it
        x = leaves(c, inp, on)
        outs = c.call(x)
        g = cotangents(outs, 4)[used]
        got = dict(zip(on, torch.autograd.grad([outs[used]], [x[n] for n in on], [g], allow_unused=True)))
        x2 = leaves(c, inp, on)
        outs2 = c.call(x2)
        want = grads_of(outs2, x2, on, [g if i == used else torch.zeros_like(o) for i, o in enumerate(outs2)])
        sync(dev)
        for n in on:                                         # (an input the used output does not depend on: None, or zeros from the Function)
            if got[n] is None and want[n] is not None and float(want[n].abs().max()) == 0.0:
                got[n] = want[n]
        _same('P7', c, f'output {1 - used} unused', got, want)


def _layout(t, kind):
    """``t``'s values in another layout: 'transposed' storage, 'expanded' (stride 0 along the first axis: the values of its first slice), or
    'offset16' (a view that starts 16 bytes into its allocation)."""
    t = t.detach()
    if kind == 'transposed':
        if t.dim() < 2:
            buf = t.new_empty(2 * t.numel())
            v = buf[::2]
            v.copy_(t)
            return v
        return t.transpose(0, -1).contiguous().transpose(0, -1)
    if kind == 'expanded':
        return t[:1].expand(t.shape) if t.dim() >= 1 and t.shape[0] > 1 else t.clone()
    assert kind == 'offset16'
    skip = 16 // t.element_size()
    buf = t.new_empty(t.numel() + skip)
    v = buf[skip:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0
    return v


def p8(c, dev, inp, kind):
    """Inputs in another layout give outputs and gradients bitwise equal to those of contiguous copies."""
    on = c.on_all
    views = {n: _layout(inp[n], kind) for n in c.layouts}
    xa, xb = dict(inp), dict(inp)
    for n in c.diff:
        va = views[n] if n in views else inp[n].detach().clone()
        xa[n] = va.requires_grad_(n in on)
        xb[n] = va.detach().contiguous().clone().requires_grad_(n in on)
    ya = c.call(xa)
    ga = grads_of(ya, xa, on, cotangents(ya))
    yb = c.call(xb)
    gb = grads_of(yb, xb, on, cotangents(yb))
    sync(dev)
    _same_outs('P8', c, f'{kind} inputs', ya, yb)
    _same('P8', c, f'{kind} inputs', ga, gb)


def p9(c, dev, inp):
    """Two backward calls without zero_grad leave p.grad = the fp32 sum of the two separately obtained gradients, bitwise; after a backward the
    gradients of distinct inputs overlap neither each other, nor g, nor any input (a range check on data_ptr and extent)."""
    on = c.on_all
    x = leaves(c, inp, on)
    outs = c.call(x)
    need = [o for o in outs if o.requires_grad]
    g1, g2 = cotangents(outs, 5), cotangents(outs, 6)
    sel = lambda gs: [g for o, g in zip(outs, gs) if o.requires_grad]
    a = grads_of(outs, x, on, g1, retain_graph=True)
    b = grads_of(outs, x, on, g2, retain_graph=True)
    torch.autograd.backward(need, sel(g1), retain_graph=True)
    sync(dev)
    held = {n: x[n].grad for n in on if x[n].grad is not None}
    names = list(held)
    for i, n in enumerate(names):
        for m in names[i + 1:]:
            if overlap(held[n], held[m]):
                raise ContractFailure('P9', f'{c.id}: the gradients of {n} and {m} share memory')
        for j, g in enumerate(g1):
            if overlap(held[n], g):
                raise ContractFailure('P9', f'{c.id}: the gradient of {n} shares memory with the incoming gradient of output {j}')
        for k, v in _tensors(x).items():
            if overlap(held[n], v):
                raise ContractFailure('P9', f'{c.id}: the gradient of {n} shares memory with input {k}')
    torch.autograd.backward(need, sel(g2), retain_graph=True)
    sync(dev)
    for n in on:
        if a[n] is None:
            continue
        if not bits_equal(x[n].grad, a[n] + b[n]):
            raise ContractFailure('P9', f'{c.id}: {n}.grad after two backward calls is not the sum of the two gradients')


def p10(c, dev, inp, call=None):
    """Higher order is refused.  ``once_differentiable`` defers its error to the moment the returned gradient is differentiated, so the refusal
    is asked for where a user meets it: a gradient penalty -- grad(..., create_graph=True) of a loss whose incoming gradient requires grad, the
    penalty added to the loss, backward -- raises RuntimeError instead of silently training without the penalty."""
    on = c.on_all
    x = leaves(c, inp, on)
    outs = (call or c.call)(x)
    loss = sum((o.float() ** 2).sum() for o in outs)
    try:
        gs = torch.autograd.grad(loss, [x[n] for n in on], create_graph=True, allow_unused=True)
        total = loss + sum((g.float() ** 2).sum() for g in gs if g is not None)
        total.backward()
    except RuntimeError as e:
        if 'once_differentiable' not in str(e):
            raise ContractFailure('P10', f'{c.id}: the gradient penalty raised, but not once_differentiable\'s refusal: {e}') from e
        return
    finally:
        sync(dev)
    raise ContractFailure('P10', f'{c.id}: a gradient penalty through create_graph=True raised nothing')


def p11(c, dev, inp):
    """The forward under no_grad, and in grad mode with nothing requiring grad, equals the grad-mode forward bitwise and does not require grad."""
    on = c.on_all if c.p11_on is None else c.p11_on
    want = c.call(leaves(c, inp, on))
    with torch.no_grad():
        a = c.call(leaves(c, inp, on))
    b = c.call(leaves(c, inp, ()))
    sync(dev)
    for what, outs in (('under no_grad', a), ('with nothing requiring grad', b)):
        _same_outs('P11', c, what, outs, want)
        if any(o.requires_grad for o in outs):
            raise ContractFailure('P11', f'{c.id}: the output {what} requires grad')
