"""Rank-r ``MixedFusion`` on the fused HIP kernels (``csrc/stc_mixed_fusion_lr.hip``, ABI v40: ``stc_mixed_fusion_lr_fwd_f32`` /
``stc_mixed_fusion_lr_bwd_f32``) and its way up to the trainer.

CPU part: the header, the ctypes table and ``FUSION_LR_CHUNK`` agree; every refusal comes back before any HIP call with its code; the
routing predicate on CPU tensors; ``MixedFusion(6, rank=3)`` on the CPU is the dense layer with weight ``U V^T``; ``Trainer`` builds the
factorised layers from ``params['fusion_rank']``; the float64 torch twin of the four binding methods equals autograd of the expression.

GPU part (-m gpu): G and all eight gradients against float64 torch autograd of

    gate = sigmoid(U_A (V_A^T vec A) + b_A + U_P (V_P^T vec P) + b_P),   G = gate * A + (1 - gate) * P

on the inputs of ``tests/test_hip_kernels.py::test_mixed_fusion`` (A 0/1 at rate 0.3 -- uniform for n <= 2 --, P a softmax of normals, a normal
cotangent), each shape at two parameter scales (``FactorisedLinear``'s own initialisation; ``randn * (D r)^(-1/4)`` with biases ``0.1 randn``);
frozen subsets; routing and launch counts; bitwise reproducibility, eager against HIP-graph replay; NaN / +Inf in each operand; the autograd
contract; one model step on both routes.

Bounds: ``TOL`` (1e-5) for G and ``FUSION_GRAD`` (2e-5) for gradients, of tests/test_hip_kernels.py, with ``rel_err``: the fp32 torch expression
stays below 9e-7 against float64 on every shape and gradient here, at both scales."""
import os
import re

import pytest
import torch

import STC_GNN as M
from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib, fusion as F, ops
from tests.conftest import REPO, rel_err
from tests.test_hip_kernels import FUSION_GRAD, TOL

CHUNK = _lib.FUSION_LR_CHUNK
ENTRIES = ('stc_mixed_fusion_lr_supported', 'stc_mixed_fusion_lr_workspace_bytes', 'stc_mixed_fusion_lr_fwd_f32', 'stc_mixed_fusion_lr_bwd_f32')
NAMES = ('A', 'P', 'UA', 'VA', 'bA', 'UP', 'VP', 'bP')                # the operator's argument order
SHAPES = [(1, 1), (2, 1), (3, 2), (6, 3), (10, 4), (15, 5), (15, 16), (33, 7), (40, 8), (64, 32), (100, 16), (100, 64)]
SCALES = ('init', 'wide')


# ---- the expression, its inputs and its float64 autograd ---------------------------------------------------------------------------------------
def expression(A, P, UA, VA, bA, UP, VP, bP):
    """``MixedFusion.forward`` with ``FactorisedLinear`` layers, written out."""
    gate = torch.sigmoid(torch.mv(UA, torch.mv(VA.t(), A.reshape(-1))) + bA + torch.mv(UP, torch.mv(VP.t(), P.reshape(-1))) + bP).reshape(A.shape)
    return gate * A + (1 - gate) * P


def inputs(n, r, scale):
    """({name: fp32 CPU tensor} in ``NAMES`` order, cotangent R)."""
    D = n * n
    g = torch.Generator().manual_seed(1000 * n + r)
    A = (torch.rand(n, n, generator=g) < 0.3).float() if n > 2 else torch.rand(n, n, generator=g)
    P = torch.softmax(torch.randn(n, n, generator=g), -1)
    R = torch.randn(n, n, generator=g)
    if scale == 'init':
        torch.manual_seed(1000 * n + r)
        mod = M.MixedFusion(n, rank=r)
        UA, VA, bA, UP, VP, bP = (t.detach().clone() for t in (mod.lin_A.U, mod.lin_A.V, mod.lin_A.bias, mod.lin_P.U, mod.lin_P.V, mod.lin_P.bias))
    else:
        UA, VA, UP, VP = (torch.randn(D, r, generator=g) * (D * r) ** -0.25 for _ in range(4))
        bA, bP = (torch.randn(D, generator=g) * 0.1 for _ in range(2))
    return dict(zip(NAMES, (A, P, UA, VA, bA, UP, VP, bP))), R


def float64_autograd(ops_, R):
    """(G, {name: gradient}) of the expression in float64 from fp32-valued operands."""
    leaves = {k: v.detach().double().cpu().requires_grad_() for k, v in ops_.items()}
    G = expression(*[leaves[k] for k in NAMES])
    (G * R.double().cpu()).sum().backward()
    return G.detach(), {k: v.grad for k, v in leaves.items()}


_REF = {}


def reference(n, r, scale):
    """The inputs of one case and their float64 result: computed once, shared, never written."""
    key = (n, r, scale)
    if key not in _REF:
        ops_, R = inputs(n, r, scale)
        _REF[key] = (ops_, R) + float64_autograd(ops_, R)
    return _REF[key]


def module_on(ops_, device, frozen=()):
    """``MixedFusion(n, rank=r)`` holding the case's parameters on ``device`` + (A, P) there; names in ``frozen`` do not require grad."""
    n, r = ops_['A'].shape[0], ops_['UA'].shape[1]
    mod = M.MixedFusion(n, rank=r)
    with torch.no_grad():
        for layer, s in ((mod.lin_A, 'A'), (mod.lin_P, 'P')):
            layer.U.copy_(ops_['U' + s])
            layer.V.copy_(ops_['V' + s])
            layer.bias.copy_(ops_['b' + s])
    mod = mod.to(device)
    for name, p in params_of(mod).items():
        p.requires_grad_(name not in frozen)
    A = ops_['A'].to(device).requires_grad_('A' not in frozen)
    P = ops_['P'].to(device).requires_grad_('P' not in frozen)
    return mod, A, P


def params_of(mod):
    return dict(UA=mod.lin_A.U, VA=mod.lin_A.V, bA=mod.lin_A.bias, UP=mod.lin_P.U, VP=mod.lin_P.V, bP=mod.lin_P.bias)


def run(mod, A, P, R):
    """One forward + backward; (G, {name: gradient or None})."""
    for t in (A, P, *mod.parameters()):
        t.grad = None
    G = mod(A, P)
    (G * R.to(G.device)).sum().backward()
    return G.detach(), dict(A=A.grad, P=P.grad, **{k: p.grad for k, p in params_of(mod).items()})


# ---- the float64 twin of the four binding methods ----------------------------------------------------------------------------------------------
class FusionLRTwin(EmulatedKernels):
    """The CPU twin with the rank-r entry points: include/stc_hip.h "Rank-r MixedFusion" in torch, in the operands' own precision."""

    mixed_fusion_lr = True

    def mixed_fusion_lr_supported(self, D, r):
        return D >= 1 and 1 <= r <= _lib.FUSION_LR_MAX_RANK and D * r < 2 ** 31

    def mixed_fusion_lr_workspace_bytes(self, D, r):
        return 16 * r * -(-D // CHUNK) if self.mixed_fusion_lr_supported(D, r) else 0

    def mixed_fusion_lr_fwd(self, UA, VA, bA, UP, VP, bP, A, P):
        t = torch.cat([VA.t() @ A.reshape(-1), VP.t() @ P.reshape(-1)])
        r = UA.shape[1]
        gate = torch.sigmoid(UA @ t[:r] + bA + UP @ t[r:] + bP).reshape(A.shape)
        return gate, gate * A + (1 - gate) * P, t

    def mixed_fusion_lr_bwd(self, UA, VA, UP, VP, A, P, gate, t, dG, want):
        r = UA.shape[1]
        dpre = (dG * (A - P) * gate * (1 - gate)).reshape(-1)
        sA, sP = UA.t() @ dpre, UP.t() @ dpre
        out = (torch.outer(dpre, t[:r]), torch.outer(A.reshape(-1), sA), torch.outer(dpre, t[r:]), torch.outer(P.reshape(-1), sP),
               dG * gate + (VA @ sA).reshape(A.shape), dG * (1 - gate) + (VP @ sP).reshape(A.shape))
        kept = [x if w else None for x, w in zip(out, want)]
        return kept[0], kept[1], kept[2], kept[3], dpre, kept[4], kept[5]


# ============================================================================================================== CPU
def test_header_table_and_chunk_agree():
    header = open(os.path.join(REPO, 'include', 'stc_hip.h')).read()
    assert re.findall(r'^#define\s+STC_FUSION_LR_CHUNK\s+(\d+)\b', header, flags=re.M) == [str(CHUNK)]
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ENTRIES:
        assert re.search(rf'\b{name}\s*\(', code), f'{name} is not declared in include/stc_hip.h'
        assert name in _lib._ABI and name in _lib.EXPORTS
    lib = _lib.load_library()
    assert lib.stc_version() == _lib.ABI_VERSION >= 40
    assert _lib.HipKernels.mixed_fusion_lr is True and not hasattr(EmulatedKernels, 'mixed_fusion_lr')
    nonfinite = header[header.index('---- Non-finite values'):]
    assert 'stc_mixed_fusion_lr_fwd/bwd_f32' in nonfinite[:nonfinite.index('*/')]


def test_the_shapes_reach_past_two_chunks_raggedly():
    assert any(n * n > 2 * CHUNK and (n * n) % CHUNK for n, _ in SHAPES)
    assert any(n * n < 64 for n, _ in SHAPES) and any((n * n) % 2 for n, _ in SHAPES) and any(r == _lib.FUSION_LR_MAX_RANK for _, r in SHAPES)


@pytest.mark.parametrize('D,r', [(1, 1), (CHUNK, 4), (CHUNK + 1, 7), (10 ** 4, 64), (90000, 16)])
def test_supported_and_workspace_bytes(D, r):
    lib = _lib.load_library()
    assert lib.stc_mixed_fusion_lr_supported(D, r) == 1
    assert lib.stc_mixed_fusion_lr_workspace_bytes(D, r) == 16 * r * -(-D // CHUNK) == FusionLRTwin().mixed_fusion_lr_workspace_bytes(D, r)


@pytest.mark.parametrize('D,r', [(0, 4), (-1, 4), (100, 0), (100, 65), (1 << 27, 16), ((1 << 31) - 1, 2)])
def test_refused_shapes_are_unsupported_and_need_no_workspace(D, r):
    lib = _lib.load_library()
    assert lib.stc_mixed_fusion_lr_supported(D, r) == 0 and lib.stc_mixed_fusion_lr_workspace_bytes(D, r) == 0


_FWD = dict(UA=0x10000, VA=0x20000, bA=0x30000, UP=0x40000, VP=0x50000, bP=0x60000, A=0x70000, P=0x80000, gate=0x90000, G=0xA0000, t=0xB0000, ws=0xC0000)
_BWD = dict(UA=0x10000, VA=0x20000, UP=0x40000, VP=0x50000, A=0x70000, P=0x80000, gate=0x90000, t=0xB0000, dG=0xD0000,
            dUA=0x110000, dVA=0x120000, dUP=0x130000, dVP=0x140000, db=0x150000, dA=0x160000, dP=0x170000, ws=0xC0000)


def _call(lib, which, D=36, r=4, ws_bytes=None, **over):
    table = dict(_FWD if which == 'fwd' else _BWD, **over)
    if ws_bytes is None:
        ws_bytes = max(lib.stc_mixed_fusion_lr_workspace_bytes(D, r), 1)
    fn = lib.stc_mixed_fusion_lr_fwd_f32 if which == 'fwd' else lib.stc_mixed_fusion_lr_bwd_f32
    ptrs = [table[k] for k in (_FWD if which == 'fwd' else _BWD) if k != 'ws']
    return fn(*ptrs, table['ws'], ws_bytes, D, r, None)


def test_refusals_come_before_any_hip_call():
    """Made-up addresses throughout: a call that got as far as a launch would fault, a refusal never touches them."""
    lib = _lib.load_library()
    err = lambda: lib.stc_last_error()
    EINVAL, EALIGN, ELIMIT, EUNSUPPORTED = -1, -2, _lib.STC_ELIMIT, -4
    for which, table in (('fwd', _FWD), ('bwd', _BWD)):
        assert _call(lib, which, D=0) == EINVAL and b'positive' in err()
        assert _call(lib, which, D=-5) == EINVAL and b'positive' in err()
        assert _call(lib, which, r=0) == EUNSUPPORTED and b'rank' in err()
        assert _call(lib, which, r=65) == EUNSUPPORTED and b'rank' in err()
        assert _call(lib, which, D=1 << 27, r=16) == ELIMIT and b'2^31' in err()
        assert _call(lib, which, D=(1 << 31) - 1, r=2) == ELIMIT and b'2^31' in err()
        optional = ('dUA', 'dVA', 'dUP', 'dVP', 'dA', 'dP')
        for name in table:
            if name not in optional:
                assert _call(lib, which, **{name: None}) == EINVAL and b'null' in err(), (which, name)
        for name in ('UA', 'VA', 'UP', 'VP') + (('dUA', 'dVA', 'dUP', 'dVP') if which == 'bwd' else ()):
            assert _call(lib, which, **{name: table[name] + 4}) == EALIGN and b'16-byte' in err(), (which, name)
        assert _call(lib, which, A=table['A'] + 2) == EALIGN and b'4-byte' in err()
        assert _call(lib, which, ws=table['ws'] + 4) == EALIGN and b'8-byte' in err()
        need = lib.stc_mixed_fusion_lr_workspace_bytes(36, 4)
        assert _call(lib, which, ws_bytes=need - 1) == EINVAL and b'workspace' in err() and str(need).encode() in err()
    assert _call(lib, 'fwd', G=_FWD['A']) == EINVAL and b'alias' in err()
    assert _call(lib, 'bwd', dP=_BWD['P']) == EINVAL and b'alias' in err()


def test_the_predicate_is_false_for_cpu_tensors(monkeypatch):
    monkeypatch.setattr(ops, '_kernels', None)
    ops_, _ = inputs(6, 3, 'init')
    assert not F.mixed_fusion_lr_supported(*[ops_[k] for k in NAMES])
    assert not F.mixed_fusion_lr_supported(*[ops_[k].double() for k in NAMES])
    assert ops._kernels is None                                  # CPU tensors never bring the kernel set up


def test_on_the_cpu_the_factorised_fusion_is_the_dense_layer_with_weight_u_vt():
    ops_, R = inputs(6, 3, 'init')
    mod, A, P = module_on(ops_, 'cpu')
    G, grads = run(mod, A, P, R)
    assert 'MixedFusionLR' not in type(mod(A, P).grad_fn).__name__
    dense = M.MixedFusion(6)
    with torch.no_grad():
        for lin, fac in ((dense.lin_A, mod.lin_A), (dense.lin_P, mod.lin_P)):
            lin.weight.copy_(fac.dense_weight())
            lin.bias.copy_(fac.bias)
    Ad, Pd = A.detach().clone().requires_grad_(), P.detach().clone().requires_grad_()
    Gd = dense(Ad, Pd)
    (Gd * R).sum().backward()
    assert rel_err(G, Gd) < 1e-6 and rel_err(grads['A'], Ad.grad) < 1e-5 and rel_err(grads['P'], Pd.grad) < 1e-5
    assert rel_err(grads['bA'], dense.lin_A.bias.grad) < 1e-5
    assert rel_err(grads['UA'], dense.lin_A.weight.grad @ mod.lin_A.V.detach()) < 1e-5      # dU = dW V, dV = dW^T U
    assert rel_err(grads['VP'], dense.lin_P.weight.grad.t() @ mod.lin_P.U.detach()) < 1e-5


def test_the_trainer_takes_fusion_rank_from_params(tmp_path, monkeypatch):
    from stc_hip.trainer import Trainer
    from tests.golden.make_golden import pipeline_inputs
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    data, params = pipeline_inputs()
    params = dict(params, output_dir=str(tmp_path), _allow_cpu_for_tests=True)
    N = params['H'] * params['W']
    plain = Trainer(params, data)
    assert isinstance(plain.model.mix_graph_pair.aggreg_S.lin_A, torch.nn.Linear)
    ranked = Trainer(dict(params, fusion_rank=3), data)
    fuse = ranked.model.mix_graph_pair.aggreg_S
    assert isinstance(fuse.lin_A, M.FactorisedLinear) and isinstance(fuse.lin_P, M.FactorisedLinear)
    assert tuple(fuse.lin_A.U.shape) == (N * N, 3) and tuple(fuse.lin_P.V.shape) == (N * N, 3)
    assert isinstance(ranked.model.mix_graph_pair.aggreg_C.lin_A, torch.nn.Linear)          # the C x C fusion stays dense
    with pytest.raises(ValueError, match='fusion_rank'):
        Trainer(dict(params, fusion_rank=3), data, graph_mode='csr-fixed')


@pytest.mark.parametrize('n,r', [(3, 2), (6, 3), (10, 4), (15, 16)])
def test_the_float64_twin_equals_autograd_of_the_expression(n, r):
    ops_, R = inputs(n, r, 'wide')
    G, grads = float64_autograd(ops_, R)
    d = {k: v.double() for k, v in ops_.items()}
    k = FusionLRTwin()
    assert k.mixed_fusion_lr_supported(n * n, r) and not k.mixed_fusion_lr_supported(n * n, 65)
    gate, Gt, t = k.mixed_fusion_lr_fwd(d['UA'], d['VA'], d['bA'], d['UP'], d['VP'], d['bP'], d['A'], d['P'])
    dUA, dVA, dUP, dVP, db, dA, dP = k.mixed_fusion_lr_bwd(d['UA'], d['VA'], d['UP'], d['VP'], d['A'], d['P'], gate, t, R.double(), (True,) * 6)
    assert rel_err(Gt, G) < 1e-13
    for name, got in dict(A=dA, P=dP, UA=dUA, VA=dVA, bA=db, UP=dUP, VP=dVP, bP=db).items():
        assert rel_err(got, grads[name]) < 1e-12, name
    some = k.mixed_fusion_lr_bwd(d['UA'], d['VA'], d['UP'], d['VP'], d['A'], d['P'], gate, t, R.double(), (False, True, False, False, False, True))
    assert [x is None for x in some] == [True, False, True, True, False, True, False]


def test_the_kernels_use_no_scratch(tmp_path):
    """The four kernels of csrc/stc_mixed_fusion_lr.hip as the compiler reports them with the library's own flags (needs hipcc, no GPU)."""
    from tests.test_first_step_isa import _resource_usage
    from tests.test_isa import HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not present')
    usage = _resource_usage('stc_mixed_fusion_lr.hip', tmp_path)
    assert len(usage) == 4, sorted(usage)
    for name, u in usage.items():
        assert u['ScratchSize'] == 0, (name, u)


# ============================================================================================================== GPU
@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.fixture
def routed(hip, monkeypatch):
    """The HIP kernel set behind ``ops.kernels()``, the switch on, and a log: ('call',) per ``fusion.mixed_fusion_lr`` and the name of every C
    entry point launched."""
    log = []
    monkeypatch.setattr(ops, '_kernels', hip)
    monkeypatch.setattr(F, '_FUSED', True)
    inner_op, inner_launch = F.mixed_fusion_lr, hip._launch
    monkeypatch.setattr(F, 'mixed_fusion_lr', lambda *a: (log.append('call'), inner_op(*a))[1])
    monkeypatch.setattr(hip, '_launch', lambda name, *a, **kw: (log.append(name), inner_launch(name, *a, **kw))[1])
    return log


def _check(tag, G, grads, want_G, want_grads, skip=()):
    errs = {'G': rel_err(G, want_G)}
    for name in NAMES:
        if name in skip:
            assert grads[name] is None, name
        else:
            errs['d' + name] = rel_err(grads[name], want_grads[name])
    print(tag, ' '.join(f'{k} {v:.1e}' for k, v in errs.items()))
    assert errs.pop('G') < TOL, tag
    for name, e in errs.items():
        assert e < FUSION_GRAD, (tag, name, e)


@pytest.mark.gpu
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('n,r', SHAPES)
def test_parity_with_float64_autograd(routed, n, r, scale):
    ops_, R, want_G, want_grads = reference(n, r, scale)
    for frozen in ((), ('A',)):
        mod, A, P = module_on(ops_, 'cuda', frozen)
        G, grads = run(mod, A, P, R)
        torch.cuda.synchronize()
        _check(f'n={n} r={r} {scale} frozen={frozen}:', G, grads, want_G, want_grads, skip=frozen)
    assert routed.count('call') == 2 and routed.count('stc_mixed_fusion_lr_fwd_f32') == 2 and routed.count('stc_mixed_fusion_lr_bwd_f32') == 2


@pytest.mark.gpu
@pytest.mark.parametrize('n,r', [(15, 5), (40, 8)])
def test_frozen_subsets_get_none_and_leave_the_other_bits_alone(routed, n, r):
    ops_, R, _, _ = reference(n, r, 'wide')
    _, full = run(*module_on(ops_, 'cuda'), R)
    for frozen in (('UA', 'UP'), ('VA', 'VP'), ('bA', 'bP'), ('P',), ('UA', 'VA', 'UP', 'VP', 'A', 'P')):
        _, grads = run(*module_on(ops_, 'cuda', frozen), R)
        for name in NAMES:
            if name in frozen:
                assert grads[name] is None, (frozen, name)
            else:
                assert torch.equal(grads[name], full[name]), (frozen, name)


@pytest.mark.gpu
def test_routing_and_launch_counts(routed, hip, monkeypatch):
    ops_, R, want_G, want_grads = reference(10, 4, 'wide')
    mod, A, P = module_on(ops_, 'cuda')
    run(mod, A, P, R)
    # one operator call; the binding launches one C entry point per direction, each at most two kernels (include/stc_hip.h): within 2 + 2
    assert routed == ['call', 'stc_mixed_fusion_lr_fwd_f32', 'stc_mixed_fusion_lr_bwd_f32']
    with torch.no_grad():
        del routed[:]
        mod(A, P)
        assert routed == ['call', 'stc_mixed_fusion_lr_fwd_f32']

    def quiet(tag, mod, A, P, want_G=want_G, want_grads=want_grads):
        del routed[:]
        G, grads = run(mod, A, P, R)
        assert routed == [], (tag, routed)
        _check(tag, G, grads, want_G, want_grads)

    monkeypatch.setattr(F, '_FUSED', False)
    quiet('switch off:', mod, A, P)
    monkeypatch.setattr(F, '_FUSED', True)

    def shifted(t):                                                              # the same values 4 bytes into a larger buffer
        buf = torch.zeros(t.numel() + 8, device='cuda')
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t.detach())
        assert view.data_ptr() % 16 == 4
        return view

    for name in NAMES:
        mod, A, P = module_on(ops_, 'cuda')
        if name == 'A':
            A = shifted(A).requires_grad_()
        elif name == 'P':
            P = shifted(P).requires_grad_()
        else:
            layer = mod.lin_A if name.endswith('A') else mod.lin_P
            attr = {'U': 'U', 'V': 'V', 'b': 'bias'}[name[0]]
            setattr(layer, attr, torch.nn.Parameter(shifted(getattr(layer, attr))))
        quiet(f'{name} 4 bytes off:', mod, A, P)

    ops65, R65 = inputs(10, 65, 'wide')
    G65, grads65 = float64_autograd(ops65, R65)
    del routed[:]
    G, grads = run(*module_on(ops65, 'cuda'), R65)
    assert routed == []
    _check('rank 65:', G, grads, G65, grads65)
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())                       # a kernel set without ``mixed_fusion_lr``: the CPU twin
    mod, A, P = module_on(ops_, 'cuda')
    assert not F.mixed_fusion_lr_supported(A, P, *params_of(mod).values())


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


@pytest.mark.gpu
@pytest.mark.parametrize('n,r', [(33, 7), (100, 16)])
def test_eager_runs_and_graph_replays_give_the_same_bits(routed, n, r):
    first, second = inputs(n, r, 'init'), inputs(n, r, 'wide')

    def eager(ops_, R):
        G, grads = run(*module_on(ops_, 'cuda'), R)
        return [_bits(G)] + [_bits(grads[k]) for k in NAMES]

    a, b = eager(*second), eager(*second)
    assert all(torch.equal(x, y) for x, y in zip(a, b))

    mod, A, P = module_on(first[0], 'cuda')
    Rg = first[1].cuda()
    leaves = dict(A=A, P=P, **params_of(mod))

    def step():
        for t in leaves.values():
            t.grad = None
        G = mod(A, P)
        (G * Rg).sum().backward()
        return G

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_G = step()
    static = [static_G] + [leaves[k].grad for k in NAMES]
    with torch.no_grad():
        for k in NAMES:
            leaves[k].copy_(second[0][k])
        Rg.copy_(second[1])
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for name, got, want in zip(('G',) + NAMES, static, a):
            assert torch.equal(_bits(got), want), name


@pytest.mark.gpu
@pytest.mark.parametrize('poison', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('where', NAMES)
def test_non_finite_values_are_handed_on(routed, where, poison):
    """One poisoned element at (6, 3): G and every gradient are non-finite exactly where the float64 torch expression is, and right elsewhere."""
    ops_, R = inputs(6, 3, 'wide')
    ops_ = {k: v.clone() for k, v in ops_.items()}
    ops_[where].view(-1)[7] = poison
    want_G, want_grads = float64_autograd(ops_, R)
    G, grads = run(*module_on(ops_, 'cuda'), R)
    torch.cuda.synchronize()
    assert routed.count('call') == 1
    for name, got, want, bound in [('G', G, want_G, TOL)] + [('d' + k, grads[k], want_grads[k], FUSION_GRAD) for k in NAMES]:
        got = got.double().cpu()
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin), (name, int(fin.sum()), int(torch.isfinite(got).sum()))
        if bool(fin.any()):
            assert rel_err(got[fin], want[fin]) < bound, name


@pytest.mark.gpu
def test_double_backward_raises_and_gradients_accumulate(routed):
    ops_, R, _, want_grads = reference(6, 3, 'wide')
    mod, A, P = module_on(ops_, 'cuda')
    loss = (mod(A, P) ** 2).sum()                                                 # a gradient penalty: the incoming gradient requires grad
    (dA,) = torch.autograd.grad(loss, A, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        (loss + (dA ** 2).sum()).backward()
    _, once = run(mod, A, P, R)
    before = {k: v.clone() for k, v in once.items()}
    G = mod(A, P)
    (G * R.cuda()).sum().backward()                                               # .grad exists: the second backward adds to it
    for name, leaf in dict(A=A, P=P, **params_of(mod)).items():
        assert rel_err(leaf.grad, 2 * before[name]) < 1e-6, name
        assert rel_err(leaf.grad, 2 * want_grads[name]) < FUSION_GRAD, name


@pytest.mark.gpu
def test_one_model_step_on_both_routes(routed, monkeypatch):
    from stc_hip.loss import ComboLoss
    torch.manual_seed(0)
    N, C, B, T, horizon = 40, 3, 2, 3, 2
    model = M.STCGNN(N, C, 2, 2, 1, 16, 1, horizon, fusion_rank=4).cuda()
    g = torch.Generator().manual_seed(5)
    X = (torch.rand(B, T, N, C, generator=g) < 0.3).float().cuda()
    Y = (torch.rand(B, horizon, N, C, generator=g) < 0.3).float().cuda()
    As = (torch.rand(N, N, generator=g) < 0.2).float().cuda()
    Ac = torch.rand(C, C, generator=g).cuda()

    def step(fused):
        monkeypatch.setattr(F, '_FUSED', fused)
        del routed[:]
        model.zero_grad(set_to_none=True)
        yhat = model(X_seq=X, As=As, Ac=Ac)
        ComboLoss()(yhat, Y).backward()
        torch.cuda.synchronize()
        return yhat.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}, routed.count('call')

    y_t, grads_t, calls_t = step(False)
    y_f, grads_f, calls_f = step(True)
    assert (calls_t, calls_f) == (0, 1)
    assert rel_err(y_f, y_t) < TOL
    for name, want in grads_t.items():
        assert rel_err(grads_f[name], want) < FUSION_GRAD, name
