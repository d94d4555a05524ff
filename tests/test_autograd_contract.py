"""The autograd contract of every operator ("Autograd contract"): what the twelve ``torch.autograd.Function``s of ``stc_hip.ops`` and
``stc_hip.small`` promise outside the one pattern the parity tests drive them in (fresh contiguous tensors, everything differentiable, one
forward, one backward).  The Functions of the package without a case here are listed in ``CONTRACT_ELSEWHERE``.

One parametrised test per property P1..P11 over the case table of tests/autograd_contract.py, each on the CPU twin (``cpu-emulated``: the host logic
of the Functions over oracle/kernel_emul.py) and on the GPU (``cuda``: the same through libstc_hip.so -- what the twin cannot say is what a HIP
kernel does to a plane it is handed).  A case the twin has no kernels for runs on the GPU only; a property that cannot apply to a case is listed
in ``NOT_APPLICABLE`` with its reason.  The negative controls show, on the CPU, that P2, P4, P5 and P10 can fail.
"""
import importlib
import os
import pkgutil

import pytest
import torch
from torch.autograd.function import once_differentiable

import STC_GNN as M
import stc_hip
from oracle.kernel_emul import EmulatedKernels
from stc_hip import ops
from tests import autograd_contract as A
from tests.autograd_contract import BY_ID, CASES, CONTRACT_ELSEWHERE, NOT_APPLICABLE, NOT_BITWISE_WHEN_FROZEN, REFUSALS, ContractFailure
from tests.conftest import REPO, rel_err


@pytest.fixture
def dev(request, monkeypatch):
    """Select the kernel set: the emulated twin on CPU tensors, or the HIP library on the GPU (as tests/test_module_parity.py does)."""
    if request.param == 'cuda':
        monkeypatch.setattr(ops, '_kernels', None)          # -> HipKernels() on first use; raises if not built
        return 'cuda'
    monkeypatch.setattr(ops, '_kernels', A.KernelTwin())
    return 'cpu'


def _pairs(prop, extra=lambda c: [()]):
    """(device, case, ...) for every case the property applies to: the twin where it has the kernels, and the GPU."""
    out = []
    for c in CASES:
        if (prop, c.id) in NOT_APPLICABLE:
            continue
        for more in extra(c):
            if (prop, c.id) + tuple(more) in NOT_APPLICABLE:
                continue
            tag = '-'.join((c.id,) + tuple(str(m) for m in more))
            if c.gpu_only is None:
                out.append(pytest.param('cpu-emulated', c.id, *more, id=f'cpu-emulated-{tag}'))
            out.append(pytest.param('cuda', c.id, *more, marks=pytest.mark.gpu, id=f'cuda-{tag}'))
    return out


def _watch_backwards(c, monkeypatch):
    """Count the backward calls of the case's Functions (the backward node looks ``backward`` up on the class at call time)."""
    ran = {}
    for cls in c.functions:
        real = cls.backward
        def counted(ctx, *grads, _real=real, _name=cls.__name__):
            ran[_name] = ran.get(_name, 0) + 1
            return _real(ctx, *grads)
        monkeypatch.setattr(cls, 'backward', staticmethod(counted))
    return ran


def _start(cid, dev, monkeypatch):
    c = BY_ID[cid]
    return c, c.setup(monkeypatch, dev)


@pytest.mark.parametrize('dev,cid', _pairs('P1'), indirect=['dev'])
def test_p1_parity_with_the_float64_reference(dev, cid, monkeypatch):
    """P1, and the coverage walk's second half: the backward of every Function the case names really ran, on the route the case asserts."""
    c, verify = _start(cid, dev, monkeypatch)
    ran = _watch_backwards(c, monkeypatch)
    A.p1(c, dev, c.make(dev, 0))
    path = verify()
    if c.op == 'STCGNN':
        assert path == A.module_path(c, c.on_all) == 'per-cell', (cid, path)
    assert set(ran) == {f.__name__ for f in c.functions}, (cid, ran)


@pytest.mark.parametrize('dev,cid,name', _pairs('P2', lambda c: [(n,) for n in c.diff]), indirect=['dev'])
def test_p2_never_a_silent_gradient(dev, cid, name, monkeypatch):
    c, verify = _start(cid, dev, monkeypatch)
    assert A.p2(c, dev, c.make(dev, 0), name) == ('refused' if c.refused(name) else 'gradient')
    if c.op == 'STCGNN':                                     # the path the module took with this input alone differentiable
        assert verify() == A.module_path(c, (name,)), (cid, name)


@pytest.mark.parametrize('dev,cid', _pairs('P3'), indirect=['dev'])
def test_p3_freezing(dev, cid, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p3(c, dev, c.make(dev, 0))


@pytest.mark.parametrize('dev,cid', _pairs('P4'), indirect=['dev'])
def test_p4_nothing_handed_in_is_modified(dev, cid, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p4(c, dev, c.make(dev, 0))


@pytest.mark.parametrize('dev,cid', _pairs('P5'), indirect=['dev'])
def test_p5_backward_is_repeatable(dev, cid, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p5(c, dev, c.make(dev, 0))


@pytest.mark.parametrize('dev,cid', _pairs('P6'), indirect=['dev'])
def test_p6_graphs_do_not_share_state(dev, cid, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p6(c, dev, c.make(dev, 0), c.make(dev, 1))


@pytest.mark.parametrize('dev,cid', _pairs('P7'), indirect=['dev'])
def test_p7_gradient_layouts(dev, cid, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p7(c, dev, c.make(dev, 0))


@pytest.mark.parametrize('dev,cid,kind', _pairs('P8', lambda c: [('transposed',), ('expanded',), ('offset16',)]), indirect=['dev'])
def test_p8_input_layouts(dev, cid, kind, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p8(c, dev, c.make(dev, 0), kind)


@pytest.mark.parametrize('dev,cid', _pairs('P9'), indirect=['dev'])
def test_p9_accumulation_and_aliasing(dev, cid, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p9(c, dev, c.make(dev, 0))


@pytest.mark.parametrize('dev,cid', _pairs('P10'), indirect=['dev'])
def test_p10_higher_order_is_refused(dev, cid, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p10(c, dev, c.make(dev, 0))


@pytest.mark.parametrize('dev,cid', _pairs('P11'), indirect=['dev'])
def test_p11_grad_mode(dev, cid, monkeypatch):
    c, _ = _start(cid, dev, monkeypatch)
    A.p11(c, dev, c.make(dev, 0))


@pytest.mark.gpu
def test_p8_a_view_at_a_4_byte_offset_is_decided_by_the_predicate():
    """Views at a 4-byte offset are never handed to a launch: ``mixed_fusion_supported`` says no for each operand in turn, and the module then
    runs the reference's torch operations -- same graph as the float64 expression, within test_mixed_fusion's bounds."""
    c = BY_ID['mixed_fusion-n10']
    x = c.make('cuda', 0)
    names = ('A', 'P', 'WA', 'bA', 'WP', 'bP')
    def off4(t):
        buf = t.new_empty(t.numel() + 1)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    assert ops.mixed_fusion_supported(*(x[n] for n in names))
    for bad in names:
        assert not ops.mixed_fusion_supported(*(off4(x[n]) if n == bad else x[n] for n in names)), bad
    fusion = M.MixedFusion(10).cuda()
    with torch.no_grad():
        for p, n in ((fusion.lin_A.weight, 'WA'), (fusion.lin_A.bias, 'bA'), (fusion.lin_P.weight, 'WP'), (fusion.lin_P.bias, 'bP')):
            p.copy_(x[n])
    launches = []
    real = ops.mixed_fusion
    try:
        ops.mixed_fusion = lambda *a: (launches.append(1), real(*a))[1]
        got = fusion(off4(x['A']), x['P'])
    finally:
        ops.mixed_fusion = real
    torch.cuda.synchronize()
    assert not launches
    want = A.reference_of(c, 0)[0][0]
    assert rel_err(got, want) < A.TOL


# ---- the coverage walk and the tables -----------------------------------------------------------------------------------------------------------
def _functions_of(mod):
    return {v for v in vars(mod).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == mod.__name__}


def test_every_function_is_named_by_a_case():
    """Every Function of every module of the ``stc_hip`` package has a case here, or is in ``CONTRACT_ELSEWHERE`` with the file that holds its properties."""
    defined = set().union(*[_functions_of(importlib.import_module(f'stc_hip.{m.name}')) for m in pkgutil.iter_modules(stc_hip.__path__)])
    by_name = {f'{f.__module__}.{f.__name__}': f for f in defined}
    assert len(CONTRACT_ELSEWHERE) == 3
    for name, path in CONTRACT_ELSEWHERE.items():
        assert name in by_name, f'{name} is no autograd Function of stc_hip'
        assert os.path.isfile(os.path.join(REPO, path)), path
    elsewhere = {by_name[name] for name in CONTRACT_ELSEWHERE}
    named = {f for c in CASES for f in c.functions}
    assert named <= defined
    assert not named & elsewhere, sorted(f.__name__ for f in named & elsewhere)
    assert len(named) == 12, sorted(f.__name__ for f in named)
    missing = defined - named - elsewhere
    assert not missing, f'autograd Functions without a case in tests/autograd_contract.py: {sorted(f.__name__ for f in missing)}'


def test_the_exception_tables_are_closed_and_name_real_cases():
    keys = {c.refusal_key for c in CASES}
    for (key, arg), reason in REFUSALS.items():
        assert key in keys and reason, (key, arg)
        assert any(c.refusal_key == key and c.argument(n) == arg for c in CASES for n in c.diff), f'no case asks for ({key}, {arg})'
    for (cid, name), reason in NOT_BITWISE_WHEN_FROZEN.items():
        assert cid in BY_ID and reason and (name == '*' or name in BY_ID[cid].diff), (cid, name)
    for (prop, cid, *name), reason in NOT_APPLICABLE.items():
        assert cid in BY_ID and reason and prop in {f'P{i}' for i in range(1, 12)} and all(n in BY_ID[cid].diff for n in name), (prop, cid, name)
    # every form of the cell-graph executor, its first-step and bf16 variants are in the table
    ids = ' '.join(BY_ID)
    for form in ('PLANAR_ONE_BWD', 'PLANAR-', 'PLANAR3', 'ROWS_POST', 'ROWS_SLABS', 'zero_state', 'bf16'):
        assert f'stc_cell_graph-{form}' in ids or form in ids, form


# ---- negative controls (CPU only): each property can fail -------------------------------------------------------------------------------------------
@pytest.fixture
def twin(monkeypatch):
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())


class _ScalesItsGradientInPlace(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return g.mul_(2.0)


class _DropsAGradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(b)
        return a * b

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


class _NotOnceDifferentiable(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return 2.0 * x

    @staticmethod
    def backward(ctx, g):
        return 2.0 * g.detach()


class _OnceDifferentiable(_NotOnceDifferentiable):
    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return 2.0 * g


class _WritesASavedPlane(EmulatedKernels):
    """A twin whose blend backward uses the saved update gate as scratch, as a kernel handed a plane can (no version counter sees it)."""

    def gru_blend_bwd(self, dHnew, U, H, Cand, dCpre, dU, dH):
        super().gru_blend_bwd(dHnew, U, H, Cand, dCpre, dU, dH)
        U.data.mul_(0.5)


def test_control_an_in_place_scaled_gradient_fails_p4(twin):
    c = BY_ID['gru_blend']
    A.p4(c, 'cpu', c.make('cpu', 0))
    with pytest.raises(ContractFailure, match='P4.*incoming gradient'):
        A.p4(c, 'cpu', c.make('cpu', 0), call=lambda x: tuple(_ScalesItsGradientInPlace.apply(o) for o in c.call(x)))


def test_control_a_dropped_gradient_fails_p2(twin):
    make = lambda dev, seed: dict(a=torch.randn(3, 4, generator=A._gen(seed)), b=torch.randn(3, 4, generator=A._gen(seed + 1)))
    c = A.Case('control-drops-b', 'control', [_DropsAGradient], make, lambda x: (_DropsAGradient.apply(x['a'], x['b']),), lambda x: (x['a'] * x['b'],),
               diff=('a', 'b'))
    assert A.p2(c, 'cpu', make('cpu', 0), 'a') == 'gradient'
    with pytest.raises(ContractFailure, match='P2.*silent'):
        A.p2(c, 'cpu', make('cpu', 0), 'b')


def test_control_a_kernel_that_writes_a_saved_plane_fails_p5(monkeypatch):
    c = BY_ID['gru_blend']
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    A.p5(c, 'cpu', c.make('cpu', 0))
    monkeypatch.setattr(ops, '_kernels', _WritesASavedPlane())
    with pytest.raises(ContractFailure, match='P5'):
        A.p5(c, 'cpu', c.make('cpu', 0))


def test_control_a_function_without_once_differentiable_fails_p10(twin):
    c = BY_ID['gru_blend']
    A.p10(c, 'cpu', c.make('cpu', 0), call=lambda x: tuple(_OnceDifferentiable.apply(o) for o in c.call(x)))
    with pytest.raises(ContractFailure, match='P10'):
        A.p10(c, 'cpu', c.make('cpu', 0), call=lambda x: (_NotOnceDifferentiable.apply(x['Cpre'] * x['U'] + x['H']),))
