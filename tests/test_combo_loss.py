"""``ComboLoss`` on the fused HIP kernels (``csrc/stc_loss.hip``, ABI v39: ``stc_combo_loss_fwd_f32`` / ``stc_combo_loss_bwd_f32``).

CPU part: the header, the ctypes table and ``LOSS_CHUNK`` agree; the workspace query follows its formula; every refusal comes back before
any HIP call with its own message; the routing predicate and the (batch, segments, seg) view builder; on CPU tensors ``ComboLoss`` is the
torch arithmetic of ``oracle.stc_oracle.combo_loss`` bit for bit.

GPU part (-m gpu): loss and gradient against the float64 oracle on the smallest shapes that reach each path of the kernels (vector and scalar
accesses, ragged and exact chunks, several samples and segments, the model's transposed view, a misaligned base); p of exactly 0 / 1 and
the poison values against the arithmetic contract of include/stc_hip.h written out in float64; bitwise reproducibility, eager against
HIP-graph replay; the autograd contract; one model step with the fused route on and off.

Bounds.  Loss: relative 1e-6 -- the per-element terms are the only fp32 roundings and all have one sign, so the sum's relative error is
that of a term (a few ulp of logf and a product) plus the final rounding; 1e-6 is about twice that.  Gradient: ``rel_err`` below ``TOL`` of
tests/test_hip_kernels.py, the project's bound for fp32 kernels against float64."""
import os
import re

import pytest
import torch

from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib, loss as L, ops
from stc_hip.loss import ComboLoss
from tests.conftest import REPO, rel_err
from tests.launch_trace import Traced
from tests.test_hip_kernels import TOL

CHUNK = _lib.LOSS_CHUNK
LOSS_RTOL = 1e-6
ENTRIES = ('stc_combo_loss_workspace_bytes', 'stc_combo_loss_fwd_f32', 'stc_combo_loss_bwd_f32')


# ============================================================================================================== CPU
def test_header_table_and_chunk_agree():
    header = open(os.path.join(REPO, 'include', 'stc_hip.h')).read()
    assert re.findall(r'^#define\s+STC_LOSS_CHUNK\s+(\d+)\b', header, flags=re.M) == [str(_lib.LOSS_CHUNK)]
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ENTRIES:
        assert re.search(rf'\b{name}\s*\(', code), f'{name} is not declared in include/stc_hip.h'
        assert name in _lib._ABI
    lib = _lib.load_library()
    assert lib.stc_version() == _lib.ABI_VERSION >= 39
    assert _lib.HipKernels.combo_loss is True and not hasattr(EmulatedKernels, 'combo_loss')


@pytest.mark.parametrize('batch,segments,seg', [(1, 1, 1), (32, 3, 500), (2, 2, CHUNK), (2, 2, CHUNK + 1), (3, 1, 5 * CHUNK - 7), (4, 0, 9), (0, 3, 9)])
def test_workspace_bytes_follow_the_formula(batch, segments, seg):
    lib = _lib.load_library()
    blocks = batch * segments * -(-seg // CHUNK)                  # three doubles per chunk + one per sample; nothing for a shape that launches nothing
    assert lib.stc_combo_loss_workspace_bytes(batch, segments, seg) == (8 * (3 * blocks + batch) if blocks else 0)


def test_workspace_bytes_of_refused_sizes_are_zero():
    lib = _lib.load_library()
    assert lib.stc_combo_loss_workspace_bytes(-1, 1, 1) == 0
    assert lib.stc_combo_loss_workspace_bytes(1 << 31, 1, 1) == 0


def _fwd(lib, p=0x1000, y=0x2000, sizes=(2, 3, 8), strides=(24, 8, 24, 8), loss=0x3000, sums=0x4000, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.stc_combo_loss_workspace_bytes(*sizes)
    return lib.stc_combo_loss_fwd_f32(p, y, *sizes, *strides, loss, sums, ws, ws_bytes, None)


def _bwd(lib, p=0x1000, y=0x2000, sums=0x4000, g=0x3000, dp=0x6000, sizes=(2, 3, 8), strides=(24, 8, 24, 8)):
    return lib.stc_combo_loss_bwd_f32(p, y, sums, g, dp, *sizes, *strides, None)


def test_refusals_come_before_any_hip_call():
    """Made-up addresses throughout: a call that got as far as a launch would fault, a refusal never touches them."""
    lib = _lib.load_library()
    err = lambda: lib.stc_last_error()
    for call in (_fwd, _bwd):
        assert call(lib, sizes=(-2, 3, 8)) == -1 and b'negative' in err()
        assert call(lib, sizes=(2, 3, -8)) == -1 and b'negative' in err()
        assert call(lib, strides=(24, 8, -24, 8)) == -1 and b'negative' in err()
        assert call(lib, p=None) == -1 and b'null' in err()
        assert call(lib, y=None) == -1 and b'null' in err()
        assert call(lib, sums=None) == -1 and b'null' in err()
        assert call(lib, p=0x1002) == -2 and b'4-byte' in err()
        assert call(lib, sums=0x4004) == -2 and b'8-byte' in err()
        assert call(lib, sizes=(1 << 31, 1, 1), strides=(1, 1, 1, 1)) == _lib.STC_ELIMIT and b'2^31' in err()
        assert call(lib, sizes=(1 << 20, 1 << 20, CHUNK + 1), strides=(1, 1, 1, 1)) == _lib.STC_ELIMIT and b'2^31' in err()
    assert _fwd(lib, loss=None) == -1 and b'null' in err()
    assert _fwd(lib, ws=None) == -1 and b'null' in err()
    assert _fwd(lib, ws=0x5004) == -2 and b'8-byte' in err()
    need = lib.stc_combo_loss_workspace_bytes(2, 3, 8)
    assert _fwd(lib, ws_bytes=need - 1) == -1 and b'workspace' in err() and str(need).encode() in err()
    assert _bwd(lib, g=None) == -1 and b'null' in err()
    assert _bwd(lib, dp=None) == -1 and b'null' in err()
    assert _bwd(lib, dp=0x6001) == -2 and b'4-byte' in err()
    assert _bwd(lib, dp=0x1000) == -1 and b'alias' in err()


@pytest.mark.parametrize('sizes', [(0, 3, 8), (2, 0, 8), (2, 3, 0)])
def test_a_zero_size_call_returns_zero_without_a_launch(sizes):
    lib = _lib.load_library()
    assert lib.stc_combo_loss_fwd_f32(None, None, *sizes, 0, 0, 0, 0, None, None, None, 0, None) == 0
    assert lib.stc_combo_loss_bwd_f32(None, None, None, None, None, *sizes, 0, 0, 0, 0, None) == 0


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g).clamp(0.01, 0.99), (torch.rand(*shape, generator=g) < 0.3).float()


def test_the_view_builder_names_runs_without_a_copy():
    t = torch.arange(3 * 4 * 20 * 5, dtype=torch.float32).reshape(3, 4, 20, 5)
    for view, want in ((t, (3, 4, 100, 400, 100)), (t.transpose(0, 1), (4, 3, 100, 100, 400)), (t[:, 1:3], (3, 2, 100, 400, 100)),
                       (t[:, :, 0], (3, 4, 5, 400, 100)), (t.reshape(3, 400), (3, 1, 400, 400, 400)), (t.reshape(-1), (1200, 1, 1, 1, 1)),
                       (t[:1].transpose(0, 1), (4, 1, 100, 100, 100))):
        v3 = L._as3(view)
        assert v3 is not None and tuple(v3.shape) + tuple(v3.stride()[:2]) == want and v3.stride(2) == 1
        assert v3.data_ptr() == view.data_ptr() and torch.equal(v3.reshape(view.shape), view)
    for bad in (t[..., ::2], t[:, :, ::2], t.reshape(3, 400).t(), t.reshape(3, 400)[:, ::2], t[0, 0, 0].expand(3, 4, 5), t[:, :1].expand(3, 4, 20, 5),
                torch.tensor(1.0)):
        assert L._as3(bad) is None


def test_the_predicate_refuses_what_the_kernels_do_not_take(monkeypatch):
    monkeypatch.setattr(ops, '_kernels', None)
    p, y = _pair((3, 2, 12, 3))
    cases = dict(cpu=(p, y), y_grad=(p, y.clone().requires_grad_()), f64=(p.double(), y.double()), mixed=(p, y.double()), shape=(p, y[:, :1]),
                 empty=(p[:0], y[:0]), strided=(p[..., ::2], y[..., ::2]))
    for name, (a, b) in cases.items():
        assert not L.combo_loss_supported(a, b), name
    assert ops._kernels is None                                  # CPU tensors never bring the kernel set up


def test_on_cpu_tensors_the_loss_is_the_oracle_arithmetic_bit_for_bit():
    p, y = _pair((3, 2, 12, 3))
    for view in (lambda t: t, lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)):
        a, b = view(p).clone().requires_grad_(), p.clone().requires_grad_()
        la, lb = ComboLoss()(a, view(y)), O.combo_loss(b, y)
        assert 'ComboLossFused' not in type(la.grad_fn).__name__
        la.backward()
        lb.backward()
        assert torch.equal(la.detach(), lb.detach()) and torch.equal(a.grad, b.grad)


def test_the_loss_kernels_use_no_scratch(tmp_path):
    """The five kernels of csrc/stc_loss.hip as the compiler reports them with the library's own flags (needs hipcc, no GPU)."""
    from tests.test_first_step_isa import _resource_usage
    from tests.test_isa import HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not present')
    usage = _resource_usage('stc_loss.hip', tmp_path)
    assert len(usage) == 5 and sum('loss_partials_kernel' in k for k in usage) == 2 and sum('loss_bwd_kernel' in k for k in usage) == 2, sorted(usage)
    for name, u in usage.items():
        assert u['ScratchSize'] == 0, (name, u)


# ============================================================================================================== GPU
@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.fixture
def traced(hip, monkeypatch):
    k = Traced(hip)
    monkeypatch.setattr(ops, '_kernels', k)
    monkeypatch.setattr(L, '_FUSED', True)
    return k


def _names(k):
    return [entry[0] for entry in k._log]


def _on_device(values, layout):
    """``values`` (CPU, contiguous) on the device in the named layout, same logical shape."""
    if layout == 'plain':
        return values.cuda()
    if layout == 'transposed':                                   # the model's: a (horizon, B, N, C) tensor seen as (B, horizon, N, C)
        return values.transpose(0, 1).contiguous().cuda().transpose(0, 1)
    assert layout == 'offset'                                    # one float into a larger buffer: 4-byte aligned, not 16
    buf = torch.zeros(values.numel() + 5, device='cuda')
    view = buf[1:1 + values.numel()].view(values.shape)
    view.copy_(values)
    assert view.data_ptr() % 16 == 4
    return view


SHAPES = {
    'smallest': ((1, 1), 'plain'),
    'samples-and-segments': ((3, 2, 12, 3), 'plain'),
    'seg35-scalar-tail': ((2, 3, 5, 7), 'plain'),
    'two-chunks-ragged-scalar': ((2, 2, CHUNK + 5), 'plain'),
    'exact-chunks-vector': ((2, 2, 2 * CHUNK), 'plain'),
    'two-d-four-chunks': ((1, 4 * CHUNK), 'plain'),
    'model-transposed-view': ((4, 3, 20, 5), 'transposed'),
    'misaligned-base': ((2, 2, 8), 'offset'),
}
_ORACLE = {}


def _oracle(sid):
    """(p, y, loss, dp) of one shape: the float64 oracle on the CPU, computed once."""
    if sid not in _ORACLE:
        shape, _ = SHAPES[sid]
        p, y = _pair(shape, seed=len(sid))
        pd = p.double().requires_grad_()
        want = O.combo_loss(pd, y.double())
        want.backward()
        _ORACLE[sid] = (p, y, want.detach(), pd.grad)
    return _ORACLE[sid]


def _loss_err(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


@pytest.mark.gpu
@pytest.mark.parametrize('sid', list(SHAPES))
def test_loss_and_gradient_against_the_float64_oracle(traced, sid):
    p, y, want, want_dp = _oracle(sid)
    layout = SHAPES[sid][1]
    pg, yg = _on_device(p, layout).requires_grad_(), _on_device(y, layout)
    assert L.combo_loss_supported(pg, yg)
    loss = ComboLoss()(pg, yg)
    loss.backward()
    torch.cuda.synchronize()
    e_loss, e_dp = _loss_err(loss.detach(), want), rel_err(pg.grad, want_dp)
    print(f'{sid}: loss rel {e_loss:.2e}, dp rel_err {e_dp:.2e}')
    assert _names(traced) == ['combo_loss_fwd', 'combo_loss_bwd']
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert e_loss < LOSS_RTOL and e_dp < TOL
    assert pg.grad.stride() == pg.stride()
    if layout == 'transposed':
        assert not pg.grad.is_contiguous() and pg.grad.transpose(0, 1).is_contiguous()


@pytest.mark.gpu
def test_an_upstream_factor_reaches_the_gradient(traced):
    p, y, want, want_dp = _oracle('seg35-scalar-tail')
    pg = p.cuda().requires_grad_()
    (ComboLoss()(pg, y.cuda()) * 0.37).backward()
    assert _names(traced) == ['combo_loss_fwd', 'combo_loss_bwd']
    assert rel_err(pg.grad, 0.37 * want_dp) < TOL


@pytest.mark.gpu
def test_a_prediction_without_grad_makes_no_backward_launch(traced):
    p, y, want, _ = _oracle('samples-and-segments')
    loss = ComboLoss()(p.cuda(), y.cuda())
    assert loss.grad_fn is None and not loss.requires_grad and _loss_err(loss, want) < LOSS_RTOL
    pg = p.cuda().requires_grad_()
    with torch.no_grad():
        quiet = ComboLoss()(pg, y.cuda())
    assert quiet.grad_fn is None and torch.equal(quiet, loss)
    assert _names(traced) == ['combo_loss_fwd', 'combo_loss_fwd']


@pytest.mark.gpu
def test_the_predicate_on_device_tensors(hip, monkeypatch):
    p, y = (t.cuda() for t in _pair((3, 2, 12, 3)))
    monkeypatch.setattr(ops, '_kernels', hip)
    assert L.combo_loss_supported(p, y) and L.combo_loss_supported(p.transpose(0, 1), y.transpose(0, 1))
    assert not L.combo_loss_supported(p, y.clone().requires_grad_())
    assert not L.combo_loss_supported(p, y.cpu()) and not L.combo_loss_supported(p.double(), y.double())
    assert not L.combo_loss_supported(p[..., ::2], y[..., ::2]) and not L.combo_loss_supported(p[:0], y[:0])
    monkeypatch.setattr(L, '_FUSED', False)
    assert not L.combo_loss_supported(p, y)
    monkeypatch.setattr(L, '_FUSED', True)
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())       # a kernel set without ``combo_loss``: the CPU twin
    assert not L.combo_loss_supported(p, y)


@pytest.mark.gpu
def test_a_target_that_requires_grad_keeps_its_gradient(traced):
    p, y = _pair((3, 2, 12, 3))
    pg, yg = p.cuda().requires_grad_(), (0.5 * y + 0.25).cuda().requires_grad_()
    ComboLoss()(pg, yg).backward()
    assert _names(traced) == [] and yg.grad is not None and bool(yg.grad.abs().sum() > 0)


# ---- the arithmetic contract written out in float64 ------------------------------------------------------------------------------------------------
def _contract(p, y):
    """(loss, dp) of include/stc_hip.h "ComboLoss" in float64 from fp32-valued operands (batch, ...); non-finite values go through as they are."""
    p, y = p.double(), y.double()
    batch, m = p.shape[0], p.numel()
    clamp = lambda v, lo: torch.where(v < lo, torch.full_like(v, lo), v)
    bce = -(y * clamp(torch.log(p), -100.0) + (1 - y) * clamp(torch.log(1 - p), -100.0))
    dims = tuple(range(1, p.dim()))
    I, D = (p * y).sum(dims, keepdim=True), (p + y).sum(dims, keepdim=True)
    loss = bce.sum() / m + (1 - 2 * I / D).sum() / batch
    dp = (p - y) / clamp(p * (1 - p), 1e-12) / m - (2.0 / batch) * (y * D - I) / D ** 2
    return loss, dp


@pytest.mark.gpu
def test_predictions_of_exactly_zero_and_one(traced):
    p, y = _pair((2, 3, 40), seed=3)
    for b in (0, 1):
        p[b, 1, 4:8] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        y[b, 1, 4:8] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    want, want_dp = _contract(p, y)
    assert torch.isfinite(want) and torch.isfinite(want_dp).all()
    pg = p.cuda().requires_grad_()
    loss = ComboLoss()(pg, y.cuda())
    loss.backward()
    got = pg.grad.double().cpu()
    assert _loss_err(loss.detach(), want) < LOSS_RTOL
    big = want_dp.abs() > 1e6                                     # the two clamped denominators per sample: +-1e12 / M
    assert int(big.sum()) == 4 and torch.isfinite(got).all()
    assert rel_err(got[~big], want_dp[~big]) < TOL
    assert bool(((got[big] - want_dp[big]).abs() <= TOL * want_dp[big].abs()).all())


@pytest.mark.gpu
@pytest.mark.parametrize('poison', [float('nan'), -0.1, 1.5, float('inf')], ids=['nan', 'below0', 'above1', 'inf'])
def test_a_poisoned_prediction_flags_its_sample_and_no_other(traced, poison):
    p, y = _pair((2, 3, 40), seed=4)
    clean = p.cuda().requires_grad_()
    ComboLoss()(clean, y.cuda()).backward()
    p[0, 1, 7] = poison
    _, want_dp = _contract(p, y)
    pg = p.cuda().requires_grad_()
    loss = ComboLoss()(pg, y.cuda())
    loss.backward()
    torch.cuda.synchronize()                                      # no device assert fired
    assert bool(torch.isnan(loss))
    assert not torch.isfinite(pg.grad[0]).any(), 'sample 0 must be flagged as a whole'
    assert torch.isfinite(pg.grad[1]).all() and rel_err(pg.grad[1], want_dp[1]) < TOL
    assert torch.equal(pg.grad[1], clean.grad[1])                 # the loss is the only value shared across samples
    assert _names(traced) == ['combo_loss_fwd', 'combo_loss_bwd'] * 2


@pytest.mark.gpu
def test_a_sample_of_zero_mass_gives_nan_as_the_reference_does(traced):
    p, y = torch.zeros(2, 8), torch.zeros(2, 8)
    p[1], y[1, 0] = 0.5, 1.0
    loss = ComboLoss()(p.cuda(), y.cuda())
    assert bool(torch.isnan(loss))


# ---- reproducibility and capture -------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.gpu
def test_eager_runs_and_graph_replays_give_the_same_bits(traced):
    shape = (2, 2, CHUNK + 5)
    first, second = _pair(shape, seed=11), _pair(shape, seed=12)
    crit = ComboLoss()

    def eager(p, y):
        pg = p.cuda().requires_grad_()
        loss = crit(pg, y.cuda())
        loss.backward()
        return _bits(loss).clone(), _bits(pg.grad).clone()

    a, b = eager(*second), eager(*second)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    sp, sy = first[0].cuda().requires_grad_(), first[1].cuda()

    def step():
        sp.grad = None
        loss = crit(sp, sy)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = step()
    static_grad = sp.grad
    with torch.no_grad():
        sp.copy_(second[0])
        sy.copy_(second[1])
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(static_loss), a[0]) and torch.equal(_bits(static_grad), a[1])


# ---- autograd contract -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_operands_keep_their_bits_and_the_gradient_is_its_own_tensor(traced):
    p, y = _pair((4, 3, 20, 5), seed=5)
    pg, yg = _on_device(p, 'transposed').requires_grad_(), _on_device(y, 'transposed')
    g = torch.tensor(0.37, device='cuda')
    before = [_bits(t).clone() for t in (pg, yg, g)]
    loss = ComboLoss()(pg, yg)
    (dp,) = torch.autograd.grad(loss, pg, g, retain_graph=False)
    torch.cuda.synchronize()
    for t, bits in zip((pg, yg, g), before):
        assert torch.equal(_bits(t), bits)
    assert dp.untyped_storage().data_ptr() != pg.untyped_storage().data_ptr() and dp.data_ptr() != yg.data_ptr()
    with pytest.raises(RuntimeError, match='second time|already been freed'):
        torch.autograd.grad(loss, pg, g)


@pytest.mark.gpu
def test_a_zero_upstream_gradient_gives_zeros(traced):
    p, y, _, _ = _oracle('samples-and-segments')
    pg = p.cuda().requires_grad_()
    (ComboLoss()(pg, y.cuda()) * 0.0).backward()
    assert _names(traced) == ['combo_loss_fwd', 'combo_loss_bwd'] and bool((pg.grad == 0).all())


# ---- module level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_model_step_with_the_fused_loss_and_without(hip, monkeypatch):
    """The ``small`` family of tests/test_nonfinite.py: every parameter gradient agrees between the two routes; the fused route copies no
    prediction and hands the head's backward a contiguous gradient."""
    import STC_GNN as M
    from stc_hip import CsrGraph
    from torch.profiler import ProfilerActivity, profile
    monkeypatch.setattr(ops, '_kernels', hip)
    H, W, C, K, B, T, horizon = 12, 20, 5, 2, 2, 3, 2
    torch.manual_seed(0)
    graph = CsrGraph.queen_grid(H, W, normalize=True)
    model = M.STCGNN(H * W, C, K, K, 1, 16, 2, horizon, graph_mode='csr-fixed').cuda()
    g = torch.Generator().manual_seed(C + K)
    X = (torch.rand(B, T, H * W, C, generator=g) < 0.3).float().cuda()
    Y = (torch.rand(B, horizon, H * W, C, generator=g) < 0.3).float().cuda()
    Gc = torch.softmax(torch.randn(C, C, generator=g), -1).cuda()
    seen = []
    inner = ops._Head.backward
    monkeypatch.setattr(ops._Head, 'backward', staticmethod(lambda ctx, dy: (seen.append(dy.is_contiguous()), inner(ctx, dy))[1]))

    def run(fused):
        monkeypatch.setattr(L, '_FUSED', fused)
        model.zero_grad(set_to_none=True)
        yhat = model(X_seq=X, As=graph, Ac=Gc)
        assert tuple(yhat.shape) == (B, horizon, H * W, C) and not yhat.is_contiguous(), 'the model no longer hands over the transposed view'
        with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as prof:
            loss = ComboLoss()(yhat, Y)
            loss.backward()
            torch.cuda.synchronize()
        copies = [e for e in prof.events() if e.name in ('aten::copy_', 'aten::clone', 'aten::contiguous')
                  and e.input_shapes and e.input_shapes[0] and torch.Size(e.input_shapes[0]).numel() == yhat.numel()]
        return float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters()}, len(copies)

    loss_t, grads_t, copies_t = run(False)
    loss_f, grads_f, copies_f = run(True)
    print(f'prediction-sized copies: torch route {copies_t}, fused route {copies_f}; dy contiguous {seen}')
    assert abs(loss_f - loss_t) < 1e-6 * abs(loss_t) + 1e-7
    for name, want in grads_t.items():
        assert rel_err(grads_f[name], want) < TOL, name
    assert copies_f == 0 and copies_t > 0
    assert len(seen) == 2 and seen[1] is True
