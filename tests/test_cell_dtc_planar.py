"""``stc_cell_dtc_gates_planar_f32`` / ``stc_cell_dtc_cand_planar_f32`` (csrc/stc_cell_dtc_planar.hip, ABI v43; ``HipKernels.cell_dtc_gates`` /
``cell_dtc_cand``): the gradient of the category graph's Chebyshev stack from the planar cells, order 2, hidden 16.

    gates      V = [X|H] . Wg[block (0, 1)] + [SX|SH] . Wg[block (1, 1)],  dG = [dHnew (Cand - H) U (1 - U) | dRH H R (1 - R)]
               dTc[1][c][d] += sum_r sum_o V[r][c][o] dG[r][d][o]
    candidate  V0 = [X|RH] . Wc[block (0, 1)], V1 = [X|RH] . Wc[block (1, 1)]
               dTc[1][c][d] += sum_r sum_o V0[r][c][o] dY[r][d][o] + V1[r][c][o] dBm[r][d][o]            dBm = S^T dY

CPU part: header, ctypes table and EXPORTS agree; every refusal comes back before any HIP call (made-up addresses); the two formulas, written out
below with plain einsums (``gates_statement`` / ``cand_statement``), add up to autograd's gradient of a float64 STC_Cell built from two
``oracle.stc_oracle.bdg_dif`` on a one-way weighted graph -- the S^T dY identity included; the kernels use no scratch.

GPU part (-m gpu): C in {32, 64}, cin in {1, 3, 4, 16}, rows in {1, W - 1, W, W + 1, 2 W + 3} with W the workgroup's run of rows (a ragged last
slot, one full slot, more than two), planes of unequal magnitudes (x 1e-3 .. x 1e2), U and R in (0, 1).  Bound against the float64 statement:
relative error <= max(1e-6, 3 x the error of the same statement evaluated by torch in fp32) -- the noise rule of tests/test_mgp_front.py and
tests/test_scale_sweep.py; error and noise go side by side to parity_errors.tsv."""
import os
import re

import pytest
import torch

from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib
from tests.conftest import REPO, rel_err
from tests.launch_trips import log_parity

GATES, CAND = 'stc_cell_dtc_gates_planar_f32', 'stc_cell_dtc_cand_planar_f32'
FLOOR, FACTOR = 1e-6, 3.0


# ============================================================================================================== the float64 statement
def gates_statement(X, H, SX, SH, Wg, U, R, Cand, dHnew, dRH):
    """(C, C) in the operands' own precision: the gates convolution's share of dTc[1]; planes (rows, C, w), Wg (4 L, 2 h)."""
    L = X.shape[-1] + H.shape[-1]
    block = lambda n: Wg[(2 * n + 1) * L:(2 * n + 2) * L]                         # (n, kc = 1)
    V = torch.einsum('rcl,lo->rco', torch.cat([X, H], -1), block(0)) + torch.einsum('rcl,lo->rco', torch.cat([SX, SH], -1), block(1))
    dG = torch.cat([dHnew * (Cand - H) * U * (1 - U), dRH * H * R * (1 - R)], -1)
    return torch.einsum('rco,rdo->cd', V, dG)


def cand_statement(X, RH, Wc, dY, dBm):
    """(C, C): the candidate convolution's share of dTc[1] in its post-aggregation form."""
    L = X.shape[-1] + RH.shape[-1]
    Z = torch.cat([X, RH], -1)
    V0, V1 = (torch.einsum('rcl,lo->rco', Z, Wc[(2 * n + 1) * L:(2 * n + 2) * L]) for n in (0, 1))
    return torch.einsum('rco,rdo->cd', V0, dY) + torch.einsum('rco,rdo->cd', V1, dBm)


class DtcTwin(EmulatedKernels):
    """The CPU twin with the two products, in the operands' own precision: the whole share goes to slot 0."""

    def cell_dtc_gates(self, X, H, SX, SH, Wg, U, Rg, Cand, dHnew, dRH, partials):
        partials[0] += gates_statement(X, H, SX, SH, Wg, U, Rg, Cand, dHnew, dRH).to(partials.dtype)

    def cell_dtc_cand(self, X, RH, Wc, dY, dBm, partials):
        partials[0] += cand_statement(X, RH, Wc, dY, dBm).to(partials.dtype)


def planes(rows, C, cin, seed=0, h=16):
    """The operands of both launches as float32 CPU tensors: planes of unequal magnitudes, gates in (0, 1), Cand in (-1, 1)."""
    g = torch.Generator().manual_seed(7919 * rows + 31 * C + cin + seed)
    rn = lambda w, scale: torch.randn(rows, C, w, generator=g) * scale
    L = cin + h
    d = dict(X=rn(cin, 1e2), H=rn(h, 1.0), SX=rn(cin, 1e-1), SH=rn(h, 10.0), Wg=torch.randn(4 * L, 2 * h, generator=g) * 0.1,
             U=torch.sigmoid(rn(h, 2.0)), R=torch.sigmoid(rn(h, 2.0)), Cand=torch.tanh(rn(h, 1.0)), dHnew=rn(h, 1e-3), dRH=rn(h, 1e2),
             RH=rn(h, 1e-2), Wc=torch.randn(4 * L, h, generator=g) * 0.3, dY=rn(h, 1e1), dBm=rn(h, 1e-3))
    return d


GATE_ARGS = ('X', 'H', 'SX', 'SH', 'Wg', 'U', 'R', 'Cand', 'dHnew', 'dRH')
CAND_ARGS = ('X', 'RH', 'Wc', 'dY', 'dBm')


# ============================================================================================================== CPU
def test_header_table_and_exports_agree():
    header = open(os.path.join(REPO, 'include', 'stc_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry, n_args in ((GATES, 15), (CAND, 10), ('stc_cell_dtc_planar_supported', 3), ('stc_cell_dtc_planar_slots', 1)):
        assert re.search(rf'\b{entry}\s*\(', code) and entry in _lib._ABI and entry in _lib.EXPORTS
        proto = re.search(rf'{entry}\s*\((.*?)\)\s*;', code, flags=re.S).group(1)
        assert len(proto.split(',')) == len(_lib._ABI[entry][1]) == n_args, entry
    assert re.findall(r'^#define\s+STC_ABI_VERSION\s+(\d+)\b', header, flags=re.M) == [str(_lib.ABI_VERSION)]
    assert _lib.load_library().stc_version() == _lib.ABI_VERSION >= 43
    for method in ('cell_dtc_planar_supported', 'cell_dtc_slots', 'cell_dtc_gates', 'cell_dtc_cand'):
        assert hasattr(_lib.HipKernels, method) and not hasattr(EmulatedKernels, method)      # the CPU twin does not get them
    assert _lib.HipKernels.cell_dtc_planar is True and not hasattr(EmulatedKernels, 'cell_dtc_planar')   # on the class: ``for_graph`` views have it
    assert 'stc_cell_dtc_planar.hip' in open(os.path.join(REPO, 'stc-gnn_amd', 'csrc', 'Makefile')).read()


def test_the_shape_predicate_and_the_slot_rule():
    lib = _lib.load_library()
    ok = lib.stc_cell_dtc_planar_supported
    assert all(ok(C, cin, 16) for C in (32, 64) for cin in (1, 2, 3, 4, 16))
    assert not any(ok(C, 16, 16) for C in (0, 5, 8, 16, 33, 48, 128)) and not any(ok(32, cin, 16) for cin in (-1, 0, 5, 8, 15, 17, 32))
    assert not ok(32, 16, 8) and not ok(64, 16, 32)
    slots = lib.stc_cell_dtc_planar_slots
    W = run_of_rows()
    assert [slots(r) for r in (-5, 0, 1, W - 1, W, W + 1, 2 * W, 2 * W + 3, 10 ** 6)] == [0, 0, 1, 1, 1, 2, 2, 3, -(-10 ** 6 // W)]


def run_of_rows():
    """W: the consecutive rows one workgroup owns = rows per slot, read off the library's own slot rule."""
    slots = _lib.load_library().stc_cell_dtc_planar_slots
    return next(r for r in range(1, 1 << 16) if slots(r + 1) == 2)


_GATE_PTR = dict(X=0x10000, H=0x20000, SX=0x30000, SH=0x40000, Wg=0x50000, U=0x60000, R=0x70000, Cand=0x80000, dHnew=0x90000, dRH=0xA0000, partials=0xB0000)
_CAND_PTR = dict(X=0x10000, RH=0x20000, Wc=0x30000, dY=0x40000, dBm=0x50000, partials=0x60000)


def _gates(lib, cin=16, rows=10, C=32, **over):
    p = dict(_GATE_PTR, **over)
    return lib.stc_cell_dtc_gates_planar_f32(p['X'], cin, p['H'], p['SX'], p['SH'], p['Wg'], p['U'], p['R'], p['Cand'], p['dHnew'], p['dRH'], p['partials'], rows, C, None)


def _cand(lib, cin=16, rows=10, C=32, **over):
    p = dict(_CAND_PTR, **over)
    return lib.stc_cell_dtc_cand_planar_f32(p['X'], cin, p['RH'], p['Wc'], p['dY'], p['dBm'], p['partials'], rows, C, None)


@pytest.mark.parametrize('call,ptrs', [(_gates, _GATE_PTR), (_cand, _CAND_PTR)], ids=['gates', 'cand'])
def test_refusals_come_before_any_hip_call(call, ptrs):
    """Made-up addresses throughout: a call that got as far as a launch would fault, a refusal never touches them."""
    lib = _lib.load_library()
    err = lambda: lib.stc_last_error()
    EINVAL, EALIGN = -1, -2
    for name in ptrs:
        assert call(lib, **{name: None}) == EINVAL and b'null' in err(), name
    for name in ptrs:
        off = 2 if name in ('Wg', 'Wc') else 4                         # (the weights are read by the float, partials by the double)
        assert call(lib, **{name: ptrs[name] + off}) == EALIGN and b'aligned' in err(), name
    for name in ('X', 'SX'):                                           # a narrow input plane is read by the float: 4-byte aligned is enough ...
        if name in ptrs:
            assert call(lib, cin=3, **{name: ptrs[name] + 2}) == EALIGN, name
    for C in (16, 0, 48, 128):
        assert call(lib, C=C) == EINVAL and b'C in (32, 64)' in err(), C
    for cin in (5, 0, -1, 8, 17):
        assert call(lib, cin=cin) == EINVAL and b'cin' in err(), cin
    assert not lib.stc_cell_dtc_planar_supported(32, 16, 8)            # (hidden 8: the entry points take no width, the predicate refuses it)
    assert call(lib, rows=-1) == EINVAL and b'rows' in err()
    assert call(lib, rows=1 << 31) == EINVAL and b'rows' in err()
    assert call(lib, rows=0) == 0                                      # launches nothing
    assert call(lib, rows=0, **{name: None for name in ptrs}) == 0


def test_the_statement_is_autograds_gradient_of_a_float64_cell():
    """dTc[1] = dGc at order 2.  A float64 STC_Cell from two ``bdg_dif`` of the oracle on a ONE-WAY weighted graph (Gs strictly upper
    triangular: S != S^T); the planes the executor would hold are rebuilt from it, dBm = S^T dY with S = Gs^T the aggregation."""
    g = torch.Generator().manual_seed(5)
    B, N, C, cin, h = 2, 5, 3, 2, 4
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Gs = torch.triu(torch.rand(N, N, generator=g, dtype=torch.float64), 1)
    Gc = rn(C, C).mul(0.5).requires_grad_()
    X, H, dHnew = rn(B, N, C, cin), rn(B, N, C, h), rn(B, N, C, h)
    L = cin + h
    Wg, bg, Wc, bc = rn(4 * L, 2 * h) * 0.3, rn(2 * h), rn(4 * L, h) * 0.3, rn(h)
    pre = O.bdg_dif(torch.cat([X, H], -1), Gs, Gc, Wg, bg, 2, 2)
    U, R = (torch.sigmoid(t) for t in torch.split(pre, h, dim=-1))
    RH = R * H
    RH.retain_grad()
    Cand = torch.tanh(O.bdg_dif(torch.cat([X, RH], -1), Gs, Gc, Wc, bc, 2, 2))
    Hnew = (1.0 - U) * H + U * Cand
    (Hnew * dHnew).sum().backward()
    agg = lambda t: torch.einsum('bncl,nm->bmcl', t, Gs)                # S.t: the 1-mode product of the reference
    dY = (dHnew * U * (1 - Cand ** 2)).detach()
    dBm = torch.einsum('bmcl,nm->bncl', dY, Gs)                        # S^T dY
    r = lambda t: t.detach().reshape(B * N, C, -1)
    got = (gates_statement(*map(r, (X, H, agg(X), agg(H))), Wg, *map(r, (U, R, Cand, dHnew, RH.grad)))
           + cand_statement(r(X), r(RH), Wc, r(dY), r(dBm)))
    assert rel_err(got, Gc.grad) < 1e-13, rel_err(got, Gc.grad)
    assert rel_err(dBm, agg(dY)) > 0.1                                 # (the graph is one-way: aggregating dY the forward way is another plane)
    twin, part = DtcTwin(), torch.zeros(1, C, C, dtype=torch.float64)
    twin.cell_dtc_gates(*map(r, (X, H, agg(X), agg(H))), Wg, *map(r, (U, R, Cand, dHnew, RH.grad)), part)
    twin.cell_dtc_cand(r(X), r(RH), Wc, r(dY), r(dBm), part)
    assert torch.equal(part[0], got)


def test_the_kernels_use_no_scratch(tmp_path):
    from tests.test_first_step_isa import _resource_usage
    from tests.test_isa import HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not present')
    usage = _resource_usage('stc_cell_dtc_planar.hip', tmp_path)
    assert len(usage) == 8, sorted(usage)                              # C in {32, 64} x wide / narrow input x gates / candidate
    for name, u in usage.items():
        assert u['ScratchSize'] == 0 and u['LDS Size'] <= 64 * 1024, (name, u)


# ============================================================================================================== GPU
@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


def _launch(hip, d, which, part=None):
    C = d['H'].shape[1]
    part = torch.zeros(hip.cell_dtc_slots(d['H'].shape[0]), C, C, dtype=torch.float64, device='cuda') if part is None else part
    if 'gates' in which:
        hip.cell_dtc_gates(*[d[n] for n in GATE_ARGS], part)
    if 'cand' in which:
        hip.cell_dtc_cand(*[d[n] for n in CAND_ARGS], part)
    return part


def _statement(d, which, dtype):
    t = {n: v.to(dtype) for n, v in d.items()}
    fn, args = (gates_statement, GATE_ARGS) if which == 'gates' else (cand_statement, CAND_ARGS)
    return fn(*[t[n] for n in args])


_W = 256      # (asserted against the library's slot rule in the test itself: the parametrisation needs it at collection time)
_ROWS = (1, _W - 1, _W, _W + 1, 2 * _W + 3)


@pytest.mark.gpu
@pytest.mark.parametrize('C', (32, 64))
@pytest.mark.parametrize('cin', (1, 3, 4, 16))
@pytest.mark.parametrize('rows', _ROWS)
def test_parity_with_the_float64_statement(hip, rows, cin, C):
    assert run_of_rows() == _W
    d = planes(rows, C, cin)
    dev = {n: v.cuda() for n, v in d.items()}
    for which in ('gates', 'cand'):
        want, fp32 = _statement(d, which, torch.float64), _statement(d, which, torch.float32)
        part = _launch(hip, dev, (which,))
        assert part.shape == (-(-rows // _W), C, C) and part.dtype == torch.float64
        err, noise = rel_err(part.sum(0), want), rel_err(fp32, want)
        bound = max(FLOOR, FACTOR * noise)
        print(f'cell_dtc {which} C={C} cin={cin} rows={rows}: {err:.3e} from float64, fp32 torch {noise:.3e} (bound {bound:.1e})')
        log_parity(f'cell_dtc_{which} C={C} cin={cin} rows={rows}', err, noise, FACTOR, bound)
        assert err <= bound, (which, err, noise)


@pytest.mark.gpu
@pytest.mark.parametrize('C,cin,rows', [(32, 16, 2 * _W + 3), (64, 3, _W + 1)])
def test_launches_add_and_the_fold_leaves_dtc0_zero(hip, C, cin, rows):
    """Two launches into one ``partials`` buffer give the sum of the two, bit for bit; slots past the last row's do not exist; the fold
    (``ops._dtc_fold``) writes dTc[0] as exact zeros; two runs give the same bits, eager and replayed."""
    from stc_hip import ops
    d = {n: v.cuda() for n, v in planes(rows, C, cin).items()}
    gates, cand = _launch(hip, d, ('gates',)), _launch(hip, d, ('cand',))
    both = _launch(hip, d, ('gates', 'cand'))
    assert torch.equal(both, gates + cand) and bool((gates != 0).any()) and bool((cand != 0).any())
    assert torch.equal(_launch(hip, d, ('gates', 'cand')), both)
    dTc = ops._dtc_fold(both, torch.empty(2, C, C, device='cuda'))
    assert dTc.shape == (2, C, C) and dTc.dtype == torch.float32 and float(dTc[0].abs().max()) == 0.0
    assert torch.equal(dTc[1], both.sum(0).float())
    static = torch.zeros_like(both)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _launch(hip, d, ('gates', 'cand'), static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static.zero_()
        _launch(hip, d, ('gates', 'cand'), static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, both)


@pytest.mark.gpu
@pytest.mark.parametrize('C,cin', [(32, 4), (64, 16)])
def test_a_nan_is_not_masked_and_leaves_nothing_behind(hip, C, cin):
    rows = _W + 5
    d = {n: v.cuda() for n, v in planes(rows, C, cin).items()}
    clean = _launch(hip, d, ('gates', 'cand'))
    bad = dict(d, dHnew=d['dHnew'].clone())
    bad['dHnew'][_W + 2] = float('nan')                                # one row, in the second slot
    got = _launch(hip, bad, ('gates',))
    assert not bool(torch.isfinite(got[1]).any()) and torch.equal(got[0], _launch(hip, d, ('gates',))[0])
    assert torch.equal(_launch(hip, d, ('gates', 'cand')), clean)      # a NaN-free run after it: the clean bits


@pytest.mark.gpu
def test_the_front_refuses_what_the_kernels_do_not_take(hip):
    d = {n: v.cuda() for n, v in planes(3, 32, 16).items()}
    part = torch.zeros(1, 32, 32, dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.StcError, match='partials'):
        hip.cell_dtc_cand(*[d[n] for n in CAND_ARGS], part.float())
    with pytest.raises(_lib.StcError, match='partials'):
        hip.cell_dtc_cand(*[d[n] for n in CAND_ARGS], torch.zeros(2, 32, 32, dtype=torch.float64, device='cuda'))
    with pytest.raises(_lib.StcError, match='plane'):
        hip.cell_dtc_gates(*[d[n][:2] if n == 'U' else d[n] for n in GATE_ARGS], part)
    with pytest.raises(_lib.StcError, match='C in'):
        hip.cell_dtc_cand(*[d[n][:, :16].contiguous() if d[n].dim() == 3 else d[n] for n in CAND_ARGS], part)
    with pytest.raises(_lib.StcError, match='ROCm'):
        hip.cell_dtc_cand(*[d[n].cpu() if n == 'dY' else d[n] for n in CAND_ARGS], part)
    assert not hip.cell_dtc_planar_supported(32, 16, 8) and hip.cell_dtc_planar_supported(64, 3, 16) and hip.cell_dtc_slots(0) == 0
