"""``stc_cell_dsx_narrow_planar_f32`` (csrc/stc_cell_dsx_narrow.hip, ABI v44; ``HipKernels.cell_dsx_narrow``): the d(S.x) plane of a planar cell whose
input plane is narrow (cin = 1..4, layer 0) -- the plane the planar gates backward does not form, and that the value gradient of a learned sparse
spatial graph needs (``stc_graph_grad_csr_pairs_f32`` pairs it with x).  Order 2, hidden 16, C in {32, 64}:

    dSx[r][c][l] = sum_o dG[r][c][o] Wg[block (1, 0)][l][o] + sum_d Tc[1][c][d] sum_o dG[r][d][o] Wg[block (1, 1)][l][o]          l < cin
    dG = [dHnew (Cand - H) U (1 - U) | dRH H R (1 - R)]                                   (as stc_cell_dtc_gates_planar_f32 re-forms it)

CPU part: header, ctypes table and EXPORTS agree; every refusal comes back before any HIP call (made-up addresses); the statement, written below
with plain einsums, equals autograd's gradient with respect to S.x of a float64 STC_Cell whose gates convolution is built from
``oracle.stc_oracle.bdg_dif`` -- which pins the orientation of the T_c mix; the kernels use no scratch.

GPU part (-m gpu): C in {32, 64}, cin in {1, 2, 3, 4}, rows in {1, W - 1, W, W + 1, 2 W + 3} with W the workgroup's run of rows (read off
``stc_cell_dtc_planar_slots``), the operands of tests/test_cell_dtc_planar.py::planes.  Bound against the float64 statement: that file's rule,
relative error <= max(1e-6, 3 x the error of the same statement evaluated by torch in fp32); both go to parity_errors.tsv."""
import os
import re

import pytest
import torch

from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib
from tests.conftest import REPO, rel_err
from tests.launch_trips import log_parity
from tests.test_cell_dtc_planar import FACTOR, FLOOR, planes, run_of_rows

ENTRY = 'stc_cell_dsx_narrow_planar_f32'
ARGS = ('H', 'Wg', 'Tc', 'U', 'R', 'Cand', 'dHnew', 'dRH')


# ============================================================================================================== the float64 statement
def dsx_statement(H, Wg, Tc, U, R, Cand, dHnew, dRH, cin):
    """(rows, C, cin) in the operands' own precision; planes (rows, C, h), Wg (4 L, 2 h) with L = cin + h, Tc (2, C, C)."""
    L = cin + H.shape[-1]
    block = lambda kc: Wg[(2 + kc) * L:(2 + kc) * L + cin]                          # (n = 1, kc): its rows of the input columns
    dG = torch.cat([dHnew * (Cand - H) * U * (1 - U), dRH * H * R * (1 - R)], -1)
    return torch.einsum('rco,lo->rcl', dG, block(0)) + torch.einsum('cd,rdo,lo->rcl', Tc[1], dG, block(1))


def operands(rows, C, cin):
    """``planes`` of tests/test_cell_dtc_planar.py and a category stack of its own."""
    d = planes(rows, C, cin)
    g = torch.Generator().manual_seed(rows + 1000 * C + cin)
    d['Tc'] = torch.randn(2, C, C, generator=g) / C ** 0.5
    return d


# ============================================================================================================== CPU
def test_header_table_and_exports_agree():
    header = open(os.path.join(REPO, 'include', 'stc_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(rf'\b{ENTRY}\s*\(', code) and ENTRY in _lib._ABI and ENTRY in _lib.EXPORTS
    proto = re.search(rf'{ENTRY}\s*\((.*?)\)\s*;', code, flags=re.S).group(1)
    assert len(proto.split(',')) == len(_lib._ABI[ENTRY][1]) == 13
    assert _lib.load_library().stc_version() == _lib.ABI_VERSION >= 44
    assert hasattr(_lib.HipKernels, 'cell_dsx_narrow') and not hasattr(EmulatedKernels, 'cell_dsx_narrow')      # the CPU twin does not get it
    assert 'stc_cell_dsx_narrow.hip' in open(os.path.join(REPO, 'stc-gnn_amd', 'csrc', 'Makefile')).read()


_PTR = dict(H=0x10000, Wg=0x20000, Tc=0x30000, U=0x40000, R=0x50000, Cand=0x60000, dHnew=0x70000, dRH=0x80000, dSx=0x90000)


def _call(lib, cin=3, rows=10, C=32, **over):
    p = dict(_PTR, **over)
    return lib.stc_cell_dsx_narrow_planar_f32(p['H'], p['Wg'], p['Tc'], p['U'], p['R'], p['Cand'], p['dHnew'], p['dRH'], p['dSx'], cin, rows, C, None)


def test_refusals_come_before_any_hip_call():
    """Made-up addresses throughout: a call that got as far as a launch would fault, a refusal never touches them."""
    lib = _lib.load_library()
    err = lambda: lib.stc_last_error()
    EINVAL, EALIGN = -1, -2
    for name in _PTR:
        assert _call(lib, **{name: None}) == EINVAL and b'null' in err(), name
    for name in _PTR:
        off = 2 if name in ('Wg', 'Tc', 'dSx') else 4                  # (read / written by the float; the state planes by 16-byte pieces)
        assert _call(lib, **{name: _PTR[name] + off}) == EALIGN and b'aligned' in err(), name
    for C in (16, 0, 48, 128):
        assert _call(lib, C=C) == EINVAL and b'C in (32, 64)' in err(), C
    for cin in (5, 0, -1, 8, 16):
        assert _call(lib, cin=cin) == EINVAL and b'cin' in err(), cin
    assert _call(lib, rows=-1) == EINVAL and b'rows' in err()
    assert _call(lib, rows=1 << 31) == EINVAL and b'rows' in err()
    assert _call(lib, rows=0) == 0                                     # launches nothing
    assert _call(lib, rows=0, **{name: None for name in _PTR}) == 0


def test_the_statement_is_autograds_gradient_with_respect_to_the_aggregated_input():
    """A float64 STC_Cell on a ONE-WAY weighted graph with a non-symmetric category graph.  Its gates convolution is ``bdg_dif`` at order 2; the
    same convolution written as its two spatial terms (``bdg_dif`` at Ks = 1 on [x | H] and on [S.x | S.H] with the weight rows of each term)
    makes S.x a leaf, whose gradient autograd then returns."""
    g = torch.Generator().manual_seed(11)
    B, N, C, cin, h = 2, 5, 3, 2, 4
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Gs = torch.triu(torch.rand(N, N, generator=g, dtype=torch.float64), 1)
    Gc = rn(C, C).mul(0.5)
    X, H, dHnew = rn(B, N, C, cin), rn(B, N, C, h), rn(B, N, C, h)
    L = cin + h
    Wg, bg, Wc, bc = rn(4 * L, 2 * h) * 0.3, rn(2 * h), rn(4 * L, h) * 0.3, rn(h)
    agg = lambda t: torch.einsum('bncl,nm->bmcl', t, Gs)                # S.t: the 1-mode product of the reference
    Sx = agg(X).detach().requires_grad_()
    pre = (O.bdg_dif(torch.cat([X, H], -1), Gs, Gc, Wg[:2 * L], bg, 1, 2) + O.bdg_dif(torch.cat([Sx, agg(H)], -1), Gs, Gc, Wg[2 * L:], None, 1, 2))
    assert rel_err(pre, O.bdg_dif(torch.cat([X, H], -1), Gs, Gc, Wg, bg, 2, 2)) < 1e-14       # the same convolution
    U, R = (torch.sigmoid(t) for t in torch.split(pre, h, dim=-1))
    RH = R * H
    RH.retain_grad()
    Cand = torch.tanh(O.bdg_dif(torch.cat([X, RH], -1), Gs, Gc, Wc, bc, 2, 2))
    Hnew = (1.0 - U) * H + U * Cand
    (Hnew * dHnew).sum().backward()
    r = lambda t: t.detach().reshape(B * N, C, -1)
    Tc = torch.stack(O.cheby_poly(Gc, 2))
    got = dsx_statement(r(H), Wg, Tc, r(U), r(R), r(Cand), r(dHnew), r(RH.grad), cin)
    assert got.shape == (B * N, C, cin) and rel_err(got, r(Sx.grad)) < 1e-13, rel_err(got, r(Sx.grad))
    wrong = dsx_statement(r(H), Wg, torch.stack([Tc[0], Tc[1].t()]), r(U), r(R), r(Cand), r(dHnew), r(RH.grad), cin)
    assert rel_err(wrong, r(Sx.grad)) > 1e-2                           # (the other orientation of the mix is another plane)


def test_the_kernels_use_no_scratch(tmp_path):
    from tests.test_first_step_isa import _resource_usage
    from tests.test_isa import HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not present')
    usage = _resource_usage('stc_cell_dsx_narrow.hip', tmp_path)
    assert len(usage) == 2, sorted(usage)                              # C in {32, 64}
    for name, u in usage.items():
        assert u['ScratchSize'] == 0 and u['LDS Size'] <= 64 * 1024, (name, u)


# ============================================================================================================== GPU
@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


_W = 256      # (asserted against the library's slot rule in the test itself: the parametrisation needs it at collection time)
_ROWS = (1, _W - 1, _W, _W + 1, 2 * _W + 3)


def _launch(hip, dev, cin):
    R, C, _ = dev['H'].shape
    out = torch.full((R, C, cin), float('nan'), device='cuda')
    hip.cell_dsx_narrow(*[dev[n] for n in ARGS], out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('C', (32, 64))
@pytest.mark.parametrize('cin', (1, 2, 3, 4))
@pytest.mark.parametrize('rows', _ROWS)
def test_parity_with_the_float64_statement(hip, rows, cin, C):
    assert run_of_rows() == _W
    d = operands(rows, C, cin)
    want, fp32 = (dsx_statement(*[d[n].to(dt) for n in ARGS], cin) for dt in (torch.float64, torch.float32))
    dev = {n: d[n].cuda() for n in ARGS}
    got = _launch(hip, dev, cin)
    assert got.shape == (rows, C, cin) and bool(torch.isfinite(got).all())          # every element of the plane is written
    err, noise = rel_err(got, want), rel_err(fp32, want)
    bound = max(FLOOR, FACTOR * noise)
    print(f'cell_dsx_narrow C={C} cin={cin} rows={rows}: {err:.3e} from float64, fp32 torch {noise:.3e} (bound {bound:.1e})')
    log_parity(f'cell_dsx_narrow C={C} cin={cin} rows={rows}', err, noise, FACTOR, bound)
    assert err <= bound, (err, noise)
    assert torch.equal(_launch(hip, dev, cin), got)                    # two runs: equal bits


@pytest.mark.gpu
def test_the_front_refuses_what_the_kernel_does_not_take(hip):
    d = {n: v.cuda() for n, v in operands(3, 32, 2).items()}
    args = lambda **over: [over.get(n, d[n]) for n in ARGS]
    out = torch.zeros(3, 32, 2, device='cuda')
    with pytest.raises(_lib.StcError, match='input plane 1..4'):
        hip.cell_dsx_narrow(*args(), torch.zeros(3, 32, 16, device='cuda'))
    with pytest.raises(_lib.StcError, match='Wg'):
        hip.cell_dsx_narrow(*args(), torch.zeros(3, 32, 3, device='cuda'))                  # cin = 3 against Wg for cin = 2
    with pytest.raises(_lib.StcError, match='plane'):
        hip.cell_dsx_narrow(*args(U=d['U'][:2].contiguous()), out)
    with pytest.raises(_lib.StcError, match='Tc'):
        hip.cell_dsx_narrow(*args(Tc=d['Tc'][:1].contiguous()), out)
    with pytest.raises(_lib.StcError, match='ROCm'):
        hip.cell_dsx_narrow(*args(dRH=d['dRH'].cpu()), out)
    assert float(out.abs().max()) == 0.0
