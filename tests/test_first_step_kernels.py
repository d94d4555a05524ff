"""The first-step forms of the planar cell launches (ABI v37): a cell whose state is the zero initial state -- the first time step of every
layer -- runs without the H, S.H, R planes and their gradients (stc_cell_gates_fwd_first_f32, stc_ring2_blend_first_f32,
stc_cell_bwd_first_f32).

GPU: each new entry point against the EXISTING one fed explicit planes of zeros as H and S.H (and, the backward, an arbitrary R): the existing
entry points are the reference.  The products that remain are the general kernels', in their order, so every result is compared with
``torch.equal``; the H rows of both weight gradients and the reset gate's half of dWg / dbg must be exact zeros.  Node counts 1, 5, 1 030 and
4 101: one wave, a ragged workgroup, more than one workgroup, and more than four nodes for some of the <= 1 024 waves of a backward launch (sums
over several nodes, the two-ahead prefetch and its tail).  Pass restarts of the fp16 x 2 format (tests/test_grad_scale.py) through the new
backward against the float64 twin, within that file's bound.
"""
import pytest
import torch

from stc_hip import CsrGraph
from stc_hip.graph import csr_operand
from tests.test_grad_scale import BOUND, EM, _cell_case, per_node_err
from tests.conftest import rel_err

H16, C32 = 16, 32
SENT = -7.25          # what result planes hold before a launch: a plane the launch did not write shows


@pytest.fixture(scope='module')
def hip():
    from stc_hip._lib import HipKernels
    return HipKernels()


def _formats(hip):
    """The kernel set on both operand formats: the default one and the 24-bit view heavy graphs get (the same object if that is the default)."""
    other = hip.for_graph(float('inf'))
    return [hip] if other is hip else [hip, other]


def _operands(nodes, cin, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s_: torch.randn(*s_, generator=g)
    Lw, K, C, h = cin + H16, 2, C32, H16
    Tc = rnd(K, C, C) / C ** 0.5
    Tc[0] = torch.eye(C)
    s = dict(Tc=Tc, Wg=rnd(K * K * Lw, 2 * h) / (2 * K * Lw) ** 0.5, bg=rnd(2 * h), Wc=rnd(K * K * Lw, h) / (2 * K * Lw) ** 0.5, bc=rnd(h),
             X=rnd(nodes, C, cin), SX=rnd(nodes, C, cin), U=torch.sigmoid(rnd(nodes, C, h)), R=torch.sigmoid(rnd(nodes, C, h)),
             Cand=torch.tanh(rnd(nodes, C, h)), dHnew=rnd(nodes, C, h), dBm=rnd(nodes, C, h), dX0=rnd(nodes, C, h), dSX0=rnd(nodes, C, h))
    return {k: v.cuda() for k, v in s.items()}


def _plane(like):
    return torch.full_like(like, SENT)


@pytest.mark.gpu
@pytest.mark.parametrize('cin', [16, 1, 4])
@pytest.mark.parametrize('nodes', [1, 5, 1030, 4101])
def test_gates_forward_and_backward_equal_the_general_kernels_on_zero_planes(hip, nodes, cin):
    s = _operands(nodes, cin, 1000 * cin + nodes)
    zero = torch.zeros(nodes, C32, H16, device='cuda')
    wide = cin == H16
    for k in _formats(hip):
        for bias in (True, False):
            bg, bc = (s['bg'], s['bc']) if bias else (None, None)
            # ---- forward: U, A, Bm and the activation maxima
            ref = {n: _plane(zero) for n in ('U', 'Rg', 'A', 'Bm')}
            am_ref = k.act_amax_buffer(zero, 4)
            k.cell_gates_fwd_planar(s['X'], zero, s['SX'], zero, s['Tc'], s['Wg'], bg, ref['U'], ref['Rg'], None,
                                    post=(s['Wc'], bc, ref['A'], ref['Bm']), act_amax=am_ref)
            got = {n: _plane(zero) for n in ('U', 'A', 'Bm')}
            am = k.act_amax_buffer(zero, 4)
            k.cell_gates_fwd_first(s['X'], s['SX'], s['Tc'], s['Wg'], bg, got['U'], (s['Wc'], bc, got['A'], got['Bm']), act_amax=am)
            for n in got:
                assert torch.equal(got[n], ref[n]), (k.operand_format, bias, n, float((got[n] - ref[n]).abs().max()))
            assert (am is None and am_ref is None) or torch.equal(am, am_ref)
            if am is not None:                                   # the H rows of the slots: wide {X, S.X, H, S.H}, narrow {H, S.H, x, S.x}
                h_rows = am[2:] if wide else am[:2]
                assert bool((h_rows == 0).all()) and bool((am.sum(1) > 0).sum() == 2)
            # ---- backward: an arbitrary R beside H = 0; with and without accumulate_x (wide input only)
            for acc in ((False, True) if wide else (False,)):
                def grads():
                    return dict(dWg=_plane(s['Wg']), dbg=_plane(s['bg']) if bias else None, dWc=_plane(s['Wc']), dbc=_plane(s['bc']) if bias else None)

                def x_planes():
                    if not wide:
                        return [None, None]
                    return [s['dX0'].clone(), s['dSX0'].clone()] if acc else [_plane(zero), _plane(zero)]
                pr, dZr = grads(), x_planes() + [_plane(zero), _plane(zero)]
                k.cell_bwd_planar(s['X'], zero, s['SX'], zero, s['Tc'], s['Wg'], s['Wc'], s['U'], s['R'], s['Cand'], s['dHnew'], s['dBm'],
                                  dZr, pr['dWg'], pr['dbg'], pr['dWc'], pr['dbc'], accumulate_x=acc, act_amax=am_ref)
                pg, dXg = grads(), x_planes()
                k.cell_bwd_first(s['X'], s['SX'], s['Tc'], s['Wg'], s['Wc'], s['U'], s['Cand'], s['dHnew'], s['dBm'], dXg,
                                 pg['dWg'], pg['dbg'], pg['dWc'], pg['dbc'], accumulate_x=acc, act_amax=am)
                tag = (k.operand_format, bias, acc)
                for n in pg:
                    assert (pg[n] is None) == (pr[n] is None)
                    if pg[n] is not None:
                        assert torch.equal(pg[n], pr[n]), (tag, n, rel_err(pg[n], pr[n]))
                if wide:
                    for i, n in enumerate(('dX', 'dSX')):
                        assert torch.equal(dXg[i], dZr[i]), (tag, n, rel_err(dXg[i], dZr[i]))
                # exact zeros: the H rows of both weight gradients (rows cin.. of every (n, c) block), the reset gate's columns of dWg and dbg
                Lw = cin + H16
                assert bool((pg['dWg'].view(4, Lw, 2 * H16)[:, cin:] == 0).all()) and bool((pg['dWc'].view(4, Lw, H16)[:, cin:] == 0).all()), tag
                assert bool((pg['dWg'][:, H16:] == 0).all()) and (pg['dbg'] is None or bool((pg['dbg'][H16:] == 0).all())), tag
                assert bool((pg['dWg'].view(4, Lw, 2 * H16)[:, :cin, :H16] != 0).any()) and bool((pg['dWc'].view(4, Lw, H16)[:, :cin] != 0).any()), tag


@pytest.mark.gpu
@pytest.mark.parametrize('Hg,Wg', [(16, 16), (9, 13)])
def test_blend_form_equals_the_two_ring_blend_on_a_zero_state(hip, Hg, Wg):
    B, n = 2, Hg * Wg
    op = csr_operand(CsrGraph.queen_grid(Hg, Wg, normalize=True), torch.device('cuda'))
    assert op.fwd_ring2 is not None and hip.ring2_fits(B, n, C32, H16)
    g = torch.Generator().manual_seed(n)
    rnd = lambda: torch.randn(B, n, C32, H16, generator=g).cuda()
    Bm, A, U, zero = rnd() * 0.5, rnd() * 0.5, torch.sigmoid(rnd()), torch.zeros(B, n, C32, H16, device='cuda')
    graph = (op.fwd_rowptr, op.fwd_colidx, op.fwd_val, op.fwd_ring2)
    for with_cand in (True, False):
        ref = {k: _plane(zero) for k in ('Cand', 'Hnew', 'SHnew')}
        got = {k: _plane(zero) for k in ('Cand', 'Hnew', 'SHnew')}
        hip.ring2_blend(*graph, Bm, A, U, zero, ref['Cand'] if with_cand else None, ref['Hnew'], ref['SHnew'])
        hip.ring2_blend_first(*graph, Bm, A, U, got['Cand'] if with_cand else None, got['Hnew'], got['SHnew'])
        for k in got:
            assert torch.equal(got[k], ref[k]), (with_cand, k)
        assert bool((got['Cand'] == SENT).all()) == (not with_cand) and not bool((got['Hnew'] == SENT).any())


@pytest.mark.gpu
@pytest.mark.parametrize('pattern', ['staircase', 'ramp', 'gates-only'])
@pytest.mark.parametrize('cin', [16, 1])
def test_first_step_backward_with_gradient_jumps_inside_a_wave(hip, monkeypatch, pattern, cin):
    """The pass restarts of the fp16 x 2 format (RunScale, cand_done, resume) through the first-step backward: 9 000 nodes = 8-9 per wave, state
    gradients that jump by 2^12 .. 2^24 from node to node; against the float64 twin on H = S.H = 0, 2e-5 per node."""
    from stc_hip import _lib
    monkeypatch.setattr(hip, 'operand_format', _lib.FMT_F16X2, raising=False)
    c = _cell_case(pattern, 9000, cin, waves=1024)
    c['H'], c['SH'] = torch.zeros_like(c['H']), torch.zeros_like(c['SH'])
    nodes, C, h, wide = c['nodes'], c['C'], c['h'], cin == 16
    d = lambda t: t.double()
    dZ_w = [torch.empty(nodes, C, h, dtype=torch.float64) if (wide or i >= 2) else None for i in range(4)]
    want = dict(dWg=torch.empty_like(d(c['Wg'])), dbg=torch.empty(2 * h, dtype=torch.float64), dWc=torch.empty_like(d(c['Wc'])), dbc=torch.empty(h, dtype=torch.float64))
    EM.cell_bwd_planar(*[d(c[n]) for n in ('X', 'H', 'SX', 'SH', 'Tc', 'Wg', 'Wc', 'U', 'R', 'Cand', 'dHn', 'dBm')], dZ_w,
                       want['dWg'], want['dbg'], want['dWc'], want['dbc'])
    cu = lambda t: t.cuda()
    dX = [torch.full((nodes, C, h), float('nan'), device='cuda') for _ in range(2)] if wide else [None, None]
    got = dict(dWg=torch.empty_like(cu(c['Wg'])), dbg=torch.empty(2 * h, device='cuda'), dWc=torch.empty_like(cu(c['Wc'])), dbc=torch.empty(h, device='cuda'))
    hip.cell_bwd_first(*[cu(c[n]) for n in ('X', 'SX', 'Tc', 'Wg', 'Wc', 'U', 'Cand', 'dHn', 'dBm')], dX, got['dWg'], got['dbg'], got['dWc'], got['dbc'])
    for name in want:
        e = rel_err(got[name], want[name])
        print(pattern, cin, name, f'{e:.3e}')
        assert e < BOUND, (pattern, cin, name, e)
    if wide:
        for i in range(2):
            assert torch.isfinite(dX[i]).all()
            e = per_node_err(dX[i], dZ_w[i])
            print(pattern, cin, 'plane', i, f'{e:.3e}')
            assert e < BOUND, (pattern, cin, 'plane', i, e)
