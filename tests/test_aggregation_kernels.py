"""The kernels that fuse a graph aggregation with something else -- stc_spmm_sum_f32 / _bf16, stc_spmm_blend_fwd_f32 / _bf16 and the four two-ring
forms (stc_ring2_sum_f32, stc_ring2_blend_f32, stc_ring2_blend_first_f32, stc_ring2_chain_f32) -- one at a time on the graph family of
tests/graph_cases.py: signed weights that differ on every entry, ragged and empty rows, one-way graphs, ring-bounded clusters.  On the
row-stochastic queen grid, which every other test of these kernels uses, a value paired with the wrong entry of its row, the other orientation's
columns in the interior, or a wrong but small row all pass (``test_rotated_values_show_on_weights_and_not_on_the_queen_grid`` shows it).

Reference: the float64 twin (oracle/kernel_emul.py, checked against dense algebra in tests/test_aggregation_graphs.py).  Linear results are
held to the elementwise a-priori bound defined there (|got - want| <= c 2^-24 M, exactly 0 where M == 0); tanh-bearing ones (Cand, Hnew,
S.Hnew: the error of ``stc_tanh`` is not derivable) to the project's 2e-6 of the plane's maximum, on graphs scaled to unit row sums.  Every
two-ring run is also compared with the two launches it replaces and repeated bit for bit; every launch is preceded by NaN-filled results and
followed by a look at which kernel ran.  Two-ring entry points run on the operand's own orientation and on the other one.
"""
import numpy as np
import pytest
import torch

from stc_hip.graph import csr_operand
from tests import graph_cases as GC
from tests.conftest import rel_err
from tests.test_aggregation_graphs import (C_FIRST, C_SECOND, EM, FAMILY, agg, assert_within, first_stage_magnitude, magnitudes, ratio_to_bound,
                                           side_csr)

B, C, HID = 2, 32, 16
SCALES = (1.0, 1.0, -1.0, 1.0, -1.0, 0.5, 1.0, -2.0)      # the signed addends of the order-3 state gradient, at the kernel's limit of 8
SIDES = ('fwd', 'bwd')


@pytest.fixture(scope='module')
def hip():
    from stc_hip._lib import HipKernels
    return HipKernels()


def cu(t):
    return None if t is None else t.cuda()


def d(t):
    return None if t is None else t.double()


def nan_plane(n, dtype=torch.float32):
    return torch.full((B, n, C, HID), float('nan'), dtype=dtype).cuda()


def new64(n):
    return torch.empty(B, n, C, HID, dtype=torch.float64)


def device_side(graph, side):
    """(CSR arrays, row-block plan, two-ring plan) of one orientation on the GPU."""
    op = csr_operand(graph, torch.device('cuda'))
    return (tuple(getattr(op, f'{side}_{k}') for k in ('rowptr', 'colidx', 'val')), getattr(op, f'{side}_plan'), getattr(op, f'{side}_ring2'))


def ran(hip, launch):
    """The kernels one call launched, in order of first launch (``KernelTimer``)."""
    from stc_hip._lib import KernelTimer
    hip.timer = t = KernelTimer()
    try:
        launch()
    finally:
        hip.timer = None
    return list(t.summary())


def drawer(seed, n):
    g = torch.Generator().manual_seed(seed)
    return lambda: torch.randn(B, n, C, HID, generator=g)


# ------------------------------------------------------------------------------------------------------- stc_spmm_sum_f32
@pytest.mark.gpu
@pytest.mark.parametrize('name,H,W', FAMILY)
def test_state_gradient_sum(hip, name, H, W):
    """``hip.spmm_sum`` with the row-blocked plan and with ``plan=None``, both orientations: three addends and two gathered planes, without and
    with the blend epilogue (dY = Y U (1 - Cand^2): the first stage's c + 4); alpha and eight signed addends (the kernel's limit).
    Largest ratio to the bound seen on the MI355X: 0.39 (Y), 0.27 (dY); the fp32 twin's own: 0.42."""
    graph, G = GC.case(name, H, W)
    n = graph.n
    rnd = drawer(n + C + 3, n)
    X, X2, U, Cand = rnd(), rnd(), torch.sigmoid(rnd()), torch.tanh(rnd())
    adds = [rnd() for _ in range(8)]
    for side in SIDES:
        csr64, _ = side_csr(graph, G, side)
        csr, blocks, _ = device_side(graph, side)
        for n_add, alpha, scales in ((3, 1.0, (1.0,) * 3), (8, -0.5, SCALES), (0, 2.0, ())):
            Y_w, dY_w = new64(n), new64(n)
            EM.spmm_sum(*csr64, None, d(X), d(X2), [(d(t), 0, s) for t, s in zip(adds, scales)], Y_w, blend=(d(U), d(Cand), dY_w), alpha=alpha)
            M = first_stage_magnitude(csr64, X, X2, alpha, list(zip(adds, scales)))
            for plan in (blocks, None):
                tag = f'{name} {H}x{W} {side} {"blocked" if plan is not None else "csr"} n_add={n_add}'
                addends = [(cu(t), 0, s) for t, s in zip(adds, scales)]
                Y = nan_plane(n)
                assert ran(hip, lambda: hip.spmm_sum(*csr, plan, cu(X), cu(X2), addends, Y, alpha=alpha)) == ['stc_spmm_sum_f32']
                assert_within(Y, Y_w, M, C_FIRST(n_add), tag + ' Y')
                Y2, dY = nan_plane(n), nan_plane(n)
                assert ran(hip, lambda: hip.spmm_sum(*csr, plan, cu(X), cu(X2), addends, Y2, blend=(cu(U), cu(Cand), dY), alpha=alpha)) == ['stc_spmm_sum_f32']
                assert torch.equal(Y2, Y)
                assert_within(dY, dY_w, M * d(U) * (1 + d(Cand) ** 2), C_FIRST(n_add) + 4, tag + ' dY')


# ------------------------------------------------------------------------------------------------------- stc_spmm_blend_fwd_f32
@pytest.mark.gpu
@pytest.mark.parametrize('name,H,W', FAMILY)
def test_blend_forward(hip, name, H, W):
    """``hip.spmm_blend_fwd`` (Cand = tanh(A + S.Bm), Hnew = (1 - U) H + U Cand) on the graph scaled to unit row sums, row-blocked and plain CSR, both
    orientations, with and without the stored candidate.  Seen on the MI355X: at most 2.6e-7."""
    graph, G = GC.case(name, H, W, unit=True)
    n = graph.n
    rnd = drawer(n, n)
    Bm, A, U, Hp = rnd(), rnd(), torch.sigmoid(rnd()), torch.tanh(rnd())
    for side in SIDES:
        csr64, _ = side_csr(graph, G, side)
        csr, blocks, _ = device_side(graph, side)
        Cd_w, Hn_w = new64(n), new64(n)
        EM.spmm_blend_fwd(*csr64, None, d(Bm), d(A), d(U), d(Hp), Cd_w, Hn_w)
        for plan in (blocks, None):
            Cd, Hn = nan_plane(n), nan_plane(n)
            assert ran(hip, lambda: hip.spmm_blend_fwd(*csr, plan, cu(Bm), cu(A), cu(U), cu(Hp), Cd, Hn)) == ['stc_spmm_blend_fwd_f32']
            e = (rel_err(Cd, Cd_w), rel_err(Hn, Hn_w))
            print(f'{name} {H}x{W} {side} {"blocked" if plan is not None else "csr"}: Cand {e[0]:.2e} Hnew {e[1]:.2e}')
            assert torch.isfinite(Cd).all() and torch.isfinite(Hn).all() and max(e) < 2e-6
            Hn2 = nan_plane(n)
            hip.spmm_blend_fwd(*csr, plan, cu(Bm), cu(A), cu(U), cu(Hp), None, Hn2)      # the candidate not stored
            assert torch.equal(Hn2, Hn)


# ------------------------------------------------------------------------------------------------------- stc_ring2_sum_f32
@pytest.mark.gpu
@pytest.mark.parametrize('name,H,W', FAMILY)
def test_two_ring_sum(hip, name, H, W):
    """``hip.ring2_sum`` on Gs with its plan and on Gs^T with its plan; 0 .. 5 addends, one and two gathered planes.  Y within
    c = 8 + 1 + n_add + 1 roundings of M, Z = S.(Y U (1 - Cand^2)) within that + 4 + 8 of |S|.(M U (1 + Cand^2)); the two launches it replaces at
    tests/test_ring2.py's 1e-6; a second launch bit for bit.  Largest ratio seen on the MI355X: 0.40 (Y), 0.18 (Z); against the two launches Y bit for bit, Z 7.5e-8."""
    graph, G = GC.case(name, H, W)
    n = graph.n
    v3 = lambda t: t.view(B, n, C * HID)
    for side in SIDES:
        csr64, _ = side_csr(graph, G, side)
        csr, blocks, ring2 = device_side(graph, side)
        assert ring2 is not None
        for n_add, dual in ((0, False), (1, True), (2, False), (3, True), (4, False), (5, True)):
            tag = f'{name} {H}x{W} {side} n_add={n_add} dual={dual}'
            rnd = drawer(n + n_add, n)
            X, X2 = rnd(), (rnd() if dual else None)
            adds = [rnd() for _ in range(n_add)]
            U, Cand = torch.sigmoid(rnd()), torch.tanh(rnd())
            Y_w, Z_w = new64(n), new64(n)
            EM.ring2_sum(*csr64, None, d(X), d(X2), [d(t) for t in adds], d(U), d(Cand), Y_w, Z_w)
            M1 = first_stage_magnitude(csr64, X, X2, 1.0, [(t, 1.0) for t in adds])
            M2 = agg(magnitudes(csr64), M1 * d(U) * (1 + d(Cand) ** 2))
            Y, Z = nan_plane(n), nan_plane(n)
            launch = lambda Y_, Z_: hip.ring2_sum(*csr, ring2, cu(X), cu(X2), [cu(t) for t in adds], cu(U), cu(Cand), Y_, Z_)
            assert ran(hip, lambda: launch(Y, Z)) == ['stc_ring2_sum_f32']
            assert_within(Y, Y_w, M1, C_FIRST(n_add), tag + ' Y')
            assert_within(Z, Z_w, M2, C_SECOND(n_add), tag + ' Z')
            # the two launches it replaces, on the same operands
            Y2, dY2, Z2 = nan_plane(n), nan_plane(n), nan_plane(n)
            hip.spmm_sum(*csr, blocks, cu(X), cu(X2), [(cu(t), 0) for t in adds], Y2, blend=(cu(U), cu(Cand), dY2))
            hip.csr_spmm(*csr, n, n, v3(dY2), None, v3(Z2), 1.0, 0.0, plan=blocks)
            e = (rel_err(Y, Y2), rel_err(Z, Z2))
            print(f'{tag}: against the two launches Y {e[0]:.2e} Z {e[1]:.2e}')
            assert max(e) < 1e-6
            Y3, Z3 = nan_plane(n), nan_plane(n)
            launch(Y3, Z3)
            assert torch.equal(Y3, Y) and torch.equal(Z3, Z)


# ------------------------------------------------------------------------------------------------------- stc_ring2_chain_f32
CHAIN_ARGS = [(False, 0, 1, True, 1.0, 2.0), (True, 2, 4, False, 2.0, 1.0), (False, 1, 2, False, 2.0, 1.0), (True, 2, 5, True, -0.5, 3.0)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,H,W', FAMILY)
def test_two_ring_chain(hip, name, H, W):
    """``hip.ring2_chain`` on both orientations with the argument sets of tests/test_ring2.py (the forward recurrence, the transposes of the order-3
    backward, the limits): V = alpha1 S.(X [+ X2]) + sum add1 within the first stage's bound, Z = alpha2 S.V + sum scale0 add0 within the second's
    (M: |alpha2| |S|.M_V + sum |scale0 add0|); the two ``spmm_sum`` launches it replaces at 2e-6; with and without the stored V bit for bit.
    Largest ratio seen on the MI355X: 0.37 (V), 0.17 (Z); against the two launches V bit for bit, Z 1.2e-7."""
    graph, G = GC.case(name, H, W)
    n = graph.n
    for side in SIDES:
        csr64, _ = side_csr(graph, G, side)
        csr, blocks, ring2 = device_side(graph, side)
        assert ring2 is not None
        for dual, n1, n0, keep, alpha1, alpha2 in CHAIN_ARGS:
            tag = f'{name} {H}x{W} {side} dual={dual} n1={n1} n0={n0}'
            rnd = drawer(n + n1 + n0, n)
            X, X2 = rnd(), (rnd() if dual else None)
            add1 = [rnd() for _ in range(n1)]
            add0 = [(rnd(), s) for s in ([1.0, -1.0, 1.0, -2.5, 0.5][:n0])]
            V_w, Z_w = new64(n), new64(n)
            EM.ring2_chain(*csr64, None, d(X), d(X2), alpha1, [d(t) for t in add1], V_w, alpha2, [(d(t), s) for t, s in add0], Z_w)
            M1 = first_stage_magnitude(csr64, X, X2, alpha1, [(t, 1.0) for t in add1])
            M2 = agg(magnitudes(csr64), M1, abs(alpha2)) + sum(abs(s) * d(t).abs() for t, s in add0)
            V, Z = (nan_plane(n) if keep else None), nan_plane(n)
            launch = lambda V_, Z_: hip.ring2_chain(*csr, ring2, cu(X), cu(X2), alpha1, [cu(t) for t in add1], V_, alpha2, [(cu(t), s) for t, s in add0], Z_)
            assert ran(hip, lambda: launch(V, Z)) == ['stc_ring2_chain_f32']
            if keep:
                assert_within(V, V_w, M1, C_FIRST(n1), tag + ' V')
            assert_within(Z, Z_w, M2, C_SECOND(n1, n0), tag + ' Z')
            V2, Z2 = nan_plane(n), nan_plane(n)
            hip.spmm_sum(*csr, blocks, cu(X), cu(X2), [(cu(t), 0) for t in add1], V2, alpha=alpha1)
            hip.spmm_sum(*csr, blocks, V2, None, [(cu(t), 0, s) for t, s in add0], Z2, alpha=alpha2)
            e = (rel_err(Z, Z2), rel_err(V, V2) if keep else 0.0)
            print(f'{tag}: against the two launches Z {e[0]:.2e} V {e[1]:.2e}')
            assert max(e) < 2e-6
            V3, Z3 = (None if keep else nan_plane(n)), nan_plane(n)      # the other way round: reproducible, with or without the stored V
            launch(V3, Z3)
            assert torch.equal(Z3, Z)


# ------------------------------------------------------------------------------------------------------- stc_ring2_blend_f32, stc_ring2_blend_first_f32
@pytest.mark.gpu
@pytest.mark.parametrize('name,H,W', FAMILY)
def test_two_ring_blend_and_its_first_step_form(hip, name, H, W):
    """``hip.ring2_blend`` and ``hip.ring2_blend_first`` on the graph scaled to unit row sums, both orientations: against the float64 twin (the
    first-step form: the twin on a zero state) and against the two launches they replace, which share ``stc_tanh`` (both 2e-6, as
    tests/test_ring2.py); the first-step form equal to the general one on a plane of zeros; a second launch bit for bit; the candidate stored or
    not.  Seen on the MI355X: at most 2.6e-7 against the twin, 1.6e-7 against the two launches."""
    graph, G = GC.case(name, H, W, unit=True)
    n = graph.n
    v3 = lambda t: t.view(B, n, C * HID)
    rnd = drawer(n, n)
    Bm, A, U, Hp = rnd(), rnd(), torch.sigmoid(rnd()), torch.tanh(rnd())
    for side in SIDES:
        csr64, _ = side_csr(graph, G, side)
        csr, blocks, ring2 = device_side(graph, side)
        assert ring2 is not None
        for first in (False, True):
            state = torch.zeros_like(Hp) if first else Hp
            want = [new64(n) for _ in range(3)]
            EM.ring2_blend(*csr64, None, d(Bm), d(A), d(U), d(state), *want)
            if first:
                launch = lambda outs: hip.ring2_blend_first(*csr, ring2, cu(Bm), cu(A), cu(U), *outs)
            else:
                launch = lambda outs: hip.ring2_blend(*csr, ring2, cu(Bm), cu(A), cu(U), cu(Hp), *outs)
            got = [nan_plane(n) for _ in range(3)]
            assert ran(hip, lambda: launch(got)) == ['stc_ring2_blend_first_f32' if first else 'stc_ring2_blend_f32']
            two = [nan_plane(n) for _ in range(3)]
            hip.spmm_blend_fwd(*csr, blocks, cu(Bm), cu(A), cu(U), cu(state), two[0], two[1])
            hip.csr_spmm(*csr, n, n, v3(two[1]), None, v3(two[2]), 1.0, 0.0, plan=blocks)
            for what, a, w, t in zip(('Cand', 'Hnew', 'S.Hnew'), got, want, two):
                e = (rel_err(a, w), rel_err(a, t))
                print(f'{name} {H}x{W} {side} first={first} {what}: twin {e[0]:.2e} two launches {e[1]:.2e}')
                assert torch.isfinite(a).all() and max(e) < 2e-6
            again = [None, nan_plane(n), nan_plane(n)]                 # the candidate not stored
            launch(again)
            assert torch.equal(again[1], got[1]) and torch.equal(again[2], got[2])
            if first:                                                 # ... and the general form on a plane of zeros
                ref = [nan_plane(n) for _ in range(3)]
                hip.ring2_blend(*csr, ring2, cu(Bm), cu(A), cu(U), cu(state), *ref)
                assert all(torch.equal(a, r) for a, r in zip(got, ref))


# ------------------------------------------------------------------------------------------------------- bf16 planes
@pytest.mark.gpu
@pytest.mark.parametrize('name,H,W', GC.grid_params(('ragged', 'one_way')))
def test_state_aggregations_on_bf16_planes(hip, name, H, W):
    """``hip.bf16.spmm_sum`` and ``hip.bf16.spmm_blend_fwd``, row-blocked and plain CSR, both orientations, on positive weights with unit row sums
    and bf16-valued inputs, against the fp32 twin exactly as tests/test_bf16_kernels.py::test_state_aggregations_bf16: within one bf16 ulp with at
    most 5 % of the elements different, the tanh-bearing planes within 2^-7.  (The reference's own share of different elements against float64:
    7e-5, tests/test_aggregation_graphs.py.)  Seen on the MI355X: at most 4e-5 of the elements different."""
    from tests.test_bf16_kernels import _close, assert_one_ulp
    bf = torch.bfloat16
    graph, G = GC.case(name, H, W, positive=True)
    n = graph.n
    g = torch.Generator().manual_seed(n + C + 3)
    rb = lambda: torch.randn(B, n, C, HID, generator=g).to(bf)
    f = lambda t: t.float()
    X, X2, adds = rb(), rb(), [(rb(), 0) for _ in range(3)]
    U, Cand = torch.rand(B, n, C, HID, generator=g).to(bf), torch.tanh(torch.randn(B, n, C, HID, generator=g)).to(bf)
    for side in SIDES:
        csr64, _ = side_csr(graph, G, side)
        csr32 = (csr64[0], csr64[1], csr64[2].float())
        csr, blocks, _ = device_side(graph, side)
        Y_w, dY_w, Cand_w, Hn_w = (torch.empty(B, n, C, HID) for _ in range(4))
        EM.spmm_sum(*csr32, None, f(X), f(X2), [(f(t), o) for t, o in adds], Y_w, blend=(f(U), f(Cand), dY_w))
        A, Hp = adds[0][0], X
        EM.spmm_blend_fwd(*csr32, None, f(X), f(A), f(U), f(Hp), Cand_w, Hn_w)
        for plan in (blocks, None):
            Y, dY = nan_plane(n, bf), nan_plane(n, bf)
            launch = lambda: hip.bf16.spmm_sum(*csr, plan, cu(X), cu(X2), [(cu(t), o) for t, o in adds], Y, blend=(cu(U), cu(Cand), dY))
            assert ran(hip, launch) == ['stc_spmm_sum_bf16']
            share = float((Y.float().cpu() != Y_w.to(bf).float()).float().mean())
            print(f'{name} {H}x{W} {side} {"blocked" if plan is not None else "csr"}: {share:.5f} of Y differs from the reference')
            assert_one_ulp(Y, Y_w.to(bf), max_mismatch=0.05)
            _close(dY, dY_w, tol=2.0 ** -7)
            Cd, Hn = nan_plane(n, bf), nan_plane(n, bf)
            assert ran(hip, lambda: hip.bf16.spmm_blend_fwd(*csr, plan, cu(X), cu(A), cu(U), cu(Hp), Cd, Hn)) == ['stc_spmm_blend_fwd_bf16']
            _close(Cd, Cand_w, tol=2.0 ** -7)
            _close(Hn, Hn_w, tol=2.0 ** -7)


# ------------------------------------------------------------------------------------------------------- what the queen grid could not see
def _rotated_values(graph, side):
    """The two-ring tables with the VALUE column of every row rotated by one entry within the row's live entries: every value goes with its
    neighbour's source row.  The offsets are untouched, so every access stays where the real plan puts it."""
    h = graph._host
    lens = np.diff(h[f'{side}_rowptr'])
    out = []
    for table, rows in ((h[f'{side}_r2_t1'], h[f'{side}_r2_l1']), (h[f'{side}_r2_t2'], h[f'{side}_r2_own'])):
        table = table.copy()
        for p, r in zip(*np.nonzero(rows >= 0)):
            k = lens[rows[p, r] & 0x3FFFFFFF]
            table[p, r, :k, 1] = np.roll(table[p, r, :k, 1], 1)
        out.append(torch.from_numpy(table).cuda())
    return out


@pytest.mark.gpu
def test_rotated_values_show_on_weights_and_not_on_the_queen_grid(hip):
    """``hip.ring2_sum`` with a plan whose values are paired with the wrong entries (``_rotated_values``).  On ``weights`` at 12 x 20 the elementwise
    check fails by far (asserted: more than 100 times the bound; seen: 1.2e7 (Y), 1.9e6 (Z)).  On the row-stochastic 12 x 20 queen grid the rows whose two
    rings lie wholly off the border come out bit for bit as with the true plan: the blindness this file closes.  (There every entry of a row carries
    1 / deg, so the rotation leaves the tables themselves as they were, border rows included: asserted on the host.)"""
    from stc_hip import CsrGraph
    Hg, Wg, n = 12, 20, 240
    rnd = drawer(7, n)
    X, add, U, Cand = rnd(), rnd(), torch.sigmoid(rnd()), torch.tanh(rnd())

    def launch(csr, ring2):
        Y, Z = nan_plane(n), nan_plane(n)
        hip.ring2_sum(*csr, ring2, cu(X), None, [cu(add)], cu(U), cu(Cand), Y, Z)
        return Y, Z

    graph, G = GC.case('weights', Hg, Wg)
    csr64, _ = side_csr(graph, G, 'bwd')
    csr, _, ring2 = device_side(graph, 'bwd')
    Y_w, Z_w = new64(n), new64(n)
    EM.ring2_sum(*csr64, None, d(X), None, [d(add)], d(U), d(Cand), Y_w, Z_w)
    M1 = first_stage_magnitude(csr64, X, None, 1.0, [(add, 1.0)])
    M2 = agg(magnitudes(csr64), M1 * d(U) * (1 + d(Cand) ** 2))
    Y, Z = launch(csr, ring2)
    assert_within(Y, Y_w, M1, C_FIRST(1), 'true plan Y')
    assert_within(Z, Z_w, M2, C_SECOND(1), 'true plan Z')
    Y, Z = launch(csr, ring2[:3] + tuple(_rotated_values(graph, 'bwd')))
    ratios = (ratio_to_bound(Y, Y_w, M1, C_FIRST(1)), ratio_to_bound(Z, Z_w, M2, C_SECOND(1)))
    print(f'rotated values on weights: {ratios[0]:.3g} (Y) and {ratios[1]:.3g} (Z) times the bound')
    assert min(ratios) > 100

    queen = CsrGraph.queen_grid(Hg, Wg, normalize=True)
    csr, _, ring2 = device_side(queen, 'bwd')
    Y, Z = launch(csr, ring2)
    Yr, Zr = launch(csr, ring2[:3] + tuple(_rotated_values(queen, 'bwd')))
    i, j = np.divmod(np.arange(n), Wg)
    interior = torch.from_numpy((i >= 3) & (i <= Hg - 4) & (j >= 3) & (j <= Wg - 4)).cuda()
    assert int(interior.sum()) == 6 * 14
    assert torch.equal(Yr[:, interior], Y[:, interior]) and torch.equal(Zr[:, interior], Z[:, interior])
    for rotated, key in zip(_rotated_values(queen, 'bwd'), ('bwd_r2_t1', 'bwd_r2_t2')):
        assert np.array_equal(rotated.cpu().numpy(), queen._host[key])  # equal weights inside every row: the wrong pairing is the same table
    assert not all(np.array_equal(r.cpu().numpy(), graph._host[k]) for r, k in zip(_rotated_values(graph, 'bwd'), ('bwd_r2_t1', 'bwd_r2_t2')))


# ------------------------------------------------------------------------------------------------------- the executor on such graphs
@pytest.mark.parametrize('dev', ['cpu-emulated', pytest.param('cuda', marks=pytest.mark.gpu)])
@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('name', ['ragged', 'one_way', 'one_side'])
def test_cell_graph_on_weighted_graphs_against_float64(name, K, dev, monkeypatch):
    """The schedule of tests/test_ring2.py::test_cell_graph_with_and_without_the_two_ring_launches (three chained planar cells, states consumed as
    X and as H) through ``ops.stc_cell_graph`` on graphs scaled to unit row sums: ``ragged`` and ``one_way`` at 12 x 20, and ``one_side`` (a
    two-ring plan for Gs only: the forward keeps its two launches, the backward fuses).  With the two-ring launches on and off: same state, same
    gradients (3e-6), and both equal to the reference's cell (oracle.stc_oracle.stc_cell) chained in float64 on the dense matrix, within
    tests/test_module_parity.py's FWD / GRAD.  Which two-ring entry points run follows from the plans the graph has.  ``cpu-emulated``: the same
    through the fp32 twins on the CPU (the host's routing and the reference, without a GPU).  Seen on the MI355X: on / off within 2.6e-7, the
    state within 5.6e-7 and the gradients within 5.1e-7 of float64 (the twins: 4.5e-7 and 6.1e-7)."""
    from oracle import stc_oracle as O
    from stc_hip import ops
    from tests.test_module_parity import FWD, GRAD, _close
    monkeypatch.setattr(ops, '_kernels', None if dev == 'cuda' else EM)      # (None: HipKernels() on first use)
    dev = torch.device('cuda' if dev == 'cuda' else 'cpu')
    graph, G = GC.case(name, unit=True)
    n = graph.n
    op = csr_operand(graph, dev)
    fwd, bwd, clusters = GC.PLANS[name]
    assert (op.fwd_ring2 is not None, op.bwd_ring2 is not None, op.ring2_clusters) == (fwd, bwd, clusters)
    g = torch.Generator().manual_seed(K)
    Gc = torch.rand(C, C, generator=g)
    Gc = Gc / Gc.sum(1, keepdim=True)
    Tc = ops.cheby_dense(Gc.to(dev), K)
    rows = K * K * 2 * HID
    base = [torch.randn(B, n, C, HID, generator=g), torch.tanh(torch.randn(B, n, C, HID, generator=g)),
            torch.randn(rows, 2 * HID, generator=g) * 0.1, torch.zeros(2 * HID), torch.randn(rows, HID, generator=g) * 0.1, torch.zeros(HID),
            torch.randn(B, n, C, HID, generator=g)]
    schedule = [(0, ('ext', 0), ('ext', 1)), (0, ('cell', 0), ('cell', 0)), (0, ('cell', 1), ('cell', 0))]
    assert ops.cell_graph_supported(op, Tc, K, C, HID, [HID])

    def run(on):
        monkeypatch.setattr(ops, '_RING2', on)
        monkeypatch.setattr(ops, '_RING2_FWD', on)
        Xt, Ht, Wg, bg, Wc, bc, R = (t.clone().to(dev) for t in base)
        leaves = [t.requires_grad_() for t in (Wg, bg, Wc, bc)]
        out = ops.stc_cell_graph(op, Tc, K, schedule, [2], [Xt, Ht], [(Wg, bg, Wc, bc)])[0]
        (out * R).sum().backward()
        return [out.detach()] + [t.grad for t in leaves]

    seen = []
    real = type(ops.kernels())
    for entry in ('ring2_sum', 'ring2_blend', 'ring2_blend_first', 'ring2_chain'):
        fn = getattr(real, entry, None)
        if fn is None:                                                # (the twin has no first-step forms: the executor does not ask it for them)
            continue
        monkeypatch.setattr(real, entry, (lambda f_, nm: lambda self, *a, **kw: (seen.append(nm), f_(self, *a, **kw))[1])(fn, entry))
    with_ring2 = run(True)
    used = set(seen)
    seen.clear()
    without = run(False)
    assert not seen
    if K == 3:                     # the chain form: the forward recurrence on Gs^T's plan, its transpose on Gs's
        expected = {'ring2_chain'} if (fwd or bwd) else set()
    else:                          # the blend form on Gs^T's plan (lattice tiles only), the sum form on Gs's
        expected = ({'ring2_blend'} if fwd and not clusters else set()) | ({'ring2_sum'} if bwd else set())
    assert used == expected, used
    # the reference's cell, chained in float64 on the dense matrix
    Xt, Ht, Wg, bg, Wc, bc, R = (t.double() for t in base)
    leaves = [t.requires_grad_() for t in (Wg, bg, Wc, bc)]
    ext, states = [Xt, Ht], []
    for _, x, hs in schedule:
        src = lambda ref: ext[ref[1]] if ref[0] == 'ext' else states[ref[1]]
        states.append(O.stc_cell(G, Gc.double(), src(x), src(hs), Wg, bg, Wc, bc, K, K))
    (states[2] * R).sum().backward()
    want = [states[2].detach()] + [t.grad for t in leaves]
    names = ('state', 'dWg', 'dbg', 'dWc', 'dbc')
    for what, a, b, w in zip(names, with_ring2, without, want):
        e = (rel_err(a, b), rel_err(a, w), rel_err(b, w))
        print(f'{name} K={K} {what}: on/off {e[0]:.2e}, against float64 {e[1]:.2e} (on) {e[2]:.2e} (off)')
    for what, a, b, w in zip(names, with_ring2, without, want):
        assert rel_err(a, b) < 3e-6
        for got in (a, b):
            _close(got.cpu(), w, FWD if what == 'state' else GRAD, f'{name} K={K} {what}')
