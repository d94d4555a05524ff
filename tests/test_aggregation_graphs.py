"""The graph family of tests/graph_cases.py (weighted, ragged, one-way, renumbered, one-sided) on the host: which plans each case gets, the
two-ring tables against the matrix in both orientations, and the float64 twins of the fused aggregation kernels against dense float64 algebra.
What the GPU tests of tests/test_aggregation_kernels.py stand on: their reference and their a-priori error bound are defined here and checked
here, without a GPU, on the fp32 twin.

The elementwise bound (``assert_within``): a result of the linear forms -- sum, chain, and the first stages of both -- is a sum of products,
each formed with a known number of fp32 roundings, so

    |got - want| <= c * 2^-24 * M      per element,

where M is the same expression evaluated on magnitudes (|S| applied to |X| + |X2|, plus sum |scale * addend|; second stage: |S| applied to the
first stage's M, in the sum form first multiplied by U (1 + Cand^2) -- not |1 - Cand^2|: the kernel forms 1 - Cand^2 in fp32) and c counts
the roundings on the path (``C_FIRST``, ``C_SECOND``).  Where M == 0 (an empty row without addends) the result must be exactly 0.  Unlike
max|a - b| / max|b| over a plane, this holds every row to its own scale: a row that is wrong but small fails.
"""
import numpy as np
import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip.graph import csr_operand
from tests import graph_cases as GC
from tests.test_bf16_kernels import assert_one_ulp
from tests.test_ring2 import check_two_ring_plan

EM = EmulatedKernels()
U24 = 2.0 ** -24
ALL = GC.grid_params(tuple(GC.CASES))
FAMILY = GC.grid_params()                                   # the four cases with two-ring plans on both orientations


def C_FIRST(n_add):
    """Roundings on the way to a first-stage element: 8 table entries (one fmaf each), X + X2, one per addend, alpha."""
    return 8 + 1 + n_add + 1


def C_SECOND(n_add, n_interior=0):
    """... to a second-stage element: the first stage's, 4 for the elementwise factors (Cand^2, 1 - ., two products), 8 table entries, the
    interior's addends."""
    return C_FIRST(n_add) + 4 + 8 + n_interior


def side_csr(graph, G, side, dtype=torch.float64):
    """(rowptr, colidx, val) of one orientation on the CPU and the dense matrix they stand for: 'bwd' = Gs, 'fwd' = Gs^T."""
    op = csr_operand(graph, torch.device('cpu'))
    csr = (getattr(op, f'{side}_rowptr'), getattr(op, f'{side}_colidx'), getattr(op, f'{side}_val').to(dtype))
    return csr, (G if side == 'bwd' else G.t().contiguous())


def agg(csr, T, alpha=1.0):
    """alpha S.T over the node axis of T (B, n, C, h), by the twin of the plain aggregation in T's precision."""
    B, n, Cc, h = T.shape
    out = torch.empty(B, n, Cc * h, dtype=T.dtype)
    EM.csr_spmm(csr[0], csr[1], csr[2].to(T.dtype), n, n, T.reshape(B, n, Cc * h), None, out, float(alpha), 0.0)
    return out.view(B, n, Cc, h)


def magnitudes(csr):
    return csr[0], csr[1], csr[2].abs()


def first_stage_magnitude(csr, X, X2, alpha, scaled_addends):
    """M of  alpha S.(X [+ X2]) + sum scale * addend  (float64)."""
    d = lambda t: t.double().abs()
    M = agg(magnitudes(csr), d(X) + (0 if X2 is None else d(X2)), abs(alpha))
    for t, s in scaled_addends:
        M = M + abs(s) * d(t)
    return M


def ratio_to_bound(got, want, M, c):
    """Largest |got - want| / (c 2^-24 M) over the elements with M > 0."""
    got, want, live = got.detach().double().cpu(), want.double(), M > 0
    return float(((got - want).abs()[live] / (c * U24 * M[live])).max()) if bool(live.any()) else 0.0


def assert_within(got, want, M, c, what=''):
    """``got`` within c 2^-24 M of ``want`` elementwise, exactly 0 where M == 0; returns the largest ratio to the bound (printed)."""
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f'{what}: not finite (a plane the launch did not write?)'
    assert bool((got[M == 0] == 0).all()), f'{what}: non-zero where every term is zero'
    ratio = ratio_to_bound(got, want, M, c)
    print(f'{what}: {ratio:.3f} of the bound (c = {c})')
    assert ratio <= 1.0, f'{what}: {ratio:.3g} times the bound c 2^-24 M, c = {c}'
    return ratio


def draw(seed, B, n, Cc, h=16):
    """Operands as the kernel tests draw them: a seeded generator on the CPU."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.randn(B, n, Cc, h, generator=g)
    return g, rnd


# ---------------------------------------------------------------------------------------------------------------- plans
@pytest.mark.parametrize('name,H,W', ALL)
def test_every_case_gets_the_plans_it_promises(name, H, W):
    """Asserted, not skipped on: a GPU test on a case that lost its plan would silently run another kernel.  Unit scaling and positive weights
    keep the pattern, hence the plans."""
    fwd, bwd, clusters = GC.PLANS[name]
    for kw in (dict(), dict(unit=True)) + ((dict(positive=True),) if name in ('ragged', 'one_way') else ()):
        graph, G = GC.case(name, H, W, **kw)
        h = graph._host
        assert ('fwd_r2_l2' in h, 'bwd_r2_l2' in h, graph.ring2_clusters) == (fwd, bwd, clusters)
        assert 'bwd_blk_ptr' in h and 'fwd_blk_ptr' in h
        if fwd and bwd:
            assert 'fwd_pt_src' in h and 'bwd_pt_src' in h
            n_p = (h['fwd_r2_l2'].shape[0], h['bwd_r2_l2'].shape[0])
            assert min(n_p) > 1 and (clusters or all(v % 8 for v in n_p))      # lattices: 9 and 15 patches, the workgroup-to-patch map pads
        assert graph.row_sum_bound < EM.HEAVY_ROW_SUM               # the operand format does not change with these graphs
        if kw.get('unit'):
            assert graph.row_sum_bound == pytest.approx(1.0, abs=1e-6)
        if kw.get('positive'):
            sums = G.sum(1)
            assert bool((G >= 0).all()) and bool(((sums - 1).abs() < 1e-6)[sums > 0].all())
    lens = {side: np.diff(graph._host[f'{side}_rowptr']) for side in ('fwd', 'bwd')}
    if name in ('ragged', 'one_way', 'clusters'):
        assert lens['bwd'].min() == 0 and min(map(len, map(np.unique, lens.values()))) >= 5      # empty rows, rows of many lengths
    if name == 'one_way':
        G = GC.case(name, H, W)[1]
        assert not bool(((G != 0) & (G.t() != 0)).any()) and lens['fwd'].min() == 0          # Gs and Gs^T share no entry


def test_a_small_ragged_graph_has_no_plan_at_all():
    graph, _ = GC.weighted_grid(6, 6, seed=6006, drop=0.3)
    assert not any('_r2_' in k or '_pt_' in k for k in graph._host)


@pytest.mark.parametrize('name,H,W', ALL)
def test_two_ring_plans_reproduce_the_matrix_in_both_orientations(name, H, W):
    """tests/test_ring2.py's check (the tables ARE the matrix) on graphs where a value paired with the wrong entry changes the sum; empty own rows
    and first-ring rows without entries of their own (all-zero table rows) included."""
    graph, _ = GC.case(name, H, W)
    fwd, bwd, _ = GC.PLANS[name]
    for side, has in (('fwd', fwd), ('bwd', bwd)):
        if has:
            check_two_ring_plan(graph, side)
    if name in ('ragged', 'one_way'):                              # the k = 0 branch of the plan's ``fill`` is on the path
        h = graph._host
        lens = np.diff(h['bwd_rowptr'])
        first = h['bwd_r2_l1']
        assert (lens[first[first >= 0] & 0x3FFFFFFF] == 0).any()


# ---------------------------------------------------------------------------------------------------------------- the float64 twins
@pytest.mark.parametrize('name,H,W', ALL)
def test_float64_twins_equal_dense_algebra(name, H, W):
    """``EM.spmm_sum``, ``EM.spmm_blend_fwd``, ``EM.ring2_sum``, ``EM.ring2_blend`` (also on a zero state: the first-step blend's twin) and
    ``EM.ring2_chain`` (the forward's arguments and the transposed set) in float64 against dense einsum algebra, both orientations.
    atol 1e-12 as tests/test_ring2.py; observed at most 1.5e-14."""
    graph, G = GC.case(name, H, W)
    B, n, Cc, h = 2, graph.n, 4, 16
    g = torch.Generator().manual_seed(n)
    rnd = lambda: torch.randn(B, n, Cc, h, generator=g, dtype=torch.float64)
    new = lambda: torch.empty(B, n, Cc, h, dtype=torch.float64)
    close = lambda a, b: torch.allclose(a, b, rtol=0, atol=1e-12)
    for side in ('fwd', 'bwd'):
        csr, S = side_csr(graph, G, side)
        mul = lambda t: torch.einsum('uv,bvcf->bucf', S, t)
        X, X2, U, Cand = rnd(), rnd(), torch.sigmoid(rnd()), torch.tanh(rnd())
        adds = [rnd() for _ in range(8)]
        scales = (1.0, 1.0, -1.0, 1.0, -1.0, 0.5, 1.0, -2.0)
        # sum: plain, with alpha and signed addends, with the blend epilogue
        Y, dY = new(), new()
        EM.spmm_sum(*csr, None, X, X2, [(t, 0, s) for t, s in zip(adds, scales)], Y, blend=(U, Cand, dY), alpha=-0.5)
        want = -0.5 * mul(X + X2) + sum(s * t for t, s in zip(adds, scales))
        assert close(Y, want) and close(dY, want * U * (1 - Cand * Cand))
        EM.spmm_sum(*csr, None, X, None, [], Y)
        assert close(Y, mul(X))
        # blend forward
        Bm, A, Hp = rnd(), rnd(), torch.tanh(rnd())
        Cd, Hn, SHn = new(), new(), new()
        EM.spmm_blend_fwd(*csr, None, Bm, A, U, Hp, Cd, Hn)
        cand = torch.tanh(A + mul(Bm))
        assert close(Cd, cand) and close(Hn, (1 - U) * Hp + U * cand)
        # two-ring sum, blend, first-step blend (a zero state), chain
        Z = new()
        EM.ring2_sum(*csr, None, X, X2, adds[:3], U, Cand, Y, Z)
        want = mul(X + X2) + adds[0] + adds[1] + adds[2]
        assert close(Y, want) and close(Z, mul(want * U * (1 - Cand * Cand)))
        EM.ring2_blend(*csr, None, Bm, A, U, Hp, Cd, Hn, SHn)
        assert close(Cd, cand) and close(Hn, (1 - U) * Hp + U * cand) and close(SHn, mul((1 - U) * Hp + U * cand))
        EM.ring2_blend(*csr, None, Bm, A, U, torch.zeros_like(U), Cd, Hn, SHn)
        assert close(Cd, cand) and close(Hn, U * cand) and close(SHn, mul(U * cand))
        T1, T2 = new(), new()
        EM.ring2_chain(*csr, None, X, None, 1.0, [], T1, 2.0, [(X, -1.0)], T2)
        assert close(T1, mul(X)) and close(T2, 2 * mul(mul(X)) - X)
        d0, d1, d2 = adds[:3]
        EM.ring2_chain(*csr, None, d2, None, 2.0, [d1], None, 1.0, [(d0, 1.0), (d2, -1.0)], T2)
        assert close(T2, d0 + mul(d1) + (2 * mul(mul(d2)) - d2))      # T_0 d0 + T_1 d1 + T_2 d2 of this orientation's matrix


@pytest.mark.parametrize('name,H,W', FAMILY)
def test_the_fp32_twin_is_well_inside_the_elementwise_bound(name, H, W):
    """The bound the GPU tests hold the kernels to, applied to the fp32 twin (another summation order, no fmaf): the reference and the bound are
    consistent before a kernel is involved.  Observed on this family: at most 0.31 of the bound in the first stage (4.0 2^-24 M against
    c = 13) and 0.14 in the second (c = 25) here, 0.42 (4.2 2^-24 M against c = 10) over the argument sets of the GPU tests; the largest
    ratio per case is printed."""
    graph, G = GC.case(name, H, W)
    B, n, Cc = 2, graph.n, 8
    _, rnd = draw(n + 1, B, n, Cc)
    d = lambda t: t.double()
    for side in ('fwd', 'bwd'):
        csr64, _ = side_csr(graph, G, side)
        csr32 = (csr64[0], csr64[1], csr64[2].float())
        X, X2, U, Cand = rnd(), rnd(), torch.sigmoid(rnd()), torch.tanh(rnd())
        adds = [rnd() for _ in range(3)]
        new = lambda dt: torch.empty(B, n, Cc, 16, dtype=dt)
        Y, Z, Yw, Zw = new(torch.float32), new(torch.float32), new(torch.float64), new(torch.float64)
        EM.ring2_sum(*csr32, None, X, X2, adds, U, Cand, Y, Z)
        EM.ring2_sum(*csr64, None, d(X), d(X2), [d(t) for t in adds], d(U), d(Cand), Yw, Zw)
        M1 = first_stage_magnitude(csr64, X, X2, 1.0, [(t, 1.0) for t in adds])
        M2 = agg(magnitudes(csr64), M1 * d(U) * (1 + d(Cand) ** 2))
        assert_within(Y, Yw, M1, C_FIRST(3), f'{name} {side} twin Y')
        assert_within(Z, Zw, M2, C_SECOND(3), f'{name} {side} twin Z')


@pytest.mark.parametrize('name,H,W', GC.grid_params(('ragged', 'one_way')))
def test_bf16_reference_on_positive_weights_stays_under_the_mismatch_cap(name, H, W):
    """What the bf16 GPU test compares with is the fp32 twin rounded to bf16, and it allows 5 % of the elements to differ by an ulp: the share
    of elements where that reference itself differs from the float64 twin rounded to bf16 must leave room under the cap.  Positive weights
    and unit row sums (no cancellation).  Observed: at most 7e-5 of the elements (0.007 %)."""
    bf = torch.bfloat16
    graph, G = GC.case(name, H, W, positive=True)
    B, n, Cc = 2, graph.n, 32
    g = torch.Generator().manual_seed(n + 32 + 3)
    rb = lambda: torch.randn(B, n, Cc, 16, generator=g).to(bf)
    X, X2, adds = rb(), rb(), [rb() for _ in range(3)]
    for side in ('fwd', 'bwd'):
        csr64, _ = side_csr(graph, G, side)
        Y32, Y64 = torch.empty(B, n, Cc, 16), torch.empty(B, n, Cc, 16, dtype=torch.float64)
        EM.spmm_sum(csr64[0], csr64[1], csr64[2].float(), None, X.float(), X2.float(), [(t.float(), 0) for t in adds], Y32)
        EM.spmm_sum(*csr64, None, X.double(), X2.double(), [(t.double(), 0) for t in adds], Y64)
        a, b = Y32.to(bf).float(), Y64.to(bf).float()
        share = float((a != b).float().mean())
        print(f'{name} {H}x{W} {side}: bf16 reference differs on {share:.5f} of the elements')
        assert_one_ulp(Y32.to(bf), Y64.to(bf), max_mismatch=0.05)      # the GPU test's own criterion, applied to its reference
