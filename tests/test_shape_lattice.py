"""Every kernel shape the library's predicates accept, run once (tests/shape_lattice.py holds the table, the references and the runners).

CPU: the closure of the table -- it IS the predicate (recomputed through ``load_library()``, so widening a predicate fails here until the lattice
grows), the points just outside are refused through the library, every family has points, no GPU test may skip one, and the float64 twin equals
the float64 reference expression at every point of the node and cell families.
GPU (-m gpu): one test per point and family; the only skip is no device.
"""
import ast
import inspect

import pytest
import torch

from stc_hip import _lib
from tests import shape_lattice as S
from tests.abi_refusal_table import ELIMIT, EUNSUPPORTED, P, call
from tests.test_abi_refusals import GOOD
from tests.test_abi_refusals_first_step import GOOD as GOOD_FIRST


@pytest.fixture(scope='module')
def hip():
    from stc_hip._lib import HipKernels
    return HipKernels()


# ---- CPU: closure ------------------------------------------------------------------------------------------------------------------------------
#: points per family: what the library accepts today.  A predicate that takes more turns ``test_the_table_is_the_predicate`` red (a point of the
#: margin accepted) -- the box grows, this count with it, and the GPU runs cover the new points; one that takes less loses points here
POINTS = {'mfma_node': 72, 'generic_node': 144, 'fused_cell': 54, 'planar': 10, 'one_launch': 5, 'planar_k': 5, 'first_step': 5, 'post': 10,
          'small_cell': 160, 'mix_dt': 192, 'bf16_node': 24, 'bf16_planar': 10, 'bf16_one_launch': 6, 'cheby': 28, 'fusion': 5}


@pytest.mark.parametrize('family', S.FAMILIES)
def test_the_table_is_the_predicate(family):
    """The family's points are exactly what the library accepts of its box AND of the margin around it: every argument of the predicate is
    asked beyond the box on each side (hidden widths 8 and 32, orders 1 .. STC_MAX_K, a C below, between and above), and nothing out there may be
    accepted -- a widened predicate fails here until the lattice grows.  At dispatch level 2 the matrix-core families lose every point."""
    lib = _lib.load_library()
    key = lambda p: frozenset(p.items())
    try:
        assert lib.stc_set_dispatch_level(0) == S.OK
        table = {key(S._full(p)) for p in S.LATTICE[family]}
        wide = S.margin_points(family)
        assert len(wide) > len(S.box_points(family)) or not S.MARGINS[family]
        took = {key(p) for p in wide if S.ACCEPTS[family](lib, p)}
        beyond = sorted(sorted(p) for p in took - table)
        assert not beyond, f'{family}: the library accepts {len(beyond)} points outside the lattice, first {beyond[0]}: grow the box'
        assert took == table and len(table) == len(S.LATTICE[family]) == POINTS[family], (family, len(table))
        assert len({S.point_id(p) for p in S.LATTICE[family]}) == len(S.LATTICE[family])
        assert lib.stc_set_dispatch_level(2) == S.OK
        if family in ('fused_cell', 'planar', 'one_launch', 'planar_k', 'first_step', 'post'):
            assert not any(S.ACCEPTS[family](lib, p) for p in wide), f'{family}: accepted with generic kernels only'
    finally:
        assert lib.stc_set_dispatch_level(0) == S.OK


def test_every_family_has_points_and_the_once_unlisted_ones_are_among_them():
    assert set(S.LATTICE) == set(S.BOXES) == set(S.ACCEPTS) == set(S.MARGINS) == set(POINTS) and all(len(v) >= 1 for v in S.LATTICE.values())
    ids = {f: {S.point_id(p) for p in pts} for f, pts in S.LATTICE.items()}
    # the points no hand-picked list had: C = 64 with K = 3 on the fused cell kernels (and C = 16 with K = 1), C = 9..15, 6 and 2 on the few-category
    # cells, an input plane of two columns on every planar form, C = 17..31, 33, 48, 63 and the tiles of 32, 16, 8 and 5 nodes on the generic kernel
    assert {'K3-C64-cin16', 'K3-C64-cin1', 'K1-C16-cin16'} <= ids['fused_cell']
    assert {f'C{C}-cin{cin}-K{K}' for C in (2, 6, 9, 10, 11, 12, 13, 14, 15) for cin in S.CINS for K in (2, 3)} <= ids['small_cell']
    for family in ('planar', 'one_launch', 'first_step', 'post'):
        assert 'C32-cin2' in ids[family], family
    assert 'C32-cin2-K3' in ids['planar_k'] and 'C64-cin2' in ids['planar']
    assert {f'C{C}-cls{c}' for C in list(range(17, 32)) + [33, 48, 63, 1, 2, 4, 6] for c in range(4)} <= ids['generic_node']
    assert {f'C{C}-L{L}-Ho{Ho}-K{K}' for C in range(1, 17) for L in (20, 32) for Ho in (16, 32) for K in (1, 2, 3)} == ids['mix_dt']
    assert {'C64-L32-Ho32-K3-pad0', 'C64-L20-Ho32-K3-pad3'} <= ids['mfma_node']          # (dT_c there: formed block by block, stc_hip/_lib.py)
    assert {'n127-K4', 'n128-K4', 'n65-K1'} <= ids['cheby'] and 'n128' in ids['fusion']


def test_the_generic_classes_cover_the_paths_of_the_kernel():
    """Four classes: Ks != Kc, a width that is no multiple of 4, pad columns, the bench width.  (That each fits the kernel's LDS limit at every C is
    shown by the GPU runs: a class that did not would come back as STC_ELIMIT and fail there.)"""
    cls = S.GENERIC_CLASSES
    assert len(cls) == 4 and (32, 32, 32, 2, 2) in cls
    assert any(Ks != Kc for _, _, _, Ks, Kc in cls) and any(L % 4 for L, *_ in cls) and any(Lw < L for L, Lw, *_ in cls)


#: (entry point, the one change to a call that passes every check, the code the library answers with): points just outside each predicate
OUTSIDE = [
    ('stc_cell_gates_fwd_f32', {'C': 48}, EUNSUPPORTED), ('stc_cell_gates_fwd_f32', {'Ks': 4, 'Kc': 4, 'Z': [P()] * 4}, EUNSUPPORTED),
    ('stc_cell_blend_fwd_f32', {'C': 8}, EUNSUPPORTED), ('stc_cell_cand_bwd_f32', {'L': 24, 'Lw': 24}, EUNSUPPORTED),
    ('stc_cell_gates_bwd_f32', {'C': 128}, EUNSUPPORTED),
    ('stc_cell_gates_fwd_planar_f32', {'C': 16}, EUNSUPPORTED), ('stc_cell_gates_bwd_planar_f32', {'C': 48}, EUNSUPPORTED),
    ('stc_cell_bwd_planar_f32', {'C': 64}, EUNSUPPORTED), ('stc_cell_bwd_planar_f32', {'C': 16}, EUNSUPPORTED),
    ('stc_cell_gates_fwd_planar_k_f32', {'C': 64}, EUNSUPPORTED), ('stc_cell_cand_bwd_planar_k_f32', {'K': 2}, EUNSUPPORTED),
    ('stc_cell_gates_fwd_first_f32', {'C': 64}, EUNSUPPORTED), ('stc_cell_bwd_first_f32', {'C': 16}, EUNSUPPORTED),
    ('stc_bdg_node_post_fwd_f32', {'Ho': 32}, EUNSUPPORTED), ('stc_bdg_node_post_bwd_f32', {'C': 16}, EUNSUPPORTED),
    ('stc_bdg_node_post_fwd_f32', {'L': 24, 'Lw': 24}, EUNSUPPORTED),
    ('stc_bdg_node_fwd_bf16', {'C': 16}, EUNSUPPORTED), ('stc_bdg_node_bwd_bf16', {'L': 20, 'Lw': 20}, EUNSUPPORTED),
    ('stc_cell_gates_fwd_planar_bf16', {'C': 16}, EUNSUPPORTED), ('stc_cell_bwd_planar_bf16', {'C': 64, 'Lw': 17}, EUNSUPPORTED),
    # a hidden width of 32 on every family that takes one
    ('stc_cell_gates_fwd_f32', {'h': 32, 'cin': 0}, EUNSUPPORTED), ('stc_cell_gates_bwd_f32', {'h': 32, 'cin': 0}, EUNSUPPORTED),
    ('stc_cell_cand_bwd_f32', {'h': 32}, EUNSUPPORTED), ('stc_cell_blend_fwd_f32', {'h': 32}, EUNSUPPORTED),
    ('stc_bdg_node_post_bwd_f32', {'Ho': 32}, EUNSUPPORTED), ('stc_bdg_node_post_bwd_bf16', {'Ho': 32}, EUNSUPPORTED),
] + [(fn, {'h': 32, 'Lw': 64}, EUNSUPPORTED) for fn in (
    'stc_cell_gates_fwd_planar_f32', 'stc_cell_gates_bwd_planar_f32', 'stc_cell_bwd_planar_f32', 'stc_cell_gates_fwd_planar_k_f32',
    'stc_cell_cand_fwd_planar_k_f32', 'stc_cell_gates_bwd_planar_k_f32', 'stc_cell_cand_bwd_planar_k_f32', 'stc_cell_gates_fwd_first_f32',
    'stc_cell_bwd_first_f32', 'stc_cell_gates_fwd_planar_bf16', 'stc_cell_gates_bwd_planar_bf16', 'stc_cell_bwd_planar_bf16')]


@pytest.mark.parametrize('fn,fault,code', OUTSIDE, ids=[f'{fn}-{i}' for i, (fn, _, _) in enumerate(OUTSIDE)])
def test_points_just_outside_a_predicate_are_refused(fn, fault, code):
    lib = _lib.load_library()
    rc = call(lib, GOOD_FIRST if fn in GOOD_FIRST else GOOD, fn, fault)
    assert rc == code, f'{fn}({fault}) returned {rc}: {lib.stc_last_error().decode()}'


def test_points_outside_the_predicates_without_a_call_table():
    """stc_mix_dt_f32, the few-category cells (their predicate; the entry points answer STC_EINVAL, tests/test_small_cell.py) and the limits of
    stc_cheby_dense_*."""
    lib = _lib.load_library()
    for C, L, Ho, K in ((17, 32, 32, 2), (0, 32, 32, 2), (8, 24, 32, 2), (8, 32, 24, 2), (8, 32, 32, 4)):
        assert not lib.stc_mix_dt_supported(K, K, C, L, Ho)
        assert lib.stc_mix_dt_f32(None, K, None, None, None, None, 0, 0, C, L, L, Ho, None) == EUNSUPPORTED
    for K, C, cin in ((2, 17, 16), (2, 0, 16), (2, 5, 5), (2, 5, 0), (2, 5, 8), (1, 5, 16), (4, 5, 16)):
        assert not lib.stc_cell_small_supported(K, K, C, cin, 16)
    assert not lib.stc_cell_small_supported(2, 3, 5, 16, 16) and not lib.stc_cell_small_supported(2, 2, 5, 16, 8)
    assert lib.stc_cheby_dense_fwd_f32(None, 129, 2, None, None) == ELIMIT and lib.stc_cheby_dense_fwd_f32(None, 128, S.MAX_K + 1, None, None) == ELIMIT
    assert not _lib.HipKernels.mixed_fusion_supported(None, 9) and not _lib.HipKernels.mixed_fusion_supported(None, 0)


def test_no_gpu_test_of_the_lattice_skips_a_point():
    """The only permitted skip is no device (tests/conftest.py): nothing in the two files names a skip or an expected failure."""
    import tests.test_shape_lattice as here
    for module in (here, S):
        names = {n.attr for n in ast.walk(ast.parse(inspect.getsource(module))) if isinstance(n, ast.Attribute)}
        assert not names & {'skip', 'skipif', 'xfail', 'importorskip'}, module.__name__


@pytest.mark.parametrize('family', ['mfma_node', 'generic_node', 'mix_dt'])
def test_the_float64_twin_is_the_reference_expression_on_the_node_families(family):
    for p in S.LATTICE[family]:
        S.twin_node(family, p)


@pytest.mark.parametrize('p', S.points('fused_cell'))
def test_the_float64_twin_is_the_reference_expression_on_the_fused_cells(p):
    S.twin_fused(p)


@pytest.mark.parametrize('p', S.points('planar'))
def test_the_float64_twin_is_the_reference_expression_on_the_planar_forms(p):
    S.twin_planar(p)


@pytest.mark.parametrize('C', S.BOXES['small_cell']['C'])
def test_the_float64_twin_is_the_oracle_cell_on_the_few_category_cells(C):
    for p in S.LATTICE['small_cell']:
        if p['C'] == C:
            S.twin_small(p)


# ---- GPU: one run per point ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('level', [0, 1])
@pytest.mark.parametrize('p', S.points('mfma_node'))
def test_matrix_core_node_kernels(hip, p, level):
    S.run_node(hip, 'mfma_node', p, level)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('generic_node'))
def test_generic_node_kernel(hip, p):
    S.run_node(hip, 'generic_node', p, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('level', [0, 2])
@pytest.mark.parametrize('C', [1, 5, 15])
def test_generic_node_kernel_at_the_widths_of_hidden_32(hip, C, level):
    """``S.HIDDEN32_GATES``: what STCGNN(hidden_dim=32) asks of the node backward on its per-cell path (tests/test_model_lattice.py, route
    hidden32).  With the tile fixed at 32 category rows the launch was refused for EVERY C (173 328 B of LDS at C = 5); the tile now shrinks to fit.
    C = 1: 32 nodes per tile become 22; C = 5: 6 become 4; C = 15: 2 become 1, the most categories that fit with dT_c.  More nodes than two
    default tiles, so the shrunken tiles number at least three and the last one is ragged."""
    nodes = 2 * (32 // C) + 1
    S.run_node_shape(hip, (nodes, C, *S.HIDDEN32_GATES), S.seed_of('hidden32', dict(C=C)), ('hidden32', C), f'hidden-32 gates C={C} level {level}', level)


@pytest.mark.gpu
@pytest.mark.parametrize('C,want_dT', [(16, True), (22, False), (32, False)])
def test_generic_node_kernel_declines_hidden_32_beyond_its_lds(hip, C, want_dT):
    """... and just beyond what fits with one node per tile the backward still answers STC_ELIMIT, before any launch: no silent fall-back."""
    from stc_hip._lib import StcError
    shape = (3, C, *S.HIDDEN32_GATES)
    d = S.node_operands(*shape, seed=7)
    Zs, Tc, W, dY = S.cu(d['Zs']), S.cu(d['Tc']), S.cu(d['W']), S.cu(d['dY'])
    with S.at_level(hip, 2), pytest.raises(StcError) as err:
        hip.bdg_node_bwd(Zs, Tc, W, dY, [S.nan(3, C, 64), S.nan(3, C, 64)], S.nan(*W.shape), S.nan(64), S.nan(2, C, C) if want_dT else None)
    assert err.value.code == ELIMIT, err.value


@pytest.mark.gpu
@pytest.mark.parametrize('level', [0, 1])
@pytest.mark.parametrize('p', S.points('fused_cell'))
def test_fused_cell_kernels(hip, p, level):
    S.run_fused(hip, p, level)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('planar'))
def test_planar_cell_kernels(hip, p):
    S.run_planar(hip, p)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('one_launch'))
def test_cell_backward_in_one_launch(hip, p):
    S.run_one_launch(hip, p)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('planar_k'))
def test_planar_cell_kernels_of_order_3(hip, p):
    """The body of tests/test_hip_kernels.py's order-3 test at the lattice's points, on both operand formats."""
    from tests.test_hip_kernels import test_planar_cell_kernels_order3 as body
    assert (p['C'], p['K']) == (32, 3)                       # what that body is written for: a wider predicate needs a wider body
    for k in S.formats(hip):
        body(k, 5, p['cin'])


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('first_step'))
def test_first_step_cells(hip, p):
    """The body of tests/test_first_step_kernels.py (the general kernels on planes of zeros are the reference, bit for bit; both formats)."""
    from tests.test_first_step_kernels import test_gates_forward_and_backward_equal_the_general_kernels_on_zero_planes as body
    assert p['C'] == 32
    body(hip, 5, p['cin'])


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('post'))
def test_post_aggregation_on_interleaved_rows(hip, p):
    S.run_post(hip, p)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('small_cell'))
def test_few_category_cell_kernels(hip, p):
    S.run_small(hip, p)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('mix_dt'))
def test_mix_dt_and_the_packed_node_route(hip, p):
    S.run_mix_dt(hip, p)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('bf16_node'))
def test_bf16_node_kernels(hip, p):
    """The bodies of tests/test_bf16_kernels.py (the twin with the kernels' rounding points is the bf16 contract), full and padded rows."""
    from tests import test_bf16_kernels as B
    for Lw in (p['L'], p['L'] - 3):
        shape = (5, p['C'], p['L'], Lw, p['Ho'], p['K'])
        for flag in (True, False):
            B.test_bdg_node_fwd_bf16(hip, shape, flag)
            B.test_bdg_node_bwd_bf16(hip, shape, flag)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('bf16_planar'))
def test_bf16_planar_cell_kernels(hip, p):
    from tests import test_bf16_kernels as B
    B.test_planar_cell_kernels_bf16(hip, 5, p['C'], p['cin'])


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('bf16_one_launch'))
def test_bf16_cell_backward_in_one_launch(hip, p):
    from tests import test_bf16_kernels as B
    B.test_cell_backward_in_one_launch_bf16(hip, 5, p['C'], p['cin'])


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('cheby'))
def test_dense_chebyshev_stack(hip, p):
    S.run_cheby(hip, p)


@pytest.mark.gpu
@pytest.mark.parametrize('p', S.points('fusion'))
def test_mixed_fusion(hip, p):
    S.run_fusion(p)
