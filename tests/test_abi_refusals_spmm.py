"""What the C front of the spatial aggregation refuses, pinned without a GPU (the companion of tests/test_abi_refusals.py).

Every case is a call that would launch a kernel except for ONE fault, which fires before the first HIP call: the test reads the status
code and ``stc_last_error()``.  Pointers are addresses inside a host buffer and are never dereferenced; only the addend pointer arrays
(and the fp32 sum's ld / off arrays) are read.  The empty launch is in the table too: it returns STC_OK without a launch.

The 15 entry points: plain products (csrc/stc_spmm.hip, stc_spmm_bf16.hip, stc_spmm_patch.hip, stc_dense.hip), the sampled product, and
the state-row forms with their blend / sum epilogues (stc_spmm.hip, stc_spmm_bf16.hip: both launch the kernels of stc_spmm_gather.h) and two-ring
launches (stc_spmm_ring2.hip).  Where fronts answer one fault with different codes the table records each as it is: too many addends is STC_EINVAL on stc_spmm_sum_* and
STC_ELIMIT on stc_ring2_*; a batch above 65535 is STC_ELIMIT everywhere but STC_EINVAL on stc_ring2_*; fewer than one category is
STC_EINVAL on the row-blocked fronts and STC_EUNSUPPORTED on stc_ring2_*; n_cols == 0 with rows to produce is refused by the CSR, bf16 and
state-row fronts only.  Not in the table, because they are no refusals: stc_csr_spmm_f32 with a misaligned operand or F % 4 != 0 (it
falls through to the generic kernel), and null column / value arrays (legal for a graph without entries).
"""
import ctypes

import pytest

from stc_hip import _lib
from tests.abi_refusal_table import EALIGN, EINVAL, ELIMIT, EUNSUPPORTED, MIS, ODD, OK, P, PP, case_into, check_refusal, with_null


def I32(*v):
    return (ctypes.c_int32 * len(v))(*v)


# ---- per entry point: (argument name, value of a call that passes every check), in ABI order
def _plain(graph, F):
    return dict(**{name: P() for name in graph}, n_rows=8, n_cols=8, X=P(), Y0=None, Y=P(), batch=2, F=F, alpha=1.0, beta=0.0, stream=None)


def _patch(F):
    return dict(patch_src=P(), patch_rows=P(), patch_cnt=P(), patch_idx=P(), patch_val=P(), n_patches=1, width=8,
                n_rows=8, n_cols=8, X=P(), Y0=None, Y=P(), batch=2, F=F, alpha=1.0, beta=0.0, stream=None)


def _graph():
    return dict(rowptr=P(), colidx=P(), val=P(), blk_ptr=P(), blk_cols=P(), blk_vals=P(), n_rows=8, n_cols=8)


def _ring2():
    return dict(l2_rows=P(), l1_rows=P(), int_rows=P(), t1=P(), t2=P(), n_patches=1, n_rows=8)


STATE = dict(batch=2, C=32, h=16, stream=None)
CSR, BCSR = ('rowptr', 'colidx', 'val'), ('blk_ptr', 'blk_cols', 'blk_vals')
GOOD = {
    'stc_csr_spmm_f32': _plain(CSR, 64),
    'stc_bcsr_spmm_f32': _plain(BCSR, 64),
    'stc_csr_spmm_bf16': _plain(CSR, 64),
    'stc_bcsr_spmm_bf16': _plain(BCSR, 64),
    'stc_patch_spmm_f32': _patch(256),
    'stc_patch_spmm_bf16': _patch(512),
    'stc_dense_agg_f32': dict(S=P(), n_rows=8, n_cols=8, X=P(), Y0=None, Y=P(), batch=2, F=64, alpha=1.0, beta=0.0, stream=None),
    'stc_csr_sddmm_f32': dict(rowptr=P(), colidx=P(), n_rows=8, n_cols=8, A=P(), Bm=P(), out=P(), batch=2, F=64, alpha=1.0, accumulate=0, stream=None),
    'stc_spmm_blend_fwd_f32': dict(**_graph(), Bm=P(), A=P(), U=P(), H=P(), Cand=P(), Hnew=P(),
                                   copy0=None, copy0_ld=0, copy0_off=0, side_src=None, side_cin=0, copy1=None, copy1_ld=0, copy1_off=0, **STATE),
    'stc_spmm_blend_fwd_bf16': dict(**_graph(), Bm=P(), A=P(), U=P(), H=P(), Cand=P(), Hnew=P(), **STATE),
    'stc_spmm_sum_f32': dict(**_graph(), X=P(), X2=None, alpha=1.0, n_add=2, add=PP(2), add_ld=I32(16, 16), add_off=I32(0, 0), add_scale=None,
                             Y=P(), U=None, Cand=None, dY=None, amax=None, n_amax=0, **STATE),
    'stc_spmm_sum_bf16': dict(**_graph(), X=P(), X2=None, n_add=2, add=PP(2), Y=P(), U=None, Cand=None, dY=None, **STATE),
    'stc_ring2_sum_f32': dict(**_ring2(), A=P(), A2=None, n_add=2, add=PP(2), U=P(), Cand=P(), Y=P(), Z=P(), **STATE),
    'stc_ring2_blend_f32': dict(**_ring2(), Bm=P(), A=P(), U=P(), H=P(), Cand=P(), Hnew=P(), SHnew=P(), **STATE),
    'stc_ring2_chain_f32': dict(**_ring2(), A=P(), A2=None, alpha1=1.0, n_add1=1, add1=PP(1), V=P(), alpha2=2.0, n_add0=2, add0=PP(2), scale0=None,
                                Z=P(), **STATE),
}


def _z(fn, name):
    return GOOD[fn][name]


CASES = []
case = case_into(CASES)


# ---------------------------------------------------------------- plain products  Y = alpha S.X + beta Y0
def plain_cases(fn, sizes=('n_rows', 'n_cols', 'batch', 'F')):
    for name in sizes:
        case(fn, {name: -1}, EINVAL, 'negative size')
    for name in ('n_rows', 'batch', 'F'):
        case(fn, {name: 0}, OK)
    case(fn, {'X': None}, EINVAL, 'null')
    case(fn, {'Y': None}, EINVAL, 'null')
    case(fn, {'beta': -1.0}, EINVAL, 'beta != 0 needs Y0')
    case(fn, {'Y': _z(fn, 'X')}, EINVAL, 'X must not alias Y')


def aligned_cases(fn):
    case(fn, {'X': MIS}, EALIGN, '16-byte aligned')
    case(fn, {'Y': MIS}, EALIGN, '16-byte aligned')
    case(fn, {'Y0': MIS}, EALIGN, '16-byte aligned')               # (checked whatever beta is)
    case(fn, {'Y0': MIS, 'beta': -1.0}, EALIGN, '16-byte aligned')


def batch_case(fn, code=ELIMIT):
    case(fn, {'batch': 65536}, code, *(('65535',) if code == ELIMIT else ('bad sizes',)))


fn = 'stc_csr_spmm_f32'
plain_cases(fn)
batch_case(fn)
case(fn, {'rowptr': None}, EINVAL, 'null')
case(fn, {'n_cols': 0}, EINVAL, 'n_cols == 0')

fn = 'stc_bcsr_spmm_f32'
plain_cases(fn)
aligned_cases(fn)
batch_case(fn)
case(fn, {'blk_ptr': None}, EINVAL, 'null')
case(fn, {'F': 66}, EINVAL, 'F=66', 'multiple of 4')
case(fn, {'F': 2}, EINVAL, 'F=2', 'multiple of 4')

for fn, graph in (('stc_csr_spmm_bf16', 'rowptr'), ('stc_bcsr_spmm_bf16', 'blk_ptr')):
    plain_cases(fn)
    aligned_cases(fn)
    batch_case(fn)
    case(fn, {graph: None}, EINVAL, 'null')
    case(fn, {'n_cols': 0}, EINVAL, 'n_cols == 0')
    case(fn, {'F': 68}, EINVAL, 'F=68', 'multiple of 8')

for fn, F in (('stc_patch_spmm_f32', 256), ('stc_patch_spmm_bf16', 512)):
    plain_cases(fn, sizes=('n_rows', 'n_cols', 'batch', 'F', 'n_patches'))
    aligned_cases(fn)
    batch_case(fn)
    for name in ('patch_src', 'patch_rows', 'patch_cnt', 'patch_idx', 'patch_val'):
        case(fn, {name: None}, EINVAL, 'null')
    case(fn, {'n_patches': 0}, EINVAL, 'cannot cover 8 rows')
    case(fn, {'n_rows': 33}, EINVAL, '1 patches', 'cannot cover 33 rows')
    case(fn, {'F': F // 2}, EUNSUPPORTED, f'F={F // 2}', f'multiple of {F}', '1 KiB')
    case(fn, {'F': F + 8}, EUNSUPPORTED, f'multiple of {F}')
    case(fn, {'width': 5}, EUNSUPPORTED, 'width 5')          # (the only refusal of the launch helper that needs no device)
    case(fn, {'width': 0}, EUNSUPPORTED, 'width 0')

fn = 'stc_dense_agg_f32'
plain_cases(fn)
case(fn, {'S': None}, EINVAL, 'null')
case(fn, {'n_rows': 1 << 16, 'n_cols': 1 << 16}, ELIMIT, 'too large')                  # S of 2^32 elements
case(fn, {'batch': 1 << 20, 'n_rows': 1 << 14}, ELIMIT, 'too large')                   # planes of 2^40 elements
case(fn, {'batch': 1 << 30, 'n_rows': 1, 'F': 128}, ELIMIT, 'workgroups')
case(fn, {'n_rows': (1 << 23) + (1 << 10)}, ELIMIT, 'row passes')

fn = 'stc_csr_sddmm_f32'
for name in ('n_rows', 'n_cols', 'batch', 'F'):
    case(fn, {name: -1}, EINVAL, 'negative size')
case(fn, {'n_rows': 0}, OK)
for name in ('rowptr', 'colidx', 'out', 'A', 'Bm'):
    case(fn, {name: None}, EINVAL, 'null')


# ---------------------------------------------------------------- state rows of C x 16 floats: blend and sum epilogues
def state_row_cases(fn, sizes, first, second):
    """``first``: the gathered operand; ``second``: the other plane checked with it."""
    case(fn, {'h': 8}, EUNSUPPORTED, 'hidden width 8')
    for name in sizes:
        case(fn, {name: -1}, EINVAL, 'bad sizes')
    case(fn, {'C': 0}, EINVAL, 'bad sizes')
    batch_case(fn)
    case(fn, {'n_rows': 0}, OK)
    case(fn, {'batch': 0}, OK)
    case(fn, {'rowptr': None, 'blk_ptr': None}, EINVAL, 'neither graph form')
    for name in (first, second):
        case(fn, {name: None}, EINVAL, 'null')
        case(fn, {name: MIS}, EALIGN, '16-byte aligned')
    case(fn, {'n_cols': 0}, EINVAL, 'null')


def addend_cases(fn, add, results, what='addend'):
    ptrs = _z(fn, add)
    case(fn, {add: with_null(ptrs, 0)}, EINVAL, f'{what} 0', 'null')
    case(fn, {add: with_null(ptrs, len(ptrs) - 1, MIS)}, EINVAL, f'{what} {len(ptrs) - 1}', 'aligned')
    for name in results:
        case(fn, {add: with_null(ptrs, 0, _z(fn, name))}, EINVAL, 'addend', 'alias')


def dy_cases(fn):
    case(fn, {'dY': P()}, EINVAL, 'dY needs U and Cand')
    case(fn, {'dY': P(), 'U': P()}, EINVAL, 'dY needs U and Cand')
    case(fn, {'dY': P(), 'Cand': P()}, EINVAL, 'dY needs U and Cand')
    case(fn, {'dY': P(), 'U': MIS, 'Cand': P()}, EINVAL, 'dY needs U and Cand', '16-byte aligned')
    case(fn, {'dY': P(), 'U': P(), 'Cand': MIS}, EINVAL, 'dY needs U and Cand', '16-byte aligned')
    case(fn, {'dY': MIS, 'U': P(), 'Cand': P()}, EINVAL, 'dY needs U and Cand', '16-byte aligned')
    case(fn, {'dY': _z(fn, 'Y'), 'U': P(), 'Cand': P()}, EINVAL, 'dY needs U and Cand', 'aliasing Y')


fn = 'stc_spmm_blend_fwd_f32'
state_row_cases(fn, ('n_rows', 'n_cols', 'batch'), 'Bm', 'A')
case(fn, {'C': 3}, ELIMIT, '48 floats', 'too narrow')
for name in ('U', 'H', 'Hnew'):
    case(fn, {name: None}, EINVAL, 'null')
for name in ('U', 'H', 'Cand', 'Hnew'):
    case(fn, {name: MIS}, EALIGN, '16-byte aligned')
for name in ('Cand', 'Hnew'):
    case(fn, {name: _z(fn, 'Bm')}, EINVAL, 'must not alias Bm')
case(fn, {'copy0': P(), 'copy0_ld': 20, 'copy0_off': 8}, EINVAL, 'do not fit', 'off+16')
case(fn, {'copy1': P(), 'copy1_ld': 32, 'copy1_off': -1}, EINVAL, 'do not fit')
case(fn, {'copy1': P(), 'copy1_ld': 32, 'copy1_off': 20}, EINVAL, 'do not fit')
case(fn, {'side_src': P()}, EINVAL, 'side_src needs copy0')
case(fn, {'copy0': P(), 'copy0_ld': 32, 'copy0_off': 4, 'side_src': P(), 'side_cin': 3}, EINVAL, 'side_src needs copy0', 'copy0_off == side_cin')
case(fn, {'copy0': ODD, 'copy0_ld': 20, 'copy0_off': 1}, EALIGN, 'misaligned copy destination')
case(fn, {'copy1': ODD, 'copy1_ld': 32, 'copy1_off': 16}, EALIGN, 'misaligned copy destination')
case(fn, {'copy0': MIS, 'copy0_ld': 32, 'copy0_off': 16}, EALIGN, 'copy0 not 16-byte aligned')
case(fn, {'copy1': MIS, 'copy1_ld': 32, 'copy1_off': 0}, EALIGN, 'copy1 not 16-byte aligned')

fn = 'stc_spmm_blend_fwd_bf16'
state_row_cases(fn, ('n_rows', 'batch'), 'Bm', 'A')
case(fn, {'n_cols': -1}, EINVAL, 'null')                    # (this front has no size check of its own for n_cols)
for name in ('U', 'H', 'Cand', 'Hnew'):
    case(fn, {name: None}, EINVAL, 'null')
    case(fn, {name: MIS}, EALIGN, '16-byte aligned')
for name in ('Cand', 'Hnew'):
    case(fn, {name: _z(fn, 'Bm')}, EINVAL, 'must not alias Bm')

fn = 'stc_spmm_sum_f32'
state_row_cases(fn, ('n_rows', 'n_cols', 'batch'), 'X', 'Y')
case(fn, {'C': 3}, ELIMIT, '48 floats', 'too narrow')
case(fn, {'amax': P()}, EINVAL, 'amax with 0 slots')
case(fn, {'n_add': 9}, EINVAL, '0..8 addends', 'got 9')
case(fn, {'n_add': -1}, EINVAL, '0..8 addends', 'got -1')
for name in ('add', 'add_ld', 'add_off'):
    case(fn, {name: None}, EINVAL, 'addends')
case(fn, {'Y': _z(fn, 'X')}, EINVAL, 'Y must not alias a gathered operand')
case(fn, {'X2': _z(fn, 'Y')}, EINVAL, 'Y must not alias a gathered operand')
case(fn, {'X2': MIS}, EALIGN, 'X2 not 16-byte aligned')
dy_cases(fn)
addend_cases(fn, 'add', ('Y',))
case(fn, {'add_off': I32(0, 4)}, EINVAL, 'addend 1', 'ld 16', 'off 4')               # columns [4, 20) of rows of 16
case(fn, {'add_off': I32(-4, 0)}, EINVAL, 'addend 0', 'off -4')
case(fn, {'add_ld': I32(16, 18)}, EINVAL, 'addend 1', 'ld 18', 'multiples of 4')
case(fn, {'add_ld': I32(34, 16), 'add_off': I32(18, 0)}, EINVAL, 'addend 0', 'off 18', 'multiples of 4')

fn = 'stc_spmm_sum_bf16'
state_row_cases(fn, ('n_rows', 'batch'), 'X', 'Y')
case(fn, {'n_cols': -1}, EINVAL, 'null')
case(fn, {'n_add': 6}, EINVAL, '0..5 addends', 'got 6')
case(fn, {'n_add': -1}, EINVAL, '0..5 addends', 'got -1')
case(fn, {'add': None}, EINVAL, 'addends')
case(fn, {'Y': _z(fn, 'X')}, EINVAL, 'Y must not alias a gathered operand')
case(fn, {'X2': _z(fn, 'Y')}, EINVAL, 'Y must not alias a gathered operand')
case(fn, {'X2': MIS}, EALIGN, '16-byte aligned')
dy_cases(fn)
addend_cases(fn, 'add', ('Y',))


# ---------------------------------------------------------------- two-ring launches
def ring2_cases(fn):
    case(fn, {'h': 8}, EUNSUPPORTED, 'hidden 16')
    case(fn, {'C': 0}, EUNSUPPORTED, 'C * h = 0 floats')
    case(fn, {'C': 4}, EUNSUPPORTED, 'C * h = 64 floats', '512-byte chunks')
    case(fn, {'C': 12}, EUNSUPPORTED, 'C * h = 192 floats', '512-byte chunks')
    for name in ('batch', 'n_rows', 'n_patches'):
        case(fn, {name: -1}, EINVAL, 'bad sizes')
    batch_case(fn, EINVAL)
    case(fn, {'n_rows': 1 << 21, 'n_patches': 1 << 16}, ELIMIT, '2^28')          # 2 x 2^21 rows of 128 pieces
    case(fn, {'n_rows': 0}, OK)
    case(fn, {'batch': 0}, OK)
    case(fn, {'n_patches': 0}, EINVAL, '0 patches cannot cover 8 rows')
    case(fn, {'n_rows': 33}, EINVAL, '1 patches cannot cover 33 rows')
    for name in ('l2_rows', 'l1_rows', 'int_rows', 't1', 't2'):
        case(fn, {name: None}, EINVAL, 'null plan array')
    for name in ('t1', 't2'):
        case(fn, {name: MIS}, EALIGN, 'tables', '8-byte aligned')


def alias_cases(fn, results, operands):
    for out in results:
        for name in operands:
            case(fn, {out: _z(fn, name)}, EINVAL, 'alias')


fn = 'stc_ring2_sum_f32'
ring2_cases(fn)
case(fn, {'n_add': 6}, ELIMIT, '0..5 addends', 'got 6')
case(fn, {'n_add': -1}, ELIMIT, '0..5 addends', 'got -1')
for name in ('A', 'U', 'Cand', 'Y', 'Z', 'add'):
    case(fn, {name: None}, EINVAL, 'null pointer')
for name in ('A', 'A2', 'U', 'Cand', 'Y', 'Z'):
    case(fn, {name: MIS}, EALIGN, '16-byte aligned')
alias_cases(fn, ('Y', 'Z'), ('A', 'U', 'Cand'))
case(fn, {'A2': _z(fn, 'Y')}, EINVAL, 'alias')
case(fn, {'A2': _z(fn, 'Z')}, EINVAL, 'alias')
case(fn, {'Z': _z(fn, 'Y')}, EINVAL, 'alias')
addend_cases(fn, 'add', ('Y', 'Z'))

fn = 'stc_ring2_blend_f32'
ring2_cases(fn)
for name in ('Bm', 'A', 'U', 'H', 'Hnew', 'SHnew'):
    case(fn, {name: None}, EINVAL, 'null pointer')
for name in ('Bm', 'A', 'U', 'H', 'Cand', 'Hnew', 'SHnew'):
    case(fn, {name: MIS}, EALIGN, '16-byte aligned')
alias_cases(fn, ('Cand', 'Hnew', 'SHnew'), ('Bm', 'A', 'U', 'H'))
case(fn, {'Cand': _z(fn, 'Hnew')}, EINVAL, 'results alias each other')
case(fn, {'Cand': _z(fn, 'SHnew')}, EINVAL, 'results alias each other')
case(fn, {'SHnew': _z(fn, 'Hnew')}, EINVAL, 'results alias each other')

fn = 'stc_ring2_chain_f32'
ring2_cases(fn)
case(fn, {'n_add1': 3}, ELIMIT, '0..2 first-ring addends', 'got 3')
case(fn, {'n_add1': -1}, ELIMIT, '0..2 first-ring addends', 'got -1')
case(fn, {'n_add0': 6}, ELIMIT, '1..5 interior addends', 'got 6')
case(fn, {'n_add0': 0}, ELIMIT, '1..5 interior addends', 'got 0')
for name in ('A', 'Z', 'add0', 'add1'):
    case(fn, {name: None}, EINVAL, 'null pointer')
for name in ('A', 'A2', 'V', 'Z'):
    case(fn, {name: MIS}, EALIGN, '16-byte aligned')
alias_cases(fn, ('Z', 'V'), ('A',))
case(fn, {'A2': _z(fn, 'Z')}, EINVAL, 'alias')
case(fn, {'A2': _z(fn, 'V')}, EINVAL, 'alias')
case(fn, {'V': _z(fn, 'Z')}, EINVAL, 'alias')
addend_cases(fn, 'add1', ('Z', 'V'), what='first-ring addend')
addend_cases(fn, 'add0', ('Z', 'V'), what='interior addend')


@pytest.fixture(scope='module')
def lib():
    return _lib.load_library()


def test_table_names_exactly_the_aggregation_entry_points():
    assert set(GOOD) == {
        'stc_csr_spmm_f32', 'stc_bcsr_spmm_f32', 'stc_csr_spmm_bf16', 'stc_bcsr_spmm_bf16', 'stc_patch_spmm_f32', 'stc_patch_spmm_bf16',
        'stc_dense_agg_f32', 'stc_csr_sddmm_f32', 'stc_spmm_blend_fwd_f32', 'stc_spmm_blend_fwd_bf16', 'stc_spmm_sum_f32', 'stc_spmm_sum_bf16',
        'stc_ring2_sum_f32', 'stc_ring2_blend_f32', 'stc_ring2_chain_f32'}
    assert len(GOOD) == 15 and set(GOOD) <= set(_lib.EXPORTS)
    assert {p.values[0] for p in CASES} == set(GOOD)
    for fn, args in GOOD.items():
        assert len(args) == len(_lib._ABI[fn][1]), fn


@pytest.mark.parametrize('fn, fault, code, needles', CASES)
def test_refusal(lib, fn, fault, code, needles):
    # (the patch launch helper reports under "<entry point> launch")
    check_refusal(lib, GOOD, fn, fault, code, needles, heads=(fn + ':', fn + ' launch:'))
