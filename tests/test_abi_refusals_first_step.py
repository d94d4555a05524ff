"""What the C front of the first-step entry points (ABI v37: stc_cell_gates_fwd_first_f32, stc_cell_bwd_first_f32, stc_ring2_blend_first_f32)
refuses, pinned without a GPU in the manner of tests/test_abi_refusals.py: every case is a call that would launch a kernel except for ONE
fault, refused before any HIP call; pointers are addresses inside a host buffer that a refusal never dereferences."""
import itertools

import pytest

from stc_hip import _lib
from tests.abi_refusal_table import EALIGN, EINVAL, ELIMIT, EUNSUPPORTED, MIS, OK, P, case_into, check_refusal
from tests.test_abi_refusals import BIG, ws_bytes

PLAN = dict(l2_rows=P(), l1_rows=P(), int_rows=P(), t1=P(), t2=P(), n_patches=4, n_rows=100)
GOOD = {
    'stc_cell_gates_fwd_first_f32': dict(X=P(), SX=P(), Tc=P(), W=P(), bias=P(), U=P(), Wc=P(), bc=P(), A=P(), Bm=P(), operand_format=0, act_amax=None,
                                         nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_bwd_first_f32': dict(X=P(), SX=P(), Tc=P(), Wg=P(), Wc=P(), U=P(), Cand=P(), dHnew=P(), dBm=P(), dX=P(), dSX=P(),
                                   dWg=P(), dbg=P(), dWc=P(), dbc=P(), accumulate_x=0, operand_format=0, act_amax=None,
                                   workspace=P(), workspace_bytes=BIG, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_ring2_blend_first_f32': dict(**PLAN, Bm=P(), A=P(), U=P(), Cand=P(), Hnew=P(), SHnew=P(), batch=2, C=32, h=16, stream=None),
}

CASES = []
case = case_into(CASES)

CELL = ('stc_cell_gates_fwd_first_f32', 'stc_cell_bwd_first_f32')
for fn in CELL:
    case(fn, {'C': 0}, EINVAL, 'bad sizes')
    case(fn, {'nodes': -1}, EINVAL, 'bad sizes')
    case(fn, {'nodes': 1 << 26}, ELIMIT, '2^31')
    case(fn, {'Lw': 21}, EINVAL, 'Lw=21', 'L=20')                    # 5 input columns: outside the padded row of 20
    case(fn, {'Lw': 16}, EINVAL, 'input width 0', 'h or 1..4')       # no input columns
    case(fn, {'operand_format': 2}, EINVAL, 'operand_format 2')      # an unknown operand format
    case(fn, {'operand_format': -1}, EINVAL, 'operand_format -1')
    case(fn, {'C': 64}, EUNSUPPORTED, 'not built', 'C=64', 'h=16')
    case(fn, {'h': 8, 'Lw': 16}, EUNSUPPORTED, 'not built', 'h=8')
    case(fn, {'Tc': None}, EINVAL, 'null')
    case(fn, {'X': None}, EINVAL, 'null pointer')
    case(fn, {'SX': None}, EINVAL, 'null pointer')
    case(fn, {'U': None}, EINVAL, 'null pointer')
    case(fn, {'Wc': None}, EINVAL, 'null')
    case(fn, {'U': MIS}, EUNSUPPORTED, 'alignment')
    case(fn, {'X': MIS}, EUNSUPPORTED, 'alignment')                  # wide input: a whole plane
    case(fn, {'X': MIS, 'SX': MIS, 'Lw': 17}, OK)                    # a narrow input plane is read float by float: no alignment asked
case('stc_cell_gates_fwd_first_f32', {'W': None}, EINVAL, 'null pointer')
case('stc_cell_gates_fwd_first_f32', {'A': None}, EINVAL, 'null pointer')      # the candidate's projection always rides along
case('stc_cell_gates_fwd_first_f32', {'Bm': None}, EINVAL, 'null pointer')
case('stc_cell_gates_fwd_first_f32', {'Bm': MIS}, EUNSUPPORTED, 'alignment')
case('stc_cell_gates_fwd_first_f32', {'bias': None, 'bc': None}, OK)

case('stc_cell_bwd_first_f32', {'Wg': None}, EINVAL, 'null W/dW/Tc')
case('stc_cell_bwd_first_f32', {'dWc': None}, EINVAL, 'null W/dW/Tc')
case('stc_cell_bwd_first_f32', {'Cand': None}, EINVAL, 'null pointer')
case('stc_cell_bwd_first_f32', {'dBm': None}, EINVAL, 'null pointer')
case('stc_cell_bwd_first_f32', {'dX': None}, EINVAL, 'null pointer')           # wide: the input plane has a gradient
case('stc_cell_bwd_first_f32', {'dSX': MIS}, EUNSUPPORTED, 'alignment')
case('stc_cell_bwd_first_f32', {'dHnew': MIS}, EUNSUPPORTED, 'alignment')
case('stc_cell_bwd_first_f32', {'Lw': 20, 'accumulate_x': 1}, EINVAL, 'accumulate_x', 'narrow')
case('stc_cell_bwd_first_f32', {'Lw': 20, 'dX': None, 'dSX': None}, OK)        # narrow: no gradient planes
case('stc_cell_bwd_first_f32', {'dbg': None, 'dbc': None}, OK)
case('stc_cell_bwd_first_f32', {'workspace': None}, EALIGN, 'workspace')
case('stc_cell_bwd_first_f32', {'workspace': MIS}, EALIGN, 'workspace')
_need = ws_bytes(2, 2, 32, 32, 32) + ws_bytes(2, 2, 32, 32, 16)
case('stc_cell_bwd_first_f32', {'workspace_bytes': _need - 1}, EINVAL, 'workspace', f'{_need - 1} B')
case('stc_cell_bwd_first_f32', {'Lw': 18, 'workspace_bytes': ws_bytes(2, 2, 32, 20, 32) + ws_bytes(2, 2, 32, 20, 16) - 1}, EINVAL, 'too small')

fn = 'stc_ring2_blend_first_f32'
case(fn, {'h': 8}, EUNSUPPORTED, 'hidden 16')
case(fn, {'C': 3}, EUNSUPPORTED, 'whole 512-byte chunks')
case(fn, {'batch': 70000}, EINVAL, 'bad sizes')
case(fn, {'n_patches': -1}, EINVAL, 'bad sizes')
case(fn, {'n_patches': 3}, EINVAL, '3 patches cannot cover 100 rows')
case(fn, {'n_rows': 1 << 22, 'n_patches': 1 << 17, 'batch': 64}, ELIMIT, '2^28')
case(fn, {'l1_rows': None}, EINVAL, 'null plan array')
case(fn, {'t2': MIS}, EALIGN, 'tables must be 8-byte aligned')
for name in ('Bm', 'A', 'U', 'Hnew', 'SHnew'):
    case(fn, {name: None}, EINVAL, 'null pointer')
for name in ('Bm', 'U', 'Cand', 'SHnew'):
    case(fn, {name: MIS}, EALIGN, 'planes must be 16-byte aligned')
case(fn, {'Hnew': GOOD[fn]['U']}, EINVAL, 'a result aliases an operand')
case(fn, {'SHnew': GOOD[fn]['Bm']}, EINVAL, 'a result aliases an operand')
case(fn, {'Cand': GOOD[fn]['Hnew']}, EINVAL, 'results alias each other')
case(fn, {'batch': 0}, OK)
case(fn, {'n_rows': 0, 'n_patches': 0}, OK)


@pytest.fixture(scope='module')
def lib():
    lib = _lib.load_library()
    assert lib.stc_set_dispatch_level(0) == OK
    return lib


def test_table_covers_the_first_step_entry_points():
    assert set(GOOD) <= set(_lib.EXPORTS) and {p.values[0] for p in CASES} == set(GOOD)
    for fn, args in GOOD.items():
        assert len(args) == len(_lib._ABI[fn][1]), fn


def _reaches_the_launch(fn, fault):
    """Cases that pass every check would go on to HIP calls: only their status up to the dispatch can be pinned without a device."""
    return fn != 'stc_ring2_blend_first_f32' or not ({'batch', 'n_rows'} & set(fault))


@pytest.mark.parametrize('fn, fault, code, needles', CASES)
def test_refusal(lib, fn, fault, code, needles):
    if code == OK and _reaches_the_launch(fn, fault):
        # a call the front accepts: the same call with one more fault that only a LATER check catches is refused by that check, not before
        later = {'stc_cell_gates_fwd_first_f32': ({'A': MIS}, EUNSUPPORTED, ('alignment',)),
                 'stc_cell_bwd_first_f32': ({'U': MIS}, EUNSUPPORTED, ('alignment',))}[fn]
        check_refusal(lib, GOOD, fn, {**fault, **later[0]}, later[1], later[2])
        return
    check_refusal(lib, GOOD, fn, fault, code, needles)


def test_predicate_and_workspace_size(lib):
    for C, h in itertools.product((8, 16, 32, 48, 64), (8, 16, 32)):
        assert lib.stc_cell_first_supported(C, h) == int(C == 32 and h == 16)
        for Lw in (2 * h, h + 1, h + 4):
            assert lib.stc_cell_bwd_first_workspace_bytes(C, Lw, h) == lib.stc_cell_bwd_planar_workspace_bytes(C, Lw, h)
