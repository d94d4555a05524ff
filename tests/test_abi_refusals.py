"""What the C front of the node / cell entry points refuses, pinned without a GPU.

Every refusal below fires before any HIP call, so the table runs on a machine with no device: each case is a call whose
arguments are valid up to the dispatch (and would launch a kernel) except for ONE fault, and the test reads the status
code and ``stc_last_error()``.  No case reaches the ``nodes == 0`` zero-filling or a launch.  Pointers are addresses
inside a host buffer: a refusal never dereferences them (only the pointer ARRAYS -- Z, dZ, Zx, Zh ... -- are read).

The 21 entry points: 15 on fp32 rows / planes (csrc/stc_node.hip) and 6 on bf16 planes (csrc/stc_node_bf16.hip).  Where
the two fronts answer the same fault with different codes (workspace alignment: STC_EALIGN vs STC_EINVAL; input width:
STC_EINVAL vs STC_EUNSUPPORTED; a null plane of the bf16 node kernel: STC_EALIGN) the table records each as it is.
"""
import itertools

import pytest

from stc_hip import _lib
from tests.abi_refusal_table import EALIGN, EINVAL, ELIMIT, EUNSUPPORTED, MIS, OK, P, PP, case_into, check_refusal, with_null

MAX_GRID = 512          # partial rows a backward workspace holds (NODE_BWD_MAX_GRID / MF_BWD_MAX_GRID)
BIG = 1 << 40           # a workspace size that is always enough (the workspace itself is never touched)


def ws_bytes(Ks, Kc, C, L, Ho):
    if min(Ks, Kc, C, L, Ho) < 1:
        return 0
    return MAX_GRID * 4 * (Ks * Kc * L * Ho + Ho + Kc * C * C)


# ---- per entry point: (argument name, value of a call that passes every check), in ABI order
NODE = dict(nodes=8, C=32, L=32, Lw=32)
GOOD = {
    'stc_bdg_node_fwd_f32': dict(Z=PP(2), Ks=2, Tc=P(), Kc=2, W=P(), bias=P(), Y=P(), **NODE, Ho=32, stream=None),
    'stc_bdg_node_bwd_f32': dict(Z=PP(2), Ks=2, Tc=P(), Kc=2, W=P(), dY=P(), dZ=PP(2), dW=P(), db=P(), dTc=None,
                                 workspace=P(), workspace_bytes=BIG, **NODE, Ho=32, stream=None),
    'stc_cell_gates_fwd_f32': dict(Z=PP(2), Ks=2, Tc=P(), Kc=2, W=P(), bias=P(), H=P(), U=P(), Rg=P(), CandIn=P(),
                                   **NODE, h=16, cin=16, stream=None),
    'stc_cell_gates_bwd_f32': dict(Z=PP(2), Ks=2, Tc=P(), Kc=2, W=P(), dCandIn=P(), dU=P(), H=P(), U=P(), Rg=P(), Cand=None, dH_in=None,
                                   dH_in_scaled=0, dZ=PP(2), dW=P(), db=P(), dXt=P(), dH=P(), workspace=P(), workspace_bytes=BIG,
                                   **NODE, h=16, cin=16, stream=None),
    'stc_cell_cand_bwd_f32': dict(Z=PP(2), Ks=2, Tc=P(), Kc=2, W=P(), dHnew=P(), U=P(), Cand=P(), dZ=PP(2), dW=P(), db=P(),
                                  workspace=P(), workspace_bytes=BIG, **NODE, h=16, stream=None),
    'stc_cell_blend_fwd_f32': dict(Z=PP(2), Ks=2, Tc=P(), Kc=2, W=P(), bias=P(), U=P(), H=P(), Cand=P(), Hnew=P(),
                                   copy0=None, copy0_ld=0, copy0_off=0, side_src=None, side_cin=0, copy1=None, copy1_ld=0, copy1_off=0,
                                   **NODE, h=16, stream=None),
    'stc_cell_gates_fwd_planar_f32': dict(X=P(), H=P(), SX=P(), SH=P(), Tc=P(), W=P(), bias=P(), U=P(), Rg=P(), RH=P(),
                                          Wc=None, bc=None, A=None, Bm=None, operand_format=0, act_amax=None,
                                          nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_gates_bwd_planar_f32': dict(X=P(), H=P(), SX=P(), SH=P(), Tc=P(), W=P(), dCandIn=P(), Cand=P(), U=P(), Rg=P(), dHnew=P(),
                                          dZ=PP(4), dW=P(), db=P(), dH=P(), operand_format=0, act_amax=None,
                                          workspace=P(), workspace_bytes=BIG, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_bwd_planar_f32': dict(X=P(), H=P(), SX=P(), SH=P(), Tc=P(), Wg=P(), Wc=P(), U=P(), Rg=P(), Cand=P(), dHnew=P(), dBm=P(),
                                    dX=P(), dSX=P(), dH=P(), dSH=P(), dWg=P(), dbg=P(), dWc=P(), dbc=P(),
                                    accumulate_x=0, accumulate_h=0, operand_format=0, act_amax=None,
                                    workspace=P(), workspace_bytes=BIG, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_gates_fwd_planar_k_f32': dict(Zx=PP(3), Zh=PP(3), K=3, Tc=P(), W=P(), bias=P(), U=P(), Rg=P(), RH=P(),
                                            operand_format=0, act_amax=None, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_cand_fwd_planar_k_f32': dict(Zx=PP(3), Zh=PP(3), K=3, Tc=P(), W=P(), bias=P(), U=P(), H=P(), Cand=P(), Hnew=P(),
                                           operand_format=0, act_amax=None, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_gates_bwd_planar_k_f32': dict(Zx=PP(3), Zh=PP(3), K=3, Tc=P(), W=P(), dRH=P(), Cand=P(), U=P(), Rg=P(), dHnew=P(),
                                            dZx=PP(3), dZh=PP(3), dW=P(), db=P(), dH=P(), accumulate_x=0, operand_format=0, act_amax=None,
                                            workspace=P(), workspace_bytes=BIG, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_cand_bwd_planar_k_f32': dict(Zx=PP(3), Zh=PP(3), K=3, Tc=P(), W=P(), dHnew=P(), U=P(), Cand=P(), dZx=PP(3), dZh=PP(3),
                                           dW=P(), db=P(), operand_format=0, act_amax=None,
                                           workspace=P(), workspace_bytes=BIG, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_bdg_node_post_fwd_f32': dict(X=P(), X2=None, Tc=P(), W=P(), bias=P(), A=P(), Bm=P(), **NODE, Ho=16, stream=None),
    'stc_bdg_node_post_bwd_f32': dict(X=P(), X2=None, Tc=P(), W=P(), dA=P(), dB=P(), dX=P(), dX2=None, dW=P(), db=P(),
                                      operand_format=0, act_amax_x=None, act_amax_x2=None, workspace=P(), workspace_bytes=BIG,
                                      **NODE, Ho=16, stream=None),
    # ---- bf16 planes
    'stc_bdg_node_fwd_bf16': dict(Z=PP(2), Ks=2, Tc=P(), Kc=2, W=P(), bias=P(), Y=P(), **NODE, Ho=32, stream=None),
    'stc_bdg_node_bwd_bf16': dict(Z=PP(2), Ks=2, Tc=P(), Kc=2, W=P(), dY=P(), dZ=PP(2), dW=P(), db=P(),
                                  workspace=P(), workspace_bytes=BIG, **NODE, Ho=32, stream=None),
    'stc_cell_gates_fwd_planar_bf16': dict(X=P(), H=P(), SX=P(), SH=P(), Tc=P(), W=P(), bias=P(), U=P(), Rg=P(), RH=P(),
                                           Wc=None, bc=None, A=None, Bm=None, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_gates_bwd_planar_bf16': dict(X=P(), H=P(), SX=P(), SH=P(), Tc=P(), W=P(), dCandIn=P(), Cand=P(), U=P(), Rg=P(), dHnew=P(),
                                           dZ=PP(4), dW=P(), db=P(), dH=P(), workspace=P(), workspace_bytes=BIG,
                                           nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_cell_bwd_planar_bf16': dict(X=P(), H=P(), SX=P(), SH=P(), Tc=P(), Wg=P(), Wc=P(), U=P(), Rg=P(), Cand=P(), dHnew=P(), dBm=P(),
                                     dX=P(), dSX=P(), dH=P(), dSH=P(), dWg=P(), dbg=P(), dWc=P(), dbc=P(),
                                     workspace=P(), workspace_bytes=BIG, nodes=8, C=32, Lw=32, h=16, stream=None),
    'stc_bdg_node_post_bwd_bf16': dict(X=P(), X2=P(), Tc=P(), W=P(), dA=P(), dB=P(), dX=P(), dX2=P(), dW=P(), db=P(),
                                       workspace=P(), workspace_bytes=BIG, nodes=8, C=32, Lw=32, Ho=16, stream=None),
}


def _z(fn, name):
    return GOOD[fn][name]


CASES = []
case = case_into(CASES)


def dims_cases(fn, order='Ks', limit_code=ELIMIT, inval_code=EINVAL):
    """The size checks every fp32 entry point runs first (check_dims)."""
    case(fn, {order: 5}, limit_code, 'Chebyshev')
    case(fn, {order: 0}, limit_code, 'Chebyshev')
    case(fn, {'C': 0}, inval_code, 'bad sizes', 'C=0')
    case(fn, {'nodes': -1}, inval_code, 'bad sizes', 'nodes=-1')
    case(fn, {'nodes': 1 << 26}, limit_code, '2^31')


def workspace_cases(fn, need, null_code, short_code=EINVAL):
    """Null / misaligned / short workspace: STC_EALIGN for the first two on the fp32 front and the bf16 node kernel,
    one STC_EINVAL for all three on the bf16 planar front."""
    case(fn, {'workspace': None}, null_code, 'workspace')
    case(fn, {'workspace': MIS}, null_code, 'workspace')
    case(fn, {'workspace_bytes': need - 1}, short_code, 'workspace', f'{need - 1} B')


# ---------------------------------------------------------------- fp32 rows: node kernel
for fn in ('stc_bdg_node_fwd_f32', 'stc_bdg_node_bwd_f32'):
    dims_cases(fn)
    case(fn, {'Kc': 5}, ELIMIT, 'Chebyshev', 'Kc=5')
    case(fn, {'Lw': 0}, EINVAL, 'Lw=0')
    case(fn, {'Lw': 33}, EINVAL, 'Lw=33', 'L=32')
    case(fn, {'Ho': 0}, EINVAL, 'bad sizes')
    case(fn, {'W': None}, EINVAL, 'null')
    case(fn, {'Tc': None}, EINVAL, 'null')
    case(fn, {'Z': None}, EINVAL, 'null')
case('stc_bdg_node_fwd_f32', {'Y': None}, EINVAL, 'null')
case('stc_bdg_node_fwd_f32', {'Z': with_null(_z('stc_bdg_node_fwd_f32', 'Z'), 1)}, EINVAL, 'Z[1] is null')
case('stc_bdg_node_bwd_f32', {'dW': None}, EINVAL, 'null')
case('stc_bdg_node_bwd_f32', {'dZ': None}, EINVAL, 'null')
case('stc_bdg_node_bwd_f32', {'dY': None}, EINVAL, 'null dY')
case('stc_bdg_node_bwd_f32', {'Z': with_null(_z('stc_bdg_node_bwd_f32', 'Z'), 1)}, EINVAL, 'Z[1]/dZ[1] is null')
case('stc_bdg_node_bwd_f32', {'dZ': with_null(_z('stc_bdg_node_bwd_f32', 'dZ'), 0)}, EINVAL, 'Z[0]/dZ[0] is null')
workspace_cases('stc_bdg_node_bwd_f32', ws_bytes(2, 2, 32, 32, 32), EALIGN)

# ---------------------------------------------------------------- fp32 rows: fused cell convolutions
for fn in ('stc_cell_gates_fwd_f32', 'stc_cell_gates_bwd_f32', 'stc_cell_cand_bwd_f32', 'stc_cell_blend_fwd_f32'):
    dims_cases(fn)
    case(fn, {'Lw': 33}, EINVAL, 'Lw=33')
    case(fn, {'C': 48}, EUNSUPPORTED, 'fused path')
    case(fn, {'Kc': 1}, EUNSUPPORTED, 'fused path')          # Ks != Kc
    case(fn, {'L': 24, 'Lw': 24, **({'cin': 8} if 'cin' in GOOD[fn] else {})}, EUNSUPPORTED, 'fused path')      # rows of 24 columns
    case(fn, {'W': None}, EINVAL, 'null')
    case(fn, {'Tc': None}, EINVAL, 'null')
    case(fn, {'Z': None}, EINVAL, 'null')
    case(fn, {'Z': with_null(_z(fn, 'Z'), 1)}, EINVAL, '[1]', 'null')
for fn in ('stc_cell_gates_fwd_f32', 'stc_cell_gates_bwd_f32'):
    case(fn, {'h': 8}, EUNSUPPORTED, 'fused path')
    case(fn, {'cin': -1}, EINVAL, 'cin=-1')
    case(fn, {'cin': 17}, EINVAL, 'cin=17', 'h=16', 'L=32')
for fn in ('stc_cell_cand_bwd_f32', 'stc_cell_blend_fwd_f32'):
    case(fn, {'h': 8}, EUNSUPPORTED, 'fused path')
case('stc_cell_gates_fwd_f32', {'H': None}, EINVAL, 'null pointer')
case('stc_cell_gates_fwd_f32', {'CandIn': None}, EINVAL, 'null pointer')
case('stc_cell_gates_fwd_f32', {'CandIn': _z('stc_cell_gates_fwd_f32', 'Z')[0]}, EINVAL, 'alias')

case('stc_cell_gates_bwd_f32', {'dW': None}, EINVAL, 'null')
case('stc_cell_gates_bwd_f32', {'dZ': None}, EINVAL, 'null')
case('stc_cell_gates_bwd_f32', {'dCandIn': None}, EINVAL, 'null pointer')
case('stc_cell_gates_bwd_f32', {'dH': None}, EINVAL, 'null pointer')
case('stc_cell_gates_bwd_f32', {'dU': None}, EINVAL, 'either dU or Cand')                                   # neither
case('stc_cell_gates_bwd_f32', {'Cand': P(), 'dH_in': P()}, EINVAL, 'either dU or Cand')                    # both
case('stc_cell_gates_bwd_f32', {'dU': None, 'Cand': P()}, EINVAL, 'Cand needs dH_in')
case('stc_cell_gates_bwd_f32', {'dZ': with_null(_z('stc_cell_gates_bwd_f32', 'dZ'), 1)}, EINVAL, 'Z[1]/dZ[1] is null')
workspace_cases('stc_cell_gates_bwd_f32', ws_bytes(2, 2, 32, 32, 32), EALIGN)

case('stc_cell_cand_bwd_f32', {'dW': None}, EINVAL, 'null')
case('stc_cell_cand_bwd_f32', {'dHnew': None}, EINVAL, 'null pointer')
case('stc_cell_cand_bwd_f32', {'Cand': None}, EINVAL, 'null pointer')
case('stc_cell_cand_bwd_f32', {'dZ': with_null(_z('stc_cell_cand_bwd_f32', 'dZ'), 0)}, EINVAL, 'Z[0]/dZ[0] is null')
workspace_cases('stc_cell_cand_bwd_f32', ws_bytes(2, 2, 32, 32, 16), EALIGN)

case('stc_cell_blend_fwd_f32', {'U': None}, EINVAL, 'null pointer')
case('stc_cell_blend_fwd_f32', {'Hnew': None}, EINVAL, 'null pointer')
case('stc_cell_blend_fwd_f32', {'copy0': P(), 'copy0_ld': 20, 'copy0_off': 8}, EINVAL, 'do not fit', 'off+16')
case('stc_cell_blend_fwd_f32', {'copy1': P(), 'copy1_ld': 32, 'copy1_off': -1}, EINVAL, 'do not fit')
case('stc_cell_blend_fwd_f32', {'side_src': P()}, EINVAL, 'side_src needs copy0')
case('stc_cell_blend_fwd_f32', {'copy0': P(), 'copy0_ld': 32, 'copy0_off': 4, 'side_src': P(), 'side_cin': 3}, EINVAL, 'side_src needs copy0', 'copy0_off == side_cin')

# ---------------------------------------------------------------- fp32 planes, order 2
PLANAR_F32 = ('stc_cell_gates_fwd_planar_f32', 'stc_cell_gates_bwd_planar_f32', 'stc_cell_bwd_planar_f32')
for fn in PLANAR_F32:
    case(fn, {'C': 0}, EINVAL, 'bad sizes')
    case(fn, {'nodes': -1}, EINVAL, 'bad sizes')
    case(fn, {'nodes': 1 << 26}, ELIMIT, '2^31')
    case(fn, {'Lw': 21}, EINVAL, 'Lw=21', 'L=20')                    # 5 input columns: already outside the padded row of 20
    case(fn, {'Lw': 16}, EINVAL, 'input width 0', 'h or 1..4')       # no input columns
    case(fn, {'operand_format': 2}, EINVAL, 'operand_format 2')
    case(fn, {'operand_format': -1}, EINVAL, 'operand_format -1')
    case(fn, {'Tc': None}, EINVAL, 'null')
    case(fn, {'X': None}, EINVAL, 'null pointer')
    case(fn, {'SH': None}, EINVAL, 'null pointer')
for fn in PLANAR_F32[:2]:
    case(fn, {'C': 16}, EUNSUPPORTED, 'planar path')
    case(fn, {'h': 8, 'Lw': 16}, EUNSUPPORTED, 'planar path')
    case(fn, {'W': None}, EINVAL, 'null')
case('stc_cell_gates_fwd_planar_f32', {'RH': None}, EINVAL, 'null pointer')          # RH may be null only with A
case('stc_cell_gates_fwd_planar_f32', {'A': P(), 'Wc': P()}, EINVAL, 'A, Bm and Wc go together')
case('stc_cell_gates_fwd_planar_f32', {'Bm': P()}, EINVAL, 'A, Bm and Wc go together')
case('stc_cell_gates_fwd_planar_f32', {'A': P(), 'Bm': P()}, EINVAL, 'A, Bm and Wc go together')

case('stc_cell_gates_bwd_planar_f32', {'dW': None}, EINVAL, 'null')
case('stc_cell_gates_bwd_planar_f32', {'dZ': None}, EINVAL, 'null')
case('stc_cell_gates_bwd_planar_f32', {'dZ': with_null(_z('stc_cell_gates_bwd_planar_f32', 'dZ'), 2)}, EINVAL, 'null pointer')
case('stc_cell_gates_bwd_planar_f32', {'dZ': with_null(_z('stc_cell_gates_bwd_planar_f32', 'dZ'), 0)}, EINVAL, 'null pointer')     # wide: all four planes
case('stc_cell_gates_bwd_planar_f32', {'dHnew': None}, EINVAL, 'null pointer')
workspace_cases('stc_cell_gates_bwd_planar_f32', ws_bytes(2, 2, 32, 32, 32), EALIGN)
case('stc_cell_gates_bwd_planar_f32', {'Lw': 20, 'workspace_bytes': ws_bytes(2, 2, 32, 20, 32) - 1}, EINVAL, 'too small')          # narrow rows are padded to 20

case('stc_cell_bwd_planar_f32', {'C': 64}, EUNSUPPORTED, 'not built', 'C=64', 'h=16')
case('stc_cell_bwd_planar_f32', {'h': 8, 'Lw': 16}, EUNSUPPORTED, 'not built', 'h=8')
case('stc_cell_bwd_planar_f32', {'Wg': None}, EINVAL, 'null')
case('stc_cell_bwd_planar_f32', {'dWc': None}, EINVAL, 'null')
case('stc_cell_bwd_planar_f32', {'Lw': 20, 'accumulate_x': 1}, EINVAL, 'accumulate_x', 'narrow')
case('stc_cell_bwd_planar_f32', {'dX': None}, EINVAL, 'null pointer')               # wide: the input plane has a gradient
case('stc_cell_bwd_planar_f32', {'dSH': None}, EINVAL, 'null pointer')
workspace_cases('stc_cell_bwd_planar_f32', ws_bytes(2, 2, 32, 32, 32) + ws_bytes(2, 2, 32, 32, 16), EALIGN)
case('stc_cell_bwd_planar_f32', {'Lw': 18, 'workspace_bytes': ws_bytes(2, 2, 32, 20, 32) + ws_bytes(2, 2, 32, 20, 16) - 1}, EINVAL, 'too small')

# ---------------------------------------------------------------- fp32 planes, order K
PLANAR_K = ('stc_cell_gates_fwd_planar_k_f32', 'stc_cell_cand_fwd_planar_k_f32', 'stc_cell_gates_bwd_planar_k_f32', 'stc_cell_cand_bwd_planar_k_f32')
for fn in PLANAR_K:
    case(fn, {'K': 5}, ELIMIT, 'Chebyshev')
    case(fn, {'K': 0}, ELIMIT, 'Chebyshev')
    case(fn, {'C': 0}, EINVAL, 'bad sizes')
    case(fn, {'nodes': -1}, EINVAL, 'bad sizes')
    case(fn, {'nodes': 1 << 26}, ELIMIT, '2^31')
    case(fn, {'Lw': 21}, EINVAL, 'Lw=21', 'L=20')
    case(fn, {'Lw': 16}, EINVAL, 'input width 0', 'h or 1..4')
    case(fn, {'K': 2}, EUNSUPPORTED, 'K=2', 'C=32', 'h=16', 'order-K planar path')
    case(fn, {'C': 64}, EUNSUPPORTED, 'C=64', 'order-K planar path')
    case(fn, {'Zx': None}, EINVAL, 'null plane arrays')
    case(fn, {'Zh': with_null(_z(fn, 'Zh'), 1)}, EINVAL, 'plane 1 is null')
    case(fn, {'operand_format': 2}, EINVAL, 'operand_format 2')
    case(fn, {'Tc': None}, EINVAL, 'null')
    case(fn, {'W': None}, EINVAL, 'null')
    case(fn, {'U': None}, EINVAL, 'null pointer')
case('stc_cell_gates_fwd_planar_k_f32', {'RH': None}, EINVAL, 'null pointer')
case('stc_cell_cand_fwd_planar_k_f32', {'Hnew': None}, EINVAL, 'null pointer')
case('stc_cell_cand_fwd_planar_k_f32', {'U': MIS}, EALIGN, 'misaligned operand')
case('stc_cell_cand_fwd_planar_k_f32', {'Hnew': MIS}, EALIGN, 'misaligned operand')
for fn, Ho in (('stc_cell_gates_bwd_planar_k_f32', 32), ('stc_cell_cand_bwd_planar_k_f32', 16)):
    case(fn, {'dW': None}, EINVAL, 'null W/dW/Tc/dZ')
    case(fn, {'dZh': None}, EINVAL, 'null W/dW/Tc/dZ')
    case(fn, {'dZx': None}, EINVAL, 'null W/dW/Tc/dZ')          # wide: the input side has gradient planes
    case(fn, {'Cand': None}, EINVAL, 'null pointer')
    case(fn, {'dHnew': None}, EINVAL, 'null pointer')
    workspace_cases(fn, ws_bytes(3, 3, 32, 32, Ho), EALIGN)
case('stc_cell_gates_bwd_planar_k_f32', {'dRH': None}, EINVAL, 'null pointer')
case('stc_cell_gates_bwd_planar_k_f32', {'Rg': None}, EINVAL, 'null pointer')

# ---------------------------------------------------------------- fp32: post-aggregation form
for fn in ('stc_bdg_node_post_fwd_f32', 'stc_bdg_node_post_bwd_f32'):
    case(fn, {'C': 0}, EINVAL, 'bad sizes')
    case(fn, {'nodes': -1}, EINVAL, 'bad sizes')
    case(fn, {'nodes': 1 << 26}, ELIMIT, '2^31')
    case(fn, {'Lw': 33}, EINVAL, 'Lw=33')
    case(fn, {'Ho': 32}, EUNSUPPORTED, 'post-aggregation path')
    case(fn, {'C': 48}, EUNSUPPORTED, 'post-aggregation path')
    case(fn, {'L': 24, 'Lw': 24}, EUNSUPPORTED, 'post-aggregation path')
    case(fn, {'X': None}, EINVAL, 'null pointer')
    case(fn, {'Tc': None}, EINVAL, 'null')
    case(fn, {'W': None}, EINVAL, 'null')
    case(fn, {'X2': P(), 'L': 20, 'Lw': 16}, EINVAL, 'planar input (X2)', 'L = 20')      # (the gradient plane dX2 is null: legal at L = 20)
case('stc_bdg_node_post_fwd_f32', {'Bm': None}, EINVAL, 'null pointer')
case('stc_bdg_node_post_fwd_f32', {'Bm': _z('stc_bdg_node_post_fwd_f32', 'A')}, EINVAL, 'alias')
case('stc_bdg_node_post_fwd_f32', {'A': _z('stc_bdg_node_post_fwd_f32', 'X')}, EINVAL, 'alias')
case('stc_bdg_node_post_bwd_f32', {'operand_format': 2}, EINVAL, 'operand_format 2')
case('stc_bdg_node_post_bwd_f32', {'dW': None}, EINVAL, 'null')
case('stc_bdg_node_post_bwd_f32', {'dA': None}, EINVAL, 'null pointer')
case('stc_bdg_node_post_bwd_f32', {'dX': None}, EINVAL, 'null pointer')
workspace_cases('stc_bdg_node_post_bwd_f32', ws_bytes(2, 2, 32, 32, 16), EALIGN)
case('stc_bdg_node_post_bwd_f32', {'X2': P()}, EINVAL, 'X2', 'dX2', 'go together')
case('stc_bdg_node_post_bwd_f32', {'dX2': P()}, EINVAL, 'X2', 'dX2', 'go together')
case('stc_bdg_node_post_bwd_f32', {'X2': P(), 'dX2': P(), 'L': 20, 'Lw': 20}, EINVAL, 'go together', 'no gradient')

# ---------------------------------------------------------------- bf16 planes: node kernel (one shape predicate: everything outside is STC_EUNSUPPORTED)
for fn in ('stc_bdg_node_fwd_bf16', 'stc_bdg_node_bwd_bf16'):
    case(fn, {'Ks': 5}, EUNSUPPORTED, 'Ks=5', 'not on the bf16 path')
    case(fn, {'Kc': 1}, EUNSUPPORTED, 'Kc=1', 'not on the bf16 path')
    case(fn, {'C': 48}, EUNSUPPORTED, 'C=48', 'not on the bf16 path')
    case(fn, {'L': 20, 'Lw': 20}, EUNSUPPORTED, 'L=20', 'not on the bf16 path')
    case(fn, {'Lw': 33}, EUNSUPPORTED, 'Lw=33', 'not on the bf16 path')
    case(fn, {'Ho': 8}, EUNSUPPORTED, 'Ho=8', 'not on the bf16 path')
    case(fn, {'nodes': -1}, EUNSUPPORTED, 'not on the bf16 path')
    case(fn, {'nodes': 1 << 26}, EUNSUPPORTED, 'not on the bf16 path')
    case(fn, {'W': None}, EINVAL, 'null')
    case(fn, {'Tc': None}, EINVAL, 'null')
    case(fn, {'Z': None}, EINVAL, 'null')
    case(fn, {'Z': with_null(_z(fn, 'Z'), 1)}, EALIGN, '[1]', 'null or not 16-byte aligned')
    case(fn, {'Z': with_null(_z(fn, 'Z'), 0, MIS)}, EALIGN, '[0]', 'null or not 16-byte aligned')
case('stc_bdg_node_fwd_bf16', {'Y': None}, EINVAL, 'null')
case('stc_bdg_node_fwd_bf16', {'Y': MIS}, EALIGN, 'Y not 16-byte aligned')
case('stc_bdg_node_bwd_bf16', {'dW': None}, EINVAL, 'null W/dW/Tc')
case('stc_bdg_node_bwd_bf16', {'dY': None}, EINVAL, 'null Z/dY/dZ')
case('stc_bdg_node_bwd_bf16', {'dZ': None}, EINVAL, 'null Z/dY/dZ')
case('stc_bdg_node_bwd_bf16', {'dZ': with_null(_z('stc_bdg_node_bwd_bf16', 'dZ'), 1, MIS)}, EALIGN, 'dZ[1]', 'not 16-byte aligned')
case('stc_bdg_node_bwd_bf16', {'dY': MIS}, EALIGN, 'dY not 16-byte aligned')
workspace_cases('stc_bdg_node_bwd_bf16', ws_bytes(2, 2, 32, 32, 32), EALIGN)

# ---------------------------------------------------------------- bf16 planes: planar cell and post-aggregation backward
PLANAR_BF16 = ('stc_cell_gates_fwd_planar_bf16', 'stc_cell_gates_bwd_planar_bf16', 'stc_cell_bwd_planar_bf16')
for fn in PLANAR_BF16:
    case(fn, {'C': 48}, EUNSUPPORTED, 'C=48', 'h=16')
    case(fn, {'h': 8, 'Lw': 24}, EUNSUPPORTED, 'h=8')
    case(fn, {'nodes': -1}, ELIMIT, 'nodes=-1')
    case(fn, {'nodes': 1 << 26}, ELIMIT, f'nodes={1 << 26}')
    case(fn, {'Tc': None}, EINVAL, 'null')
    case(fn, {'X': None}, EINVAL, 'null pointer')
    case(fn, {'H': MIS}, EALIGN, 'planes must be 16-byte aligned')
    case(fn, {'X': MIS}, EALIGN, 'planes must be 16-byte aligned')          # wide input plane
for fn in PLANAR_BF16[:2]:
    case(fn, {'Lw': 21}, EUNSUPPORTED, ' 5 ', '1..4')          # (needles: the value and the accepted range -- the wording is the fp32 twin's)
    case(fn, {'Lw': 16}, EUNSUPPORTED, ' 0 ', '1..4')
    case(fn, {'W': None}, EINVAL, 'null')
case('stc_cell_gates_fwd_planar_bf16', {'RH': None}, EINVAL, 'null pointer')
case('stc_cell_gates_fwd_planar_bf16', {'A': P(), 'Wc': P()}, EINVAL, 'Wc, A, Bm go together')
case('stc_cell_gates_fwd_planar_bf16', {'A': P(), 'Bm': P()}, EINVAL, 'Wc, A, Bm go together')
case('stc_cell_gates_fwd_planar_bf16', {'Wc': P()}, EINVAL, 'Wc, A, Bm go together')           # (the fp32 twin accepts a lone Wc)
case('stc_cell_gates_fwd_planar_bf16', {'A': MIS, 'Bm': P(), 'Wc': P()}, EALIGN, 'planes must be 16-byte aligned')
case('stc_cell_gates_fwd_planar_bf16', {'Rg': MIS}, EALIGN, 'planes must be 16-byte aligned')

case('stc_cell_gates_bwd_planar_bf16', {'dW': None}, EINVAL, 'null W/dW/Tc')
case('stc_cell_gates_bwd_planar_bf16', {'dZ': None}, EINVAL, 'null pointer')
case('stc_cell_gates_bwd_planar_bf16', {'dZ': with_null(_z('stc_cell_gates_bwd_planar_bf16', 'dZ'), 3)}, EINVAL, 'null pointer')
case('stc_cell_gates_bwd_planar_bf16', {'dZ': with_null(_z('stc_cell_gates_bwd_planar_bf16', 'dZ'), 1)}, EINVAL, 'null pointer')
case('stc_cell_gates_bwd_planar_bf16', {'dH': MIS}, EALIGN, 'planes must be 16-byte aligned')
case('stc_cell_gates_bwd_planar_bf16', {'dZ': with_null(_z('stc_cell_gates_bwd_planar_bf16', 'dZ'), 0, MIS)}, EALIGN, 'planes must be 16-byte aligned')
workspace_cases('stc_cell_gates_bwd_planar_bf16', ws_bytes(2, 2, 32, 32, 32), EINVAL)
case('stc_cell_gates_bwd_planar_bf16', {'Lw': 20, 'workspace_bytes': ws_bytes(2, 2, 32, 32, 32) - 1}, EINVAL, 'workspace')         # narrow: still rows of 32

case('stc_cell_bwd_planar_bf16', {'Lw': 21}, EUNSUPPORTED, 'not built', 'input width 5')
case('stc_cell_bwd_planar_bf16', {'C': 64, 'Lw': 20}, EUNSUPPORTED, 'not built', 'C=64', 'input width 4')      # C = 64 has the wide form only
case('stc_cell_bwd_planar_bf16', {'Wc': None}, EINVAL, 'null W/dW/Tc')
case('stc_cell_bwd_planar_bf16', {'dWg': None}, EINVAL, 'null W/dW/Tc')
case('stc_cell_bwd_planar_bf16', {'dSX': None}, EINVAL, 'null pointer')
case('stc_cell_bwd_planar_bf16', {'dBm': MIS}, EALIGN, 'planes must be 16-byte aligned')
case('stc_cell_bwd_planar_bf16', {'dSX': MIS}, EALIGN, 'planes must be 16-byte aligned')
workspace_cases('stc_cell_bwd_planar_bf16', ws_bytes(2, 2, 32, 32, 32) + ws_bytes(2, 2, 32, 32, 16), EINVAL)

fn = 'stc_bdg_node_post_bwd_bf16'
case(fn, {'C': 48}, EUNSUPPORTED, 'C=48', 'Ho=16')
case(fn, {'Ho': 32}, EUNSUPPORTED, 'Ho=32')
case(fn, {'Lw': 21}, EUNSUPPORTED, ' 5 ', '1..4')
case(fn, {'Lw': 16}, EUNSUPPORTED, ' 0 ', '1..4')
case(fn, {'nodes': -1}, ELIMIT, 'nodes=-1')
case(fn, {'nodes': 1 << 26}, ELIMIT, f'nodes={1 << 26}')
case(fn, {'W': None}, EINVAL, 'null W/dW/Tc')
case(fn, {'dW': None}, EINVAL, 'null W/dW/Tc')
case(fn, {'X2': None}, EINVAL, 'null pointer')
case(fn, {'dX2': None}, EINVAL, 'null pointer')                                     # wide: both planes have gradients
case(fn, {'Lw': 20}, EINVAL, 'null pointer', 'dX2 must be null')                    # narrow: the input plane gets none
case(fn, {'dA': MIS}, EALIGN, 'planes must be 16-byte aligned')
case(fn, {'dX2': MIS}, EALIGN, 'planes must be 16-byte aligned')
workspace_cases(fn, ws_bytes(2, 2, 32, 32, 16), EINVAL)

# ---------------------------------------------------------------- added last: the ids above carry their position in the table
# dT_c is formed by the generic kernel at every dispatch level: C = 64, Ho = 32 at order 3 exceeds its LDS limit in ONE call -- the code that
# HipKernels._node_bwd_dT_by_block (stc_hip/_lib.py) answers with calls that fit
for L in (32, 20):
    case('stc_bdg_node_bwd_f32', {'C': 64, 'Ks': 3, 'Kc': 3, 'L': L, 'Lw': L, 'Z': PP(3), 'dZ': PP(3), 'dTc': P(), 'workspace_bytes': BIG}, ELIMIT, 'B of LDS', 'C=64', 'Ks=3')


@pytest.fixture(scope='module')
def lib():
    lib = _lib.load_library()
    assert lib.stc_set_dispatch_level(0) == OK
    return lib


def test_table_covers_every_node_and_cell_entry_point():
    assert len(GOOD) == 21 and set(GOOD) <= set(_lib.EXPORTS)
    assert {p.values[0] for p in CASES} == set(GOOD)
    for fn, args in GOOD.items():
        assert len(args) == len(_lib._ABI[fn][1]), fn


@pytest.mark.parametrize('fn, fault, code, needles', CASES)
def test_refusal(lib, fn, fault, code, needles):
    check_refusal(lib, GOOD, fn, fault, code, needles)


def test_dispatch_level_is_checked(lib):
    assert lib.stc_set_dispatch_level(3) == EINVAL and b'level 3' in lib.stc_last_error()
    assert lib.stc_set_dispatch_level(-1) == EINVAL
    assert lib.stc_set_dispatch_level(0) == OK


def test_workspace_sizes_follow_their_formulas(lib):
    for Ks, Kc, C, L, Ho in itertools.product((0, 1, 2, 3), (1, 2, 3), (0, 3, 32, 64), (0, 5, 20, 32), (0, 4, 16, 32)):
        for want_dTc in (0, 1):         # (the flag does not change the size: the partial rows always carry the dT columns)
            assert lib.stc_bdg_node_bwd_workspace_bytes(Ks, Kc, C, L, Ho, want_dTc) == ws_bytes(Ks, Kc, C, L, Ho), (Ks, Kc, C, L, Ho)
    for C, h in itertools.product((32, 64), (8, 16)):
        for Lw in (2 * h, h + 1, h + 4, h + 7, h):         # a row that is not two whole planes is a padded row of 20 columns, whatever its width
            L = 2 * h if Lw == 2 * h else 20
            assert lib.stc_cell_bwd_planar_workspace_bytes(C, Lw, h) == ws_bytes(2, 2, C, L, 2 * h) + ws_bytes(2, 2, C, L, h), (C, Lw, h)


def test_supported_predicates_at_dispatch_level_0(lib):
    Ks_, C_, L_, H_ = (0, 1, 2, 3, 4), (8, 16, 32, 48, 64), (16, 20, 24, 32), (8, 16, 32)
    for Ks, Kc, C, L, h in itertools.product(Ks_, Ks_, C_, L_, H_):
        same = Ks == Kc
        assert lib.stc_cell_fused_supported(Ks, Kc, C, L, h) == int(same and 1 <= Ks <= 3 and C in (16, 32, 64) and L in (20, 32) and h == 16)
        assert lib.stc_bdg_node_post_supported(Ks, Kc, C, L, h) == int(same and Ks == 2 and C in (32, 64) and L in (20, 32) and h == 16)
        assert lib.stc_bdg_node_bf16_supported(Ks, Kc, C, L, h) == int(same and 1 <= Ks <= 3 and C in (32, 64) and L in (16, 32) and h in (16, 32))
    for Ks, Kc, C, h in itertools.product(Ks_, Ks_, C_, H_):
        planar = int(Ks == 2 and Kc == 2 and C in (32, 64) and h == 16)
        assert lib.stc_cell_planar_supported(Ks, Kc, C, h) == planar
        assert lib.stc_cell_planar_bf16_supported(Ks, Kc, C, h) == planar
    for K, C, h in itertools.product(Ks_, C_, H_):
        assert lib.stc_cell_planar_k_supported(K, C, h) == int(K == 3 and C == 32 and h == 16)
    for C, h in itertools.product(C_, H_):
        assert lib.stc_cell_bwd_planar_supported(C, h) == int(C == 32 and h == 16)
        for cin in (0, 1, 4, 5, 16):
            want = int(C in (32, 64) and h == 16 and (cin == 16 or (C == 32 and 1 <= cin <= 4)))
            assert lib.stc_cell_bwd_planar_bf16_supported(C, h + cin, h) == want, (C, h, cin)
