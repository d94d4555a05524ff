"""Helpers of tests/test_launch_trips.py: the table of every launch whose kernel LOOPS over a capped or residency-sized grid, the sizes at which such a
loop takes two full trips and a ragged one, and the checker of an elementwise launch ("Launch geometry").

A kernel whose grid is capped walks its work in trips (``for (i = blockIdx.x * ...; i < n; i += gridDim.x * ...)``).  What goes wrong there goes wrong
on the SECOND trip (an accumulator or an LDS tile carried over, a barrier only needed between trips, an index formed in the wrong width) or on the
RAGGED last one (a tail guard that was only ever false).  The other tables of the suite enumerate shapes (tests/shape_lattice.py) and contracts
(tests/autograd_contract.py); this one enumerates launch geometry.

``ROWS`` has one row per kernel that reads ``gridDim.x`` and per call site of ``stc::persistent_grid`` in csrc/ (tests/test_launch_trips.py scans the
sources: a kernel or call site without a row fails the suite, and so does a row the scan no longer finds).  A row holds

    kernel, site      the ``__global__`` kernel (or the ``__device__`` function, where no kernel encloses the use) and, for the matrix-core forms,
                      the label of the ``persistent_grid`` call site that sizes its grid
    entry             the C entry point that launches it
    file, cap         the source file and the LITERAL text of the cap expression in it, with enough of its line (the launch's kernel, the call
                      site's label) that it occurs exactly ONCE in the file: when somebody moves a cap the text no longer occurs, the pinned-cap
                      test fails and names the row whose sizes have to be revisited (``EW_CAP`` is one function, ``ew_grid``, shared by its rows)
    per_trip          items one trip covers (a number, or a function of the case's size record where the template arm decides), and ``unit``:
                      what an item is
    status            one of
                          'case'        GPU cases of tests/test_launch_trips.py, their sizes in ``sizes``: each takes >= 2 full trips, whole
                                        workgroups of a last trip and one partial workgroup whose lanes the guard splits
                          'covered_by'  an existing test (``covered_by``: file::function, ``params``: which of its cases) with the argument (``why``)
                                        that its size takes >= 2 trips under ANY occupancy
                          'exempt'      with the reason (``why``), checkable from the code

The rule for a size: the smallest that gives two full trips, at least one whole workgroup of a third and a partial one.
"""
import dataclasses
import glob
import math
import os
import re
import tempfile
from typing import Callable, Optional, Union

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'stc-gnn_amd', 'csrc')

# ---- geometry constants, as csrc/ has them (each is pinned by a row's ``cap`` text or named in its ``why``) ------------------------------------------
NUM_CU = 256                                   # stc::kNumCu
EW_THREADS = 256
EW_TRIP = NUM_CU * 8 * EW_THREADS              # ew_grid: 2048 workgroups x 256 lanes = 524 288 elements (scalar forms) or float4s (vector forms)
HEAD_PARTS = 1024                              # the head backward's cap: half the forward's
ADAM_BLOCK = 256 * 4                           # float4s of a workgroup and trip: AD_THREADS x AD_PIECES
ADAM_TRIP = 256 * 8 * ADAM_BLOCK               # 2048 workgroups: 2 097 152 float4s = 8 388 608 floats
BF16_BLEND_TRIP = 8192 * 256                   # pieces of 8 bf16
MGP_TRIP = 4096 * 256                          # outputs (uv forward) or entries (softmax backward)
MF_WAVES = 4                                   # waves of a matrix-core workgroup: one node each
MAX_WAVES_PER_CU = 32                          # residency ceiling of a compute unit (8 waves on each of 4 SIMDs): no occupancy answer passes it
MF_BWD_TRIP = 512 * MF_WAVES                   # MF_BWD_MAX_GRID workgroups x 4 waves = 2048 nodes: the most a backward trip can hold


def head_lpr(h):
    """Lanes per row of head_fwd/bwd_kernel<LPR> (the dispatch of stc_head_fwd_f32)."""
    h4 = h // 4
    return 1 if h4 <= 1 else 2 if h4 <= 2 else 4 if h4 <= 4 else 8 if h4 <= 8 else 16


def head_rows(h):
    """Rows of the head case at hidden width h: two full FORWARD trips (= four backward ones), five whole workgroups and three rows of a sixth."""
    rpb = EW_THREADS // head_lpr(h)
    return 2 * (EW_TRIP // head_lpr(h)) + 5 * rpb + 3


def mfma_nodes(cus=NUM_CU):
    """Nodes of a forward matrix-core case: twice what the device can hold resident at the ceiling of 32 waves per compute unit, 75 whole workgroups
    and one node of a 76th (any occupancy gives trips that are multiples of the 4-wave workgroup, so the odd node is a partial workgroup at all of them)."""
    return 2 * MAX_WAVES_PER_CU * cus + 300 + 1


# ---- sizes of the GPU cases (read by tests/test_launch_trips.py; the CPU tests check them against ``per_trip``) ----------------------------------------
ADAM_N = 2 * 8388608 + 5 * 4096 + 300 * 4                  # 16 798 896 floats: the last workgroup has piece 0 full, 44 lanes of piece 1, pieces 2, 3 empty
SCALAR_ROWS = dict(rows=70000, a=1, b=16, pad=3)           # rows [cin | h | pad] = 20 floats: no width a multiple of 4 -> the scalar forms
VECTOR_ROWS = dict(rows=131072 + 5 * 32 + 3, a=16, b=16, pad=0)   # 8 float4 per row, every width a multiple of 4 -> the float4 forms
FLAT_SCALAR_N = 2 * EW_TRIP + 5 * EW_THREADS + 77          # odd: the scalar forms of the flat kernels
FLAT_VECTOR_N = 4 * FLAT_SCALAR_N
BF16_BLEND_N = 8 * (2 * BF16_BLEND_TRIP + 5 * 256 + 77)
HEAD_WIDTHS = (4, 8, 32, 64)                               # LPR 1, 2, 8, 16 (16 -> LPR 4: covered_by)
MGP_NODES = dict(B=7, T=7, N=1501, C=3, h=32, rows_axis=2)     # R K h = 1501 x 49 x 32 = 2 353 568, R^2 = 2 253 001
MGP_CATEGORIES = dict(B=347, T=3, N=7, C=63, h=32, rows_axis=3)  # R K h = 63 x 1041 x 32 = 2 098 656 (R^2: one trip -- the softmax backward is the nodes case's)


def _mgp_outputs(s):
    R = s['N'] if s['rows_axis'] == 2 else s['C']
    return R * s['B'] * s['T'] * s['h']


def _mgp_entries(s):
    R = s['N'] if s['rows_axis'] == 2 else s['C']
    return R * R


def _rows_items(s, vec):
    return s['rows'] * (s['a'] + s['b'] + s['pad']) // (4 if vec else 1)


@dataclasses.dataclass(frozen=True)
class Size:
    """One GPU case of a row: ``items`` loop items in workgroups of ``block`` items; ``unroll`` > 0: the guard sits inside an unroll over pieces of
    that many items each (Adam)."""
    id: str
    items: int
    block: int
    unroll: int = 0
    arm: Optional[int] = None            # what ``per_trip`` takes where it is a function (the head's LPR)


@dataclasses.dataclass(frozen=True)
class Row:
    kernel: str
    entry: str
    file: str
    cap: str
    per_trip: Union[int, Callable, None]
    unit: str
    status: str
    why: str = ''
    site: Optional[str] = None
    sizes: tuple = ()
    covered_by: Optional[str] = None
    params: str = ''
    also: tuple = ()                     # further (file, literal text) pins: the constants the cap expression is made of

    def trip(self, size=None):
        return self.per_trip(size) if callable(self.per_trip) else self.per_trip


EW_CAP = 'const long long cap = (long long)stc::kNumCu * 8;'
_GATES = 'stc_gates.hip'


_EW_PINS = (('stc_common.h', 'constexpr int kNumCu = 256;'), (_GATES, 'constexpr int EW_THREADS = 256;'))
_BWD_PINS = (('stc_node_frag.h', 'constexpr int MF_BWD_MAX_GRID = 512;'), ('stc_node_frag.h', 'constexpr int MF_THREADS = 256;'))


def _ew(kernel, entry, vec, size_id, items, unit=None):
    return Row(kernel, entry, _GATES, EW_CAP, EW_TRIP, unit or ('float4s' if vec else 'elements'), 'case', sizes=(Size(size_id, items, EW_THREADS),), also=_EW_PINS)


def _site_cap(site, args):
    """The call site's own text: its label and every argument of ``persistent_grid`` up to the cap (no two sites share it)."""
    return f'stc::persistent_grid<kern>("hipFuncSetAttribute({site})", {args})'


def _bwd_site(kernel, site, entry, file, covered_by, params, args):
    return Row(kernel, entry, file, _site_cap(site, args + ', MF_BWD_MAX_GRID, n_partials'),
               MF_BWD_TRIP, 'nodes (one per wave)', 'covered_by', site=site, covered_by=covered_by, params=params, also=_BWD_PINS,
               why='the grid is min(resident, MF_BWD_MAX_GRID = 512) workgroups of 4 waves, so a trip holds at most 2048 nodes whatever the occupancy '
                   'query answers: 4 500 nodes are two full trips and 404 nodes of a third')


def _fwd_site(kernel, site, entry, file, size_id, args):
    return Row(kernel, entry, file, _site_cap(site, args + ', INT_MAX, &grid'), MAX_WAVES_PER_CU * NUM_CU, 'nodes (one per wave)', 'case', site=site,
               sizes=(Size(size_id, mfma_nodes(), MF_WAVES),), also=_BWD_PINS[1:],
               why='no cap but residency: a compute unit holds at most 32 waves, so 2 x 32 x CUs + 301 nodes take two trips at any occupancy')


_HK, _BF = 'tests/test_hip_kernels.py', 'tests/test_bf16_kernels.py'

ROWS = (
    # ---- Adam ---------------------------------------------------------------------------------------------------------------------------------------
    Row('adam_kernel', 'stc_adam_f32', 'stc_adam.hip', 'want > 256 * 8 ? 256 * 8 : want', ADAM_TRIP, 'float4s', 'case',
        sizes=(Size('adam', ADAM_N // 4, ADAM_BLOCK, unroll=256),), also=(('stc_adam.hip', 'constexpr int AD_THREADS = 256, AD_PIECES = 4;'),)),
    # ---- the ew_grid launches of stc_gates.hip -------------------------------------------------------------------------------------------------------
    _ew('gru_gates_fwd_kernel', 'stc_gru_gates_fwd_f32', False, 'gates-scalar', _rows_items(SCALAR_ROWS, False)),
    _ew('gru_gates_bwd_kernel', 'stc_gru_gates_bwd_f32', False, 'gates-scalar', _rows_items(SCALAR_ROWS, False)),
    _ew('gru_gates_fwd_vec_kernel', 'stc_gru_gates_fwd_f32', True, 'gates-vector', _rows_items(VECTOR_ROWS, True)),
    _ew('gru_gates_bwd_vec_kernel', 'stc_gru_gates_bwd_f32', True, 'gates-vector', _rows_items(VECTOR_ROWS, True)),
    _ew('gru_blend_fwd_kernel', 'stc_gru_blend_fwd_f32', False, 'blend-scalar', FLAT_SCALAR_N),
    _ew('gru_blend_bwd_kernel', 'stc_gru_blend_bwd_f32', False, 'blend-scalar', FLAT_SCALAR_N),
    _ew('gru_blend_fwd_vec_kernel', 'stc_gru_blend_fwd_f32', True, 'blend-vector', FLAT_VECTOR_N // 4),
    _ew('gru_blend_bwd_vec_kernel', 'stc_gru_blend_bwd_f32', True, 'blend-vector', FLAT_VECTOR_N // 4),
    _ew('concat2_kernel', 'stc_concat2_f32', False, 'concat-split-scalar', _rows_items(SCALAR_ROWS, False)),
    _ew('split2_kernel', 'stc_split2_f32', False, 'concat-split-scalar', _rows_items(SCALAR_ROWS, False)),
    _ew('concat2_vec_kernel', 'stc_concat2_f32', True, 'concat-split-vector', _rows_items(VECTOR_ROWS, True)),
    _ew('split2_vec_kernel', 'stc_split2_f32', True, 'concat-split-vector', _rows_items(VECTOR_ROWS, True)),
    _ew('axpy_kernel', 'stc_axpy_f32', False, 'axpy', FLAT_SCALAR_N),
    # ---- output head: LPR lanes share a row, so a trip is EW_TRIP / LPR rows forward and half of that backward -----------------------------------------
    Row('head_fwd_kernel', 'stc_head_fwd_f32', _GATES, 'hipLaunchKernelGGL(head_fwd_kernel<LPR_>, ew_grid(rows * LPR_)', lambda s: EW_TRIP // s.arm, 'rows', 'case',
        why='h = 16 (LPR 4) wraps at the 300 000 rows of tests/test_hip_kernels.py::test_output_head: two full trips of 131 072 rows and a ragged third',
        sizes=tuple(Size(f'head-h{h}', head_rows(h), EW_THREADS // head_lpr(h), arm=head_lpr(h)) for h in HEAD_WIDTHS), also=_EW_PINS + ((_GATES, EW_CAP),)),
    Row('head_bwd_kernel', 'stc_head_bwd_f32', _GATES,
        'long long blocks = (rows * lpr + EW_THREADS - 1) / EW_THREADS;\n    const int grid = (int)(blocks < HEAD_PARTS ? blocks : HEAD_PARTS);',
        lambda s: HEAD_PARTS * EW_THREADS // s.arm, 'rows', 'case',
        why='HEAD_PARTS = 1024 workgroups; h = 16 takes four full trips of 65 536 rows at the 300 000 rows of test_output_head',
        sizes=tuple(Size(f'head-h{h}', head_rows(h), EW_THREADS // head_lpr(h), arm=head_lpr(h)) for h in HEAD_WIDTHS),
        also=((_GATES, 'constexpr int HEAD_PARTS = 1024;'), _EW_PINS[1])),
    Row('head_fwd_bf16_kernel', 'stc_head_fwd_bf16', _GATES, 'ew_grid(rows * 2)', EW_TRIP // 2, 'rows', 'covered_by',
        covered_by=_BF + '::test_output_head_bf16', params='shape (1, 300000)', also=_EW_PINS + ((_GATES, EW_CAP),),
        why='two lanes per row under the fixed cap of 2048 workgroups: a trip is 262 144 rows, 300 000 rows are one full trip and 37 856 rows of a second'),
    Row('head_bwd_bf16_kernel', 'stc_head_bwd_bf16', _GATES,
        'long long blocks = (rows * 2 + EW_THREADS - 1) / EW_THREADS;\n    const int grid = (int)(blocks < HEAD_PARTS ? blocks : HEAD_PARTS);',
        HEAD_PARTS * EW_THREADS // 2, 'rows', 'covered_by', covered_by=_BF + '::test_output_head_bf16', params='shape (1, 300000)',
        also=((_GATES, 'constexpr int HEAD_PARTS = 1024;'), _EW_PINS[1]),
        why='HEAD_PARTS = 1024 workgroups of 128 rows: a trip is 131 072 rows, 300 000 rows are two full trips and a ragged third'),
    # ---- bf16 blend backward ---------------------------------------------------------------------------------------------------------------------------
    Row('blend_bwd_bf16_kernel', 'stc_gru_blend_bwd_bf16', 'stc_node_bf16.hip', 'hipLaunchKernelGGL(blend_bwd_bf16_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192))', BF16_BLEND_TRIP, 'pieces of 8 bf16', 'case',
        sizes=(Size('blend-bf16', BF16_BLEND_N // 8, 256),)),
    # ---- learned-graph front end -----------------------------------------------------------------------------------------------------------------------
    Row('mgp_uv_fwd_kernel', 'stc_mgp_uv_fwd_f32', 'stc_mgp_front.hip', '(total + MG_THREADS - 1) / MG_THREADS < 4096 ? (total + MG_THREADS - 1) / MG_THREADS : 4096);\n    hipLaunchKernelGGL(mgp_uv_fwd_kernel, dim3(grid)',
        MGP_TRIP, 'outputs (R K h)', 'case', also=(('stc_mgp_front.hip', 'constexpr int MG_THREADS = 256;'),), sizes=(Size('mgp-nodes', _mgp_outputs(MGP_NODES), 256), Size('mgp-categories', _mgp_outputs(MGP_CATEGORIES), 256))),
    Row('mgp_softmax_bwd_kernel', 'stc_mgp_softmax_bwd_f32', 'stc_mgp_front.hip',
        '(total + MG_THREADS - 1) / MG_THREADS < 4096 ? (total + MG_THREADS - 1) / MG_THREADS : 4096);\n    hipLaunchKernelGGL(mgp_softmax_bwd_kernel, dim3(grid)', MGP_TRIP, 'entries (R R)', 'case',
        also=(('stc_mgp_front.hip', 'constexpr int MG_THREADS = 256;'),), sizes=(Size('mgp-nodes', _mgp_entries(MGP_NODES), 256),)),
    # ---- kernels whose trips existing tests reach ---------------------------------------------------------------------------------------------------
    Row('mix_dt_kernel', 'stc_mix_dt_f32', 'stc_mix_dt.hip', 'const int grid = want < DT_MAX_GRID ? want : DT_MAX_GRID;', 512 * 4, 'tiles of floor(16 / C) nodes',
        'covered_by', covered_by=_HK + '::test_mix_dT_for_few_categories', also=(('stc_mix_dt.hip', 'constexpr int DT_MAX_GRID = 512;'),), params='(6400, 8, 32, 32, 32, 2) and (6400, 8, 32, 32, 32, 3)',
        why='DT_MAX_GRID = 512 workgroups x DT_WAVES = 4 tiles: 6 400 nodes of 8 categories are 3 200 tiles of two nodes, one full trip of 2 048 and 1 152 tiles of a second'),
    Row('bdg_node_fwd_kernel', 'stc_bdg_node_fwd_f32', 'stc_node.hip', 'n_tiles < 4 * stc::kNumCu ? n_tiles : 4 * stc::kNumCu', 4 * NUM_CU, 'tiles of max(1, 32 / C) nodes',
        'covered_by', covered_by=_HK + '::test_bdg_node_fwd', also=_EW_PINS[:1], params='shapes (4500, 32, ...) under generic-only',
        why='a fixed cap of 1 024 workgroups, one tile each per trip; at C = 32 a tile is one node: 4 500 tiles are four full trips and 404 tiles of a fifth'),
    Row('bdg_node_bwd_kernel', 'stc_bdg_node_bwd_f32', 'stc_node.hip', 'n_tiles < NODE_BWD_MAX_GRID ? n_tiles : NODE_BWD_MAX_GRID', 512, 'tiles of max(1, 32 / C) nodes',
        'covered_by', covered_by=_HK + '::test_bdg_node_bwd', also=(('stc_node.hip', 'constexpr int NODE_BWD_MAX_GRID = 512;'),),
        params='shapes (4500, 32, ...) under generic-only; also test_bdg_node_bwd_many_tiles_exercises_grid_stride',
        why='NODE_BWD_MAX_GRID = 512 workgroups, one tile each per trip: 4 500 one-node tiles are eight full trips and a ragged ninth'),
    Row('graph_grad_kernel', 'stc_graph_grad_f32', 'stc_graph_grad.hip', 'hipLaunchKernelGGL(graph_grad_kernel, dim3((unsigned)n_chunks, (unsigned)groups)', None, 'planes (selected cells x samples)',
        'covered_by', covered_by='tests/test_graph_grad_blocked.py::test_blocked_partials_equal_the_tile_per_wave_ones_bit_for_bit', params='(129, 3, 20, 3, 4), form 1',
        why='gridDim.x is the caller\'s chunk count, a trip is one plane per chunk: 9 planes over 4 chunks are two full trips and one plane of a third (no occupancy '
            'enters); the float64 comparison at two trips: tests/test_small_cell.py::test_graph_gradient_products, 288 planes over at most 256 chunks'),
    Row('graph_grad_blocked_kernel', 'stc_graph_grad_f32', 'stc_graph_grad.hip', 'hipLaunchKernelGGL(graph_grad_blocked_kernel, dim3((unsigned)n_chunks, (unsigned)(NB * NB))', None, 'planes (selected cells x samples)',
        'covered_by', covered_by='tests/test_graph_grad_blocked.py::test_blocked_partials_equal_the_tile_per_wave_ones_bit_for_bit', params='(129, 3, 20, 3, 4), form 2',
        why='as graph_grad_kernel: 9 planes over 4 chunks, and this form prefetches the next trip\'s plane (g + gridDim.x) while it multiplies'),
    Row('mix_grad_kernel', 'stc_mix_grad_f32', 'stc_graph_grad.hip', 'hipLaunchKernelGGL(mix_grad_kernel, dim3((unsigned)n_chunks, (unsigned)groups)', None, 'planes (selected cells x samples)',
        'covered_by', covered_by='tests/test_small_cell.py::test_graph_gradient_products', params='(9, 32, 100, 5, 32, 32, (0, 1, 9))',
        why='gridDim.x is the chunk count, min(GRAD_CHUNKS = 96, planes): 9 cells x 32 samples = 288 planes are three trips of 96'),
    # ---- backward matrix-core forms: capped at MF_BWD_MAX_GRID workgroups ------------------------------------------------------------------------------
    _bwd_site('node_bwd_x3_kernel', 'node bwd x3', 'stc_bdg_node_bwd_f32', 'stc_node_x3.hip', _HK + '::test_bdg_node_bwd', 'shapes (4500, 32, ...) under default',
              'MF_THREADS, lds, BwdSched<NB2, K>::waves, nodes, MF_WAVES'),
    _bwd_site('node_bwd2_x3_kernel', 'node bwd2 x3', 'stc_bdg_node_post_bwd_f32', 'stc_node_x3.hip', _HK + '::test_post_aggregation_backward', '(4500, 32, 32, 32)',
              'MF_THREADS, lds, NB2 == 1 ? 2 : 1, nodes, MF_WAVES'),
    _bwd_site('node_bwd_mfma_kernel', 'node bwd mfma', 'stc_bdg_node_bwd_f32', 'stc_node_mfma.hip', _HK + '::test_bdg_node_bwd', 'shapes (4500, 32, ...) under fp32-mfma',
              'MF_THREADS, lds, 1, nodes, MF_WAVES'),
    _bwd_site('cell_bwd_x3_kernel', 'cell bwd x3', 'stc_cell_bwd_planar_f32', 'stc_cell_bwd_x3.hip', _HK + '::test_cell_backward_in_one_launch',
              '(4500, 16, True) and (4500, 1, True)', 'CB_THREADS, lds, 1, a.nodes, CB_WAVES'),
    _bwd_site('node_bwd_bf16_kernel', 'node bwd bf16', 'stc_bdg_node_bwd_bf16', 'stc_node_bf16.hip', _BF + '::test_bdg_node_bwd_bf16', '(4500, 64, 32, 32, 32, 2)',
              'MF_THREADS, lds, BwdWaves<NB2, K>::v, nodes, MF_WAVES'),
    _bwd_site('node_bwd_bf16_kernel', 'gates bwd bf16', 'stc_cell_gates_bwd_planar_bf16', 'stc_node_bf16.hip', _BF + '::test_planar_cell_kernels_bf16',
              '(4500, 64, 16) and (4500, 64, 1)', 'MF_THREADS, lds, WAVES, nodes, MF_WAVES'),
    _bwd_site('node_post_bwd_bf16_kernel', 'post bwd bf16', 'stc_bdg_node_post_bwd_bf16', 'stc_node_bf16.hip', _BF + '::test_planar_cell_kernels_bf16',
              '(4500, 64, 16) and (4500, 64, 1)', 'MF_THREADS, lds, NB2 == 1 ? 2 : 1, nodes, MF_WAVES'),
    _bwd_site('cell_bwd_bf16_kernel', 'cell bwd bf16', 'stc_cell_bwd_planar_bf16', 'stc_node_bf16.hip', _BF + '::test_cell_backward_in_one_launch_bf16',
              '(4500, 64, 16), (4500, 32, 16), (4500, 32, 4)', 'MF_THREADS, lds, 1, a.nodes, MF_WAVES'),
    # ---- forward matrix-core forms: sized by residency alone -------------------------------------------------------------------------------------------
    _fwd_site('node_fwd_x3_kernel', 'node fwd x3', 'stc_bdg_node_fwd_f32', 'stc_node_x3.hip', 'node-fwd[default]', 'MF_THREADS, lds, 2, nodes, MF_WAVES'),
    _fwd_site('node_fwd2_x3_kernel', 'node fwd2 x3', 'stc_bdg_node_post_fwd_f32', 'stc_node_x3.hip', 'node-post-fwd[default]',
              'MF_THREADS, lds, NB2 == 1 ? 2 : 1, nodes, MF_WAVES'),
    _fwd_site('node_fwd_mfma_kernel', 'node fwd mfma', 'stc_bdg_node_fwd_f32', 'stc_node_mfma.hip', 'node-fwd[fp32-mfma]', 'MF_THREADS, lds, 2, nodes, MF_WAVES'),
    _fwd_site('node_fwd_bf16_kernel', 'node fwd bf16', 'stc_bdg_node_fwd_bf16', 'stc_node_bf16.hip', 'node-fwd-bf16', 'MF_THREADS, lds, 2, nodes, MF_WAVES'),
    _fwd_site('cell_gates_fwd_bf16_kernel', 'gates fwd bf16', 'stc_cell_gates_fwd_planar_bf16', 'stc_node_bf16.hip', 'gates-fwd-bf16', 'MF_THREADS, lds, 2, nodes, MF_WAVES'),
    # ---- exempt ------------------------------------------------------------------------------------------------------------------------------------------
    Row('mixed_fusion_fwd_kernel', 'stc_mixed_fusion_fwd_f32', 'stc_mixed_fusion.hip', 'hipLaunchKernelGGL(mixed_fusion_fwd_kernel, dim3(blocks < 8192 ? blocks : 8192)', 8192 * 4, 'rows of the D x D weights (one per wave)',
        'exempt', why='a second trip needs D > 8192 x 4 = 32 768 rows: two D x D float matrices of 4.3 GB each; the dense fusion is not used at that size '
                      '(the rank-r form of stc_mixed_fusion_lr.hip takes over, whose grids are exact)'),
    Row('wave_done', 'stc_spmm_sum_f32', 'stc_spmm.hip', 'blockIdx.x + blockIdx.y * gridDim.x', None, '-', 'exempt',
        why='no loop: gridDim.x only linearises the workgroup index into a slot of the |Y| maxima (RowsF32::wave_done); the aggregation grids are exact'),
)

STATUSES = ('case', 'covered_by', 'exempt')


# ---- the scan of csrc/ --------------------------------------------------------------------------------------------------------------------------
_KERNEL = re.compile(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(')
_DEVICE_FN = re.compile(r'__device__[^;{(]*?\b(\w+)\s*\(')
_USE = re.compile(r'gridDim\.x|persistent_grid<')
_SITE = re.compile(r'"hipFuncSetAttribute\(([^)"]*)\)"')


def scan(csrc=CSRC):
    """{(file, kernel or site label)}: per use of ``gridDim.x`` the enclosing ``__global__`` kernel (the nearest definition above it; where the file
    has none above it, the nearest ``__device__`` function), per call of ``stc::persistent_grid<`` the label it passes.

    A limitation: "enclosing" is decided by position, not by parsing.  A ``gridDim.x`` in a ``__device__`` helper that is defined BELOW some kernel
    of the same file is booked to that kernel, so a new grid-stride helper placed there hides behind the existing row.  It holds for the tree as
    it is (every use sits in the body of the kernel named, or in ``RowsF32::wave_done`` above the first kernel of stc_spmm.hip); who adds such a
    helper adds its row by hand."""
    found = set()
    for path in sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h'))):
        with open(path) as f:
            text = f.read()
        name = os.path.basename(path)
        kernels = [(m.start(), m.group(1)) for m in _KERNEL.finditer(text)]
        for m in _USE.finditer(text):
            if m.group(0) == 'gridDim.x':
                above = [k for at, k in kernels if at < m.start()]
                if not above:
                    above = [d.group(1) for d in _DEVICE_FN.finditer(text, 0, m.start())]
                found.add((name, above[-1] if above else '?'))
            else:
                label = _SITE.search(text, m.start(), m.start() + 300)
                found.add((name, label.group(1) if label else '?'))
    return found


def table_keys(rows=ROWS):
    """What the rows claim to cover, as ``scan`` names it: (file, kernel) of every row and (file, site) of the rows that have one."""
    keys = set()
    for r in rows:
        keys.add((r.file, r.kernel))
        if r.site:
            keys.add((r.file, r.site))
    return keys


def pins(row):
    """[(file, literal text)] a row pins: its cap expression and the constants that expression is made of."""
    return [(row.file, row.cap)] + list(row.also)


# ---- trip arithmetic -------------------------------------------------------------------------------------------------------------------------------
def trips(items, per_trip, block):
    """(full trips, whole workgroups of the last trip, items of its partial workgroup)."""
    full, rest = divmod(items, per_trip)
    whole, partial = divmod(rest, block)
    return full, whole, partial


def geometry_problems(row, size):
    """Why ``size`` is NOT two full trips and a ragged one for ``row`` (an empty list: it is)."""
    per_trip = row.trip(size)
    full, whole, partial = trips(size.items, per_trip, size.block)
    out = []
    if full < 2:
        out.append(f'{full} full trips of {per_trip} {row.unit}')
    if whole < 1:
        out.append('no whole workgroup in the last trip')
    if not 0 < partial < size.block:
        out.append(f'the last workgroup holds {partial} of {size.block} items: the guard splits no lane from another')
    if size.unroll and (partial % size.unroll == 0 or partial >= size.block - size.unroll):
        out.append(f'{partial} items: the guard does not split inside the unroll over pieces of {size.unroll} and leave a whole piece empty')
    return out


def regions(rows, trip_rows):
    """[(name, lo, hi)] of the rows (dim 0) of a launch's operands: the first trip, the full trips after it, the ragged one.  ``trip_rows`` may be
    fractional (a row of L items): a boundary row belongs to the earlier region."""
    full = int(rows // trip_rows)
    a = min(rows, math.ceil(trip_rows))
    b = max(a, min(rows, math.ceil(full * trip_rows)))
    return [(n, lo, hi) for n, lo, hi in (('first', 0, a), ('second', a, b), ('ragged', b, rows)) if hi > lo]


# ---- the checker of an elementwise launch ----------------------------------------------------------------------------------------------------------
def slices(rows, limit, step=4):
    """Consecutive [lo, hi) that cover 0..rows, each at most ``limit`` rows, every start a multiple of ``step`` rows."""
    width = max(step, limit // step * step)
    return [(lo, min(rows, lo + width)) for lo in range(0, rows, width)]


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    d = float(b.abs().max())
    return float((a - b).abs().max()) / (d if d > 0 else 1.0)


def check_launch(run, rows, trip_rows, ref=None, bound=None, parts=None, judge=None, what=''):
    """The three checks of a launch whose every result element is a function of its own inputs alone.

    ``run(lo, hi)`` -> {name: tensor}: ONE launch over rows lo..hi of the operands, every output pre-filled with NaN (in-place operators on clones);
    dim 0 of every returned tensor is the rows.  Returns the list of what is wrong:
      (a) an output element that is not finite;
      (b) the launch over all rows is not bitwise the concatenation of launches over ``parts`` (default: slices under half a trip) -- no tolerance;
      (c) against ``ref`` {name: float64 tensor}: per trip region (first / second / ragged), ``judge(name, got, want)`` -> message or None; the
          default judge is max|a - b| / max|b| < ``bound`` within the region.
    """
    problems = []
    whole = run(0, rows)
    for name, t in whole.items():
        bad = ~torch.isfinite(t.float())
        if bool(bad.any()):
            first = int(bad.flatten(1).any(1).nonzero()[0]) if t.dim() > 1 else int(bad.nonzero()[0])
            problems.append(f'(a) {what}{name}: {int(bad.sum())} elements are not finite, the first in row {first} (trip {first // max(1, int(trip_rows))})')
    parts = parts if parts is not None else slices(rows, max(1, int(trip_rows / 2) - 1))
    assert all(hi - lo < trip_rows / 2 for lo, hi in parts), 'a slice reaches half a trip'
    pieces = [run(lo, hi) for lo, hi in parts]
    for name, t in whole.items():
        joined = torch.cat([p[name] for p in pieces], 0)
        same = joined.view(torch.int16 if t.element_size() == 2 else torch.int32) == t.view(torch.int16 if t.element_size() == 2 else torch.int32)
        if not bool(same.all()):
            row = int((~same).flatten(1).any(1).nonzero()[0]) if t.dim() > 1 else int((~same).nonzero()[0])
            problems.append(f'(b) {what}{name}: {int((~same).sum())} elements differ from the sliced launches, the first in row {row} (trip {row // max(1, int(trip_rows))})')
    if ref is not None:
        judge = judge or (lambda name, got, want: None if rel(got, want) < bound else f'{rel(got, want):.3e} >= {bound:.1e}')
        for name, t in whole.items():
            for region, lo, hi in regions(rows, trip_rows):
                msg = judge(name, t[lo:hi], ref[name][lo:hi])
                if msg:
                    problems.append(f'(c) {what}{name}, {region} trip (rows {lo}..{hi}): {msg}')
    return problems


def log_parity(what, err, noise, factor, bound):
    """Error, the yardstick's own noise and the factor allowed over it, side by side in parity_errors.tsv of the directory ``STC_PARITY_DIR`` names
    (where a job keeps its records; else the temporary directory), as tests/test_mgp_csr.py does."""
    out = os.environ.get('STC_PARITY_DIR') or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'parity_errors.tsv'), 'a') as f:
        f.write(f'{os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]}\t{what}\t{err:.3e}\tfp32-torch-noise\t{noise:.3e}\tfactor\t{factor:g}\tbound\t{bound:.3e}\n')
