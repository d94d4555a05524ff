"""The STCGNN module and the cell-graph executors over depth, sequence length, horizon and bias, on every kernel route, against the float64 oracle
(tests/model_lattice.py holds the table, the oracle cache and the checkers).

What the goldens never ran end to end: T = 1 (every encoder cell a first-step cell, the decoder reads first-step cells directly), T = 2,
horizon = 1 (no decoder-to-decoder edge), one layer (the decoder's layer 0 reads one cell as ``x`` and as ``hs``), three layers (a middle layer
both consumer and producer), ``use_bias=False`` through the whole model, hidden widths 8 and 32.  Every case runs in grad mode (prediction,
ComboLoss, every parameter gradient) and under ``torch.no_grad()`` (the forward-only route, against float64 by the forward criterion), and asserts
the route taken: the executor (spies on ``ops.*``) and, on the GPU, the C entry points launched.

CPU: the table through the kernels' CPU twins (host logic: schedules, ledger, forms), two negative controls and the closure over the constructor.
GPU (-m gpu): one test per case.
"""
import inspect

import pytest
import torch

import STC_GNN as M
from stc_hip import ops
from tests import model_lattice as L


def _ids(cases):
    return [L.case_id(*c) for c in cases]


# ---- CPU: the table on the twins -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route,topo,bias', L.CASES, ids=_ids(L.CASES))
def test_the_lattice_on_the_cpu_twins(monkeypatch, route, topo, bias):
    """Host logic against float64: the exact twin (with the first-step capability on the routes that have it on the GPU) and, for the planar,
    C = 64, order-3 and two-ring routes, the twin with the fp16 x 2 operand format emulated."""
    found = []
    for kind in route.twins:
        with monkeypatch.context() as mp:
            mp.setattr(ops, '_kernels', L.twin_of(kind))
            found += L.check_case(route, topo, bias, 'cpu', mp, twin=kind)
    assert not found, '\n'.join(found)


_CONTROL_A = [(L.BY_NAME[r], t, b) for r in ('planar-f16x2', 'planar-bf16x3') for t in L.TOPOLOGIES for b in L.BIASES]


@pytest.mark.parametrize('route,topo,bias', _CONTROL_A, ids=_ids(_CONTROL_A))
def test_control_a_first_step_launch_that_loses_its_bias(monkeypatch, route, topo, bias):
    """Negative control 1: ``cell_gates_fwd_first`` receives ``bias=None``.  Caught by EVERY use_bias=True case of the planar routes (a, b) --
    each has a first-step cell per layer, whatever T -- and by no use_bias=False case (there is no bias to lose)."""
    monkeypatch.setattr(ops, '_kernels', L.BiaslessFirstStep())
    found = L.check_case(route, topo, bias, 'cpu', monkeypatch, twin='biasless-first-step')
    assert bool(found) == bias, '\n'.join(found) or 'a dropped first-step bias went unnoticed'
    if bias:                                                        # caught by the values -- the route is the one the table names
        assert not any('executor' in f for f in found), '\n'.join(found)


_CONTROL_B = [(L.BY_NAME[r], t, b) for r in ('planar-f16x2', 'c64', 'order3', 'few-cat-k2') for t in L.TOPOLOGIES for b in L.BIASES]


@pytest.mark.parametrize('route,topo,bias', _CONTROL_B, ids=_ids(_CONTROL_B))
def test_control_b_wrong_schedule_edge(monkeypatch, route, topo, bias):
    """Negative control 2: the decoder's first step takes layer l's state from encoder layer (l + 1) % layers.  Caught by EVERY case with two or
    three layers (at three the permutation is a rotation: a table of depth 2 alone could not tell it from a swap), on both executors; with one
    layer the edge is the right one and the case passes."""
    monkeypatch.setattr(ops, '_kernels', L.twin_of(route.twins[0]))
    monkeypatch.setattr(ops, 'stc_cell_graph', L.wrong_decoder_edge(ops.stc_cell_graph))
    found = L.check_case(route, topo, bias, 'cpu', monkeypatch, twin='wrong-edge')
    assert bool(found) == (topo[0] >= 2), '\n'.join(found) or 'a wrong schedule edge went unnoticed'


# ---- CPU: closure ----------------------------------------------------------------------------------------------------------------------------------
def test_every_constructor_argument_is_an_axis_fixed_by_a_route_or_named_as_not_swept():
    """A new argument of ``STCGNN.__init__`` fails here until someone decides where it goes."""
    args = [p for p in inspect.signature(M.STCGNN.__init__).parameters if p != 'self']
    placed = {**L.AXES, **L.BY_ROUTE, **L.NOT_SWEPT}
    assert len(placed) == len(L.AXES) + len(L.BY_ROUTE) + len(L.NOT_SWEPT), 'an argument is placed twice'
    assert set(args) == set(placed), sorted(set(args) ^ set(placed))
    fields = {f.name for f in L.dataclasses.fields(L.Route)}
    assert set(L.BY_ROUTE.values()) <= fields and all(hasattr(L, v) for v in L.AXES.values())
    for name in ('fusion_rank', 'csr_cells'):                       # the ones a route fixes through ``ctor``
        assert any(name in dict(r.ctor) for r in L.ROUTES), name
    assert all(isinstance(why, str) and len(why) > 20 for why in L.NOT_SWEPT.values())


def test_the_table_is_full_and_closed():
    """Seven topologies x two bias settings x every route; the axes hold the edge values the file is about; the two-ring route found its grid."""
    assert len(L.CASES) == len(L.ROUTES) * len(L.TOPOLOGIES) * 2 and len(set(_ids(L.CASES))) == len(L.CASES)
    layers, Ts, horizons = (set(v) for v in zip(*L.TOPOLOGIES))
    assert layers == {1, 2, 3} and {1, 2} <= Ts and {1, 2, 3} <= horizons and (2, 3, 2) in L.TOPOLOGIES
    assert {r.hidden for r in L.ROUTES} == {8, 16, 32} and {r.graph_mode for r in L.ROUTES} == {'csr-fixed', 'dense-learned', 'csr-learned'}
    assert L.ring2_grid() == (1, 16) and 'two-ring' in L.BY_NAME and len(L.ROUTES) == 15
    from stc_hip import _lib
    for r in L.ROUTES:                                              # every name of the table is an entry point of the library
        names = set(r.both + r.must[0] + r.must[1] + r.never)
        assert names <= set(_lib.EXPORTS), (r.name, sorted(names - set(_lib.EXPORTS)))
        assert not names & set(r.never) & set(r.both + r.must[0] + r.must[1]), r.name


# ---- GPU: one run per case -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('route,topo,bias', L.CASES, ids=_ids(L.CASES))
def test_the_lattice_on_the_gpu(monkeypatch, route, topo, bias):
    from stc_hip import _lib
    monkeypatch.setattr(ops, '_kernels', None)
    k = ops.kernels()
    if route.fmt is not None:
        monkeypatch.setattr(k, 'operand_format', {'f16x2': _lib.FMT_F16X2, 'bf16x3': _lib.FMT_BF16X3}[route.fmt], raising=False)
    found = L.check_case(route, topo, bias, 'cuda', monkeypatch)
    assert not found, '\n'.join(found)
