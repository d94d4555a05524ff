"""Guard-band cases of ``stc_cell_dtc_gates_planar_f32`` / ``stc_cell_dtc_cand_planar_f32`` (ABI v43) on the harness of tests/test_guard_bands.py:
every plane and weight table 16 bytes (mod 128) into a larger allocation with NaN margins, ``partials`` (slots, C, C) banded as well and
holding values before the launch (the kernels ADD); margins keep their bits, the inputs keep theirs, the result is finite, equals the launch on
plain tensors bit for bit and, summed over its slots, lies within 1e-6 of the float64 statement of tests/test_cell_dtc_planar.py (its floor:
the planes here are plain standard normals).  Shapes: both C, a wide and a narrow input plane, a ragged last slot and more than two slots.

The cases are run here, and importing this file also appends them to ``tests.test_guard_bands.CASES``, exactly as
tests/test_graph_grad_csr_guard_bands.py does."""
import pytest
import torch

from stc_hip import _lib
from tests import test_guard_bands as gb
from tests.test_cell_dtc_planar import CAND, CAND_ARGS, FLOOR, GATE_ARGS, GATES, DtcTwin, _W

DTC_CASES = []
TWIN = DtcTwin()
START = 0.25                          # what every element of ``partials`` holds before the launch: the kernels add to it


def _dtc(which, rows, C, cin, h=16):
    names = GATE_ARGS if which == 'gates' else CAND_ARGS
    slots = -(-rows // _W)

    def make():
        g = gb._g(1000 * rows + C + cin)
        L = cin + h
        shape = dict(X=(rows, C, cin), SX=(rows, C, cin), Wg=(4 * L, 2 * h), Wc=(4 * L, h))
        spec = {n: ('in', torch.randn(*shape.get(n, (rows, C, h)), generator=g)) for n in names}
        for gate in ('U', 'R'):
            if gate in spec:
                spec[gate] = ('in', torch.sigmoid(spec[gate][1]))
        if 'Cand' in spec:
            spec['Cand'] = ('in', torch.tanh(spec['Cand'][1]))
        spec['part'] = ('io', torch.full((slots, C, C), START, dtype=torch.float64))
        return spec

    def call(k, t):
        getattr(k, 'cell_dtc_' + which)(*[getattr(t, n) for n in names], t.part)

    return dict(make=make, call=call, reduce=dict(part=lambda v: v.sum(0) - slots * START))


for which, rows, C, cin in (('gates', _W + 1, 32, 16), ('gates', 7, 64, 3), ('gates', 2 * _W + 3, 32, 1), ('cand', _W + 1, 64, 16), ('cand', 2 * _W + 3, 32, 4), ('cand', 5, 32, 2)):
    DTC_CASES.append(gb.Case(f'cell_dtc_{which}-rows{rows}-C{C}-cin{cin}', {GATES if which == 'gates' else CAND}, **_dtc(which, rows, C, cin), tol=FLOOR))

gb.CASES.extend(c for c in DTC_CASES if c.id not in {d.id for d in gb.CASES})
_BY_ID = {c.id: c for c in DTC_CASES}


@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(_BY_ID))
def test_banded_cell_dtc_launch(hip, cid, monkeypatch):
    findings = gb.run_case(_BY_ID[cid], hip, 'cuda', monkeypatch, twin=TWIN)
    assert not findings, findings


@pytest.mark.parametrize('cid', list(_BY_ID))
def test_the_harness_passes_the_twin(cid, monkeypatch):
    """The same cases through the twin on banded CPU tensors: the harness itself raises no finding."""
    assert gb.run_case(_BY_ID[cid], TWIN, 'cpu', monkeypatch, twin=TWIN) == []


def test_the_entry_points_are_named_by_banded_cases():
    assert set().union(*[c.entries for c in DTC_CASES]) == {GATES, CAND} <= set(_lib._ABI)
    assert all(c in gb.CASES for c in DTC_CASES)
    assert {c.id.split('-')[2] for c in DTC_CASES} == {'C32', 'C64'} and {c.id.split('-')[3] for c in DTC_CASES} >= {'cin16', 'cin1', 'cin4'}
