"""The launches of the cell-graph executor against a recording: same kernels, same operands, same order.

tests/cell_graph_traces.json holds, per case of tests/launch_trace.py and kernel set, the launch names of the forward and of the backward and
a hash of their full encoding (every argument; tensors as buffer number, offset, shape, stride, dtype), recorded from a checkout known to be
right.  A change to ``stc_hip.ops`` that is meant to leave the launches alone passes here without touching the fixture; one that means to change
them re-records the fixture from the commit BEFORE it for every case it leaves alone, and says which cases it changes and why.
"""
import json

import pytest

from tests import launch_trace as LT

CASES = ([pytest.param('cpu', n, id=f'cpu-{n}') for n in LT.cases_of('cpu')]
         + [pytest.param('gpu', n, id=f'gpu-{n}', marks=pytest.mark.gpu) for n in LT.cases_of('gpu')])


@pytest.fixture(scope='module')
def recorded():
    with open(LT.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('kind,name', CASES)
def test_launches_match_the_recording(kind, name, recorded, tmp_path):
    want = recorded[kind][name]
    fwd, bwd, _ = LT.run_case(name, kind)
    for direction, launches in (('forward', fwd), ('backward', bwd)):
        got = LT.summary(launches)
        if got != want[direction]:
            full = tmp_path / f'{kind}-{name}-{direction}.json'
            full.write_text(json.dumps(launches, indent=1))
        assert got['names'] == want[direction]['names'], f'{name} {direction}: other launches than recorded; full trace in {full}'
        assert got['sha256'] == want[direction]['sha256'], f'{name} {direction}: the recorded launches with other operands; full trace in {full}'


def test_every_case_is_recorded(recorded):
    for kind in ('cpu', 'gpu'):
        assert set(recorded[kind]) - {'recorded_at'} == set(LT.cases_of(kind))
