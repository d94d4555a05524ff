"""Guard-band cases of ``stc_graph_grad_csr_pairs_f32`` and ``stc_cell_dsx_narrow_planar_f32`` (ABI v44) on the harness of tests/test_guard_bands.py:
every plane and table 16 bytes (mod 128) into a larger allocation with NaN margins; the float64 accumulator banded as well and holding values
before the launch (the kernel ADDS), the d(S.x) plane banded and NaN before it (the kernel WRITES every element); margins keep their bits, the
inputs keep theirs, the results are finite, equal the launch on plain tensors bit for bit and lie within ``EINSUM_BOUND`` = 1e-6 of the float64
twin of tests/test_graph_grad_csr_pairs.py, within 1e-6 of the statement of tests/test_cell_dsx_narrow.py (the floor of its rule: the planes here
are plain standard normals).  The index arrays stay plain, as everywhere in that harness.  Patterns and widths: the hub (a row of 79 entries) with
three pairs of F = 60, 1024, 260; ragged with two of F = 512, 32; one_way (empty rows) with one of F = 4; three rows with F = 128.

The cases are run here, and importing this file also appends them to ``tests.test_guard_bands.CASES``, exactly as
tests/test_graph_grad_csr_guard_bands.py does."""
import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib
from tests import test_guard_bands as gb
from tests.test_cell_dsx_narrow import ARGS, ENTRY as DSX, _W, dsx_statement
from tests.test_cell_dtc_planar import FLOOR
from tests.test_graph_grad_blocked import EINSUM_BOUND
from tests.test_graph_grad_csr_pairs import ENTRY as PAIRS, PairsTwin, pattern

NEW_CASES = []
START = 0.25                          # what every element of the accumulator holds before the launch: the kernel adds to it


class Twin(PairsTwin):
    """The CPU twin with both operations, in the operands' own precision (the harness hands it float64)."""

    def cell_dsx_narrow(self, H, Wg, Tc, U, Rg, Cand, dHnew, dRH, dSx):
        dSx.copy_(dsx_statement(H, Wg, Tc, U, Rg, Cand, dHnew, dRH, dSx.shape[-1]))


TWIN = Twin()


def _pairs(name, widths, B):
    N, rowptr, colidx = pattern(name)
    n = len(widths)

    def make():
        g = gb._g(1000 * N + sum(widths) + B)
        spec = {f'{side}{p}': ('in', torch.randn(B, N, F, generator=g)) for p, F in enumerate(widths) for side in 'AB'}
        spec.update(rowptr=('idx', rowptr), colidx=('idx', colidx), acc=('io', torch.full((colidx.numel(),), START, dtype=torch.float64)))
        return spec

    def call(k, t):
        k.graph_grad_csr_pairs(t.rowptr, t.colidx, [(getattr(t, f'A{p}'), getattr(t, f'B{p}')) for p in range(n)], N, t.acc)

    return dict(make=make, call=call, reduce=dict(acc=lambda v: v - START))


def _dsx(rows, C, cin, h=16):
    def make():
        g = gb._g(1000 * rows + C + cin)
        shape = dict(Wg=(4 * (cin + h), 2 * h), Tc=(2, C, C))
        spec = {n: ('in', torch.randn(*shape.get(n, (rows, C, h)), generator=g)) for n in ARGS}
        for gate in ('U', 'R'):
            spec[gate] = ('in', torch.sigmoid(spec[gate][1]))
        spec['Cand'] = ('in', torch.tanh(spec['Cand'][1]))
        spec['Tc'] = ('in', spec['Tc'][1] / C ** 0.5)
        spec['dSx'] = ('out', torch.zeros(rows, C, cin))
        return spec

    def call(k, t):
        k.cell_dsx_narrow(*[getattr(t, n) for n in ARGS], t.dSx)

    return dict(make=make, call=call)


for name, widths, B in (('hub', (60, 1024, 260), 2), ('ragged', (512, 32), 3), ('one_way', (4,), 1), ('three_rows', (128,), 2)):
    NEW_CASES.append(gb.Case(f'graph_grad_csr_pairs-{name}-F{"+".join(map(str, widths))}-B{B}', {PAIRS}, **_pairs(name, widths, B), tol=EINSUM_BOUND))
for rows, C, cin in ((_W + 1, 32, 1), (7, 64, 3), (2 * _W + 3, 32, 4), (_W - 1, 64, 2)):
    NEW_CASES.append(gb.Case(f'cell_dsx_narrow-rows{rows}-C{C}-cin{cin}', {DSX}, **_dsx(rows, C, cin), tol=FLOOR))

gb.CASES.extend(c for c in NEW_CASES if c.id not in {d.id for d in gb.CASES})
_BY_ID = {c.id: c for c in NEW_CASES}


@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(_BY_ID))
def test_banded_launch(hip, cid, monkeypatch):
    findings = gb.run_case(_BY_ID[cid], hip, 'cuda', monkeypatch, twin=TWIN)
    assert not findings, findings


@pytest.mark.parametrize('cid', list(_BY_ID))
def test_the_harness_passes_the_twin(cid, monkeypatch):
    """The same cases through the twin on banded CPU tensors: the harness itself raises no finding."""
    assert gb.run_case(_BY_ID[cid], TWIN, 'cpu', monkeypatch, twin=TWIN) == []


def test_the_entry_points_are_named_by_banded_cases():
    assert set().union(*[c.entries for c in NEW_CASES]) == {PAIRS, DSX} <= set(_lib._ABI)
    assert all(c in gb.CASES for c in NEW_CASES)
    assert not hasattr(EmulatedKernels, 'graph_grad_csr_pairs') and not hasattr(EmulatedKernels, 'cell_dsx_narrow')      # the twins live in the tests
    assert {c.id.split('-')[2] for c in NEW_CASES if c.id.startswith('cell_dsx')} == {'C32', 'C64'}
