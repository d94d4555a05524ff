"""Guard-band cases of ``stc_graph_grad_csr_f32`` (ABI v42) on the harness of tests/test_guard_bands.py: A and B 16 bytes (mod 128) into larger
allocations with NaN margins, the product written into ITS block of a banded (chunks, total) float64 buffer that also holds a neighbour's block
and guard columns; margins and everything outside the block keep their bits, the block is finite, equals the launch on plain tensors bit for
bit and lies within 1e-6 (``EINSUM_BOUND``) of the float64 twin of tests/test_graph_grad_csr.py.  The index arrays stay plain, as everywhere in
that harness.  Patterns and widths: the hub (a row of 79 entries) at F = 60, ragged at F = 256, one_way (empty rows) at F = 512.

The cases are run here, and importing this file also appends them to ``tests.test_guard_bands.CASES``, exactly as
tests/test_mgp_csr_guard_bands.py does."""
import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib
from tests import test_guard_bands as gb
from tests.test_graph_grad_blocked import EINSUM_BOUND
from tests.test_graph_grad_csr import ENTRY, pattern, sampled_twin

CSR_CASES = []
GUARD, OTHER = gb.GUARD, 50


class SampledTwin(EmulatedKernels):
    """The CPU twin with the sampled product, in the operands' own precision (the harness hands it float64)."""

    def graph_grad_csr(self, rowptr, colidx, A, Bm, cell0, cell_step, n_sel, N, into=None):
        out = sampled_twin(rowptr, colidx, A, Bm, cell0, cell_step, n_sel, N)
        if into is None:
            return out
        part, off = into
        part[:, off:off + out.numel()] = 0.0
        part[0, off:off + out.numel()] = out


TWIN = SampledTwin()


def _sampled(name, cells, B, C, w, sel, chunks):
    N, rowptr, colidx = pattern(name)
    nnz = colidx.numel()
    first = GUARD + OTHER + GUARD
    total = first + nnz + GUARD

    def make():
        g = gb._g(cells * N + w)
        A, Bm = torch.randn(cells, B, N * C, w, generator=g), torch.randn(cells, B, N * C, w, generator=g)
        return dict(A=('in', A), Bm=('in', Bm), rowptr=('idx', rowptr), colidx=('idx', colidx), part=('io', torch.full((chunks, total), 9.0, dtype=torch.float64)))

    def call(k, t):
        k.graph_grad_csr(t.rowptr, t.colidx, t.A, t.Bm, *sel, N, into=(t.part, first))

    def check(t, _):
        keep = torch.ones(total, dtype=torch.bool)
        keep[first:first + nnz] = False
        return [] if bool((t.part[:, keep.to(t.part.device)] == 9.0).all()) else ['the neighbouring block or a guard column of the partial buffer changed']
    return dict(make=make, call=call, check=check, reduce=dict(part=lambda v: v[:, first:first + nnz].sum(0)))


for name, cells, B, C, w, sel, chunks in (('hub', 6, 2, 3, 20, (1, 2, 3), 11), ('ragged', 4, 3, 8, 32, (0, 3, 2), 3), ('one_way', 3, 2, 16, 32, (2, 1, 1), 1)):
    CSR_CASES.append(gb.Case(f'graph_grad_csr-{name}-F{C * w}-chunks{chunks}', {ENTRY}, **_sampled(name, cells, B, C, w, sel, chunks), tol=EINSUM_BOUND))

gb.CASES.extend(c for c in CSR_CASES if c.id not in {d.id for d in gb.CASES})
_BY_ID = {c.id: c for c in CSR_CASES}


@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(_BY_ID))
def test_banded_graph_grad_csr_launch(hip, cid, monkeypatch):
    findings = gb.run_case(_BY_ID[cid], hip, 'cuda', monkeypatch, twin=TWIN)
    assert not findings, findings


@pytest.mark.parametrize('cid', list(_BY_ID))
def test_the_harness_passes_the_twin(cid, monkeypatch):
    """The same cases through the twin on banded CPU tensors: the harness itself raises no finding."""
    assert gb.run_case(_BY_ID[cid], TWIN, 'cpu', monkeypatch, twin=TWIN) == []


def test_the_entry_point_is_named_by_banded_cases():
    assert set().union(*[c.entries for c in CSR_CASES]) == {ENTRY} <= set(_lib._ABI)
    assert all(c in gb.CASES for c in CSR_CASES)
    assert sorted(c.id.split('-')[2] for c in CSR_CASES) == ['F256', 'F512', 'F60']
