"""Guard-band cases of the pattern entry points of the learned graph generator (ABI v41: ``stc_mgp_csr_score_f32``,
``stc_mgp_csr_softmax_fwd_f32`` / ``_bwd_f32``, ``stc_mgp_csr_score_bwd_f32``), on the harness of tests/test_guard_bands.py: U, V and the
cotangent 16 bytes (mod 128) into larger allocations with NaN margins, the results the binding allocates banded as well; margins keep their
bits, results are finite, equal the launch on plain tensors bit for bit and lie within ``TOL`` / ``FUSION_GRAD`` of the float64 twin of
tests/test_mgp_csr.py.  The index arrays stay plain, as everywhere in that harness.

The cases are run here, and importing this file also appends them to ``tests.test_guard_bands.CASES``, exactly as
tests/test_mixed_fusion_lr_guard_bands.py does."""
import pytest
import torch

from stc_hip import _lib
from stc_hip.graph import csr_pattern
from tests import test_guard_bands as gb
from tests.conftest import rel_err
from tests.test_hip_kernels import FUSION_GRAD, TOL
from tests.test_mgp_csr import MgpCsrTwin, graph_of, reference

CSR_CASES = []
TWIN = MgpCsrTwin()
ENTRIES = {'stc_mgp_csr_score_f32', 'stc_mgp_csr_softmax_fwd_f32', 'stc_mgp_csr_softmax_bwd_f32', 'stc_mgp_csr_score_bwd_f32'}
INDEX = ('rowptr', 'colidx', 't_rowptr', 't_colidx', 't_entry')


def _mgp_csr(name, KH):
    def make():
        ref = reference(name, KH, 'quarter')
        pat = csr_pattern(graph_of(name), 'cpu')
        return dict(U=('in', ref['U']), V=('in', ref['V']), dPs=('in', ref['R']), **{k: ('idx', pat[k]) for k in INDEX})

    def call(k, t):
        score = k.mgp_csr_score(t.U, t.V, t.rowptr, t.colidx)
        Ps = k.mgp_csr_softmax_fwd(score, t.rowptr)
        ds = k.mgp_csr_softmax_bwd(score, Ps, t.dPs, t.rowptr)
        dU, dV = k.mgp_csr_score_bwd(t.U, t.V, ds, t.rowptr, t.colidx, t.t_rowptr, t.t_colidx, t.t_entry)
        return score, Ps, ds, dU, dV

    def check(t, ret):
        d = lambda x: x.double().cpu()
        idx = [getattr(t, k).cpu() for k in INDEX]
        score = TWIN.mgp_csr_score(d(t.U), d(t.V), idx[0], idx[1])
        Ps = TWIN.mgp_csr_softmax_fwd(score, idx[0])
        ds = TWIN.mgp_csr_softmax_bwd(score, Ps, d(t.dPs), idx[0])
        dU, dV = TWIN.mgp_csr_score_bwd(d(t.U), d(t.V), ds, *idx)
        errs = [(n, rel_err(got, want), bound) for n, got, want, bound in zip(('score', 'Ps', 'ds', 'dU', 'dV'), ret, (score, Ps, ds, dU, dV),
                                                                              (TOL, TOL, FUSION_GRAD, FUSION_GRAD, FUSION_GRAD))]
        return [f'mgp_csr.{n}: {e:.2e} from float64 (bound {bound})' for n, e, bound in errs if not e < bound]
    return dict(make=make, call=call, check=check)


for name, KH in (('hub83', 4), ('hub80', 60), ('ragged', 260)):
    CSR_CASES.append(gb.Case(f'mgp_csr-{name}-KH{KH}', ENTRIES, **_mgp_csr(name, KH), twin=False, fronts=5))      # score, Ps, ds, dU, dV

gb.CASES.extend(c for c in CSR_CASES if c.id not in {d.id for d in gb.CASES})
_BY_ID = {c.id: c for c in CSR_CASES}


@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(_BY_ID))
def test_banded_mgp_csr_launch(hip, cid, monkeypatch):
    findings = gb.run_case(_BY_ID[cid], hip, 'cuda', monkeypatch)
    assert not findings, findings


@pytest.mark.parametrize('cid', list(_BY_ID))
def test_the_harness_passes_the_twin(cid, monkeypatch):
    """The same cases through the twin on banded CPU tensors: the harness itself raises no finding."""
    assert gb.run_case(_BY_ID[cid], TWIN, 'cpu', monkeypatch) == []


def test_the_entry_points_are_named_by_banded_cases():
    named = set().union(*[c.entries for c in CSR_CASES])
    assert named == ENTRIES and named <= set(_lib._ABI)
    assert all(c in gb.CASES for c in CSR_CASES)
    assert 'stc_mgp_csr_supported' in _lib._ABI                                  # no device buffers: no case
