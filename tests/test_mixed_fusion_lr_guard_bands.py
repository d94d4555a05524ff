"""Guard-band cases of the rank-r MixedFusion entry points (ABI v40), on the harness of tests/test_guard_bands.py: every operand 16 bytes
(mod 128) into a larger allocation with NaN margins, the results and the workspace banded as well, the workspace at exactly the queried
size; margins keep their bits, results are finite, equal the launch on plain tensors bit for bit and lie within ``TOL`` / ``FUSION_GRAD`` of
the float64 twin of tests/test_mixed_fusion_lr.py.

The cases are run here, and importing this file also appends them to ``tests.test_guard_bands.CASES``, exactly as
tests/test_combo_loss_guard_bands.py does: that file's coverage walk (``test_every_entry_point_has_a_banded_case``) goes over the whole ctypes
table and wants every entry point named by a case of ITS table; it imports every tests/test_*_guard_bands.py itself."""
import pytest
import torch

from stc_hip import _lib
from tests import test_guard_bands as gb
from tests.conftest import rel_err
from tests.test_hip_kernels import FUSION_GRAD, TOL
from tests.test_mixed_fusion_lr import NAMES, FusionLRTwin, inputs

LR_CASES = []
TWIN = FusionLRTwin()
ENTRIES = {'stc_mixed_fusion_lr_fwd_f32', 'stc_mixed_fusion_lr_bwd_f32'}
OUT = ('dUA', 'dVA', 'dUP', 'dVP', 'db', 'dA', 'dP')


def _fusion_lr(n, r, want):
    def make():
        ops_, R = inputs(n, r, 'wide')
        return dict({k: ('in', v) for k, v in ops_.items()}, dG=('in', R))

    def call(k, t):
        gate, G, tt = k.mixed_fusion_lr_fwd(t.UA, t.VA, t.bA, t.UP, t.VP, t.bP, t.A, t.P)
        grads = k.mixed_fusion_lr_bwd(t.UA, t.VA, t.UP, t.VP, t.A, t.P, gate, tt, t.dG, want)
        return (gate, G, tt) + tuple(x for x in grads if x is not None)

    def check(t, ret):
        d = lambda x: x.double().cpu()
        gate, G, tt = TWIN.mixed_fusion_lr_fwd(d(t.UA), d(t.VA), d(t.bA), d(t.UP), d(t.VP), d(t.bP), d(t.A), d(t.P))
        grads = TWIN.mixed_fusion_lr_bwd(d(t.UA), d(t.VA), d(t.UP), d(t.VP), d(t.A), d(t.P), gate, tt, d(t.dG), want)
        kept = [(name, x) for name, x in zip(OUT, grads) if x is not None]
        assert [name for name, _ in kept] == [name for name, w in zip(OUT, want[:4] + (True,) + want[4:]) if w] and len(ret) == 3 + len(kept)
        errs = [('gate', rel_err(ret[0], gate), TOL), ('G', rel_err(ret[1], G), TOL), ('t', rel_err(ret[2], tt), TOL)]
        errs += [(name, rel_err(got.reshape(x.shape), x), FUSION_GRAD) for got, (name, x) in zip(ret[3:], kept)]
        return [f'mixed_fusion_lr.{name}: {e:.2e} from float64 (bound {bound})' for name, e, bound in errs if not e < bound]
    return dict(make=make, call=call, check=check)


for n, r in ((3, 2), (10, 4), (15, 16)):
    for tag, want in (('all', (True,) * 6), ('db-only', (False,) * 6)):
        LR_CASES.append(gb.Case(f'mixed_fusion_lr-n{n}-r{r}-{tag}', ENTRIES, **_fusion_lr(n, r, want), twin=False,
                                fronts=3 + 1 + sum(want)))                     # gate, G, t; db (+ the wanted gradients); the workspace is scratch

gb.CASES.extend(c for c in LR_CASES if c.id not in {d.id for d in gb.CASES})
_BY_ID = {c.id: c for c in LR_CASES}


@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(_BY_ID))
def test_banded_mixed_fusion_lr_launch(hip, cid, monkeypatch):
    findings = gb.run_case(_BY_ID[cid], hip, 'cuda', monkeypatch)
    assert not findings, findings


@pytest.mark.parametrize('cid', list(_BY_ID))
def test_the_harness_passes_the_twin(cid, monkeypatch):
    """The same cases through the twin on banded CPU tensors: the harness itself raises no finding."""
    assert gb.run_case(_BY_ID[cid], TWIN, 'cpu', monkeypatch) == []


def test_the_entry_points_are_named_by_banded_cases():
    named = set().union(*[c.entries for c in LR_CASES])
    assert named == ENTRIES and named <= set(_lib._ABI)
    assert all(c in gb.CASES for c in LR_CASES)
    assert 'stc_mixed_fusion_lr_supported' in _lib._ABI and 'stc_mixed_fusion_lr_workspace_bytes' in _lib._ABI       # no device buffers: no case
    assert NAMES == ('A', 'P', 'UA', 'VA', 'bA', 'UP', 'VP', 'bP')
