"""Guard-band cases of the ComboLoss entry points (ABI v39), on the harness of tests/test_guard_bands.py: every operand 16 bytes (mod 128)
into a larger allocation, NaN / bit-pattern margins, the workspace at exactly the queried size; margins keep their bits, results are finite,
equal the launch on plain tensors bit for bit and lie within ``TOL`` of the float64 twin.

The cases are run here, and importing this file also appends them to ``tests.test_guard_bands.CASES``: that file's coverage walk
(``test_every_entry_point_has_a_banded_case``) goes over the whole ctypes table and wants every entry point named by a case of ITS table; it
imports every tests/test_*_guard_bands.py itself, so it also passes when tests/test_guard_bands.py is run alone."""
import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib
from tests import test_guard_bands as gb

CHUNK = _lib.LOSS_CHUNK
LOSS_CASES = []


class ComboLossTwin(EmulatedKernels):
    """The CPU twin with the loss entry points: include/stc_hip.h "ComboLoss" in torch, in the operands' own precision (float64 in the harness)."""

    combo_loss = True

    @staticmethod
    def _clamp(v, lo):
        return torch.where(v < lo, torch.full_like(v, lo), v)          # hands a NaN on

    def combo_loss_fwd(self, p3, y3, loss, sums):
        batch = p3.shape[0]
        bce = -(y3 * self._clamp(torch.log(p3), -100.0) + (1 - y3) * self._clamp(torch.log(1 - p3), -100.0))
        sums[:, 0], sums[:, 1] = (p3 * y3).sum((1, 2)).to(sums.dtype), (p3 + y3).sum((1, 2)).to(sums.dtype)
        loss.copy_(bce.sum() / p3.numel() + (1 - 2 * sums[:, 0] / sums[:, 1]).sum() / batch)

    def combo_loss_bwd(self, p3, y3, sums, grad_out, dp3):
        batch = p3.shape[0]
        I, D = sums[:, 0].reshape(batch, 1, 1), sums[:, 1].reshape(batch, 1, 1)
        dp3.copy_(grad_out.reshape(()) * ((p3 - y3) / self._clamp(p3 * (1 - p3), 1e-12) / p3.numel() - (2.0 / batch) * (y3 * D - I) / D ** 2))


def case(*a, **kw):
    LOSS_CASES.append(gb.Case(*a, **kw))


def _operands(shape):
    g = gb._g(sum(shape))
    return torch.rand(*shape, generator=g).clamp(0.01, 0.99), (torch.rand(*shape, generator=g) < 0.3).float()


def _loss_fwd(shape):
    def make():
        p, y = _operands(shape)
        return dict(p=('in', p), y=('in', y), loss=('out', torch.empty(1)), sums=('out', torch.empty(shape[0], 2, dtype=torch.float64)))

    def call(k, t):
        k.combo_loss_fwd(t.p, t.y, t.loss, t.sums)
    return make, call


def _loss_bwd(shape):
    def make():
        p, y = _operands(shape)
        sums = torch.stack([(p * y).double().sum((1, 2)), (p + y).double().sum((1, 2))], 1)
        return dict(p=('in', p), y=('in', y), sums=('in', sums), g=('in', torch.tensor([0.37])), dp=('out', torch.empty(*shape)))

    def call(k, t):
        k.combo_loss_bwd(t.p, t.y, t.sums, t.g, t.dp)
    return make, call


for shape in ((2, 2, CHUNK + 8), (3, 1, 36)):
    sid = 'x'.join(str(n) for n in shape)
    case(f'combo_loss_fwd-{sid}', {'stc_combo_loss_fwd_f32'}, *_loss_fwd(shape))
    case(f'combo_loss_bwd-{sid}', {'stc_combo_loss_bwd_f32'}, *_loss_bwd(shape))

gb.CASES.extend(c for c in LOSS_CASES if c.id not in {d.id for d in gb.CASES})
_BY_ID = {c.id: c for c in LOSS_CASES}
TWIN = ComboLossTwin()


@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(_BY_ID))
def test_banded_combo_loss_launch(hip, cid, monkeypatch):
    findings = gb.run_case(_BY_ID[cid], hip, 'cuda', monkeypatch, twin=TWIN)
    assert not findings, findings


@pytest.mark.parametrize('cid', list(_BY_ID))
def test_the_harness_passes_the_loss_twin(cid, monkeypatch):
    """The same cases through the twin on banded CPU tensors: the harness itself raises no finding, and the twin is its own float64 run."""
    assert gb.run_case(_BY_ID[cid], TWIN, 'cpu', monkeypatch, twin=TWIN) == []


def test_the_loss_entry_points_are_named_by_banded_cases():
    named = set().union(*[c.entries for c in LOSS_CASES])
    assert named == {'stc_combo_loss_fwd_f32', 'stc_combo_loss_bwd_f32'} and named <= set(_lib._ABI)
    assert all(c in gb.CASES for c in LOSS_CASES)
