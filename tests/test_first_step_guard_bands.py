"""Guard-band cases of the first-step entry points (ABI v37), on the harness of tests/test_guard_bands.py: every operand 16 bytes (mod 128)
into a larger allocation, NaN / bit-pattern margins, the workspace at exactly the queried size; margins keep their bits, results are finite,
equal the launch on plain tensors bit for bit and lie within the family's bound of the float64 twin.

The cases are run here, and importing this file also appends them to ``tests.test_guard_bands.CASES``: that file's coverage walk
(``test_every_entry_point_has_a_banded_case``) goes over the whole ctypes table and wants every entry point named by a case of ITS table; it
imports every tests/test_*_guard_bands.py itself, so it also passes when tests/test_guard_bands.py is run alone.  The follow-up is to move these cases into
tests/test_guard_bands.py and delete this file."""
import pytest
import torch

from stc_hip import _lib
from stc_hip.graph import csr_operand
from tests import test_guard_bands as gb
from tests.test_first_step_route import FirstStepTwin
from tests.test_grad_scale import BOUND

FIRST_CASES = []


def case(*a, **kw):
    FIRST_CASES.append(gb.Case(*a, **kw))


def _first(kind, nodes, cin, acc=False, with_amax=False):
    C, h = 32, 16
    Lw, wide = cin + h, cin == h

    def make():
        g = gb._g(7 * nodes + cin)
        rnd = lambda *s: torch.randn(*s, generator=g)
        new = lambda *s: torch.empty(*s)
        X, SX = rnd(nodes, C, cin), rnd(nodes, C, cin)
        spec = dict(X=('in', X), SX=('in', SX), Tc=('in', gb._mix(g, 2, C)), Wg=('in', rnd(4 * Lw, 2 * h) / (4 * Lw) ** 0.5),
                    Wc=('in', rnd(4 * Lw, h) / (4 * Lw) ** 0.5))
        if kind == 'gates_fwd':
            spec.update(bg=('in', rnd(2 * h)), bc=('in', rnd(h)), U=('out', new(nodes, C, h)), A=('out', new(nodes, C, h)), Bm=('out', new(nodes, C, h)))
            return spec
        spec.update(U=('in', torch.sigmoid(rnd(nodes, C, h))), Cand=('in', torch.tanh(rnd(nodes, C, h))), dHnew=('in', rnd(nodes, C, h)), dBm=('in', rnd(nodes, C, h)),
                    dWg=('out', new(4 * Lw, 2 * h)), dbg=('out', new(2 * h)), dWc=('out', new(4 * Lw, h)), dbc=('out', new(h)))
        spec['dXs'] = ('io' if acc else 'out', [rnd(nodes, C, h), rnd(nodes, C, h)] if wide else [None, None])
        if with_amax:                                        # what the first-step forward leaves: the H rows zero
            zero = torch.zeros(1)
            spec['amax'] = ('in', gb._amax_rows((X, SX, zero, zero) if wide else (zero, zero, X, SX)))
        return spec

    def call(k, t):
        amax = dict(act_amax=t.amax) if with_amax else {}
        if kind == 'gates_fwd':
            k.cell_gates_fwd_first(t.X, t.SX, t.Tc, t.Wg, t.bg, t.U, (t.Wc, t.bc, t.A, t.Bm))
        else:
            k.cell_bwd_first(t.X, t.SX, t.Tc, t.Wg, t.Wc, t.U, t.Cand, t.dHnew, t.dBm, t.dXs, t.dWg, t.dbg, t.dWc, t.dbc, accumulate_x=acc, **amax)
    return make, call


for fmt in ('f16x2', 'bf16x3'):
    for nodes in (13, 4500):
        for cin in (16, 3, 1):
            sid = f'{fmt}-nodes{nodes}-cin{cin}'
            amax = fmt == 'f16x2'
            case(f'first_gates_fwd-{sid}', {'stc_cell_gates_fwd_first_f32'}, *_first('gates_fwd', nodes, cin), fmt=fmt)
            case(f'first_cell_bwd-{sid}', {'stc_cell_bwd_first_f32'}, *_first('cell_bwd', nodes, cin, with_amax=amax), fmt=fmt, tol=BOUND)
            if cin == 16:
                case(f'first_cell_bwd-{sid}-accumulate', {'stc_cell_bwd_first_f32'}, *_first('cell_bwd', nodes, cin, acc=True, with_amax=amax), fmt=fmt, tol=BOUND)


def _blend_first(H, W, B):
    C, h = 32, 16

    def make():
        graph = gb._grid_graph(H, W)
        rnd, unit, _ = gb._state_planes(gb._g(H * W), B, graph.n, C, h)
        return dict(graph=('arg', graph), Bm=('in', rnd()), A=('in', rnd()), U=('in', unit()), Cand=('out', rnd()), Hnew=('out', rnd()), SHnew=('out', rnd()))

    def call(k, t):
        op = csr_operand(t.graph, t.Bm.device)
        k.ring2_blend_first(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, op.fwd_ring2, t.Bm, t.A, t.U, t.Cand, t.Hnew, t.SHnew)
    return make, call


for H, W, B in ((9, 33, 1), (12, 20, 2)):
    case(f'first_ring2_blend-{H}x{W}', {'stc_ring2_blend_first_f32'}, *_blend_first(H, W, B))

gb.CASES.extend(c for c in FIRST_CASES if c.id not in {d.id for d in gb.CASES})
_BY_ID = {c.id: c for c in FIRST_CASES}
TWIN = FirstStepTwin()


@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(_BY_ID))
def test_banded_first_step_launch(hip, cid, monkeypatch):
    findings = gb.run_case(_BY_ID[cid], hip, 'cuda', monkeypatch, twin=TWIN)
    assert not findings, findings


def test_the_first_step_entry_points_are_named_by_banded_cases():
    named = set().union(*[c.entries for c in FIRST_CASES])
    assert named == {'stc_cell_gates_fwd_first_f32', 'stc_cell_bwd_first_f32', 'stc_ring2_blend_first_f32'} and named <= set(_lib._ABI)
    assert all(c in gb.CASES for c in FIRST_CASES)
