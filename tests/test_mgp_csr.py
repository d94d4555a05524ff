"""Learned spatial graphs on a sparsity pattern: ``graph_mode='csr-learned'`` (``csrc/stc_mgp_csr.hip``, ABI v41: ``stc_mgp_csr_score_f32``,
``stc_mgp_csr_softmax_fwd/bwd_f32``, ``stc_mgp_csr_score_bwd_f32``; ``stc_hip.learned``, ``graph.learned_csr_operand``, ``MGP_Gen_Csr``).

    score_e = <u_i, v_j> - <v_i, u_j>,   Ps_e = softmax over the stored entries of row i of relu(score),   G = rank-r MixedFusion(A, Ps) over nnz

CPU part: header, ctypes table and EXPORTS agree; every refusal comes back before any HIP call; the torch route against a float64
dense-masked restatement written here (dense P, -inf off the pattern, softmax); on the full pattern the generator equals
``MGP_Gen(..., fusion_rank=r)`` from the same ``state_dict``; the model and the trainer build the mode; the score is additive over the K slices.

GPU part (-m gpu): kernels and operators against float64 autograd of the restatement on the patterns ``weights``, ``ragged``, ``one_way`` of
tests/graph_cases.py (first shapes) and a hub pattern (R = 80: a row of 79 entries, a single-entry row, a reciprocal pair, a diagonal entry,
empty rows; R = 83 as well, which the kernels' four rows per workgroup do not divide), rows of KH in {4, 60, 256, 260, 2304} floats,
``U, V = tanh(randn)`` raw and times KH^(-1/4), a normal cotangent.  relu's mask is discontinuous at 0, so the inputs must keep every score
away from it: asserted on the FLOAT64 reference, |score_e| >= 1e-5 max|score| except entries that are exactly 0 by construction (the
diagonal); a draw that fails advances the seed, at most 8 times.

Bounds: ``TOL`` (1e-5) of tests/test_hip_kernels.py for score and Ps; gradients max(``FUSION_GRAD`` = 2e-5, 10 x the error of the fp32 torch
expression itself against float64 on the same inputs).  Error and noise go side by side to parity_errors.tsv in the directory
``STC_PARITY_DIR`` names (where a job keeps its records; else the temporary directory), as tests/test_small_dense_split.py does."""
import os
import re
import tempfile

import numpy as np
import pytest
import torch

import STC_GNN as M
from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, _lib, fusion as F, learned, ops
from stc_hip.graph import csr_pattern, learned_csr_operand
from stc_hip.learned import csr as L
from tests import graph_cases
from tests.conftest import REPO, rel_err
from tests.test_hip_kernels import FUSION_GRAD, TOL
from tests.test_mixed_fusion_lr import expression as fusion_expression
from tests.test_module_parity import FWD, GPU

ENTRIES = ('stc_mgp_csr_supported', 'stc_mgp_csr_score_f32', 'stc_mgp_csr_softmax_fwd_f32', 'stc_mgp_csr_softmax_bwd_f32', 'stc_mgp_csr_score_bwd_f32')
LAUNCHED = ENTRIES[1:]
KHS = (4, 60, 256, 260, 2304)
SCALES = ('raw', 'quarter')
MARGIN = 1e-5


# ---- patterns -------------------------------------------------------------------------------------------------------------------------------
def hub_graph(R=80):
    """Row 5 holds every other node (R - 1 entries: more than a wave), row 7 a single entry, (10, 11) / (11, 10) a reciprocal pair, row 12 a
    diagonal entry and one more, the odd rows from 21 on three random entries each; rows 0 .. 4 and the even rows from 22 on are empty."""
    g = torch.Generator().manual_seed(R)
    pairs = {(5, j) for j in range(R) if j != 5} | {(7, 20), (10, 11), (11, 10), (12, 12), (12, 30)}
    for i in range(21, R, 2):
        pairs |= {(i, int(j)) for j in torch.randperm(R, generator=g)[:3] if int(j) != i}
    rows, cols = (np.array(x) for x in zip(*sorted(pairs)))
    vals = (torch.rand(len(rows), generator=g) + 0.1).numpy()
    return CsrGraph(R, rows, cols, vals)


_GRAPHS = {}


def graph_of(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = hub_graph(int(name[3:])) if name.startswith('hub') else graph_cases.case(name)[0]
    return _GRAPHS[name]


PATTERNS = ('weights', 'ragged', 'one_way', 'hub80', 'hub83')


def entries(graph):
    """(rows, cols) of the stored entries as int64 CPU tensors, in the entry order of Gs (rows ascending, columns ascending)."""
    h = graph._host
    rows = np.repeat(np.arange(graph.n), np.diff(h['bwd_rowptr']))
    return torch.from_numpy(rows).long(), torch.from_numpy(h['bwd_colidx'].astype(np.int64))


# ---- the restatement: dense P, -inf off the pattern, softmax ---------------------------------------------------------------------------------
def restatement(U, V, rows, cols, reduce=None):
    """(score, Ps) at the stored entries from rows U, V (R, ...), through the dense (R, R) matrices, in the operands' precision."""
    u, v = U.flatten(1), V.flatten(1)
    n = u.shape[0]
    P = u @ v.t()
    D = P - P.t()
    if reduce is not None:
        D = reduce(D)
    mask = torch.zeros(n, n, dtype=torch.bool)
    mask[rows, cols] = True
    Z = torch.where(mask, torch.relu(D), torch.full_like(D, float('-inf')))
    Z = torch.where(mask.any(-1, keepdim=True), Z, torch.zeros_like(Z))          # a row without entries produces nothing: any finite row
    return D[rows, cols], torch.softmax(Z, -1)[rows, cols]


def margin_ok(score64, rows, cols, exact=None):
    """The condition on the inputs, on the float64 reference: no score within MARGIN max|score| of relu's edge but the exact zeros."""
    exact = (rows == cols) if exact is None else exact
    s = score64.detach().abs()
    return bool((s[~exact] >= MARGIN * s.max()).all()) and bool((s[exact] == 0).all())


_REF = {}


def reference(name, KH, scale):
    """Inputs of one case and their float64 / fp32 torch results, computed once and shared: dict(U, V, R, score, Ps, dU, dV, noise_*)."""
    key = (name, KH, scale)
    if key in _REF:
        return _REF[key]
    graph = graph_of(name)
    rows, cols = entries(graph)
    for attempt in range(9):
        g = torch.Generator().manual_seed(1000 * KH + attempt)
        U, V = (torch.tanh(torch.randn(graph.n, KH, generator=g)) * (1.0 if scale == 'raw' else KH ** -0.25) for _ in range(2))
        Rc = torch.randn(graph.nnz, generator=g)
        out = {}
        for dt in (torch.float64, torch.float32):
            u, v = U.to(dt).clone().requires_grad_(), V.to(dt).clone().requires_grad_()      # (clone: .to(float32) is U itself)
            score, Ps = restatement(u, v, rows, cols)
            (Ps * Rc.to(dt)).sum().backward()
            out[dt] = (score.detach(), Ps.detach(), u.grad, v.grad)
        if margin_ok(out[torch.float64][0], rows, cols):
            break
    else:
        raise AssertionError(f'{key}: no draw in 9 seeds keeps every score {MARGIN} max|score| away from 0')
    s64, p64, du64, dv64 = out[torch.float64]
    s32, p32, du32, dv32 = out[torch.float32]
    _REF[key] = dict(U=U, V=V, R=Rc, score=s64, Ps=p64, dU=du64, dV=dv64, seed=1000 * KH + attempt,
                     noise=dict(score=rel_err(s32, s64), Ps=rel_err(p32, p64), dU=rel_err(du32, du64), dV=rel_err(dv32, dv64)))
    return _REF[key]


def _log(what, err, noise, bound):
    out = os.environ.get('STC_PARITY_DIR') or tempfile.gettempdir()       # (where a job keeps its records, else the temporary directory)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'parity_errors.tsv'), 'a') as f:
        f.write(f'{os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]}\t{what}\t{err:.3e}\tfp32-torch-noise\t{noise:.3e}\tbound\t{bound:.1e}\n')


def grad_bound(noise):
    return max(FUSION_GRAD, 10 * noise)


# ---- the generator restatement (float64 or fp32), for the module tests -----------------------------------------------------------------------
def generator_restatement(X, A_vals, rows, cols, Ac, sd, alpha=3.0, p='mix_graph_pair'):
    """(score, G values (nnz), Gc) of ``MGP_Gen_Csr.forward`` from a state dict, in the operands' precision."""
    Us = torch.tanh(alpha * torch.matmul(X, sd[f'{p}.params_S.Wu'])).flatten(0, 1).transpose(0, 1)          # (N, K, h)
    Vs = torch.tanh(alpha * torch.matmul(X, sd[f'{p}.params_S.Wv'])).flatten(0, 1).transpose(0, 1)
    score, Ps = restatement(Us, Vs, rows, cols)
    G = fusion_expression(A_vals, Ps, *[sd[f'{p}.aggreg_S.lin_{s}.{k}'] for s in 'AP' for k in ('U', 'V', 'bias')])
    Xc = X.transpose(2, 3)
    Uc = torch.tanh(alpha * torch.matmul(Xc, sd[f'{p}.params_C.Wu']))
    Vc = torch.tanh(alpha * torch.matmul(Xc, sd[f'{p}.params_C.Wv']))
    Gc = O.mixed_fusion(Ac, O._antisym_softmax(Uc, Vc), sd[f'{p}.aggreg_C.lin_A.weight'], sd[f'{p}.aggreg_C.lin_A.bias'],
                        sd[f'{p}.aggreg_C.lin_P.weight'], sd[f'{p}.aggreg_C.lin_P.bias'])
    return score, G, Gc


def model_restatement(X, graph, Ac, sd, K, hidden, layers, horizon):
    """(prediction, score) of ``STCGNN(graph_mode='csr-learned')``: the generator restatement, Gs scattered into a dense matrix, the oracle."""
    rows, cols = entries(graph)
    A_vals = torch.from_numpy(graph._host['bwd_val']).to(X.dtype)
    score, G, Gc = generator_restatement(X, A_vals, rows, cols, Ac, sd)
    Gs = torch.zeros(graph.n, graph.n, dtype=X.dtype).index_put((rows, cols), G)
    return O.encdec_forward(X, Gs, Gc, sd, K, K, hidden, layers, horizon), score


# ---- the float64 twin of the four binding methods --------------------------------------------------------------------------------------------
class MgpCsrTwin(EmulatedKernels):
    """The CPU twin with the pattern entry points: include/stc_hip.h "the learned spatial graph on a sparsity pattern" in torch, in the
    operands' own precision, from the same index arrays the kernels read."""

    def mgp_csr_supported(self, R, KH, nnz):
        return R >= 1 and nnz >= 0 and 4 <= KH <= _lib.MGP_CSR_MAX_KH and KH % 4 == 0 and R * KH < 2 ** 31

    @staticmethod
    def _rows(rowptr):
        rp = rowptr.long()
        return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])

    def mgp_csr_score(self, U, V, rowptr, colidx):
        u, v, i, j = U.flatten(1), V.flatten(1), self._rows(rowptr), colidx.long()
        return (u[i] * v[j]).sum(-1) - (v[i] * u[j]).sum(-1)

    def mgp_csr_softmax_fwd(self, score, rowptr):
        i, n = self._rows(rowptr), rowptr.numel() - 1
        r = torch.relu(score)
        ex = torch.exp(r - torch.zeros(n, dtype=score.dtype).scatter_reduce(0, i, r, 'amax', include_self=True)[i])
        return ex / torch.zeros(n, dtype=score.dtype).index_add(0, i, ex)[i]

    def mgp_csr_softmax_bwd(self, score, Ps, dPs, rowptr):
        i, n = self._rows(rowptr), rowptr.numel() - 1
        dot = torch.zeros(n, dtype=score.dtype).index_add(0, i, Ps * dPs)
        return torch.where(score <= 0, torch.zeros_like(score), Ps * (dPs - dot[i]))

    def mgp_csr_score_bwd(self, U, V, ds, rowptr, colidx, t_rowptr, t_colidx, t_entry):
        u, v = U.flatten(1), V.flatten(1)
        i, j, ti, tj, dt = self._rows(rowptr), colidx.long(), self._rows(t_rowptr), t_colidx.long(), ds[t_entry.long()]
        dU = torch.zeros_like(u).index_add(0, i, ds[:, None] * v[j]).index_add(0, ti, -dt[:, None] * v[tj])
        dV = torch.zeros_like(v).index_add(0, i, -ds[:, None] * u[j]).index_add(0, ti, dt[:, None] * u[tj])
        return dU.view(U.shape), dV.view(V.shape)


# ============================================================================================================== CPU
@pytest.mark.parametrize('name', PATTERNS)
def test_the_float64_twin_equals_autograd_of_the_restatement(name):
    """The backward formulas of the header -- the second sums run over the transposed pattern through ``t_entry`` -- against float64 autograd."""
    graph = graph_of(name)
    pat = csr_pattern(graph, 'cpu')
    rows, cols = entries(graph)
    g = torch.Generator().manual_seed(5)
    U, V = torch.tanh(torch.randn(graph.n, 8, generator=g)).double(), torch.tanh(torch.randn(graph.n, 8, generator=g)).double()
    Rc = torch.randn(graph.nnz, generator=g).double()
    u, v = U.clone().requires_grad_(), V.clone().requires_grad_()
    score, Ps = restatement(u, v, rows, cols)
    (Ps * Rc).sum().backward()
    k = MgpCsrTwin()
    s = k.mgp_csr_score(U, V, pat['rowptr'], pat['colidx'])
    p = k.mgp_csr_softmax_fwd(s, pat['rowptr'])
    ds = k.mgp_csr_softmax_bwd(s, p, Rc, pat['rowptr'])
    dU, dV = k.mgp_csr_score_bwd(U, V, ds, pat['rowptr'], pat['colidx'], pat['t_rowptr'], pat['t_colidx'], pat['t_entry'])
    for what, a, b in (('score', s, score), ('Ps', p, Ps), ('dU', dU, u.grad), ('dV', dV, v.grad)):
        assert rel_err(a, b) < 1e-12, what


def test_header_table_and_exports_agree():
    header = open(os.path.join(REPO, 'include', 'stc_hip.h')).read()
    assert re.findall(r'^#define\s+STC_MGP_CSR_MAX_KH\s+(\d+)\b', header, flags=re.M) == [str(_lib.MGP_CSR_MAX_KH)]
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ENTRIES:
        assert re.search(rf'\b{name}\s*\(', code), f'{name} is not declared in include/stc_hip.h'
        assert name in _lib._ABI and name in _lib.EXPORTS
    lib = _lib.load_library()
    assert lib.stc_version() == _lib.ABI_VERSION >= 41
    assert not hasattr(EmulatedKernels, 'mgp_csr_score') and all(hasattr(_lib.HipKernels, m) for m in
                                                                 ('mgp_csr_supported', 'mgp_csr_score', 'mgp_csr_softmax_fwd', 'mgp_csr_softmax_bwd', 'mgp_csr_score_bwd'))
    nonfinite = header[header.index('---- Non-finite values'):]
    nonfinite = nonfinite[:nonfinite.index('*/')]
    assert 'stc_mgp_csr_score_f32' in nonfinite and 'test_non_finite_values_are_handed_on' in nonfinite and 'tests/test_mgp_csr.py' in nonfinite
    assert 'stc_mgp_csr.hip' in open(os.path.join(REPO, 'stc-gnn_amd', 'csrc', 'Makefile')).read()


@pytest.mark.parametrize('R,KH,nnz,ok', [(1, 4, 0, 1), (50176, 2304, 400000, 1), (80, 4096, 7, 1), (0, 4, 3, 0), (5, 0, 3, 0), (5, 15, 3, 0), (5, 6, 3, 0),
                                         (5, 4100, 3, 0), (-1, 4, 3, 0), (5, 4, -1, 0), (1 << 20, 2048, 3, 0)])
def test_the_predicate(R, KH, nnz, ok):
    assert _lib.load_library().stc_mgp_csr_supported(R, KH, nnz) == ok


_PTR = dict(U=0x10000, V=0x20000, rowptr=0x30000, colidx=0x40000, score=0x50000, Ps=0x60000, dPs=0x70000, ds=0x80000, t_rowptr=0x90000,
            t_colidx=0xA0000, t_entry=0xB0000, dU=0xC0000, dV=0xD0000)
_ARGS = {'stc_mgp_csr_score_f32': ('U', 'V', 'rowptr', 'colidx', 'score'), 'stc_mgp_csr_softmax_fwd_f32': ('score', 'rowptr', 'Ps'),
         'stc_mgp_csr_softmax_bwd_f32': ('score', 'Ps', 'dPs', 'rowptr', 'ds'),
         'stc_mgp_csr_score_bwd_f32': ('U', 'V', 'ds', 'rowptr', 'colidx', 't_rowptr', 't_colidx', 't_entry', 'dU', 'dV')}
_ROWS = ('stc_mgp_csr_score_f32', 'stc_mgp_csr_score_bwd_f32')          # the entry points that read U, V rows (and take KH)


def _call(lib, fn, R=10, KH=8, nnz=30, **over):
    table = dict(_PTR, **over)
    sizes = (R, KH, nnz) if fn in _ROWS else (R, nnz)
    return getattr(lib, fn)(*[table[k] for k in _ARGS[fn]], *sizes, None)


def test_refusals_come_before_any_hip_call():
    """Made-up addresses throughout: a call that got as far as a launch would fault, a refusal never touches them."""
    lib = _lib.load_library()
    err = lambda: lib.stc_last_error()
    EINVAL, EALIGN, ELIMIT, EUNSUPPORTED = -1, -2, _lib.STC_ELIMIT, -4
    for fn, names in _ARGS.items():
        assert len(names) + (3 if fn in _ROWS else 2) + 1 == len(_lib._ABI[fn][1]), fn
        assert _call(lib, fn, R=-1) == EINVAL and b'negative' in err(), fn
        assert _call(lib, fn, nnz=-1) == EINVAL and b'negative' in err(), fn
        assert _call(lib, fn, R=0) == 0, fn                                      # zero sizes launch nothing
        for name in names:
            assert _call(lib, fn, **{name: None}) == EINVAL and b'null' in err(), (fn, name)
            wide = name in ('U', 'V', 'dU', 'dV')
            assert _call(lib, fn, **{name: _PTR[name] + (4 if wide else 2)}) == EALIGN and (b'16-byte' if wide else b'4-byte') in err(), (fn, name)
    for fn in _ROWS:
        assert _call(lib, fn, KH=-4) == EINVAL and b'negative' in err()
        for KH in (0, 6, 15, _lib.MGP_CSR_MAX_KH + 4):
            assert _call(lib, fn, KH=KH) == EUNSUPPORTED and b'multiple of 4' in err(), (fn, KH)
        assert _call(lib, fn, R=1 << 20, KH=2048) == ELIMIT and b'2^31' in err()
    assert _call(lib, 'stc_mgp_csr_score_f32', nnz=0) == 0 and _call(lib, 'stc_mgp_csr_softmax_fwd_f32', nnz=0) == 0
    assert _call(lib, 'stc_mgp_csr_softmax_bwd_f32', nnz=0) == 0
    assert _call(lib, 'stc_mgp_csr_score_f32', score=_PTR['U']) == EINVAL and b'alias' in err()
    assert _call(lib, 'stc_mgp_csr_softmax_fwd_f32', Ps=_PTR['score']) == EINVAL and b'alias' in err()
    for name in ('score', 'Ps', 'dPs'):
        assert _call(lib, 'stc_mgp_csr_softmax_bwd_f32', ds=_PTR[name]) == EINVAL and b'alias' in err(), name
    for out, other in (('dU', 'U'), ('dU', 'V'), ('dV', 'U'), ('dV', 'dU'), ('dU', 'ds')):
        assert _call(lib, 'stc_mgp_csr_score_bwd_f32', **{out: _PTR[other]}) == EINVAL and b'alias' in err(), (out, other)


def test_the_hub_patterns_hold_what_they_promise():
    for R in (80, 83):
        g = hub_graph(R)
        deg = np.diff(g._host['bwd_rowptr'])
        rows, cols = entries(g)
        pairs = set(zip(rows.tolist(), cols.tolist()))
        assert deg[5] == R - 1 > 64 and deg[7] == 1 and (deg == 0).sum() > 5 and {(10, 11), (11, 10), (12, 12)} <= pairs
    assert 80 % 4 == 0 and 83 % 4 != 0                                             # four rows per workgroup (csrc/stc_mgp_csr.hip MC_WAVES)
    g, _ = graph_cases.case('one_way')
    rows, cols = entries(g)
    pairs = set(zip(rows.tolist(), cols.tolist()))
    assert not any((j, i) in pairs for i, j in pairs if i != j)
    assert (np.diff(graph_cases.case('ragged')[0]._host['bwd_rowptr']) == 0).any()


@pytest.mark.parametrize('name', PATTERNS)
def test_the_pattern_arrays(name):
    """``csr_pattern``: entry f of CSR(Gs^T) is entry t_entry[f] of Gs, and ``learned_csr_operand`` gathers the values into that order."""
    graph = graph_of(name)
    pat = csr_pattern(graph, 'cpu')
    rows, cols = entries(graph)
    assert torch.equal(pat['rows'], rows) and torch.equal(pat['cols'], cols) and pat['n'] == graph.n and pat['nnz'] == graph.nnz
    t_rows = torch.from_numpy(np.repeat(np.arange(graph.n), np.diff(graph._host['fwd_rowptr'])))
    e = pat['t_entry'].long()
    assert torch.equal(rows[e], pat['t_colidx'].long()) and torch.equal(cols[e], t_rows) and torch.equal(torch.sort(e).values, torch.arange(graph.nnz))
    vals = torch.from_numpy(graph._host['bwd_val']).clone().requires_grad_()
    op = learned_csr_operand(graph, vals)
    assert torch.equal(op.fwd_val.detach(), torch.from_numpy(graph._host['fwd_val'])) and op.fwd_val.requires_grad and not op.bwd_val.requires_grad
    assert op.fwd_plan is None and op.bwd_plan is None and op.fwd_ring2 is None and op.bwd_ring2 is None and op.source is None
    assert op.row_sum_bound == max(graph.row_sum_bound, 1.0) and op.nnz == graph.nnz
    (op.fwd_val * torch.arange(graph.nnz)).sum().backward()
    assert torch.equal(vals.grad[e], torch.arange(graph.nnz, dtype=torch.float32))
    with pytest.raises(ValueError, match='values'):
        learned_csr_operand(graph, vals.detach()[:-1])


@pytest.mark.parametrize('name', PATTERNS)
def test_the_torch_route_against_the_dense_masked_restatement(name, monkeypatch):
    monkeypatch.setattr(ops, '_kernels', None)
    graph = graph_of(name)
    rows, cols = entries(graph)
    pat = csr_pattern(graph, 'cpu')
    g = torch.Generator().manual_seed(3)
    U, V = torch.tanh(torch.randn(graph.n, 3, 5, generator=g)).double(), torch.tanh(torch.randn(graph.n, 3, 5, generator=g)).double()
    Rc = torch.randn(graph.nnz, generator=g).double()
    got, want = [], []
    for fn, store in ((lambda u, v: (lambda s: (s, learned.mgp_csr_softmax(s, pat)))(learned.mgp_csr_score(u, v, pat)), got),
                      (lambda u, v: restatement(u, v, rows, cols), want)):
        u, v = U.clone().requires_grad_(), V.clone().requires_grad_()
        score, Ps = fn(u, v)
        (Ps * Rc).sum().backward()
        store += [score.detach(), Ps.detach(), u.grad, v.grad]
    for what, a, b in zip(('score', 'Ps', 'dU', 'dV'), got, want):
        assert rel_err(a, b) < 1e-12, what
    sums = torch.zeros(graph.n, dtype=torch.float64).index_add(0, rows, got[1])
    deg = torch.from_numpy(np.diff(graph._host['bwd_rowptr']))
    assert torch.allclose(sums[deg > 0], torch.ones(int((deg > 0).sum()), dtype=torch.float64)) and not sums[deg == 0].any()
    assert ops._kernels is None                                                   # CPU tensors never bring the kernel set up


def _full_pattern_pair(n=7, C=3, h=4, r=3, seed=0):
    torch.manual_seed(seed)
    full = CsrGraph.from_dense(torch.rand(n, n) + 0.1)
    dense = M.MGP_Gen(n, C, h, fusion_rank=r)
    gen = M.MGP_Gen_Csr(full, C, h, fusion_rank=r)
    return full, dense, gen


def test_on_the_full_pattern_the_generator_is_mgp_gen_with_a_fusion_rank():
    full, dense, gen = _full_pattern_pair()
    assert [k for k, _ in gen.named_parameters()] == [k for k, _ in dense.named_parameters()]
    assert {k: tuple(v.shape) for k, v in gen.state_dict().items()} == {k: tuple(v.shape) for k, v in dense.state_dict().items()}
    assert gen.load_state_dict(dense.state_dict()).missing_keys == []
    gen, dense = gen.double(), dense.double()                                    # float64: the two routes differ by rounding alone
    X, Ac = torch.rand(2, 3, 7, 3).double(), torch.softmax(torch.randn(3, 3), -1).double()
    Gs, Gc = dense(X, full.to_dense().double(), Ac)
    op, Gc2 = gen(X, full, Ac)
    assert torch.equal(Gc, Gc2)
    assert rel_err(op.bwd_val.view(7, 7), Gs) < 1e-12 and rel_err(op.fwd_val.view(7, 7), Gs.t()) < 1e-12
    w = torch.arange(49.).view(7, 7).double()
    (Gs * w).sum().backward()
    (op.fwd_val.view(7, 7).t() * w).sum().backward()
    for (k, p), (_, q) in zip(gen.named_parameters(), dense.named_parameters()):
        if 'S' in k.split('.')[0]:
            assert rel_err(p.grad, q.grad) < 1e-11, k
    assert isinstance(gen.aggreg_S.lin_A, M.FactorisedLinear) and gen.aggreg_S.lin_A.dim == full.nnz == 49


def test_the_generator_against_the_float64_restatement_on_a_sparse_pattern():
    graph = graph_of('hub80')
    torch.manual_seed(1)
    gen = M.MGP_Gen_Csr(graph, 3, 4, fusion_rank=2).double()
    sd = {'mix_graph_pair.' + k: v for k, v in gen.state_dict().items()}
    X, Ac = torch.rand(2, 3, 80, 3).double(), torch.softmax(torch.randn(3, 3), -1).double()
    rows, cols = entries(graph)
    op, Gc = gen(X, graph, Ac)
    _, G, Gc_want = generator_restatement(X, torch.from_numpy(graph._host['bwd_val']).double(), rows, cols, Ac, sd)
    assert rel_err(op.bwd_val, G) < 1e-12 and rel_err(Gc, Gc_want) < 1e-12
    assert gen.aggreg_S.lin_A.rank == 2 and M.MGP_Gen_Csr(graph, 3, 4).aggreg_S.lin_A.rank == 16          # the rank is mandatory: 16 by default


def test_the_model_constructs_in_the_mode():
    graph = graph_of('hub80')
    with pytest.raises(ValueError, match='spatial_graph'):
        M.STCGNN(80, 3, 2, 2, 1, 4, 1, 2, graph_mode='csr-learned', fusion_rank=3)
    model = M.STCGNN(80, 3, 2, 2, 1, 4, 1, 2, graph_mode='csr-learned', fusion_rank=3, spatial_graph=graph)
    assert isinstance(model.mix_graph_pair, M.MGP_Gen_Csr) and model.mix_graph_pair.batch_sharded is False
    assert tuple(model.mix_graph_pair.aggreg_S.lin_P.U.shape) == (graph.nnz, 3)
    assert {k.split('.')[1] for k in model.state_dict() if k.startswith('mix_graph_pair.')} == {'params_S', 'aggreg_S', 'params_C', 'aggreg_C'}
    sparse = graph.to_dense().to_sparse()
    assert M.STCGNN(80, 3, 2, 2, 1, 4, 1, 2, graph_mode='csr-learned', spatial_graph=sparse).mix_graph_pair.aggreg_S.lin_A.rank == 16
    with pytest.raises(ValueError, match='nodes'):
        M.STCGNN(81, 3, 2, 2, 1, 4, 1, 2, graph_mode='csr-learned', spatial_graph=graph)
    with pytest.raises(ValueError, match='bfloat16'):
        M.STCGNN(80, 3, 2, 2, 1, 4, 1, 2, graph_mode='csr-learned', spatial_graph=graph, storage_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='pattern'):
        model.mix_graph_pair(torch.rand(1, 2, 80, 3), hub_graph(83), torch.rand(3, 3))
    # a dense-learned + fusion_rank state dict loads on the full pattern unchanged
    full = CsrGraph.from_dense(torch.rand(6, 6) + 0.1)
    a = M.STCGNN(6, 2, 2, 2, 1, 4, 1, 2, fusion_rank=2)
    b = M.STCGNN(6, 2, 2, 2, 1, 4, 1, 2, graph_mode='csr-learned', fusion_rank=2, spatial_graph=full)
    assert list(a.state_dict()) == list(b.state_dict()) and b.load_state_dict(a.state_dict()).missing_keys == []


def test_the_trainer_builds_the_mode_from_params(tmp_path, monkeypatch):
    from stc_hip import data as sdata
    from stc_hip.trainer import Trainer
    from tests.golden.make_golden import pipeline_inputs
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
    _, params = pipeline_inputs()
    params = dict(params, H=6, W=8, C=3, output_dir=str(tmp_path), _allow_cpu_for_tests=True)
    data = sdata.synthetic_incidents(6, 8, 3, 40, sparse_graph=True)
    t = Trainer(dict(params, fusion_rank=5), data, graph_mode='csr-learned')
    gen = t.model.mix_graph_pair
    assert isinstance(gen, M.MGP_Gen_Csr) and gen.graph is data['s_adj'] and t.prior_graph[0] is data['s_adj'] and gen.batch_sharded is False
    assert tuple(gen.aggreg_S.lin_A.U.shape) == (data['s_adj'].nnz, 5)
    assert Trainer(params, data, graph_mode='csr-learned').model.mix_graph_pair.aggreg_S.lin_A.rank == 16
    with pytest.raises(ValueError, match="csr-fixed"):
        Trainer(params, data, graph_mode='dense-learned')                        # unchanged: the dense mode mixes a dense prior
    dense_prior = sdata.synthetic_incidents(6, 8, 3, 40)
    t2 = Trainer(params, dense_prior, graph_mode='csr-learned')                  # a dense 0/1 prior: its non-zero entries are the pattern
    assert isinstance(t2.prior_graph[0], CsrGraph) and t2.prior_graph[0].nnz == data['s_adj'].nnz
    src = open(os.path.join(REPO, 'tools', 'train.py')).read()
    assert "'csr-learned'" in src and "in ('csr-fixed', 'csr-learned')" in src


def test_the_score_is_additive_over_the_slices_and_reduce_sees_it_once():
    graph = graph_of('ragged')
    pat = csr_pattern(graph, 'cpu')
    rows, cols = entries(graph)
    g = torch.Generator().manual_seed(11)
    X = torch.rand(4, 3, graph.n, 3, generator=g).double()
    Wu, Wv = torch.randn(3, 5, generator=g).double(), torch.randn(3, 5, generator=g).double()
    seen = []
    whole = learned.mgp_csr_front(X, Wu, Wv, pat, 3.0, reduce=lambda s: (seen.append(s.detach().clone()), s)[1])
    assert len(seen) == 1 and tuple(seen[0].shape) == (graph.nnz,)
    halves = []
    for part in (X[:1], X[1:]):
        learned.mgp_csr_front(part, Wu, Wv, pat, 3.0, reduce=lambda s: (halves.append(s.detach().clone()), s)[1])
    assert rel_err(halves[0] + halves[1], seen[0]) < 1e-12
    other = halves[1]                                                            # rank 0's all-reduce: its own share plus the other rank's
    assert rel_err(learned.mgp_csr_front(X[:1], Wu, Wv, pat, 3.0, reduce=lambda s: s + other), whole) < 1e-12
    U = torch.tanh(3.0 * X @ Wu).flatten(0, 1).transpose(0, 1)
    V = torch.tanh(3.0 * X @ Wv).flatten(0, 1).transpose(0, 1)
    assert rel_err(whole, restatement(U, V, rows, cols)[1]) < 1e-12
    with pytest.raises(ValueError, match='X requires grad'):
        learned.mgp_csr_front(X.clone().requires_grad_(), Wu, Wv, pat, 3.0)


def test_the_fusion_predicate_takes_vectors_on_a_device_only(monkeypatch):
    monkeypatch.setattr(ops, '_kernels', None)
    mod = M.MixedFusion(5, rank=3, dim=17)
    A, P = torch.rand(17), torch.rand(17)
    params = (mod.lin_A.U, mod.lin_A.V, mod.lin_A.bias, mod.lin_P.U, mod.lin_P.V, mod.lin_P.bias)
    assert not F.mixed_fusion_lr_supported(A, P, *params) and ops._kernels is None
    assert rel_err(mod(A, P), fusion_expression(A, P, *params)) < 1e-6
    with pytest.raises(ValueError, match='rank'):
        M.MixedFusion(5, dim=17)


def test_the_kernels_use_no_scratch(tmp_path):
    """The four kernels of csrc/stc_mgp_csr.hip as the compiler reports them with the library's own flags (needs hipcc, no GPU)."""
    from tests.test_first_step_isa import _resource_usage
    from tests.test_isa import HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not present')
    usage = _resource_usage('stc_mgp_csr.hip', tmp_path)
    assert len(usage) == 4, sorted(usage)
    for name, u in usage.items():
        assert u['ScratchSize'] == 0, (name, u)


# ============================================================================================================== GPU
@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.fixture
def routed(hip, monkeypatch):
    """The HIP kernel set behind ``ops.kernels()``, the switches on, and a log of the name of every C entry point launched."""
    log = []
    monkeypatch.setattr(ops, '_kernels', hip)
    monkeypatch.setattr(L, '_FUSED', True)
    monkeypatch.setattr(F, '_FUSED', True)
    inner = hip._launch
    monkeypatch.setattr(hip, '_launch', lambda name, *a, **kw: (log.append(name), inner(name, *a, **kw))[1])
    return log


def run(pat, U, V, Rc, frozen=()):
    """One forward + backward of score -> softmax on the device; (score, Ps, dU, dV)."""
    u, v = U.cuda().requires_grad_('U' not in frozen), V.cuda().requires_grad_('V' not in frozen)
    score = learned.mgp_csr_score(u, v, pat)
    Ps = learned.mgp_csr_softmax(score, pat)
    (Ps * Rc.cuda()).sum().backward()
    return score.detach(), Ps.detach(), u.grad, v.grad


@pytest.mark.gpu
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('KH', KHS)
@pytest.mark.parametrize('name', PATTERNS)
def test_parity_with_float64_autograd(routed, name, KH, scale):
    ref = reference(name, KH, scale)
    pat = csr_pattern(graph_of(name), torch.device('cuda'))
    score, Ps, dU, dV = run(pat, ref['U'], ref['V'], ref['R'])
    torch.cuda.synchronize()
    assert routed == list(LAUNCHED[:2]) + list(LAUNCHED[2:]), routed               # one launch each: score, softmax, softmax backward, score backward
    tag = f'{name} KH={KH} {scale} seed={ref["seed"]}'
    failures = []
    for what, got, bound in (('score', score, TOL), ('Ps', Ps, TOL), ('dU', dU, grad_bound(ref['noise']['dU'])), ('dV', dV, grad_bound(ref['noise']['dV']))):
        err = rel_err(got, ref[what])
        print(tag, what, f'{err:.2e} noise {ref["noise"][what]:.2e} bound {bound:.1e}')
        _log(f'{tag} {what}', err, ref['noise'][what], bound)
        if not err < bound:
            failures.append((what, err, bound))
    assert not failures, (tag, failures)


@pytest.mark.gpu
def test_exact_zeros_for_identical_rows_and_the_diagonal(routed):
    """Nodes 10 and 11 (a reciprocal pair of the hub pattern) and nodes 5 and 40 (a hub entry) are given identical rows; (12, 12) is stored:
    their scores are 0.0 bit for bit -- not a rounding residue whose sign would decide relu's mask -- and ds is 0 there."""
    graph = graph_of('hub80')
    pat = csr_pattern(graph, torch.device('cuda'))
    rows, cols = entries(graph)
    for KH in (60, 2304):
        g = torch.Generator().manual_seed(KH)
        U, V = torch.tanh(torch.randn(80, KH, generator=g)), torch.tanh(torch.randn(80, KH, generator=g))
        for a, b in ((10, 11), (5, 40)):
            U[b], V[b] = U[a], V[a]
        Rc = torch.randn(graph.nnz, generator=g)
        exact = (rows == cols) | ((rows == 10) & (cols == 11)) | ((rows == 11) & (cols == 10)) | ((rows == 5) & (cols == 40))
        assert int(exact.sum()) == 4
        u64, v64 = U.double().requires_grad_(), V.double().requires_grad_()
        s64, p64 = restatement(u64, v64, rows, cols)
        assert margin_ok(s64, rows, cols, exact)
        (p64 * Rc.double()).sum().backward()
        u, v = U.cuda().requires_grad_(), V.cuda().requires_grad_()
        score = learned.mgp_csr_score(u, v, pat)
        score.retain_grad()
        Ps = learned.mgp_csr_softmax(score, pat)
        (Ps * Rc.cuda()).sum().backward()
        assert torch.equal(score.detach().cpu()[exact].view(torch.int32), torch.zeros(4, dtype=torch.int32))
        assert not score.grad.cpu()[exact].any()
        assert rel_err(Ps, p64) < TOL and rel_err(u.grad, u64.grad) < FUSION_GRAD and rel_err(v.grad, v64.grad) < FUSION_GRAD


@pytest.mark.gpu
def test_frozen_subsets_views_saved_tensors_and_double_backward(routed):
    """The autograd contract of ``_MgpCsrScore`` and ``_MgpCsrSoftmax``."""
    ref = reference('ragged', 60, 'raw')
    pat = csr_pattern(graph_of('ragged'), torch.device('cuda'))
    full = run(pat, ref['U'], ref['V'], ref['R'])
    # frozen subsets: None, the other gradient bit for bit; nothing wanted: no launch in the backward
    for frozen, keep in ((('U',), 3), (('V',), 2)):
        got = run(pat, ref['U'], ref['V'], ref['R'], frozen)
        assert got[5 - keep] is None and torch.equal(got[keep], full[keep]), frozen
    del routed[:]
    s = learned.mgp_csr_score(ref['U'].cuda(), ref['V'].cuda(), pat)
    assert not s.requires_grad and routed == ['stc_mgp_csr_score_f32']
    # non-contiguous and offset inputs: a transposed (KH, R) buffer, and rows that start 16 floats into a larger one
    Ut = ref['U'].cuda().t().contiguous().t().requires_grad_()
    big = torch.zeros(240 * 60 + 16).cuda()
    Vo = big[16:].view(240, 60)
    Vo.copy_(ref['V'])
    Vo = Vo.detach().requires_grad_()
    assert not Ut.is_contiguous() and Vo.storage_offset() == 16
    Rv = torch.stack([ref['R'], ref['R']], 1).cuda()[:, 0]                        # a strided cotangent
    score = learned.mgp_csr_score(Ut, Vo, pat)
    Ps = learned.mgp_csr_softmax(score, pat)
    (Ps * Rv).sum().backward()
    assert torch.equal(Ps.detach(), full[1]) and torch.equal(Ut.grad, full[2]) and torch.equal(Vo.grad, full[3])
    # saved tensors are not clobbered by a second forward on other data
    u, v = ref['U'].cuda().requires_grad_(), ref['V'].cuda().requires_grad_()
    Ps = learned.mgp_csr_softmax(learned.mgp_csr_score(u, v, pat), pat)
    other = reference('ragged', 60, 'quarter')
    run(pat, other['U'], other['V'], other['R'])
    (Ps * ref['R'].cuda()).sum().backward()
    assert torch.equal(u.grad, full[2]) and torch.equal(v.grad, full[3])
    # double backward is refused
    u, v = ref['U'].cuda().requires_grad_(), ref['V'].cuda().requires_grad_()
    score = learned.mgp_csr_score(u, v, pat)
    s2 = score.detach().clone().requires_grad_()
    for out, leaf in ((score, u), (learned.mgp_csr_softmax(s2, pat), s2)):
        (d,) = torch.autograd.grad((out ** 2).sum(), leaf, create_graph=True)
        with pytest.raises(RuntimeError, match='once_differentiable'):
            (d ** 2).sum().backward()
    # the data window gets no gradient: refused by name, never a silent zero
    X = torch.rand(2, 3, 240, 3).cuda().requires_grad_()
    W = torch.randn(3, 4).cuda().requires_grad_()
    with pytest.raises(ValueError, match='X requires grad'):
        learned.mgp_csr_front(X, W, W, pat, 3.0)
    Wv = torch.randn(3, 4).cuda().requires_grad_()                               # (Wv = Wu would give U = V: every score exactly 0)
    Ps = learned.mgp_csr_front(X.detach(), W, Wv, pat, 3.0)
    Ps.square().sum().backward()
    assert bool(W.grad.abs().max() > 0) and bool(Wv.grad.abs().max() > 0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


@pytest.mark.gpu
@pytest.mark.parametrize('name,KH', [('hub83', 260), ('weights', 2304)])
def test_eager_runs_and_graph_replays_give_the_same_bits(routed, name, KH):
    first, second = reference(name, KH, 'quarter'), reference(name, KH, 'raw')
    pat = csr_pattern(graph_of(name), torch.device('cuda'))
    a, b = ([_bits(x) for x in run(pat, second['U'], second['V'], second['R'])] for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    u, v, Rg = first['U'].cuda().requires_grad_(), first['V'].cuda().requires_grad_(), first['R'].cuda()

    def step():
        u.grad = v.grad = None
        score = learned.mgp_csr_score(u, v, pat)
        Ps = learned.mgp_csr_softmax(score, pat)
        (Ps * Rg).sum().backward()
        return score, Ps

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_score, s_Ps = step()
    static = [s_score, s_Ps, u.grad, v.grad]
    with torch.no_grad():
        u.copy_(second['U'])
        v.copy_(second['V'])
        Rg.copy_(second['R'])
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for what, got, want in zip(('score', 'Ps', 'dU', 'dV'), static, a):
            assert torch.equal(_bits(got), want), what


@pytest.mark.gpu
def test_launch_counts_and_routing(routed, hip, monkeypatch):
    """One launch each for score, softmax forward, softmax backward and score backward -- through tests/launch_trace.py's wrapper as well --;
    rows the predicate refuses (KH = 15) and the switch take the torch route and are right; 1-D fusion operands equal the (n, n) call."""
    from tests.launch_trace import Traced
    ref = reference('hub80', 60, 'raw')
    pat = csr_pattern(graph_of('hub80'), torch.device('cuda'))
    traced = Traced(hip)
    monkeypatch.setattr(ops, '_kernels', traced)
    run(pat, ref['U'], ref['V'], ref['R'])
    assert [rec[0] if isinstance(rec, (list, tuple)) else rec['name'] for rec in traced._log] == ['mgp_csr_score', 'mgp_csr_softmax_fwd', 'mgp_csr_softmax_bwd', 'mgp_csr_score_bwd']
    assert routed == list(LAUNCHED[:2]) + list(LAUNCHED[2:])
    monkeypatch.setattr(ops, '_kernels', hip)
    with torch.no_grad():
        del routed[:]
        learned.mgp_csr_softmax(learned.mgp_csr_score(ref['U'].cuda(), ref['V'].cuda(), pat), pat)
        assert routed == ['stc_mgp_csr_score_f32', 'stc_mgp_csr_softmax_fwd_f32']
    rows, cols = entries(graph_of('hub80'))

    def quiet(tag, U, V, Rc):
        del routed[:]
        got = run(pat, U, V, Rc)
        assert not [n for n in routed if n in LAUNCHED[:1] + LAUNCHED[3:]], (tag, routed)
        u, v = U.double().requires_grad_(), V.double().requires_grad_()
        s64, p64 = restatement(u, v, rows, cols)
        assert margin_ok(s64, rows, cols), tag
        (p64 * Rc.double()).sum().backward()
        for what, a, b, bound in zip(('score', 'Ps', 'dU', 'dV'), got, (s64, p64, u.grad, v.grad), (TOL, TOL, FUSION_GRAD, FUSION_GRAD)):
            assert rel_err(a, b) < bound, (tag, what)

    g = torch.Generator().manual_seed(15)
    U15, V15 = torch.tanh(torch.randn(80, 15, generator=g)), torch.tanh(torch.randn(80, 15, generator=g))
    assert not hip.mgp_csr_supported(80, 15, pat['nnz']) and hip.mgp_csr_supported(80, 16, pat['nnz'])
    quiet('KH = 15', U15, V15, ref['R'])
    monkeypatch.setattr(L, '_FUSED', False)
    del routed[:]
    run(pat, ref['U'], ref['V'], ref['R'])
    assert routed == []
    monkeypatch.setattr(L, '_FUSED', True)
    monkeypatch.setattr(ops, '_kernels', EmulatedKernels())                       # a kernel set without the entry points: the CPU twin
    assert not learned.mgp_csr_supported(ref['U'].cuda(), ref['V'].cuda(), pat)
    monkeypatch.setattr(ops, '_kernels', hip)
    # fusion on vectors: the same data as an (n, n) matrix and as its n^2 values
    from tests.test_mixed_fusion_lr import NAMES, inputs
    ops_, Rf = inputs(10, 4, 'wide')
    outs = []
    for flat in (False, True):
        leaves = {k: v.cuda().requires_grad_() for k, v in ops_.items()}
        A, P = (leaves[k].reshape(-1) if flat else leaves[k] for k in ('A', 'P'))
        del routed[:]
        assert F.mixed_fusion_lr_supported(A, P, *[leaves[k] for k in NAMES[2:]])
        G = F.mixed_fusion_lr(A, P, *[leaves[k] for k in NAMES[2:]])
        (G * Rf.cuda().reshape(G.shape)).sum().backward()
        assert routed == ['stc_mixed_fusion_lr_fwd_f32', 'stc_mixed_fusion_lr_bwd_f32'] and G.dim() == (1 if flat else 2)
        outs.append([G.detach().reshape(-1)] + [leaves[k].grad.reshape(-1) for k in NAMES])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert not F.mixed_fusion_lr_supported(leaves['A'].reshape(-1), leaves['P'].reshape(-1)[:-1], *[leaves[k] for k in NAMES[2:]])


@pytest.mark.gpu
@pytest.mark.parametrize('poison', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('where', ['U', 'V', 'score'])
def test_non_finite_values_are_handed_on(routed, where, poison):
    """One poisoned element of U, of V (node 30: its own row, and the hub row 5 and the rows that point at it) or of the score (an entry of the
    hub row).  ``want`` is the float64 twin under the pattern semantics of the entry points (entries absent from the pattern take no part):
    every result is non-finite exactly where want is, equals the clean run BIT FOR BIT outside the poison's reach (what want marks or
    changes), and is right within the parity bounds where want is finite."""
    graph = graph_of('hub80')
    pat = csr_pattern(graph, torch.device('cuda'))
    cpu = csr_pattern(graph, 'cpu')
    rows, cols = entries(graph)
    ref = reference('hub80', 60, 'quarter')
    twin = MgpCsrTwin()
    index = [cpu[k] for k in ('rowptr', 'colidx', 't_rowptr', 't_colidx', 't_entry')]

    def want_of(U, V, score=None):
        s = twin.mgp_csr_score(U.double(), V.double(), index[0], index[1]) if score is None else score.double().cpu()
        Ps = twin.mgp_csr_softmax_fwd(s, index[0])
        ds = twin.mgp_csr_softmax_bwd(s, Ps, ref['R'].double(), index[0])
        return (s, Ps, ds) + twin.mgp_csr_score_bwd(U.double(), V.double(), ds, *index)

    def got_of(U, V, score=None):
        u, v = U.cuda().requires_grad_(), V.cuda().requires_grad_()
        s = learned.mgp_csr_score(u, v, pat) if score is None else score.clone().requires_grad_()
        s.retain_grad()
        Ps = learned.mgp_csr_softmax(s, pat)
        (Ps * ref['R'].cuda()).sum().backward()
        return (s.detach(), Ps.detach(), s.grad) + ((u.grad, v.grad) if score is None else ())

    clean_got, clean_want = got_of(ref['U'], ref['V']), want_of(ref['U'], ref['V'])
    U, V = ref['U'].clone(), ref['V'].clone()
    if where == 'score':
        e = int(((rows == 5) & (cols == 30)).nonzero()[0])
        s = clean_got[0].clone()
        s[e] = poison
        got, want, base_want = got_of(U, V, s), want_of(U, V, s)[:3], want_of(U, V, clean_got[0])[:3]
        assert not torch.isfinite(want[1][rows == 5]).any() and torch.isfinite(want[1][rows != 5]).all()      # the hub row, and nothing else
    else:
        (U if where == 'U' else V)[30, 7] = poison
        got, want, base_want = got_of(U, V), want_of(U, V), clean_want
        assert torch.equal(~torch.isfinite(want[0]), (rows == 30) | (cols == 30))                              # the entries of row 30 and column 30 only
    torch.cuda.synchronize()
    names = ('score', 'Ps', 'ds', 'dU', 'dV')
    bounds = dict(score=TOL, Ps=TOL, ds=grad_bound(ref['noise']['dU']), dU=grad_bound(ref['noise']['dU']), dV=grad_bound(ref['noise']['dV']))
    for what, g_, w, w0, base in zip(names, got, want, base_want, clean_got):
        g_, base = g_.cpu(), base.cpu()
        fin = torch.isfinite(w)
        reach = ~fin | (w != w0)
        assert bool(reach.any()) or what in ('dU', 'dV'), what
        assert not torch.isfinite(g_[~fin]).any(), what                          # A: non-finite wherever want is
        assert torch.isfinite(g_[fin]).all(), what
        assert torch.equal(g_[~reach].view(torch.int32), base[~reach].view(torch.int32)), what      # B: the clean run's bits outside the reach
        if bool(fin.any()):
            assert rel_err(g_[fin], w[fin]) < bounds[what], what                 # C: the finite part is still right


# ---- the module ------------------------------------------------------------------------------------------------------------------------------
def _model_case(graph, C, K, hidden, seed, layers=2, T=3, horizon=2, B=2, rank=3):
    torch.manual_seed(seed)
    model = M.STCGNN(graph.n, C, K, K, 1, hidden, layers, horizon, graph_mode='csr-learned', fusion_rank=rank, spatial_graph=graph)
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(B, T, graph.n, C, generator=g)                                # dense-valued: every node's row is distinct
    Ac = torch.softmax(torch.randn(C, C, generator=g), -1)
    Rw = torch.randn(B, horizon, graph.n, C, generator=g)
    return model, X, Ac, Rw


def _restated(model, graph, X, Ac, Rw, K, hidden, layers=2, horizon=2):
    """Prediction and parameter gradients of the restatement in float64, and the fp32 run's distance from them (the noise)."""
    out = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in model.state_dict().items()}
        y, score = model_restatement(X.to(dt), graph, Ac.to(dt), sd, K, hidden, layers, horizon)
        (y * Rw.to(dt)).sum().backward()
        out[dt] = (y.detach(), {k: v.grad for k, v in sd.items()}, score.detach())
    rows, cols = entries(graph)
    assert margin_ok(out[torch.float64][2], rows, cols), 'a score of the window sits on the edge of relu'
    y64, g64, _ = out[torch.float64]
    y32, g32, _ = out[torch.float32]
    return y64, g64, {k: rel_err(g32[k], g64[k]) for k in g64}, rel_err(y32, y64)


def _check_model(tag, y, grads, y64, g64, noise):
    failures = []
    err = rel_err(y, y64)
    _log(f'{tag} yhat', err, 0.0, max(FWD, GPU))
    if not err < max(FWD, GPU):
        failures.append(('yhat', err, max(FWD, GPU)))
    for k, want in g64.items():
        err, bound = rel_err(grads[k], want), grad_bound(noise[k])
        _log(f'{tag} d{k}', err, noise[k], bound)
        print(tag, k, f'{err:.2e} noise {noise[k]:.2e}')
        if not err < bound:
            failures.append((k, err, bound))
    assert not failures, (tag, failures)


@pytest.mark.gpu
@pytest.mark.parametrize('K,hidden', [(2, 16), (3, 16), (2, 4), (3, 4)])
def test_the_model_against_the_float64_restatement(routed, K, hidden):
    graph = graph_cases.case('ragged')[0]
    model, X, Ac, Rw = _model_case(graph, 3, K, hidden, seed=10 * K + hidden)
    y64, g64, noise, _ = _restated(model, graph, X, Ac, Rw, K, hidden)
    model = model.cuda()
    y = model(X_seq=X.cuda(), As=graph, Ac=Ac.cuda())
    (y * Rw.cuda()).sum().backward()
    torch.cuda.synchronize()
    for name in LAUNCHED:
        assert routed.count(name) == 1, (name, routed.count(name))
    assert 'stc_csr_sddmm_f32' in routed and routed.count('stc_mixed_fusion_lr_fwd_f32') == 1          # the general per-cell path forms the value gradient
    _check_model(f'csr-learned ragged K={K} h={hidden}', y, {k: p.grad for k, p in model.named_parameters()}, y64, g64, noise)
    with torch.no_grad():
        assert rel_err(model(X_seq=X.cuda(), As=graph, Ac=Ac.cuda()), y) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize('hidden', [16, 4])
def test_on_the_full_pattern_both_learned_modes_agree(routed, hidden):
    torch.manual_seed(hidden)
    N, C, K = 12, 3, 2
    full = CsrGraph.from_dense(torch.rand(N, N) + 0.1)
    dense = M.STCGNN(N, C, K, K, 1, hidden, 2, 2, fusion_rank=3)
    model, X, Ac, Rw = _model_case(full, C, K, hidden, seed=hidden)
    assert model.load_state_dict(dense.state_dict()).missing_keys == []
    y64, g64, noise, _ = _restated(model, full, X, Ac, Rw, K, hidden)
    results = []
    for tag, m, As in (('csr-learned full', model.cuda(), full), ('dense-learned rank', dense.cuda(), full.to_dense().cuda())):
        y = m(X_seq=X.cuda(), As=As, Ac=Ac.cuda())
        (y * Rw.cuda()).sum().backward()
        grads = {k: p.grad for k, p in m.named_parameters()}
        _check_model(f'{tag} h={hidden}', y, grads, y64, g64, noise)
        results.append((y.detach(), grads))
    assert rel_err(results[0][0], results[1][0]) < max(FWD, GPU)
    for k, g_ in results[0][1].items():
        assert rel_err(g_, results[1][1][k]) < grad_bound(noise[k]), k


@pytest.mark.gpu
def test_one_trainer_epoch_eager_and_replayed(tmp_path, monkeypatch):
    from stc_hip import data as sdata
    from stc_hip.trainer import Trainer
    monkeypatch.setattr(ops, '_kernels', None)
    data = sdata.synthetic_incidents(6, 8, 3, 40, sparse_graph=True)
    params = dict(device='cuda:0', H=6, W=8, C=3, batch_size=4, obs_len=3, pred_len=2, split_ratio=[6, 1, 1], model='STC-GNN', cheby_order=2,
                  hidden_dim=16, nn_layers=1, learn_rate=2e-3, decay_rate=1e-4, num_epochs=2, time_slice=4, city='SYN', fusion_rank=4)
    flat, hist = {}, {}
    for graphed in (False, True):
        out = tmp_path / str(graphed)
        os.makedirs(out)
        loaders = sdata.get_data_loader(params, data, params['obs_len'], params['pred_len'], params['split_ratio'])
        torch.manual_seed(123)
        trainer = Trainer(dict(params, output_dir=str(out)), data, graph_mode='csr-learned', hip_graph=graphed)
        hist[graphed] = trainer.train(loaders, verbose=False)['loss']
        flat[graphed] = {k: p.detach().clone() for k, p in trainer.model.named_parameters()}
        if graphed:
            assert any(slot[1] is not None for slot in trainer._captured.values()), 'no step was captured'
    assert hist[False]['train'][1] < hist[False]['train'][0], hist                # the loss falls
    differ = {k: float((flat[True][k] - v).abs().max()) for k, v in flat[False].items() if not torch.equal(flat[True][k].view(torch.int32), v.view(torch.int32))}
    print('parameters that differ between eager and replayed training:', differ)
    assert not differ, differ
