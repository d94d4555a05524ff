"""``stc_graph_grad_csr_f32`` (csrc/stc_graph_grad_csr.hip, ABI v42; ``HipKernels.graph_grad_csr``): the graph product of stc_graph_grad_f32 sampled
at the stored entries of a CSR pattern -- the value gradient of a learned graph on a sparse pattern.

    partials[chunk][e] = sum_{planes g of the chunk} sum_f A[g][i(e)][f] * B[g][colidx[e]][f]          e: the entries of row i(e)

CPU part: header, ctypes table and EXPORTS agree; every refusal comes back before any HIP call (made-up addresses); the float64 twin written
here equals the dense einsum masked to the pattern; the chunk rule is a pure function; the kernels use no scratch.

GPU part (-m gpu): the patterns ``ragged`` (12 x 20), ``one_way`` (12 x 20: 8 empty rows in the forward orientation) and ``weights`` (9 x 33) of
tests/graph_cases.py as the executor passes them (CSR of Gs^T), and ``hub_graph`` of tests/test_mgp_csr.py as the CSR of Gs itself (row 5: N - 1
= 79 entries, more than a wave and no multiple of the kernel's tile; empty rows; a single-entry row), at (C, width, batch) in {(3, 20, 2), (5, 20, 3),
(8, 32, 2), (16, 32, 3)} (F = 60, 100: a partial wave of 16-byte pieces; 256: one piece on every lane; 512: two), 6 cells of which 1, 3, 5 are
selected, as tests/test_graph_grad_blocked.py does.  Bound: that file's ``EINSUM_BOUND`` = 1e-6, the project's bound for the dense product of the
same arithmetic (an all-fp32 torch evaluation of these inputs sits at 0.7 - 1.6e-7 from float64)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib
from tests import graph_cases
from tests.conftest import REPO, rel_err
from tests.test_graph_grad_blocked import CELLS, EINSUM_BOUND, SEL, SENTINEL
from tests.test_mgp_csr import hub_graph

ENTRY = 'stc_graph_grad_csr_f32'
PATTERNS = ('ragged', 'one_way', 'weights', 'hub')
SHAPES = [(3, 20, 2), (5, 20, 3), (8, 32, 2), (16, 32, 3)]           # (C, row width, batch): planes = 3 * batch


def pattern(name):
    """(N, rowptr, colidx) as int32 CPU tensors: the grid cases in the forward orientation (CSR of Gs^T), the hub pattern as the CSR of Gs."""
    if name == 'hub':
        g, side = hub_graph(80), 'bwd'
    else:
        g, side = graph_cases.case(name, *{'weights': (9, 33)}.get(name, (12, 20)))[0], 'fwd'
    return g.n, torch.from_numpy(g._host[f'{side}_rowptr']), torch.from_numpy(g._host[f'{side}_colidx'])


def rows_of(rowptr):
    rp = rowptr.long()
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])


def sampled_twin(rowptr, colidx, A, Bm, cell0, cell_step, n_sel, N):
    """(nnz,) float64: < A_g[i(e)], B_g[colidx[e]] > summed over the selected cells and samples, rows read as (N, C * width)."""
    cells = [cell0 + s * cell_step for s in range(n_sel)]
    a = A[cells].double().reshape(-1, N, A.shape[2] // N * A.shape[3])
    b = Bm[cells].double().reshape(a.shape)
    return (a[:, rows_of(rowptr)] * b[:, colidx.long()]).sum((0, 2))


def operands(N, C, w, B):
    g = torch.Generator().manual_seed(1000 * N + 10 * C + w + B)
    return tuple(torch.randn(CELLS, B, N * C, w, generator=g) for _ in range(2))


# ============================================================================================================== CPU
def test_header_table_and_exports_agree():
    header = open(os.path.join(REPO, 'include', 'stc_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(rf'\b{ENTRY}\s*\(', code) and ENTRY in _lib._ABI and ENTRY in _lib.EXPORTS
    proto = re.search(rf'{ENTRY}\s*\((.*?)\)\s*;', code, flags=re.S).group(1)
    assert len(proto.split(',')) == len(_lib._ABI[ENTRY][1]) == 15
    assert re.findall(r'^#define\s+STC_ABI_VERSION\s+(\d+)\b', header, flags=re.M) == [str(_lib.ABI_VERSION)]
    assert _lib.load_library().stc_version() == _lib.ABI_VERSION >= 42
    assert hasattr(_lib.HipKernels, 'graph_grad_csr') and hasattr(_lib.HipKernels, 'graph_grad_csr_chunks')
    assert not hasattr(EmulatedKernels, 'graph_grad_csr')                          # the CPU twin does not get it
    assert 'stc_graph_grad_csr.hip' in open(os.path.join(REPO, 'stc-gnn_amd', 'csrc', 'Makefile')).read()


_PTR = dict(rowptr=0x10000, colidx=0x20000, A=0x30000, B=0x40000, partials=0x50000)


def _call(lib, n_rows=10, nnz=30, n_chunks=4, cell0=0, cell_step=1, n_sel=2, batch=2, F=60, chunk_stride=0, **over):
    p = dict(_PTR, **over)
    return lib.stc_graph_grad_csr_f32(p['rowptr'], p['colidx'], n_rows, nnz, p['A'], p['B'], p['partials'], n_chunks, cell0, cell_step, n_sel, batch, F,
                                      chunk_stride, None)


def test_refusals_come_before_any_hip_call():
    """Made-up addresses throughout: a call that got as far as a launch would fault, a refusal never touches them."""
    lib = _lib.load_library()
    err = lambda: lib.stc_last_error()
    EINVAL, EALIGN = -1, -2
    for name in _PTR:
        assert _call(lib, **{name: None}) == EINVAL and b'null' in err(), name
    for name, off in (('A', 4), ('B', 8), ('partials', 4), ('rowptr', 2), ('colidx', 2)):
        assert _call(lib, **{name: _PTR[name] + off}) == EALIGN and b'unaligned' in err(), name
    for F in (0, 2, 6, 63, 516, 1024):
        assert _call(lib, F=F) == EINVAL and b'multiple of 4' in err(), F
    for size in ('n_rows', 'nnz', 'F'):
        assert _call(lib, **{size: -1}) == EINVAL and b'negative' in err(), size
    for sel in (dict(cell0=-1), dict(cell_step=0), dict(n_sel=-1), dict(batch=0), dict(n_chunks=0), dict(n_chunks=65536)):
        assert _call(lib, **sel) == EINVAL and b'cell0=' in err(), sel
    assert _call(lib, chunk_stride=29) == EINVAL and b'chunk stride' in err()
    assert _call(lib, chunk_stride=-1) == EINVAL and b'chunk stride' in err()
    assert _call(lib, nnz=0) == 0 and _call(lib, n_sel=0) == 0                      # launch nothing


@pytest.mark.parametrize('name', PATTERNS)
def test_the_float64_twin_equals_the_dense_einsum_masked_to_the_pattern(name):
    N, rowptr, colidx = pattern(name)
    A, Bm = operands(N, 3, 20, 2)
    dense = EmulatedKernels().graph_grad(A, Bm, *SEL, N)                          # (N, N) float64
    got = sampled_twin(rowptr, colidx, A, Bm, *SEL, N)
    rows, cols = rows_of(rowptr), colidx.long()
    assert got.dtype == torch.float64 and got.shape == (colidx.numel(),) and rel_err(got, dense[rows, cols]) < 1e-13
    mask = torch.zeros(N, N, dtype=torch.bool)
    mask[rows, cols] = True
    assert int(mask.sum()) == colidx.numel()                                       # no duplicate entries: the scatter is the masked matrix
    assert torch.equal(torch.zeros(N, N, dtype=torch.float64).index_put((rows, cols), got) != 0, mask & (dense != 0))


def test_the_patterns_hold_what_they_promise():
    deg = {name: np.diff(pattern(name)[1].numpy()) for name in PATTERNS}
    assert deg['hub'].max() == 79 and (deg['hub'] == 0).sum() > 5 and (deg['hub'] == 1).any()
    assert (deg['one_way'] == 0).sum() == 8 and len(set(deg['ragged'].tolist())) > 4 and deg['weights'].min() >= 3
    assert [pattern(n)[0] for n in PATTERNS] == [240, 240, 297, 80]


def test_the_chunk_rule_is_a_pure_function_of_its_arguments():
    rule = _lib.HipKernels.graph_grad_csr_chunks
    assert rule(6, 240, 1500) == rule(6, 240, 1500, 'cuda:0') == rule(6, 240, 1500, None) == 6          # never more chunks than planes
    assert rule(160, 1024, 7812) == 4 and rule(20, 8100, 63368) == 1 and rule(20, 4096, 32000) == 1     # enough waves: 4096 / N
    assert rule(400, 36, 200) == 64                                                                     # capped
    assert rule(400, 10, 1 << 20) == 4 and rule(0, 10, 5) == 1 and rule(5, 10, 0) == 5                   # the partial block stays small; at least one


def test_the_kernels_use_no_scratch(tmp_path):
    from tests.test_first_step_isa import _resource_usage
    from tests.test_isa import HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not present')
    usage = _resource_usage('stc_graph_grad_csr.hip', tmp_path)
    assert len(usage) == 2, sorted(usage)                                          # one and two 16-byte pieces per lane
    for name, u in usage.items():
        assert u['ScratchSize'] == 0 and u['VGPRs'] <= 128, (name, u)


# ============================================================================================================== GPU
@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


_CASES = [(name, *shape) for name in PATTERNS for shape in SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize('name,C,w,B', _CASES)
def test_parity_with_the_float64_sampled_product_and_the_dense_kernel(hip, name, C, w, B):
    N, rowptr, colidx = pattern(name)
    A, Bm = operands(N, C, w, B)
    want = sampled_twin(rowptr, colidx, A, Bm, *SEL, N)
    Ad, Bd, rp, ci = A.cuda(), Bm.cuda(), rowptr.cuda(), colidx.cuda()
    got = hip.graph_grad_csr(rp, ci, Ad, Bd, *SEL, N)
    dense = hip.graph_grad(Ad, Bd, *SEL, N)[rows_of(rowptr).cuda(), ci.long()]
    err, err_dense = rel_err(got, want), rel_err(got, dense)
    print(f'graph_grad_csr {name} F={C * w} B={B}: {err:.3e} from float64, {err_dense:.3e} from the dense kernel (bound {EINSUM_BOUND:.1e})')
    assert got.dtype == torch.float64 and got.shape == (colidx.numel(),)
    assert err < EINSUM_BOUND and err_dense < EINSUM_BOUND


def _partials(hip, rp, ci, A, Bm, N, chunks, offset=3, tail=5):
    """The whole (chunks, offset + nnz + tail) buffer after one launch into its block at ``offset``."""
    part = torch.full((chunks, offset + ci.numel() + tail), SENTINEL, dtype=torch.float64, device=A.device)
    assert hip.graph_grad_csr(rp, ci, A, Bm, *SEL, N, into=(part, offset)) is None
    return part


@pytest.mark.gpu
@pytest.mark.parametrize('name,C,w,B,chunks', [('hub', 3, 20, 2, 11), ('ragged', 5, 20, 3, 4), ('one_way', 8, 32, 2, 4), ('weights', 16, 32, 3, 11)])
def test_the_partial_buffer(hip, name, C, w, B, chunks):
    """A sentinel before and after the block survives in every chunk; every element of every chunk is written; with more chunks than planes the
    surplus chunks hold zeros; the chunks add up to the product; two launches, and an eager launch and a graph replay, give equal bits."""
    N, rowptr, colidx = pattern(name)
    A, Bm = (t.cuda() for t in operands(N, C, w, B))
    rp, ci, nnz = rowptr.cuda(), colidx.cuda(), colidx.numel()
    part = _partials(hip, rp, ci, A, Bm, N, chunks)
    torch.cuda.synchronize()
    first = part.cpu()
    assert torch.equal(first[:, :3], torch.full((chunks, 3), SENTINEL, dtype=torch.float64))
    assert torch.equal(first[:, -5:], torch.full((chunks, 5), SENTINEL, dtype=torch.float64))
    block = first[:, 3:3 + nnz]
    assert bool((block != SENTINEL).all())
    planes = SEL[2] * B
    if chunks > planes:
        assert float(block[planes:].abs().max()) == 0.0 and bool((block[:planes] != 0).any(1).all())
    assert rel_err(block.sum(0), sampled_twin(rowptr, colidx, A.cpu(), Bm.cpu(), *SEL, N)) < EINSUM_BOUND
    assert torch.equal(_partials(hip, rp, ci, A, Bm, N, chunks).cpu(), first)
    static = torch.full_like(part, SENTINEL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.graph_grad_csr(rp, ci, A, Bm, *SEL, N, into=(static, 3))
    torch.cuda.current_stream().wait_stream(side)
    static.fill_(SENTINEL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.graph_grad_csr(rp, ci, A, Bm, *SEL, N, into=(static, 3))
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static.cpu(), first)


@pytest.mark.gpu
@pytest.mark.parametrize('name,C,w,B', [('hub', 5, 20, 3), ('ragged', 16, 32, 3)])
def test_a_nan_reaches_its_row_or_column_only(hip, name, C, w, B):
    """A NaN in row i of A reaches exactly the entries of row i, a NaN in row j of B exactly the entries with column j; a NaN in a cell that is
    not selected reaches nothing.  Every other entry keeps the bits of the clean run."""
    N, rowptr, colidx = pattern(name)
    A, Bm = (t.cuda() for t in operands(N, C, w, B))
    rp, ci = rowptr.cuda(), colidx.cuda()
    rows, cols = rows_of(rowptr), colidx.long()
    clean = hip.graph_grad_csr(rp, ci, A, Bm, *SEL, N).cpu()
    deg = np.diff(rowptr.numpy())
    i = int(deg.argmax())                                            # the longest row (the hub: 79 entries)
    j = int(torch.bincount(cols, minlength=N).argmax())              # the column most rows hold
    for which, node, reach in ((0, i, rows == i), (1, j, cols == j)):
        assert int(reach.sum()) > 1
        ops_ = [A.clone(), Bm.clone()]
        ops_[which][3, 1, node * C + C - 1, w - 1] = float('nan')    # cell 3 is selected; the last float of the node's row
        got = hip.graph_grad_csr(rp, ci, *ops_, *SEL, N).cpu()
        assert torch.equal(~torch.isfinite(got), reach), f'operand {which}: {int((~torch.isfinite(got)).sum())} non-finite entries, reach {int(reach.sum())}'
        assert torch.equal(got[~reach], clean[~reach])
        ops_ = [A.clone(), Bm.clone()]
        ops_[which][2, 1, node * C + C - 1, w - 1] = float('nan')    # cell 2 is not
        assert torch.equal(hip.graph_grad_csr(rp, ci, *ops_, *SEL, N).cpu(), clean)


@pytest.mark.gpu
def test_the_front_refuses_what_the_kernel_does_not_take(hip):
    N, rowptr, colidx = pattern('hub')
    A, Bm = (t.cuda() for t in operands(N, 3, 20, 2))
    rp, ci = rowptr.cuda(), colidx.cuda()
    with pytest.raises(_lib.StcError, match='outside the buffer'):
        hip.graph_grad_csr(rp, ci, A, Bm, 0, 1, CELLS + 1, N)
    with pytest.raises(_lib.StcError, match='rowptr'):
        hip.graph_grad_csr(rp[:-1].contiguous(), ci, A, Bm, *SEL, N)
    with pytest.raises(_lib.StcError, match='into'):
        hip.graph_grad_csr(rp, ci, A, Bm, *SEL, N, into=(torch.empty(2, ci.numel() - 1, dtype=torch.float64, device='cuda'), 0))
    wide = torch.zeros(1, 1, N * 17, 32, device='cuda')
    with pytest.raises(_lib.StcError, match='512'):
        hip.graph_grad_csr(rp, ci, wide, wide, 0, 1, 1, N)
    assert float(hip.graph_grad_csr(rp, ci, A, Bm, 0, 1, 0, N).abs().max()) == 0.0          # no selected cell: zeros, nothing launched
