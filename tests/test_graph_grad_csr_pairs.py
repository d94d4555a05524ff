"""``stc_graph_grad_csr_pairs_f32`` (csrc/stc_graph_grad_csr_pairs.hip, ABI v44; ``HipKernels.graph_grad_csr_pairs``): the value gradient of a learned
spatial graph on a sparse pattern from the planar cells of the cell-graph executor -- the sampled product of ``stc_graph_grad_csr_f32`` over up to
three pairs of planes of unequal widths, ADDED to one float64 accumulator.

    acc[e] += sum_{p < n_pairs} sum_{b < batch} sum_{f < F_p} A_p[b][i(e)][f] * B_p[b][colidx[e]][f]          e: the entries of row i(e)

CPU part: header, ctypes table and EXPORTS agree; every refusal comes back before any HIP call (made-up device addresses in real host arrays); the
float64 twin written here equals the dense einsum masked to the pattern; the kernels use no scratch.

GPU part (-m gpu): the patterns of tests/test_graph_grad_csr.py -- ``ragged``, ``one_way`` (empty rows), ``weights``, the hub (a row of 79 entries: no
multiple of either tile) -- and a pattern of 3 rows (fewer than the XCDs and than the waves of a workgroup); launches of 1, 2 and 3 pairs whose widths
cover F in {4, 32, 128, 260, 512, 1024} (one lane busy, the narrow plane at C = 32, half a wave, a second piece partly filled, two and four full
pieces) with unequal widths in one launch, batch 1 and 3, A and B of a pair at magnitudes 1e-3 .. 1e2 apart.  Bound: ``EINSUM_BOUND`` = 1e-6 of
tests/test_graph_grad_blocked.py against the float64 sampled product, the project's bound for this arithmetic."""
import ctypes
import os
import re

import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib
from tests.conftest import REPO, rel_err
from tests.test_graph_grad_blocked import EINSUM_BOUND, SENTINEL
from tests.test_graph_grad_csr import pattern as csr_pattern, rows_of

ENTRY = 'stc_graph_grad_csr_pairs_f32'
PATTERNS = ('ragged', 'one_way', 'weights', 'hub', 'three_rows')
# (widths of the pairs of one launch, batch): every width of {4, 32, 128, 260, 512, 1024}, 1 / 2 / 3 pairs, each kernel form (1, 2, 4 pieces per lane)
CONFIGS = [((4,), 1), ((32,), 3), ((128, 260), 1), ((260, 512), 3), ((1024,), 1), ((512, 32, 1024), 3), ((4, 128, 32), 1)]
SCALES = (1e-3, 1e2, 1.0)             # A_p times this, B_p divided by it: every pair's product is of order one


def pattern(name):
    if name == 'three_rows':
        return 3, torch.tensor([0, 2, 2, 3], dtype=torch.int32), torch.tensor([1, 2, 0], dtype=torch.int32)
    return csr_pattern(name)


def pairs_twin(rowptr, colidx, pairs, N):
    """(nnz,) float64: sum over the pairs and samples of < A[b, i(e)], B[b, colidx[e]] >, planes read as (batch, N, F)."""
    rows, cols = rows_of(rowptr), colidx.long()
    out = torch.zeros(colidx.numel(), dtype=torch.float64)
    for A, Bm in pairs:
        a, b = A.double().reshape(A.shape[0], N, -1), Bm.double().reshape(A.shape[0], N, -1)
        for s in range(a.shape[0]):
            out += (a[s, rows] * b[s, cols]).sum(-1)
    return out


def operands(N, widths, B, seed=0):
    g = torch.Generator().manual_seed(1000 * N + sum(widths) + 7 * B + seed)
    return [(torch.randn(B, N, F, generator=g) * s, torch.randn(B, N, F, generator=g) / s) for F, s in zip(widths, SCALES)]


class PairsTwin(EmulatedKernels):
    """The CPU twin with the product, in the operands' own precision."""

    def graph_grad_csr_pairs(self, rowptr, colidx, pairs, N, acc):
        acc += pairs_twin(rowptr, colidx, pairs, N).to(acc.dtype)


# ============================================================================================================== CPU
def test_header_table_and_exports_agree():
    header = open(os.path.join(REPO, 'include', 'stc_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(rf'\b{ENTRY}\s*\(', code) and ENTRY in _lib._ABI and ENTRY in _lib.EXPORTS
    proto = re.search(rf'{ENTRY}\s*\((.*?)\)\s*;', code, flags=re.S).group(1)
    assert len(proto.split(',')) == len(_lib._ABI[ENTRY][1]) == 11
    assert re.findall(r'^#define\s+STC_ABI_VERSION\s+(\d+)\b', header, flags=re.M) == [str(_lib.ABI_VERSION)]
    assert _lib.load_library().stc_version() == _lib.ABI_VERSION >= 44
    assert hasattr(_lib.HipKernels, 'graph_grad_csr_pairs') and _lib.HipKernels.cell_graph_vals is True      # on the class: ``for_graph`` views have it
    assert not hasattr(EmulatedKernels, 'graph_grad_csr_pairs') and not hasattr(EmulatedKernels, 'cell_graph_vals')   # the CPU twin gets neither
    assert 'stc_graph_grad_csr_pairs.hip' in open(os.path.join(REPO, 'stc-gnn_amd', 'csrc', 'Makefile')).read()


_PTR = dict(rowptr=0x10000, colidx=0x20000, acc=0x30000)
_PLANES = dict(A=(0x40000, 0x50000, 0x60000), B=(0x70000, 0x80000, 0x90000))


def _call(lib, n_rows=10, nnz=30, n_pairs=2, batch=2, F=(60, 512, 1024), A=_PLANES['A'], B=_PLANES['B'], **over):
    """Real host arrays of made-up device addresses; ``A`` / ``B`` / ``F`` = None pass a null host array."""
    p = dict(_PTR, **over)
    arr = lambda v: None if v is None else (ctypes.c_void_p * 3)(*v)
    widths = None if F is None else (ctypes.c_int32 * 3)(*F)
    return lib.stc_graph_grad_csr_pairs_f32(p['rowptr'], p['colidx'], n_rows, nnz, arr(A), arr(B), widths, n_pairs, batch, p['acc'], None)


def test_refusals_come_before_any_hip_call():
    """Made-up addresses throughout: a call that got as far as a launch would fault, a refusal never touches them."""
    lib = _lib.load_library()
    err = lambda: lib.stc_last_error()
    EINVAL, EALIGN = -1, -2
    for n_pairs in (0, 4, -1):
        assert _call(lib, n_pairs=n_pairs) == EINVAL and b'n_pairs' in err(), n_pairs
    for F in (0, 2, 1028, 6, -4):
        for slot in (0, 1):                                            # (the third width is not read with two pairs)
            widths = [60, 512, 1024]
            widths[slot] = F
            assert _call(lib, F=widths) == EINVAL and b'multiple of 4' in err(), (F, slot)
    assert _call(lib, n_pairs=3, F=(60, 512, 6)) == EINVAL and b'multiple of 4' in err()
    for name in _PTR:
        assert _call(lib, **{name: None}) == EINVAL and b'null' in err(), name
    for host in ('A', 'B', 'F'):
        assert _call(lib, **{host: None}) == EINVAL and b'null' in err(), host
    for host in ('A', 'B'):
        for slot in (0, 1):
            planes = list(_PLANES[host])
            planes[slot] = 0
            assert _call(lib, **{host: planes}) == EINVAL and b'null' in err(), (host, slot)
            planes[slot] = _PLANES[host][slot] + (4, 8)[slot]
            assert _call(lib, **{host: planes}) == EALIGN and b'unaligned' in err(), (host, slot)
    for name, off in (('acc', 4), ('rowptr', 2), ('colidx', 2)):
        assert _call(lib, **{name: _PTR[name] + off}) == EALIGN and b'unaligned' in err(), name
    for size in ('n_rows', 'nnz', 'batch'):
        assert _call(lib, **{size: -1}) == EINVAL and b'negative' in err(), size
    for nothing in (dict(nnz=0), dict(batch=0), dict(n_rows=0)):       # launch nothing, whatever the device pointers are
        assert _call(lib, **nothing) == 0 and _call(lib, rowptr=None, colidx=None, acc=None, **nothing) == 0, nothing


@pytest.mark.parametrize('name', PATTERNS)
def test_the_float64_twin_equals_the_dense_einsum_masked_to_the_pattern(name):
    N, rowptr, colidx = pattern(name)
    pairs = operands(N, (4, 260, 32), 2)
    dense = sum(torch.einsum('bif,bjf->ij', A.double(), Bm.double()) for A, Bm in pairs)
    got = pairs_twin(rowptr, colidx, pairs, N)
    rows, cols = rows_of(rowptr), colidx.long()
    assert got.dtype == torch.float64 and got.shape == (colidx.numel(),) and rel_err(got, dense[rows, cols]) < 1e-13
    mask = torch.zeros(N, N, dtype=torch.bool)
    mask[rows, cols] = True
    assert int(mask.sum()) == colidx.numel()                                       # no duplicate entries: the scatter is the masked matrix
    acc = torch.ones(colidx.numel(), dtype=torch.float64)
    PairsTwin().graph_grad_csr_pairs(rowptr, colidx, pairs, N, acc)
    assert torch.equal(acc, 1.0 + got)


def test_the_kernels_use_no_scratch(tmp_path):
    from tests.test_first_step_isa import _resource_usage
    from tests.test_isa import HIPCC
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not present')
    usage = _resource_usage('stc_graph_grad_csr_pairs.hip', tmp_path)
    assert len(usage) == 3, sorted(usage)                                          # one, two and four 16-byte pieces per lane
    for name, u in usage.items():
        assert u['ScratchSize'] == 0 and u['LDS Size'] == 0 and u['VGPRs'] <= 160, (name, u)


# ============================================================================================================== GPU
@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


_REF = {}


def reference(name, widths, B):
    """(N, rowptr, colidx, pairs, float64 product) of one case: computed once, shared, never modified."""
    key = (name, widths, B)
    if key not in _REF:
        N, rowptr, colidx = pattern(name)
        pairs = operands(N, widths, B)
        _REF[key] = (N, rowptr, colidx, pairs, pairs_twin(rowptr, colidx, pairs, N))
    return _REF[key]


def _banded(nnz, fill=SENTINEL, lead=8, tail=16):
    """(whole buffer, the (nnz,) accumulator inside it): sentinel bands before and after."""
    buf = torch.full((lead + nnz + tail,), fill, dtype=torch.float64, device='cuda')
    return buf, buf[lead:lead + nnz]


def _dev(pairs):
    return [(A.cuda(), Bm.cuda()) for A, Bm in pairs]


@pytest.mark.gpu
@pytest.mark.parametrize('widths,B', CONFIGS, ids=[f'F{"+".join(map(str, w))}-B{b}' for w, b in CONFIGS])
@pytest.mark.parametrize('name', PATTERNS)
def test_parity_accumulation_and_the_bands(hip, name, widths, B):
    """Against the float64 sampled product at ``EINSUM_BOUND``: one launch into zeros; a second launch into the same accumulator (the sum of
    both); a pre-filled accumulator is added to; the sentinel bands before and after [0, nnz) keep their bits; two runs give equal bits."""
    N, rowptr, colidx, pairs, want = reference(name, widths, B)
    rp, ci, nnz, dev = rowptr.cuda(), colidx.cuda(), colidx.numel(), _dev(pairs)
    buf, acc = _banded(nnz)
    acc.zero_()
    hip.graph_grad_csr_pairs(rp, ci, dev, N, acc)
    once = acc.clone()
    err = rel_err(once, want)
    print(f'graph_grad_csr_pairs {name} F={widths} B={B}: {err:.3e} from float64 (bound {EINSUM_BOUND:.1e})')
    assert err < EINSUM_BOUND, err
    hip.graph_grad_csr_pairs(rp, ci, dev, N, acc)
    assert torch.equal(acc, once + once) and rel_err(acc, 2 * want) < EINSUM_BOUND
    g = torch.Generator().manual_seed(nnz)
    start = torch.randn(nnz, generator=g, dtype=torch.float64) * float(want.abs().max())
    acc.copy_(start)
    hip.graph_grad_csr_pairs(rp, ci, dev, N, acc)
    assert torch.equal(acc.cpu(), start + once.cpu()) and rel_err(acc, start + want) < EINSUM_BOUND
    torch.cuda.synchronize()
    whole = buf.cpu()
    assert bool((whole[:8] == SENTINEL).all()) and bool((whole[8 + nnz:] == SENTINEL).all())
    acc.zero_()
    hip.graph_grad_csr_pairs(rp, ci, dev, N, acc)
    assert torch.equal(acc, once)


@pytest.mark.gpu
@pytest.mark.parametrize('name,widths,B', [('hub', (512, 32, 1024), 3), ('ragged', (128, 260), 1)])
def test_one_launch_of_pairs_is_the_launches_of_each_and_replays_give_the_same_bits(hip, name, widths, B):
    """The pairs of one launch are added in order: launched one by one into the same accumulator they leave a sum within the bound of the
    joint launch (float64 addition in another order); an eager launch and a graph replay give equal bits."""
    N, rowptr, colidx, pairs, want = reference(name, widths, B)
    rp, ci, nnz, dev = rowptr.cuda(), colidx.cuda(), colidx.numel(), _dev(pairs)
    joint = torch.zeros(nnz, dtype=torch.float64, device='cuda')
    hip.graph_grad_csr_pairs(rp, ci, dev, N, joint)
    split = torch.zeros_like(joint)
    for pr in dev:
        hip.graph_grad_csr_pairs(rp, ci, [pr], N, split)
    assert rel_err(split, want) < EINSUM_BOUND and rel_err(split, joint) < 1e-12
    static = torch.zeros_like(joint)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.graph_grad_csr_pairs(rp, ci, dev, N, static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static.zero_()
        hip.graph_grad_csr_pairs(rp, ci, dev, N, static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, joint)


@pytest.mark.gpu
@pytest.mark.parametrize('name,widths,B', [('hub', (260, 512), 3), ('ragged', (512, 32, 1024), 3)])
def test_a_nan_reaches_its_row_or_column_only(hip, name, widths, B):
    """A NaN in row i of some A_p reaches exactly the entries of row i, a NaN in row j of some B_p exactly the entries with column j; every
    other entry keeps the bits of the clean run."""
    N, rowptr, colidx, pairs, want = reference(name, widths, B)
    rp, ci, nnz = rowptr.cuda(), colidx.cuda(), colidx.numel()
    rows, cols = rows_of(rowptr), colidx.long()
    clean = torch.zeros(nnz, dtype=torch.float64, device='cuda')
    hip.graph_grad_csr_pairs(rp, ci, _dev(pairs), N, clean)
    i = int(torch.bincount(rows, minlength=N).argmax())              # the longest row (the hub: 79 entries)
    j = int(torch.bincount(cols, minlength=N).argmax())              # the column most rows hold
    for which, node, reach in ((0, i, rows == i), (1, j, cols == j)):
        assert int(reach.sum()) > 1
        for p in range(len(pairs)):
            bad = [[A.clone(), Bm.clone()] for A, Bm in pairs]
            bad[p][which][B - 1, node, widths[p] - 1] = float('nan')  # the last float of the node's row in the last sample
            got = torch.zeros(nnz, dtype=torch.float64, device='cuda')
            hip.graph_grad_csr_pairs(rp, ci, _dev(bad), N, got)
            got = got.cpu()
            assert torch.equal(~torch.isfinite(got), reach), f'operand {which} of pair {p}: {int((~torch.isfinite(got)).sum())} non-finite entries, reach {int(reach.sum())}'
            assert torch.equal(got[~reach], clean.cpu()[~reach])


@pytest.mark.gpu
def test_the_front_refuses_what_the_kernel_does_not_take(hip):
    N, rowptr, colidx, pairs, _ = reference('hub', (128, 260), 1)
    rp, ci, dev = rowptr.cuda(), colidx.cuda(), _dev(pairs)
    acc = torch.zeros(colidx.numel(), dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.StcError, match='pairs'):
        hip.graph_grad_csr_pairs(rp, ci, [], N, acc)
    with pytest.raises(_lib.StcError, match='pairs'):
        hip.graph_grad_csr_pairs(rp, ci, dev * 2, N, acc)
    with pytest.raises(_lib.StcError, match='acc'):
        hip.graph_grad_csr_pairs(rp, ci, dev, N, acc.float())
    with pytest.raises(_lib.StcError, match='acc'):
        hip.graph_grad_csr_pairs(rp, ci, dev, N, acc[:-1])
    with pytest.raises(_lib.StcError, match='rowptr'):
        hip.graph_grad_csr_pairs(rp[:-1].contiguous(), ci, dev, N, acc)
    with pytest.raises(_lib.StcError, match='floats per node'):
        hip.graph_grad_csr_pairs(rp, ci, [(torch.zeros(1, N, 1028, device='cuda'),) * 2], N, acc)
    with pytest.raises(_lib.StcError, match='floats per node'):
        hip.graph_grad_csr_pairs(rp, ci, [(torch.zeros(1, N, 6, device='cuda'),) * 2], N, acc)
    with pytest.raises(_lib.StcError, match='shape'):
        hip.graph_grad_csr_pairs(rp, ci, [(dev[0][0], dev[1][1])], N, acc)
    with pytest.raises(_lib.StcError, match='ROCm'):
        hip.graph_grad_csr_pairs(rp, ci, [(dev[0][0].cpu(), dev[0][1])], N, acc)
    assert float(acc.abs().max()) == 0.0                              # nothing was launched
    empty = torch.zeros(0, N, 128, device='cuda')                     # batch 0: launches nothing
    hip.graph_grad_csr_pairs(rp, ci, [(empty, empty)], N, acc)
    assert float(acc.abs().max()) == 0.0
