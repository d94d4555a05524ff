"""The BLOCKED form of stc_graph_grad_f32 (csrc/stc_graph_grad.hip: a workgroup per 64 x 64 output block, operand rows through LDS once per block
and plane) behind ``stc_set_graph_grad_form`` (ABI v38: 0 = by rule, 1 = tile per wave, 2 = blocked).

The two forms run the same fp32 product chain per plane and 16 x 16 tile and fold into float64 in the same order, so the blocked partials are
compared with the tile-per-wave ones by plain equality -- no tolerance: block edges (N = 17, 64, 65, 129, 200), row widths 20 and 32 at C = 3, 5, 8
(F = 60 and 100: a partial group of column quads; 96, 160, 256), a strided cell selection, several planes per chunk and chunks without a plane.
Then: against the float64 einsum at the bound of tests/test_small_cell.py::test_graph_gradient_products, run-to-run bits, the reach of a NaN (the
``rows`` class of tests/nonfinite.py: the output row / column of the poisoned operand row, nothing else), and the selector's refusals.
"""
import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip import _lib
from tests.conftest import rel_err

EM = EmulatedKernels()
EINSUM_BOUND = 1e-6                   # that of tests/test_small_cell.py::test_graph_gradient_products
CELLS, SEL = 6, (1, 2, 3)             # cells 1, 3, 5 out of 6
SENTINEL = -7.0                       # what a launch must leave between the blocks of a strided partial buffer

# (N, C, row width, batch, chunks): planes = 3 * batch
CASES = [(17, 3, 20, 2, 11),          # one block, ragged; F = 60; more chunks than planes: empty chunks
         (64, 5, 20, 3, 4),           # one block exactly; F = 100; three planes in the first chunk
         (65, 3, 32, 2, 4),           # one row past the block boundary; F = 96
         (129, 5, 32, 2, 11),         # one row past the second boundary; F = 160
         (129, 3, 20, 3, 4),          # F = 60
         (200, 8, 32, 2, 5),          # 4 x 4 blocks, the last with 8 live rows; F = 256
         (200, 5, 20, 3, 11)]         # F = 100


@pytest.fixture
def hip():
    k = _lib.HipKernels()
    yield k
    k.set_graph_grad_form(0)


def _operands(N, C, w, B):
    g = torch.Generator().manual_seed(1000 * N + 10 * C + w + B)
    return tuple(torch.randn(CELLS, B, N * C, w, generator=g) for _ in range(2))


def _partials(hip, form, A, Bm, N, chunks, offset=3, tail=5):
    """The whole (chunks, offset + N * N + tail) buffer after one launch of ``form`` into its block at ``offset``."""
    hip.set_graph_grad_form(form)
    part = torch.full((chunks, offset + N * N + tail), SENTINEL, dtype=torch.float64, device=A.device)
    assert hip.graph_grad(A, Bm, *SEL, N, into=(part, offset)) is None
    torch.cuda.synchronize()
    return part.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,w,B,chunks', CASES)
def test_blocked_partials_equal_the_tile_per_wave_ones_bit_for_bit(hip, N, C, w, B, chunks):
    A, Bm = (t.cuda() for t in _operands(N, C, w, B))
    tile, blocked = _partials(hip, 1, A, Bm, N, chunks), _partials(hip, 2, A, Bm, N, chunks)
    assert torch.equal(blocked, tile), f'{int((blocked != tile).sum())} of {tile.numel()} partials differ'
    assert torch.equal(blocked[:, :3], torch.full((chunks, 3), SENTINEL, dtype=torch.float64))          # outside the block: untouched
    assert torch.equal(blocked[:, -5:], torch.full((chunks, 5), SENTINEL, dtype=torch.float64))
    block = blocked[:, 3:-5]
    assert bool((block != SENTINEL).all())                                                              # every element of every chunk written
    planes = SEL[2] * B
    if chunks > planes:
        assert float(block[planes:].abs().max()) == 0.0                                                 # a chunk without a plane: zeros
    assert torch.equal(_partials(hip, 2, A, Bm, N, chunks), blocked)                                    # run to run: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,w,B', [(17, 3, 20, 2), (65, 3, 32, 2), (200, 5, 20, 3), (200, 8, 32, 2)])
def test_blocked_form_against_the_float64_einsum(hip, N, C, w, B):
    A, Bm = _operands(N, C, w, B)
    want = EM.graph_grad(A, Bm, *SEL, N)
    hip.set_graph_grad_form(2)
    got = hip.graph_grad(A.cuda(), Bm.cuda(), *SEL, N).cpu()
    err = rel_err(got, want)
    print(f'blocked graph_grad N={N} F={C * w}: {err:.3e} (bound {EINSUM_BOUND:.1e})')
    assert got.dtype == torch.float64 and got.shape == (N, N) and err < EINSUM_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,w,B', [(65, 3, 32, 2), (200, 5, 20, 3)])
def test_a_nan_reaches_its_row_or_column_only(hip, N, C, w, B):
    """A[.., (n, c), f] enters row n of out = sum A . B^T, B[.., (m, c), f] its column m; an unselected cell reaches nothing.  Every other element
    keeps the bits of the clean run."""
    A, Bm = (t.cuda() for t in _operands(N, C, w, B))
    hip.set_graph_grad_form(2)
    clean = hip.graph_grad(A, Bm, *SEL, N).cpu()
    n = N - 1                                                        # the last live row of the last, ragged block
    for which in (0, 1):
        ops_ = [A.clone(), Bm.clone()]
        ops_[which][3, 1, n * C + 1, 7] = float('nan')               # cell 3 is selected
        got = hip.graph_grad(*ops_, *SEL, N).cpu()
        got = got if which == 0 else got.t()
        bad = ~torch.isfinite(got)
        assert bool(bad[n].all()) and int(bad.sum()) == N, f'operand {which}: {int(bad.sum())} non-finite elements'
        keep = torch.arange(N) != n
        assert torch.equal(got[keep], (clean if which == 0 else clean.t())[keep])
        ops_ = [A.clone(), Bm.clone()]
        ops_[which][2, 1, n * C + 1, 7] = float('nan')               # cell 2 is not
        assert torch.equal(hip.graph_grad(*ops_, *SEL, N).cpu(), clean)


def test_the_selector_refuses_unknown_forms():
    lib = _lib.load_library()
    try:
        for form in (0, 1, 2):
            assert lib.stc_set_graph_grad_form(form) == 0
        assert lib.stc_set_graph_grad_form(3) == -1 and b'form 3' in lib.stc_last_error()
        assert lib.stc_set_graph_grad_form(-1) == -1 and b'form -1' in lib.stc_last_error()
    finally:
        assert lib.stc_set_graph_grad_form(0) == 0
    assert 'stc_set_graph_grad_form' in _lib.EXPORTS and _lib.ABI_VERSION >= 38


@pytest.mark.gpu
def test_the_front_names_a_refused_form(hip):
    with pytest.raises(_lib.StcError, match='form 3'):
        hip.set_graph_grad_form(3)
