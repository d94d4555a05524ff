"""One family of spatial graphs for the tests of the kernels that fuse an aggregation with something else (stc_spmm_sum_*, stc_spmm_blend_fwd_*,
the two-ring forms): the 8-neighbour grid with what the row-stochastic queen grid hides from them --

* signed random weights, a different one on every entry (on the queen grid every entry of a row carries 1 / deg: a kernel or plan that pairs a
  value with the wrong entry of its row computes the same sums);
* dropped edges (rows of 0 .. 8 entries, a pattern that is not symmetric any more) and rows without entries;
* the upper triangle alone (``one_way``: Gs and Gs^T share no entry, rows whose first ring has rows with no entries of their own);
* a random node order, renumbered by the host (ring-bounded clusters instead of lattice tiles).

A plain module, no fixtures: ``weighted_grid`` builds a graph, ``case`` the named ones (cached: graphs are read-only).  Both return the
``CsrGraph`` and its matrix in float64 -- the fp32 values widened, so a float64 reference runs on exactly the kernel's weights.
"""
import functools

import torch

from stc_hip import CsrGraph


def weighted_grid(H, W, seed, drop=0.0, one_way=False, empty_rows=(), permute_seed=None, renumber=False, unit=False, positive=False):
    """(CsrGraph, dense float64 G) of the H x W 8-neighbour grid times ``randn`` weights times a keep-mask (``rand >= drop``), optionally cut to
    its upper triangle, with ``empty_rows`` zeroed.  ``permute_seed``: under that random node order; ``renumber``: then renumbered by the host
    (reverse Cuthill-McKee, ``with_locality``) -- asserted to happen.  ``unit``: G divided by the graph's ``row_sum_bound``, so that one
    aggregation cannot amplify a state.  ``positive``: weights ``rand + 0.1`` instead, every row scaled to sum 1 (no cancellation inside a
    row: for comparisons in bf16 ulps)."""
    G = CsrGraph.queen_grid(H, W, normalize=False, permute_seed=permute_seed).to_dense()
    gen = torch.Generator().manual_seed(seed)
    weights = torch.randn(G.shape, generator=gen)
    keep = torch.rand(G.shape, generator=gen) >= drop
    if positive:
        weights = torch.rand(G.shape, generator=gen) + 0.1
    G = G * weights * keep
    if one_way:
        G = torch.triu(G)
    for r in empty_rows:
        G[r] = 0
    if positive:
        sums = G.sum(1, keepdim=True)
        G = G / torch.where(sums > 0, sums, torch.ones_like(sums))
    graph = CsrGraph.from_dense(G)
    if renumber:
        graph, order = graph.with_locality(collective=False)
        assert order is not None, 'the random order did not cost enough row fetches for the host to renumber'
        order = torch.from_numpy(order)
        G = G[order][:, order]
    if unit:
        G = G / graph.row_sum_bound
        graph = CsrGraph.from_dense(G)
    assert torch.equal(graph.to_dense(), G)
    return graph, G.double()


#: name -> (shapes, construction).  The shapes are the smallest with several patches (9 and 15 tiles, 24 clusters), partial last patches and
#: interior tiles; the lattices' patch counts are no multiple of 8, so the padding of the workgroup-to-patch map is in play.
CASES = {
    'weights': (((12, 20), (9, 33)), dict()),
    'ragged': (((12, 20), (9, 33)), dict(drop=0.15, empty_rows=(3, 10))),
    'one_way': (((12, 20), (9, 33)), dict(one_way=True, drop=0.15, empty_rows=(3,))),
    'clusters': (((24, 30),), dict(drop=0.15, empty_rows=(3, 10), permute_seed=7, renumber=True)),
    'one_side': (((6, 6),), dict(drop=0.15, permute_seed=10)),
}

#: what each case promises: two-ring plans per orientation (fwd, bwd), ring-bounded clusters
PLANS = {'weights': (True, True, False), 'ragged': (True, True, False), 'one_way': (True, True, False), 'clusters': (True, True, True),
         'one_side': (False, True, False)}


def shapes(name):
    return CASES[name][0]


@functools.lru_cache(maxsize=None)
def case(name, H=None, W=None, unit=False, positive=False):
    """The named case at (H, W) -- its first shape by default."""
    shp, kw = CASES[name]
    H, W = shp[0] if H is None else (H, W)
    assert (H, W) in shp
    return weighted_grid(H, W, seed=1000 * H + W, unit=unit, positive=positive, **kw)


def grid_params(names=('weights', 'ragged', 'one_way', 'clusters')):
    """(name, H, W) of every shape of the named cases, for ``pytest.mark.parametrize``."""
    return [(n, H, W) for n in names for H, W in shapes(n)]
