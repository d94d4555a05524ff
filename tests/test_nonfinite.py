"""NaN / +-Inf through the kernels: the contract of include/stc_hip.h, "Non-finite values" (mirrored in DESIGN.md), case by case.

One float element of one operand is replaced by NaN, +Inf or -Inf (never an index, count or plan array; graph values before the host plan
builders run) and the kernel is held to tests/nonfinite.py: A no masking, B bitwise containment outside the reach, C the finite part within the
kernel's own parity tolerance, D reductions as one unit.  The reference is the float64 run of the CPU twin (oracle/kernel_emul.py) or, where a
kernel has no twin (learned-graph front end, MixedFusion, Adam), a float64 restatement in torch.

CPU part (always runs): the same cases with the twin in float32 as the code under test -- helpers, poison positions and the reach computation are
checked without a GPU; two negative controls show that parts A and B bite.  GPU part (-m gpu): the HIP kernels.

An INF in a table every row reads (a weight, a bias, a category table) makes the whole launch one unit: the split-operand kernels scale such a
table by its own maximum, so with an Inf in it the finite columns are not meaningful; only A is asked there.  A NaN in such a table is dropped by
that maximum: it is held to B and C like any other poison, on every dispatch level.
"""
import pytest
import torch

import STC_GNN as M
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, ops
from tests import nonfinite as nf
from tests.test_grad_scale import _cell_bwd, _cell_case, node_factors

EM = EmulatedKernels()
NAN = float('nan')
ALL = ('nan', '+inf', '-inf')


def new(like, *shape, dtype=None):
    return torch.full(shape, NAN, dtype=dtype or like.dtype, device=like.device)


def is_twin(k):
    return isinstance(k, EmulatedKernels)


class Case:
    """``make() -> operands`` (seeded, O(1) data), ``run(k, d) -> outputs``, ``kinds`` per output, ``sites``: label -> (operand, index, table?)."""

    def __init__(self, name, make, run, kinds, sites, tols=None, spread=None, coverage=True, default_tol=nf.F32_TOL, values=None, exempt=None):
        self.name, self.make, self.run, self.kinds, self.sites, self.exempt = name, make, run, kinds, sites, exempt
        self.tols, self.spread, self.coverage, self.default_tol, self.values = tols, spread, coverage, default_tol, values or {}
        self._ops = self._want_clean = None

    @property
    def operands(self):
        if self._ops is None:
            self._ops = self.make()
        return self._ops

    def want(self, operands):
        return self.run(EM, nf.mapped(operands, lambda t: t.double()))

    @property
    def want_clean(self):
        if self._want_clean is None:
            self._want_clean = self.want(self.operands)
        return self._want_clean

    def check(self, k, to, site, run=None):
        """The contract at one poison site, for every value of the site; ``run``: the code under test where it is not ``self.run`` (controls)."""
        run = run or self.run
        operand, index, table = self.sites[site]
        clean = run(k, to(self.operands))
        for v in self.values.get(site, ALL):
            bad_ops = nf.poisoned(self.operands, operand, index, nf.POISONS[v])
            got = run(k, to(bad_ops))
            spread = None if self.spread is None else (lambda name, bad, every: (setattr(self, 'touched_all', every), self.spread(self, name, bad))[1])
            nf.check_contract(f'{self.name}[{site}={v}]', self.want(bad_ops), self.want_clean, got, clean, self.kinds, self.tols, spread,
                              table and v != 'nan', self.default_tol, self.coverage, expect_nonfinite=v == 'nan', table_site=table,
                              exempt_strict=v == 'nan', exempt=None if self.exempt is None else {**self.exempt.get('*', {}), **self.exempt.get(site, {})})


def on_cpu(operands):
    return nf.mapped(operands, lambda t: t.clone())


def on_gpu(operands):
    return nf.mapped(operands, lambda t: t.cuda(), ints=lambda t: t.cuda())


CASES = {}


def case(c):
    assert c.name not in CASES
    CASES[c.name] = c
    return c


def _ids(names=None):
    return [(n, s) for n, c in CASES.items() if names is None or n in names for s in c.sites]


# ============================================================================================================== aggregation
def _random_csr(n, density, seed, empty_rows):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(n, n, generator=g) < density
    for r in empty_rows:
        mask[r] = False
    vals = torch.randn(n, n, generator=g) * mask
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(mask.sum(1), 0)
    return rowptr.to(torch.int32), mask.nonzero()[:, 1].to(torch.int32).contiguous(), vals[mask].contiguous()


def _csr_case(name, F, dt, beta, inplace=False):
    n, B = 33, 2

    def make():
        rowptr, colidx, val = _random_csr(n, 0.25, seed=n * 7 + F, empty_rows=(1,))
        g = torch.Generator().manual_seed(F)
        return dict(rowptr=rowptr, colidx=colidx, val=val, X=torch.randn(B, n, F, generator=g).to(dt), Y0=torch.randn(B, n, F, generator=g).to(dt))

    def run(k, d):
        Y = d['Y0'].clone() if inplace else new(d['X'], B, n, F)
        k.csr_spmm(d['rowptr'], d['colidx'], d['val'], n, n, d['X'], (Y if inplace else d['Y0']) if beta else None, Y, 2.0, beta)
        return dict(Y=Y)

    sites = dict(X=('X', (0, 5, 3), False), val=('val', (7,), False))
    if beta:
        sites['Y0'] = ('Y0', (1, 4, 2), False)
    return case(Case(name, make, run, dict(Y='rows'), sites, default_tol=nf.F32_TOL if dt == torch.float32 else nf.BF16_TOL))


_csr_case('csr_spmm_f32_F85', 85, torch.float32, 0.0)
_csr_case('csr_spmm_f32_F85_y0', 85, torch.float32, -1.0)
_csr_case('csr_spmm_f32_F256_y0_inplace', 256, torch.float32, -1.0, inplace=True)
_csr_case('csr_spmm_bf16_F256', 256, torch.bfloat16, 0.0)
_csr_case('csr_spmm_bf16_F256_y0_inplace', 256, torch.bfloat16, -1.0, inplace=True)

_GRAPHS = {}


def _graph(G):
    """The project's own host plans (row blocks, patches, two-ring tables) of the graph with these VALUES, poison included."""
    Gc = G.detach().cpu().float().contiguous()
    key = (tuple(Gc.shape), Gc.numpy().tobytes())
    if key not in _GRAPHS:
        _GRAPHS[key] = CsrGraph.from_dense(Gc)
    return _GRAPHS[key]


def _graph_args(G, like, form, side='bwd'):
    graph = _graph(G)
    if like.is_cuda:
        d = graph.on(like.device)
        csr = (d[f'{side}_rowptr'], d[f'{side}_colidx'], d[f'{side}_val'])
        plan = None if form == 'csr' else (d[f'{side}_blk_ptr'], d[f'{side}_blk_cols'], d[f'{side}_blk_vals'])
        if form == 'patch':
            plan = plan + (tuple(d[f'{side}_pt_{k}'] for k in ('src', 'rows', 'cnt', 'idx', 'val')),)
        return graph, csr, plan
    h = graph._host
    return graph, (torch.from_numpy(h[f'{side}_rowptr']), torch.from_numpy(h[f'{side}_colidx']), torch.from_numpy(h[f'{side}_val']).to(G.dtype)), None


def _banded(n, half_width, seed):
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    mask = ((i[:, None] - i[None, :]).abs() <= half_width) & (torch.rand(n, n, generator=g) < 0.7)
    mask[3] = False
    return torch.randn(n, n, generator=g) * mask


def _weighted_grid(H, W, seed):
    G = CsrGraph.queen_grid(H, W, normalize=False).to_dense()
    g = torch.Generator().manual_seed(seed)
    G = G * torch.randn(G.shape, generator=g) * (torch.rand(G.shape, generator=g) > 0.15)
    G[3] = 0
    G[10] = 0
    return G


def _row_groups(c, form):
    """Rows a launch computes together: the 4-row block of the row-blocked form, the plan's patch of the patch form."""
    n = c.operands['G'].shape[0]
    if form == 'blocked':
        return nf.blocks_of(n, 4)
    rows = _graph(c.operands['G'])._host['bwd_pt_rows']
    return [sorted(set(int(r) for r in p if r >= 0)) for p in rows]


def _graph_spmm_case(name, G_of, F, B, dt, form, beta=0.0):
    def make():
        G = G_of()
        g = torch.Generator().manual_seed(F)
        return dict(G=G, X=torch.randn(B, G.shape[0], F, generator=g).to(dt), Y0=torch.randn(B, G.shape[0], F, generator=g).to(dt))

    def run(k, d):
        n = d['G'].shape[0]
        _, csr, plan = _graph_args(d['G'], d['X'], form)
        Y = d['Y0'].clone()
        k.csr_spmm(*csr, n, n, d['X'], Y if beta else None, Y, 2.0, beta, plan=plan)
        return dict(Y=Y)

    def sites():
        G = G_of()
        i, j = (int(v) for v in G.nonzero()[G.nonzero().shape[0] // 2])
        return dict(X=('X', (0, j, 5), False), G=('G', (i, j), False))

    spread = lambda c, name, bad: nf.spread_groups(bad, 1, _row_groups(c, form))
    return case(Case(name, make, run, dict(Y='rows'), sites(), spread=spread, default_tol=nf.F32_TOL if dt == torch.float32 else nf.BF16_TOL))


_graph_spmm_case('bcsr_spmm_f32', lambda: _banded(77, 3, 77 + 640), 640, 2, torch.float32, 'blocked')
_graph_spmm_case('bcsr_spmm_f32_y0', lambda: _banded(77, 3, 77 + 640), 640, 2, torch.float32, 'blocked', beta=-1.0)
_graph_spmm_case('bcsr_spmm_bf16', lambda: _banded(77, 3, 77 + 640), 640, 2, torch.bfloat16, 'blocked')
_graph_spmm_case('patch_spmm_f32', lambda: _weighted_grid(12, 12, 12 + 12 + 768), 768, 2, torch.float32, 'patch')
_graph_spmm_case('patch_spmm_f32_y0', lambda: _weighted_grid(17, 41, 17 + 41 + 512), 512, 3, torch.float32, 'patch', beta=-1.0)
_graph_spmm_case('patch_spmm_bf16', lambda: _weighted_grid(17, 41, 17 + 41 + 512), 512, 2, torch.bfloat16, 'patch')
FORM_KERNEL = {'bcsr_spmm_f32': 'stc_bcsr_spmm_f32', 'bcsr_spmm_f32_y0': 'stc_bcsr_spmm_f32', 'bcsr_spmm_bf16': 'stc_bcsr_spmm_bf16', 'patch_spmm_f32': 'stc_patch_spmm_f32',
               'patch_spmm_f32_y0': 'stc_patch_spmm_f32', 'patch_spmm_bf16': 'stc_patch_spmm_bf16', 'dense_agg': 'stc_dense_agg_f32'}


def _spmm_sum_case(name, blend, amax=False):
    grid, B, C, h = (5, 5), 2, 32, 16

    def make():
        G = CsrGraph.queen_grid(*grid, normalize=True).to_dense()
        n = G.shape[0]
        g = torch.Generator().manual_seed(n + C)
        rnd = lambda *s: torch.randn(*s, generator=g)
        return dict(G=G, X=rnd(B, n, C, h), X2=rnd(B, n, C, h), add0=rnd(B, n, C, h), add1=rnd(B, n, C, 32), U=torch.rand(B, n, C, h, generator=g),
                    Cand=torch.tanh(rnd(B, n, C, h)))

    def run(k, d):
        n = d['G'].shape[0]
        _, csr, plan = _graph_args(d['G'], d['X'], 'blocked')
        Y, dY = new(d['X'], B, n, C, h), new(d['X'], B, n, C, h)
        am = torch.zeros(64, dtype=torch.float32, device=d['X'].device) if amax else None
        k.spmm_sum(*csr, plan, d['X'], d['X2'], [(d['add0'], 0), (d['add1'], 16, -1.0)], Y, blend=(d['U'], d['Cand'], dY) if blend else None, amax=am)
        return dict(Y=Y, dY=dY) if blend else dict(Y=Y)

    sites = dict(X2=('X2', (0, 12, 3, 5), False), addend=('add1', (1, 7, 2, 20), False), G=('G', (6, 7), False))
    if blend:
        sites['U'] = ('U', (0, 3, 1, 2), False)
    spread = lambda c, name, bad: nf.spread_groups(bad, 1, nf.blocks_of(25, 4))
    return case(Case(name, make, run, dict(Y='rows', dY='rows'), sites, spread=spread))


_spmm_sum_case('spmm_sum_addends', blend=False)
_spmm_sum_case('spmm_sum_dY_epilogue', blend=True)
_spmm_sum_case('spmm_sum_amax', blend=False, amax=True)


def _spmm_blend_case():
    grid, B, C, h = (5, 5), 2, 32, 16

    def make():
        G = CsrGraph.queen_grid(*grid, normalize=True).to_dense()
        n = G.shape[0]
        g = torch.Generator().manual_seed(n + C + 1)
        rnd = lambda *s: torch.randn(*s, generator=g)
        return dict(G=G, Bm=rnd(B, n, C, h), A=rnd(B, n, C, h), U=torch.rand(B, n, C, h, generator=g), H=rnd(B, n, C, h))

    def run(k, d):
        n = d['G'].shape[0]
        _, csr, plan = _graph_args(d['G'], d['A'], 'blocked', side='fwd')
        Cand, Hn = new(d['A'], B, n, C, h), new(d['A'], B, n, C, h)
        k.spmm_blend_fwd(*csr, plan, d['Bm'], d['A'], d['U'], d['H'], Cand, Hn)
        return dict(Cand=Cand, Hnew=Hn)

    sites = dict(Bm=('Bm', (0, 12, 3, 5), False), A=('A', (1, 7, 2, 9), False), H=('H', (0, 2, 0, 1), False), G=('G', (6, 7), False))
    spread = lambda c, name, bad: nf.spread_groups(bad, 1, nf.blocks_of(25, 4))
    return case(Case('spmm_blend_fwd', make, run, dict(Cand='rows', Hnew='rows'), sites, spread=spread))


_spmm_blend_case()


def _ring2_graph():
    if 'ring2' not in _GRAPHS:
        _GRAPHS['ring2'] = CsrGraph.queen_grid(40, 56, normalize=True)      # (12 x 20 is too small: the reach of two rings would cover most patches)
    return _GRAPHS['ring2']


def _ring2_spread(side):
    """Two chained aggregations per launch, patch by patch: the first result spreads to its patch-mates (zero-weight repeats), the second is
    formed from the first AS THE LAUNCH HOLDS IT -- neighbours of those patch-mates included -- and spreads to its own patch-mates."""
    def spread(c, name, touched):
        h = _ring2_graph()._host
        groups = [sorted(set(int(r) for r in p if r >= 0)) for p in h[f'{side}_pt_rows']]
        if name != 'second':
            return nf.spread_groups(touched, 1, groups)
        B, n = touched.shape[:2]
        rp, ci = h[f'{side}_rowptr'].astype('int64'), torch.from_numpy(h[f'{side}_colidx']).long()
        rows = torch.repeat_interleave(torch.arange(n), torch.from_numpy(rp[1:] - rp[:-1]))
        first = nf.spread_groups(c.touched_all['first'], 1, groups).reshape(B, n, -1)      # (from the reference runs: no order of checking assumed)
        reach = touched.clone().reshape(B, n, -1)
        for b, f in first.any(1).nonzero().tolist():
            hit = torch.zeros(n, dtype=torch.bool)
            hit[rows[first[b, ci, f]]] = True                                # rows with an entry in a marked column
            reach[b, :, f] |= hit
        return nf.spread_groups(reach.reshape(touched.shape), 1, groups)
    return spread


def _ring2_cases():
    from stc_hip.graph import csr_operand
    B, C, h = 2, 8, 16                                                       # rows of C h = 128 floats: the narrowest the two-ring launches take
    n = 40 * 56

    def make():
        g = torch.Generator().manual_seed(n)
        rnd = lambda: torch.randn(B, n, C, h, generator=g)
        return dict(X=rnd(), X2=rnd(), add=rnd(), U=torch.sigmoid(rnd()), Cand=torch.tanh(rnd()), Bm=rnd(), A=rnd(), H=torch.tanh(rnd()))

    def ring_sum(k, d):
        op = csr_operand(_ring2_graph(), d['X'].device)
        Y, Z = new(d['X'], B, n, C, h), new(d['X'], B, n, C, h)
        k.ring2_sum(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, None if is_twin(k) else op.bwd_ring2, d['X'], d['X2'], [d['add']], d['U'], d['Cand'], Y, Z)
        return dict(first=Y, second=Z)

    def ring_blend(k, d):
        op = csr_operand(_ring2_graph(), d['X'].device)
        Cand, Hn, SHn = (new(d['X'], B, n, C, h) for _ in range(3))
        k.ring2_blend(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, None if is_twin(k) else op.fwd_ring2, d['Bm'], d['A'], d['U'], d['H'], Cand, Hn, SHn)
        return dict(Cand=Cand, first=Hn, second=SHn)

    def ring_chain(k, d):                                                   # the order-3 recurrence: V = a1 S.(X + X2) + add, Z = a2 S.V - X
        op = csr_operand(_ring2_graph(), d['X'].device)
        V, Z = new(d['X'], B, n, C, h), new(d['X'], B, n, C, h)
        k.ring2_chain(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, None if is_twin(k) else op.bwd_ring2, d['X'], d['X2'], 2.0, [d['add']], V, 1.0, [(d['A'], -1.0)], Z)
        return dict(first=V, second=Z)

    def ring_blend_first(k, d):                                             # zero state: the general form on an explicit plane of zeros is the restatement
        op = csr_operand(_ring2_graph(), d['X'].device)
        Cand, Hn, SHn = (new(d['X'], B, n, C, h) for _ in range(3))
        graph = (op.fwd_rowptr, op.fwd_colidx, op.fwd_val, None if is_twin(k) else op.fwd_ring2)
        if is_twin(k):
            k.ring2_blend(*graph, d['Bm'], d['A'], d['U'], torch.zeros_like(d['H']), Cand, Hn, SHn)
        else:
            k.ring2_blend_first(*graph, d['Bm'], d['A'], d['U'], Cand, Hn, SHn)
        return dict(Cand=Cand, first=Hn, second=SHn)

    at = (0, 20 * 56 + 30, 3, 5)                                            # an interior node of sample 0
    case(Case('ring2_chain', make, ring_chain, dict(first='rows', second='rows'), dict(X2=('X2', at, False), add1=('add', at, False), add0=('A', at, False)), spread=_ring2_spread('bwd')))
    case(Case('ring2_blend_first', make, ring_blend_first, dict(Cand='rows', first='rows', second='rows'), dict(Bm=('Bm', at, False), U=('U', at, False)),
              spread=_ring2_spread('fwd')))
    case(Case('ring2_sum', make, ring_sum, dict(first='rows', second='rows'), dict(X=('X', at, False), addend=('add', at, False), U=('U', at, False)), spread=_ring2_spread('bwd')))
    case(Case('ring2_blend', make, ring_blend, dict(Cand='rows', first='rows', second='rows'), dict(Bm=('Bm', at, False), A=('A', at, False), H=('H', at, False)),
              spread=_ring2_spread('fwd')))


_ring2_cases()


def _dense_agg_case():
    n, F, B = 12, 20, 2

    def make():
        g = torch.Generator().manual_seed(n + F)
        return dict(S=torch.softmax(torch.randn(n, n, generator=g), -1), X=torch.randn(B, n, F, generator=g), Y0=torch.randn(B, n, F, generator=g))

    def run(k, d):
        from stc_hip.graph import full_pattern
        rowptr, colidx = full_pattern(n, d['X'].device)
        Y = d['Y0'].clone()
        k.csr_spmm(rowptr, colidx, d['S'].reshape(-1), n, n, d['X'], Y, Y, 2.0, -1.0)
        return dict(Y=Y)

    # S X is dense arithmetic: X[b, j, f] reaches column f of every row of sample b (in want itself); an entry of S reaches its row in every sample
    sites = dict(X=('X', (0, 5, 3), False), S=('S', (4, 7), False), Y0=('Y0', (1, 2, 3), False))
    return case(Case('dense_agg', make, run, dict(Y='rows'), sites))


_dense_agg_case()


def _sddmm_case():
    n, F, B = 12, 7, 2

    def make():
        rowptr, colidx, _ = _random_csr(n, 0.6, seed=n + F, empty_rows=(0,))
        g = torch.Generator().manual_seed(n)
        return dict(rowptr=rowptr, colidx=colidx, A=torch.randn(B, n, F, generator=g), Bm=torch.randn(B, n, F, generator=g), base=torch.randn(colidx.numel(), generator=g))

    def run(k, d):
        out = d['base'].clone()
        k.csr_sddmm(d['rowptr'], d['colidx'], n, n, d['A'], d['Bm'], out, 2.0, True)
        return dict(dval=out)

    return case(Case('csr_sddmm', make, run, dict(dval='rows'), dict(A=('A', (0, 5, 3), False), Bm=('Bm', (1, 4, 6), False), base=('base', (9,), False))))


_sddmm_case()


def _cheby_case(n, K):
    def make():
        g = torch.Generator().manual_seed(n * 10 + K)
        return dict(G=torch.randn(n, n, generator=g) / n ** 0.5, dT=torch.randn(K, n, n, generator=g))

    def run_fwd(k, d):
        T = new(d['G'], K, n, n)
        k.cheby_dense_fwd(d['G'], K, T)
        return dict(T=T)

    def run_bwd(k, d):
        T = torch.empty_like(d['dT'])
        EM.cheby_dense_fwd(d['G'].cpu(), K, T_cpu := torch.empty(K, n, n, dtype=d['G'].dtype))
        T.copy_(T_cpu)
        dG = new(d['G'], n, n)
        k.cheby_dense_bwd(d['G'], T, d['dT'].clone(), dG)
        return dict(dG=dG)

    # G G is dense: G[i, j] reaches row i and column j of T_2 (no row of T_2 stays clear: no row count)
    case(Case(f'cheby_dense_fwd_n{n}_K{K}', make, run_fwd, dict(T='rows'), dict(G=('G', (2, 3), False)), coverage=False))
    case(Case(f'cheby_dense_bwd_n{n}_K{K}', make, run_bwd, dict(dG='rows'), dict(dT1=('dT', (1, 2, 3), False)), coverage=False))


_cheby_case(5, 2)
_cheby_case(8, 3)


# ============================================================================================================== node kernels
NODE_SHAPES = {'n50_c32': (50, 32, 32, 32, 16, 2), 'n13_c64': (13, 64, 20, 20, 16, 2), 'generic': (30, 3, 8, 5, 4, 3)}     # nodes, C, L, Lw, Ho, K


def _node_operands(nodes, C, L, Lw, Ho, K, seed):
    g = torch.Generator().manual_seed(seed)
    Zs = [torch.randn(nodes, C, L, generator=g) for _ in range(K)]
    for z in Zs:
        z[..., Lw:] = 0.0                                                  # what the host writes into the pad columns
    Tc = torch.randn(K, C, C, generator=g) / C ** 0.5
    Tc[0] = torch.eye(C)
    return dict(Zs=Zs, Tc=Tc, W=torch.randn(K * K * Lw, Ho, generator=g) / (K * K * Lw) ** 0.5, b=torch.randn(Ho, generator=g), dY=torch.randn(nodes, C, Ho, generator=g))


def pad_spread(Lw):
    """Node kernels have no spread unit but this: a node whose gradient is non-finite gets non-finite PAD columns in its own slab-gradient rows
    (the zero weight rows the matrix-core paths multiply it by) where the math has zeros."""
    def spread(c, name, touched):
        reach = touched.clone()
        if name.startswith('dZ') and touched.shape[-1] > Lw:
            reach[..., Lw:] |= touched.flatten(1).any(1).view(-1, 1, 1)
        return reach
    return spread


def _node_fwd(k, d):
    Y = new(d['W'], *d['Zs'][0].shape[:2], d['W'].shape[1], dtype=d['Zs'][0].dtype)
    k.bdg_node_fwd(d['Zs'], d['Tc'], d['W'], d['b'], Y)
    return dict(Y=Y)


def _node_bwd(k, d, want_dT=True):
    dZ = [new(z, *z.shape) for z in d['Zs']]
    dW, db = new(d['W'], *d['W'].shape), new(d['W'], d['W'].shape[1])
    dT = new(d['Tc'], *d['Tc'].shape) if want_dT else None
    k.bdg_node_bwd(d['Zs'], d['Tc'], d['W'], d['dY'], dZ, dW, db, dT)
    out = {f'dZ{i}': z for i, z in enumerate(dZ)}
    out.update(dW=dW, db=db)
    if want_dT:
        out['dTc'] = dT[1:]                                                # (T_0 = I is a constant: the kernels write zeros there, the twin its product)
    return out


def _node_cases(tag, shape):
    nodes, C, L, Lw, Ho, K = shape
    make = lambda: _node_operands(*shape, seed=sum(shape))
    r = nodes // 2
    sites_f = dict(Z=(('Zs', 1), (r, 1, 2), False), W=('W', (3, 2), True), bias=('b', (1,), True), Tc=('Tc', (1, 2, 1), True))
    case(Case(f'bdg_node_fwd_{tag}', make, _node_fwd, dict(Y='rows'), sites_f))
    kinds = {f'dZ{i}': 'rows' for i in range(K)}
    kinds.update(dW='reduce', db='reduce', dTc='reduce')
    sites_b = dict(dY=('dY', (r, 1, 2), False), Z=(('Zs', 0), (r, 2, 1), False), W=('W', (3, 2), True), Tc=('Tc', (1, 2, 1), True))
    case(Case(f'bdg_node_bwd_{tag}', make, _node_bwd, kinds, sites_b, spread=pad_spread(Lw)))


for _tag, _shape in NODE_SHAPES.items():
    _node_cases(_tag, _shape)
NODE_CASES = [n for n in CASES if n.startswith('bdg_node_')]


def _node_bf16_cases():
    shape = (50, 32, 32, 32, 16, 2)
    bf = torch.bfloat16

    def make():
        d = _node_operands(*shape, seed=sum(shape) + 7)
        d['Zs'], d['dY'] = [z.to(bf) for z in d['Zs']], d['dY'].to(bf)
        return d

    def fwd(k, d):
        if is_twin(k) and d['W'].dtype == torch.float64:                  # want: fp64 math on the bf16-valued planes
            return _node_fwd(k, d)
        Y = new(d['Zs'][0], *d['Zs'][0].shape[:2], d['W'].shape[1])
        k.bdg_node_fwd_bf16(d['Zs'], d['Tc'], d['W'], d['b'], Y)
        return dict(Y=Y)

    def bwd(k, d):
        if is_twin(k) and d['W'].dtype == torch.float64:
            return _node_bwd(k, d, want_dT=False)
        dZ = [new(z, *z.shape) for z in d['Zs']]
        dW, db = new(d['W'], *d['W'].shape), new(d['W'], d['W'].shape[1])
        k.bdg_node_bwd_bf16(d['Zs'], d['Tc'], d['W'], d['dY'], dZ, dW, db)
        out = {f'dZ{i}': z for i, z in enumerate(dZ)}
        out.update(dW=dW, db=db)
        return out

    case(Case('bdg_node_fwd_bf16', make, fwd, dict(Y='rows'), dict(Z=(('Zs', 1), (25, 1, 2), False), W=('W', (3, 2), True)), default_tol=nf.BF16_TOL))
    case(Case('bdg_node_bwd_bf16', make, bwd, dict(dZ0='rows', dZ1='rows', dW='reduce', db='reduce'), dict(dY=('dY', (25, 1, 2), False), Z=(('Zs', 0), (25, 2, 1), False)),
              default_tol=nf.BF16_TOL))


_node_bf16_cases()


def _node_post_cases():
    nodes, C, L, Ho, K = 50, 32, 32, 16, 2

    def make():
        g = torch.Generator().manual_seed(nodes + C + L)
        rnd = lambda *s: torch.randn(*s, generator=g)
        Tc = rnd(K, C, C) / C ** 0.5
        Tc[0] = torch.eye(C)
        return dict(X=rnd(nodes, C, L), Tc=Tc, W=rnd(K * K * L, Ho) / (K * K * L) ** 0.5, b=rnd(Ho), dA=rnd(nodes, C, Ho), dB=rnd(nodes, C, Ho))

    def fwd(k, d):
        A, Bm = new(d['X'], nodes, C, Ho), new(d['X'], nodes, C, Ho)
        k.node_post_fwd(d['X'], d['Tc'], d['W'], d['b'], A, Bm)
        return dict(A=A, Bm=Bm)

    def bwd(k, d):
        dX, dW, db = new(d['X'], nodes, C, L), new(d['W'], *d['W'].shape), new(d['W'], Ho)
        k.node_post_bwd(d['X'], d['Tc'], d['W'], d['dA'], d['dB'], dX, dW, db)
        return dict(dX=dX, dW=dW, db=db)

    case(Case('node_post_fwd', make, fwd, dict(A='rows', Bm='rows'), dict(X=('X', (20, 3, 4), False), W=('W', (5, 2), True))))
    case(Case('node_post_bwd', make, bwd, dict(dX='rows', dW='reduce', db='reduce'), dict(dA=('dA', (20, 3, 4), False), dB=('dB', (31, 0, 7), False), X=('X', (20, 3, 4), False))))


_node_post_cases()


def _mix_dT_case():
    nodes, C, L, Ho, K = 40, 5, 32, 16, 2

    def make():
        g = torch.Generator().manual_seed(nodes + C)
        rnd = lambda *s: torch.randn(*s, generator=g)
        return dict(Zs=[rnd(nodes, C, L) for _ in range(K)], W=rnd(K * K * L, Ho) / (K * K * L) ** 0.5, dY=rnd(nodes, C, Ho))

    def run(k, d):
        dT = new(d['W'], K, C, C)
        k.mix_dT(d['Zs'], d['W'], d['dY'], dT)
        return dict(dTc=dT[1:])

    case(Case('mix_dT', make, run, dict(dTc='reduce'), dict(Z=(('Zs', 1), (7, 2, 3), True), dY=('dY', (7, 2, 3), True))))


_mix_dT_case()


# ============================================================================================================== fused and planar cells
def _fused_cases(nodes, C, cin, K):
    h = 16
    Lw = cin + h
    L = Lw + (-Lw) % 4
    tag = f'n{nodes}_c{C}_in{cin}_k{K}'

    def make():
        g = torch.Generator().manual_seed(nodes + C + cin + K)
        rnd = lambda *s: torch.randn(*s, generator=g)
        Zs = [rnd(nodes, C, L) for _ in range(K)]
        for z in Zs:
            z[..., Lw:] = 0.0
        Tc = rnd(K, C, C) / C ** 0.5
        Tc[0] = torch.eye(C)
        return dict(Zs=Zs, Tc=Tc, H=rnd(nodes, C, h), Wg=rnd(K * K * Lw, 2 * h) / (K * K * Lw) ** 0.5, bg=rnd(2 * h), Wc=rnd(K * K * Lw, h) / (K * K * Lw) ** 0.5, bc=rnd(h),
                    U=torch.rand(nodes, C, h, generator=g), R=torch.rand(nodes, C, h, generator=g), Cand=torch.tanh(rnd(nodes, C, h)), dHn=rnd(nodes, C, h), dCand=rnd(nodes, C, L))

    def gates_fwd(k, d):
        U, R, Ci = new(d['H'], nodes, C, h), new(d['H'], nodes, C, h), new(d['H'], nodes, C, L)
        k.cell_gates_fwd(d['Zs'], d['Tc'], d['Wg'], d['bg'], d['H'], U, R, Ci)
        return dict(U=U, R=R, CandIn=Ci)

    def blend_fwd(k, d):
        Cand, Hn = new(d['H'], nodes, C, h), new(d['H'], nodes, C, h)
        k.cell_blend_fwd(d['Zs'], d['Tc'], d['Wc'], d['bc'], d['U'], d['H'], Cand, Hn)
        return dict(Cand=Cand, Hnew=Hn)

    def cand_bwd(k, d):
        dZ = [new(z, *z.shape) for z in d['Zs']]
        dW, db = new(d['Wc'], *d['Wc'].shape), new(d['Wc'], h)
        k.cell_cand_bwd(d['Zs'], d['Tc'], d['Wc'], d['dHn'], d['U'], d['Cand'], dZ, dW, db)
        return dict(dW=dW, db=db, **{f'dZ{i}': z for i, z in enumerate(dZ)})

    def gates_bwd(k, d):
        dZ = [new(z, *z.shape) for z in d['Zs']]
        dW, db, dH = new(d['Wg'], *d['Wg'].shape), new(d['Wg'], 2 * h), new(d['H'], nodes, C, h)
        k.cell_gates_bwd(d['Zs'], d['Tc'], d['Wg'], d['dCand'], None, d['H'], d['U'], d['R'], d['dHn'], dZ, dW, db, None, dH, dH_in_scaled=True, Cand=d['Cand'])
        return dict(dW=dW, db=db, dH=dH, **{f'dZ{i}': z for i, z in enumerate(dZ)})

    r = nodes // 2
    zk = {f'dZ{i}': 'rows' for i in range(K)}
    case(Case(f'cell_gates_fwd_{tag}', make, gates_fwd, dict(U='rows', R='rows', CandIn='rows'), dict(Z=(('Zs', 1), (r, 1, 2), False), H=('H', (r, 0, 3), False), bias=('bg', (5,), True))))
    case(Case(f'cell_blend_fwd_{tag}', make, blend_fwd, dict(Cand='rows', Hnew='rows'), dict(Z=(('Zs', 0), (r, 1, 2), False), U=('U', (r, 0, 3), False), H=('H', (1, 0, 3), False))))
    case(Case(f'cell_cand_bwd_{tag}', make, cand_bwd, dict(dW='reduce', db='reduce', **zk), dict(dHnew=('dHn', (r, 1, 2), False), U=('U', (r, 0, 3), False)), spread=pad_spread(Lw)))
    case(Case(f'cell_gates_bwd_{tag}', make, gates_bwd, dict(dW='reduce', db='reduce', dH='rows', **zk),
              dict(dHnew=('dHn', (r, 1, 2), False), dCandIn=('dCand', (r, 0, cin + 3), False), R=('R', (r, 0, 3), False)), spread=pad_spread(Lw)))


for _s in ((50, 32, 16, 2), (21, 16, 16, 3), (13, 64, 1, 2)):
    _fused_cases(*_s)
FUSED_CASES = [n for n in CASES if n.startswith('cell_') and '_in' in n]


def _planar_cases(nodes, C, cin):
    h, K = 16, 2
    tag = f'n{nodes}_c{C}_in{cin}'
    make = lambda: {k_: v for k_, v in _cell_case('zeros', nodes, cin, waves=1024, C=C).items()} | dict(
        bg=torch.randn(2 * h, generator=torch.Generator().manual_seed(nodes)), dRH=torch.randn(nodes, C, h, generator=torch.Generator().manual_seed(C)))

    def gates_fwd(k, d, with_amax=False):
        U, R, RH = (new(d['H'], nodes, C, h) for _ in range(3))
        am = k.act_amax_buffer(d['H'], 4) if with_amax else None
        k.cell_gates_fwd_planar(d['X'], d['H'], d['SX'], d['SH'], d['Tc'], d['Wg'], d['bg'], U, R, RH, act_amax=am)
        return dict(U=U, R=R, RH=RH)

    def gates_bwd(k, d):
        wide = cin == h
        dZ = [new(d['H'], nodes, C, h) if (wide or i >= 2) else None for i in range(4)]
        dW, db, dH = new(d['Wg'], *d['Wg'].shape), new(d['Wg'], 2 * h), new(d['H'], nodes, C, h)
        k.cell_gates_bwd_planar(d['X'], d['H'], d['SX'], d['SH'], d['Tc'], d['Wg'], d['dRH'], d['Cand'], d['U'], d['R'], d['dHn'], dZ, dW, db, dH)
        return dict(dW=dW, db=db, dH=dH, **{f'dZ{i}': z for i, z in enumerate(dZ)})

    r = nodes // 2
    case(Case(f'planar_gates_fwd_{tag}', make, gates_fwd, dict(U='rows', R='rows', RH='rows'), dict(SX=('SX', (r, 1, 0), False), H=('H', (r, 2, 5), False), W=('Wg', (3, 2), True)),
              default_tol=nf.GRAD_TOL))
    case(Case(f'planar_gates_fwd_amax_{tag}', make, lambda k, d: gates_fwd(k, d, True), dict(U='rows', R='rows', RH='rows'), dict(SH=('SH', (r, 1, 0), False)), default_tol=nf.GRAD_TOL))
    zk = {f'dZ{i}': 'rows' for i in range(4)}
    case(Case(f'planar_gates_bwd_{tag}', make, gates_bwd, dict(dW='reduce', db='reduce', dH='rows', **zk), dict(dHnew=('dHn', (r, 1, 2), False), dRH=('dRH', (r, 0, 3), False)),
              default_tol=nf.GRAD_TOL))


for _s in ((50, 32, 16), (13, 64, 16), (9, 32, 3)):
    _planar_cases(*_s)
PLANAR_CASES = [n for n in CASES if n.startswith('planar_')]


def _one_launch_case(name, nodes, cin, pattern, waves, accumulate, sites, values):
    """stc_cell_bwd_planar_f32 on tests/test_grad_scale.py's operands; accumulate: the planes hold another consumer's gradients."""
    def make():
        c = _cell_case(pattern, nodes, cin, waves=waves)
        if accumulate:
            g = torch.Generator().manual_seed(5)
            c['acc'] = [torch.randn(nodes, 32, 16, generator=g) for _ in range(4)]
        return c

    def run(k, d):
        dZ, par = _cell_bwd(k, d, lambda t: t, acc=d.get('acc'))
        return dict(par, **{f'dZ{i}': z for i, z in enumerate(dZ)})

    kinds = dict(dWg='reduce', dbg='reduce', dWc='reduce', dbc='reduce', **{f'dZ{i}': 'rows' for i in range(4)})
    return case(Case(name, make, run, kinds, sites, default_tol=nf.GRAD_TOL, values=values))


_SMALL_SITES = dict(dHnew=('dHn', (25, 3, 4), False), dBm=('dBm', (25, 3, 4), False), H=('H', (25, 3, 4), False), SX=('SX', (25, 3, 0), False))
for _cin in (16, 1):
    _one_launch_case(f'cell_bwd_planar_in{_cin}', 50, _cin, 'zeros', 1024, False, _SMALL_SITES, {})
    _one_launch_case(f'cell_bwd_planar_acc_in{_cin}', 50, _cin, 'zeros', 1024, True, _SMALL_SITES, {})
ONE_LAUNCH_CASES = [n for n in CASES if n.startswith('cell_bwd_planar')]

# RunScale with a non-finite node (csrc/stc_x3_frag.h): 9 000 nodes = 8-9 per wave; node 4 * 1024 + 17 is the fifth node of wave 17.  An Inf maximum
# has exponent 255: the node takes the smallest scale (kn clamps to -100) for its own fragments, ends no pass and sets NO new reference -- the
# wave's later nodes keep the scales of the clean run (a restart at the smallest reference changed the rounding of their planes)
RUNSCALE_NODE = 4 * 1024 + 17
_RS_SITES = dict(dHnew_nan=('dHn', (RUNSCALE_NODE, 3, 4), False), dHnew_inf=('dHn', (RUNSCALE_NODE, 3, 4), False), dBm_inf=('dBm', (RUNSCALE_NODE, 3, 4), False))
_RS_VALUES = dict(dHnew_nan=('nan',), dHnew_inf=('+inf', '-inf'), dBm_inf=('+inf',))
_one_launch_case('runscale_plain', 9000, 16, 'ramp', 1024, False, _RS_SITES, _RS_VALUES)
_one_launch_case('runscale_accumulate', 9000, 16, 'ramp', 1024, True, _RS_SITES, _RS_VALUES)
# CPU stand-ins of the two: 48 nodes over four emulated waves, node 4 * 4 + 1 is the fifth node of wave 1
_CPU_RS_SITES = {k_: (v[0], (17, 3, 4), False) for k_, v in _RS_SITES.items()}
_one_launch_case('runscale_emulated_plain', 48, 16, 'ramp', 4, False, _CPU_RS_SITES, _RS_VALUES)
_one_launch_case('runscale_emulated_accumulate', 48, 16, 'ramp', 4, True, _CPU_RS_SITES, _RS_VALUES)
RUNSCALE_GPU = ['runscale_plain', 'runscale_accumulate']
RUNSCALE_CPU = ['runscale_emulated_plain', 'runscale_emulated_accumulate']


def _planes(k, like, shape, n, have=True):
    return [new(like, *shape) if have else None for _ in range(n)]


def _two_launch_cases(tag, nodes, C, pattern, r, values=None):
    """The C = 64 cells' backward: stc_cell_gates_bwd_planar_f32 and stc_bdg_node_post_bwd_f32 (tests/test_grad_scale.py's operands)."""
    h, K = 16, 2

    def make():
        g = torch.Generator().manual_seed(C)
        rnd = lambda *s_: torch.randn(*s_, generator=g)
        X, H, SX, SH = rnd(nodes, C, h), torch.tanh(rnd(nodes, C, h)), rnd(nodes, C, h), rnd(nodes, C, h)
        Tc = rnd(K, C, C) / C ** 0.5
        Tc[0] = torch.eye(C)
        Wg, Wc = rnd(K * K * 2 * h, 2 * h) / (8 * h) ** 0.5, rnd(K * K * 2 * h, h) / (8 * h) ** 0.5
        U, R, Cand = torch.sigmoid(rnd(nodes, C, h)), torch.sigmoid(rnd(nodes, C, h)), torch.tanh(rnd(nodes, C, h))
        f = node_factors(pattern, nodes, 1024).float().view(-1, 1, 1)
        return dict(X=X, H=H, SX=SX, SH=SH, Tc=Tc, Wg=Wg, Wc=Wc, U=U, R=R, Cand=Cand, RH=R * H, dRH=rnd(nodes, C, h) * f, dHn=rnd(nodes, C, h) * f,
                    dA=rnd(nodes, C, h) * f, dB=rnd(nodes, C, h) * f)

    def gates(k, d):
        dZ = _planes(k, d['X'], (nodes, C, h), 4)
        dW, db = new(d['Wg'], *d['Wg'].shape), new(d['Wg'], 2 * h)
        k.cell_gates_bwd_planar(*[d[n] for n in ('X', 'H', 'SX', 'SH', 'Tc', 'Wg', 'dRH', 'Cand', 'U', 'R', 'dHn')], dZ, dW, db, None)
        return dict(dW=dW, db=db, **{f'dZ{i}': z for i, z in enumerate(dZ)})

    def post(k, d):
        dX, dX2 = _planes(k, d['X'], (nodes, C, h), 2)
        dW, db = new(d['Wc'], *d['Wc'].shape), new(d['Wc'], h)
        k.node_post_bwd(d['X'], d['Tc'], d['Wc'], d['dA'], d['dB'], dX, dW, db, X2=d['RH'], dX2=dX2)
        return dict(dW=dW, db=db, dZ0=dX, dZ1=dX2)

    at = (r, 3, 4)
    kg = dict(dW='reduce', db='reduce', **{f'dZ{i}': 'rows' for i in range(4)})
    case(Case(f'{tag}_gates', make, gates, kg, dict(dHnew=('dHn', at, False), dRH=('dRH', at, False)), default_tol=nf.GRAD_TOL, values=values))
    case(Case(f'{tag}_post', make, post, dict(dW='reduce', db='reduce', dZ0='rows', dZ1='rows'), dict(dA=('dA', at, False), dB=('dB', at, False)), default_tol=nf.GRAD_TOL,
              values=values))


def _order3_cases(tag, nodes, cin, pattern, r, values=None, backward_only=False):
    """Order-3 planar cell kernels (stc_cell_{gates,cand}_{fwd,bwd}_planar_k_f32): three Chebyshev planes per side."""
    h, K, C = 16, 3, 32
    Lw = cin + h
    wide = cin == h

    def make():
        g = torch.Generator().manual_seed(nodes + cin)
        rnd = lambda *s_: torch.randn(*s_, generator=g)
        Zx, Zh, Zr = [rnd(nodes, C, cin) for _ in range(K)], [rnd(nodes, C, h) for _ in range(K)], [rnd(nodes, C, h) for _ in range(K)]
        Tc = rnd(K, C, C) / C ** 0.5
        Tc[0] = torch.eye(C)
        f = node_factors(pattern, nodes, 1024).float().view(-1, 1, 1)
        return dict(Zx=Zx, Zh=Zh, Zr=Zr, Tc=Tc, Wg=rnd(K * K * Lw, 2 * h) / (K * K * Lw) ** 0.5, bg=rnd(2 * h), Wc=rnd(K * K * Lw, h) / (K * K * Lw) ** 0.5, bc=rnd(h),
                    U=torch.sigmoid(rnd(nodes, C, h)), R=torch.sigmoid(rnd(nodes, C, h)), Cand=torch.tanh(rnd(nodes, C, h)), dHn=rnd(nodes, C, h) * f, dRH=rnd(nodes, C, h) * f,
                    acc=[rnd(nodes, C, cin) for _ in range(K)])

    def gates_fwd(k, d):
        U, R, RH = _planes(k, d['U'], (nodes, C, h), 3)
        k.cell_gates_fwd_planar_k(d['Zx'], d['Zh'], d['Tc'], d['Wg'], d['bg'], U, R, RH)
        return dict(U=U, R=R, RH=RH)

    def cand_fwd(k, d):
        Cand, Hn = _planes(k, d['U'], (nodes, C, h), 2)
        k.cell_cand_fwd_planar_k(d['Zx'], d['Zr'], d['Tc'], d['Wc'], d['bc'], d['U'], d['Zh'][0], Cand, Hn)
        return dict(Cand=Cand, Hnew=Hn)

    def cand_bwd(k, d):
        dXs, dHs = _planes(k, d['U'], (nodes, C, cin), K, wide), _planes(k, d['U'], (nodes, C, h), K)
        dW, db = new(d['Wc'], *d['Wc'].shape), new(d['Wc'], h)
        k.cell_cand_bwd_planar_k(d['Zx'], d['Zr'], d['Tc'], d['Wc'], d['dHn'], d['U'], d['Cand'], dXs, dHs, dW, db)
        return dict(dW=dW, db=db, **{f'dZh{i}': z for i, z in enumerate(dHs)}, **{f'dZx{i}': z for i, z in enumerate(dXs)})

    def gates_bwd(k, d):                                                    # accumulate_x (wide input): the X-side planes hold the candidate's gradients
        dXs = [t.clone() for t in d['acc']] if wide else [None] * K
        dHs = _planes(k, d['U'], (nodes, C, h), K)
        dW, db = new(d['Wg'], *d['Wg'].shape), new(d['Wg'], 2 * h)
        k.cell_gates_bwd_planar_k(d['Zx'], d['Zh'], d['Tc'], d['Wg'], d['dRH'], d['Cand'], d['U'], d['R'], d['dHn'], dXs, dHs, dW, db, None, accumulate_x=wide)
        return dict(dW=dW, db=db, **{f'dZh{i}': z for i, z in enumerate(dHs)}, **{f'dZx{i}': z for i, z in enumerate(dXs)})

    at = (r, 3, 4)
    kb = dict(dW='reduce', db='reduce', **{f'dZh{i}': 'rows' for i in range(K)}, **{f'dZx{i}': 'rows' for i in range(K)})
    if not backward_only:
        case(Case(f'{tag}_gates_fwd', make, gates_fwd, dict(U='rows', R='rows', RH='rows'), dict(Zh=(('Zh', 1), at, False), Zx=(('Zx', 2), (r, 3, 0), False), W=('Wg', (3, 2), True)),
                  default_tol=nf.GRAD_TOL))
        case(Case(f'{tag}_cand_fwd', make, cand_fwd, dict(Cand='rows', Hnew='rows'), dict(Zr=(('Zr', 1), at, False), U=('U', at, False)), default_tol=nf.GRAD_TOL))
    case(Case(f'{tag}_cand_bwd', make, cand_bwd, kb, dict(dHnew=('dHn', at, False)), default_tol=nf.GRAD_TOL, values=values))
    case(Case(f'{tag}_gates_bwd', make, gates_bwd, kb, dict(dHnew=('dHn', at, False), dRH=('dRH', at, False)), default_tol=nf.GRAD_TOL, values=values))


_before = set(CASES)
_two_launch_cases('two_launch_c64', 13, 64, 'zeros', 6)
_order3_cases('planar_k_n50_in16', 50, 16, 'zeros', 25)
_order3_cases('planar_k_n37_in1', 37, 1, 'zeros', 18)
SMALL_F32_FORMAT_CASES = [n for n in CASES if n not in _before]          # run under both operand formats on the GPU
_before = set(CASES)
_INF_ONLY = dict(dHnew=('+inf',), dRH=('-inf',), dA=('-inf',), dB=('+inf',))      # (one value per site: 9 000 nodes of C = 64 in float64 are not cheap)
_two_launch_cases('runscale_c64', 9000, 64, 'ramp', RUNSCALE_NODE, values=_INF_ONLY)
_order3_cases('runscale_k3', 9000, 16, 'ramp', RUNSCALE_NODE, values=_INF_ONLY, backward_only=True)
RUNSCALE_GPU += [n for n in CASES if n not in _before]


def _bf16_planar_cases(nodes, C, cin):
    """bf16 planes (state / gate / gradient planes bfloat16, weights and their gradients fp32): gates forward and the backward in one launch."""
    h, K = 16, 2
    bf = torch.bfloat16
    tag = f'bf16_planar_n{nodes}_c{C}_in{cin}'
    PLANES = ('X', 'H', 'SX', 'SH', 'U', 'R', 'Cand', 'dHn', 'dBm')

    def make():
        c = _cell_case('zeros', nodes, cin, waves=1024, C=C)
        c['bg'] = torch.randn(2 * h, generator=torch.Generator().manual_seed(nodes))
        return {k_: (v.to(bf) if k_ in PLANES else v) for k_, v in c.items()}

    def on(k, d):
        return k.bf16 if d['H'].dtype == bf else k                           # (want: float64 math on the bf16-valued planes)

    def gates_fwd(k, d):
        U, R, RH = _planes(k, d['H'], (nodes, C, h), 3)
        on(k, d).cell_gates_fwd_planar(d['X'], d['H'], d['SX'], d['SH'], d['Tc'], d['Wg'], d['bg'], U, R, RH)
        return dict(U=U, R=R, RH=RH)

    def bwd(k, d):
        wide = cin == h
        dZ = [new(d['H'], nodes, C, h) if (wide or i >= 2) else None for i in range(4)]
        dWg, dbg, dWc, dbc = new(d['Wg'], *d['Wg'].shape), new(d['Wg'], 2 * h), new(d['Wc'], *d['Wc'].shape), new(d['Wc'], h)
        on(k, d).cell_bwd_planar(*[d[n] for n in ('X', 'H', 'SX', 'SH', 'Tc', 'Wg', 'Wc', 'U', 'R', 'Cand', 'dHn', 'dBm')], dZ, dWg, dbg, dWc, dbc)
        return dict(dWg=dWg, dbg=dbg, dWc=dWc, dbc=dbc, **{f'dZ{i}': z for i, z in enumerate(dZ)})

    r = nodes // 2
    case(Case(f'{tag}_gates_fwd', make, gates_fwd, dict(U='rows', R='rows', RH='rows'), dict(SX=('SX', (r, 1, 0), False), H=('H', (r, 2, 5), False)), default_tol=nf.BF16_TOL))
    kinds = dict(dWg='reduce', dbg='reduce', dWc='reduce', dbc='reduce', **{f'dZ{i}': 'rows' for i in range(4)})
    case(Case(f'{tag}_bwd', make, bwd, kinds, dict(dHnew=('dHn', (r, 1, 2), False), dBm=('dBm', (r, 0, 3), False)), default_tol=nf.BF16_TOL))


_before = set(CASES)
for _s in ((50, 32, 16), (13, 64, 16), (9, 32, 3)):
    _bf16_planar_cases(*_s)
BF16_PLANAR_CASES = [n for n in CASES if n not in _before]


def _first_step_cases(nodes, cin):
    """First-step forms (zero initial state): the general entry points on explicit planes of zeros are the restatement.  The forms' shortcut
    x * 0 := 0 writes exact zeros -- the H rows of both weight gradients, the reset-gate half of dWg / dbg -- where the general kernels on zero
    planes form NaN * 0 = NaN from a non-finite gradient; likewise what reaches a result only through R * H or dR (factor H = 0).  Those entries, and
    only those, are exempt from part A -- site by site -- and for a NaN pinned to the clean run's value, bit for bit (an Inf gives its node the
    smallest activation scale of the fp16 x 2 format: the node's exempt entries are then finite without meaning; its U and new state are non-finite)."""
    h, K, C = 16, 2, 32
    Lw = cin + h
    wide = cin == h
    tag = f'first_step_n{nodes}_in{cin}'

    def make():
        c = _cell_case('zeros', nodes, cin, waves=1024)
        c['bg'], c['bc'] = (torch.randn(w, generator=torch.Generator().manual_seed(nodes + w)) for w in (2 * h, h))
        c['H'], c['SH'] = torch.zeros_like(c['H']), torch.zeros_like(c['SH'])
        return c

    def fwd(k, d):
        U, A, Bm = _planes(k, d['U'], (nodes, C, h), 3)
        if is_twin(k):
            Rg = torch.empty_like(U)
            k.cell_gates_fwd_planar(d['X'], d['H'], d['SX'], d['SH'], d['Tc'], d['Wg'], d['bg'], U, Rg, None, post=(d['Wc'], d['bc'], A, Bm))
        else:
            k.cell_gates_fwd_first(d['X'], d['SX'], d['Tc'], d['Wg'], d['bg'], U, (d['Wc'], d['bc'], A, Bm))
        return dict(U=U, A=A, Bm=Bm)

    def bwd(k, d):
        dX = _planes(k, d['U'], (nodes, C, h), 2, wide)
        dWg, dbg, dWc, dbc = new(d['Wg'], *d['Wg'].shape), new(d['Wg'], 2 * h), new(d['Wc'], *d['Wc'].shape), new(d['Wc'], h)
        if is_twin(k):
            dZ = dX + _planes(k, d['U'], (nodes, C, h), 2)
            k.cell_bwd_planar(*[d[n] for n in ('X', 'H', 'SX', 'SH', 'Tc', 'Wg', 'Wc', 'U', 'R', 'Cand', 'dHn', 'dBm')], dZ, dWg, dbg, dWc, dbc)
        else:
            k.cell_bwd_first(*[d[n] for n in ('X', 'SX', 'Tc', 'Wg', 'Wc', 'U', 'Cand', 'dHn', 'dBm')], dX, dWg, dbg, dWc, dbc)
        return dict(dWg=dWg, dbg=dbg, dWc=dWc, dbc=dbc, dX=dX[0], dSX=dX[1])

    h_rows_g, h_rows_c = torch.zeros(4, Lw, 2 * h, dtype=torch.bool), torch.zeros(4, Lw, h, dtype=torch.bool)
    h_rows_g[:, cin:] = True
    h_rows_g[:, :, h:] = True
    h_rows_c[:, cin:] = True
    reset = torch.zeros(2 * h, dtype=torch.bool)
    reset[h:] = True
    # backward, every site: the zero rows / columns of the weight gradients; a poison that arrives through the reset gate only (dBm -> d(R*H) -> dR,
    # which carries the factor H = 0) also leaves dSX at the clean value.  Forward: S.X reaches the candidate's A, Bm only through R * H = R * 0.
    exempt_b = {'*': dict(dWg=h_rows_g.view(4 * Lw, 2 * h), dWc=h_rows_c.view(4 * Lw, h), dbg=reset), 'dBm': dict(dSX=True)}
    exempt_f = {'SX': dict(A=True, Bm=True)}
    r = nodes // 2
    case(Case(f'{tag}_fwd', make, fwd, dict(U='rows', A='rows', Bm='rows'), dict(X=('X', (r, 1, 0), False), SX=('SX', (r, 2, 0), False)), default_tol=nf.GRAD_TOL,
              exempt=exempt_f))
    case(Case(f'{tag}_bwd', make, bwd, dict(dWg='reduce', dbg='reduce', dWc='reduce', dbc='reduce', dX='rows', dSX='rows'),
              dict(dHnew=('dHn', (r, 1, 2), False), dBm=('dBm', (r, 0, 3), False), SX=('SX', (r, 2, 0), False)), default_tol=nf.GRAD_TOL, exempt=exempt_b))


_before = set(CASES)
for _s in ((5, 16), (1030, 16), (5, 1), (1030, 1)):
    _first_step_cases(*_s)
FIRST_STEP_CASES = [n for n in CASES if n not in _before]


# ============================================================================================================== few-category cells
def _sample_spread(c, name, touched):
    """One workgroup (or one group of workgroups) per sample: the sample is the spread unit of the few-category cell kernels."""
    hit = touched.flatten(1).any(1)
    return touched | hit.view(-1, *([1] * (touched.dim() - 1)))


def _small_cell_case(tag, B, N, C, cin, K=2, dense=False, splits=1):
    """stc_cell_small_fwd/bwd_f32 through tests/test_small_cell.py's own driver: a cell step forward and backward; the parameter-gradient
    partials are compared as the sums the caller forms (the kernels spread them over the rows of a sample's group, the twin adds to the first)."""
    from stc_hip.graph import csr_operand, dense_operand
    from tests import test_small_cell as S
    PLANES = ('U', 'R', 'RH', 'Zg', 'Zc', 'Cand', 'Hnew', 'dX', 'dH') + (('Zg2', 'Zc2') if K == 3 else ())

    def make():
        t = S._inputs(B, N, C, cin, seed=3 * N + C + cin, K=K)
        del t['Gc']
        return t

    def run(k, d):
        dev, dt = d['H'].device, d['H'].dtype
        graph = S._graph(N, seed=N + cin, dense=dense)
        op = dense_operand(graph.to_dense().to(dev)) if dense else csr_operand(graph, dev)
        buf, P = S._buffers(B, N, C, cin, dt, k, K=K)
        out = S._run(k, op, d, buf, P, lambda v: v.to(device=dev, dtype=dt), splits=1 if is_twin(k) else splits)
        extra = 0.125 * (out['dP'].shape[0] - 1)                             # every row of the partials starts at 0.125
        dWg, dbg, dWc, dbc = (p - extra for p in S._split_params(out['dP'], cin, K=K)[:4])
        return dict(dWg=dWg, dbg=dbg, dWc=dWc, dbc=dbc, **{n: out[n] for n in PLANES})

    kinds = dict(dWg='reduce', dbg='reduce', dWc='reduce', dbc='reduce', **{n: 'rows' for n in PLANES})
    at = (0, N // 2, 1, 0)
    sites = dict(X=('X', at, False), H=('H', at, False), dHnew=('dHnew', at, False), W=('Wg', (3, 2), True))
    case(Case(f'cell_small_{tag}', make, run, kinds, sites, spread=_sample_spread, tols=dict(dWg=nf.GRAD_TOL, dbg=nf.GRAD_TOL, dWc=nf.GRAD_TOL, dbc=nf.GRAD_TOL)))


_before = set(CASES)
_small_cell_case('b2_n9_c4_in16', 2, 9, 4, 16)
_small_cell_case('b3_n12_c5_in1', 3, 12, 5, 1)
_small_cell_case('b2_n37_c8_in3_split2', 2, 37, 8, 3, splits=2)
_small_cell_case('b2_n9_c4_in16_dense', 2, 9, 4, 16, dense=True)
_small_cell_case('b2_n9_c4_in16_k3', 2, 9, 4, 16, K=3)


def _graph_grad_case():
    cells, B, N, C, wa, wb, sel = 4, 2, 37, 8, 20, 32, (0, 3, 2)

    def make():
        g = torch.Generator().manual_seed(cells * N + wa)
        return dict(A=torch.randn(cells, B, N * C, wa, generator=g), Bm=torch.randn(cells, B, N * C, wa, generator=g), Bn=torch.randn(cells, B, N * C, wb, generator=g))

    def run(k, d):
        f = (lambda t: t.float()) if is_twin(k) and d['A'].dtype == torch.float64 else (lambda t: t)     # (the twin sums in float64 itself)
        return dict(dGs=k.graph_grad(f(d['A']), f(d['Bm']), *sel, N), dGc=k.mix_grad(f(d['A']), f(d['Bn']), *sel, N))

    # sums over the selected cells and samples: A[cell, b, (n, c), w] reaches row n of dGs and row (c, w) of dGc; an unselected cell reaches nothing
    at = (3, 1, 5 * C + 2, 7)
    case(Case('graph_grad_mix_grad', make, run, dict(dGs='rows', dGc='rows'), dict(A=('A', at, False), Bm=('Bm', at, False), Bn=('Bn', at, False)), coverage=False,
              default_tol=1e-6))


_graph_grad_case()
SMALL_CELL_CASES = [n for n in CASES if n not in _before]


# ============================================================================================================== elementwise kernels, head, optimizer
def _gru_cases():
    rows, cin, h = (3, 50, 5), 16, 16

    def make():
        g = torch.Generator().manual_seed(cin * 100 + h)
        rnd = lambda *s: torch.randn(*s, generator=g)
        return dict(G=rnd(*rows, 2 * h), Xt=rnd(*rows, cin), H=rnd(*rows, h), U=torch.rand(*rows, h, generator=g), R=torch.rand(*rows, h, generator=g), dCi=rnd(*rows, cin + h),
                    dU=rnd(*rows, h), Cpre=2 * rnd(*rows, h), Cand=torch.tanh(rnd(*rows, h)), dHn=rnd(*rows, h))

    def gates_fwd(k, d):
        U, R, Ci = new(d['H'], *rows, h), new(d['H'], *rows, h), new(d['H'], *rows, cin + h)
        k.gru_gates_fwd(d['G'], d['Xt'], d['H'], U, R, Ci)
        return dict(U=U, R=R, CandIn=Ci)

    def gates_bwd(k, d):
        dG, dX, dH = new(d['H'], *rows, 2 * h), new(d['H'], *rows, cin), new(d['H'], *rows, h)
        k.gru_gates_bwd(d['dCi'], d['dU'], d['H'], d['U'], d['R'], dG, dX, dH)
        return dict(dG=dG, dXt=dX, dH=dH)

    def blend_fwd(k, d):
        Cand, Hn = new(d['H'], *rows, h), new(d['H'], *rows, h)
        k.gru_blend_fwd(d['Cpre'], d['U'], d['H'], Cand, Hn)
        return dict(Cand=Cand, Hnew=Hn)

    def blend_bwd(k, d):
        outs = [new(d['H'], *rows, h) for _ in range(3)]
        k.gru_blend_bwd(d['dHn'], d['U'], d['H'], d['Cand'], *outs)
        return dict(dCpre=outs[0], dU=outs[1], dH=outs[2])

    at = (1, 20, 3, 4)
    case(Case('gru_gates_fwd', make, gates_fwd, dict(U='rows', R='rows', CandIn='rows'), dict(G=('G', at, False), G_reset=('G', (1, 20, 3, h + 4), False), Xt=('Xt', at, False), H=('H', at, False))))
    case(Case('gru_gates_bwd', make, gates_bwd, dict(dG='rows', dXt='rows', dH='rows'), dict(dCandIn=('dCi', (1, 20, 3, cin + 4), False), dU=('dU', at, False), R=('R', at, False))))
    case(Case('gru_blend_fwd', make, blend_fwd, dict(Cand='rows', Hnew='rows'), dict(Cpre=('Cpre', at, False), U=('U', at, False), H=('H', at, False))))
    case(Case('gru_blend_bwd', make, blend_bwd, dict(dCpre='rows', dU='rows', dH='rows'), dict(dHnew=('dHn', at, False), Cand=('Cand', at, False))))


_gru_cases()


def _head_cases(dt, h):
    shape = (3, 7)
    tag = 'f32' if dt == torch.float32 else 'bf16'

    def make():
        g = torch.Generator().manual_seed(h + 2)
        H = torch.randn(*shape, h, generator=g).to(dt)
        w, b = torch.randn(h, generator=g) * 0.5, torch.randn(1, generator=g)
        y = torch.sigmoid(H.float() @ w + b)
        return dict(H=H, w=w, b=b, y=y, dy=torch.randn(*shape, generator=g))

    def fwd(k, d):
        y = new(d['w'], *shape)
        k.head_fwd(d['H'], d['w'], d['b'], y)
        return dict(y=y)

    def bwd(k, d):
        dH, dwb = new(d['H'], *shape, h), new(d['w'], h + 1)
        k.head_bwd(d['H'], d['w'], d['y'], d['dy'], dH, dwb)
        return dict(dH=dH, dwb=dwb)

    tol = nf.F32_TOL if dt == torch.float32 else nf.BF16_TOL
    case(Case(f'head_fwd_{tag}', make, fwd, dict(y='rows'), dict(H=('H', (1, 2, 5), False), w=('w', (3,), True)), default_tol=tol))
    case(Case(f'head_bwd_{tag}', make, bwd, dict(dH='rows', dwb='reduce'), dict(dy=('dy', (1, 2), False), y=('y', (2, 4), False), H=('H', (1, 2, 5), False)), tols=dict(dwb=nf.GRAD_TOL),
              default_tol=tol))


_head_cases(torch.float32, 64)
_head_cases(torch.bfloat16, 16)

ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-3)


def _adam_case():
    n = 1000

    def make():
        g = torch.Generator().manual_seed(n)
        rnd = lambda: torch.randn(n, generator=g)
        return dict(p=rnd(), g=rnd(), m=0.1 * rnd(), v=0.01 * rnd().abs())

    def run(k, d):
        p, m, v = d['p'].clone(), d['m'].clone(), d['v'].clone()
        if is_twin(k):                                                      # torch.optim.Adam's arithmetic, L2 weight decay, step 3
            g = d['g'] + ADAM['weight_decay'] * p
            m.mul_(ADAM['beta1']).add_(g, alpha=1 - ADAM['beta1'])
            v.mul_(ADAM['beta2']).addcmul_(g, g, value=1 - ADAM['beta2'])
            denom = v.sqrt() / (1 - ADAM['beta2'] ** 3) ** 0.5 + ADAM['eps']
            p.addcdiv_(m, denom, value=-ADAM['lr'] / (1 - ADAM['beta1'] ** 3))
        else:
            k.adam(p, d['g'], m, v, torch.tensor([3.0], device=p.device), **ADAM)
        return dict(p=p, m=m, v=v)

    # (elementwise: pinned tighter than part D asks -- every other element is held to B and C)
    case(Case('adam', make, run, dict(p='rows', m='rows', v='rows'), dict(g=('g', (123,), False), v=('v', (456,), False))))


_adam_case()


def _helper_cases():
    def make():
        g = torch.Generator().manual_seed(3)
        rnd = lambda *s: torch.randn(*s, generator=g)
        return dict(x=rnd(1000), y=rnd(1000), A=rnd(4, 9, 3, 1), Bm=rnd(4, 9, 3, 16), src=rnd(4, 9, 3, 20), addA=rnd(4, 9, 3, 1), addB=rnd(4, 9, 3, 16))

    def axpy(k, d):
        y = d['y'].clone()
        k.axpy(-1.0, d['x'], y)
        return dict(y=y)

    def concat(k, d):
        out = new(d['A'], 4, 9, 3, 20)
        k.concat2(d['A'], d['Bm'], out)
        return dict(out=out)

    def split(k, d):
        A, Bm = d['addA'].clone(), d['addB'].clone()
        k.split2(d['src'], A, Bm, addA=A, addB=Bm)
        return dict(A=A, Bm=Bm)

    case(Case('axpy', make, axpy, dict(y='rows'), dict(x=('x', (17,), False), y=('y', (900,), False))))
    case(Case('concat2', make, concat, dict(out='rows'), dict(A=('A', (2, 3, 1, 0), False), Bm=('Bm', (2, 3, 1, 9), False))))
    case(Case('split2', make, split, dict(A='rows', Bm='rows'), dict(src=('src', (2, 3, 1, 9), False), addA=('addA', (1, 1, 1, 0), False))))


_helper_cases()


# ============================================================================================================== learned-graph generator
def _mgp_x(X, rows_axis):
    B, T, N, C = X.shape
    x = X.reshape(B * T, N, C)
    return x if rows_axis == 2 else x.transpose(1, 2)                      # x[k][r][f]


def softmax_relu(P, relu=torch.relu):
    """MGP_Gen's last line (reference STC_GNN.py:232): ``relu`` is replaced by the negative control."""
    return torch.softmax(relu(P - P.t()), dim=-1)


def _mgp_cases(rows_axis):
    B, T, N, C, h = 2, 3, 7, 3, 4
    R, F = (N, C) if rows_axis == 2 else (C, N)
    tag = f'rows_axis{rows_axis}'

    def make():
        g = torch.Generator().manual_seed(B * 1000 + N + rows_axis)
        X = (torch.rand(B, T, N, C, generator=g) < 0.3).float()
        Wu, Wv = (torch.randn(F, h, generator=g) * (2.0 / (F + h)) ** 0.5 for _ in range(2))
        U, V = (torch.tanh(3.0 * _mgp_x(X, rows_axis) @ w).permute(1, 0, 2).contiguous() for w in (Wu, Wv))
        return dict(X=X, Wu=Wu, Wv=Wv, U=U, V=V, dU=torch.randn(R, B * T, h, generator=g), dV=torch.randn(R, B * T, h, generator=g), P=torch.randn(R, R, generator=g),
                    dPs=torch.randn(R, R, generator=g))

    def uv_fwd(k, d):
        if is_twin(k):
            x = _mgp_x(d['X'], rows_axis)
            U, V = (torch.tanh(3.0 * (x @ w)).permute(1, 0, 2).contiguous() for w in (d['Wu'], d['Wv']))
        else:
            U, V = k.mgp_uv_fwd(d['X'], rows_axis, d['Wu'], d['Wv'], 3.0)
        return dict(U=U, V=V)

    def uv_bwd(k, d):
        if is_twin(k):
            x = _mgp_x(d['X'], rows_axis)
            dWu, dWv = (3.0 * torch.einsum('krf,rkj->fj', x, (1 - t * t) * dt) for t, dt in ((d['U'], d['dU']), (d['V'], d['dV'])))
        else:
            dWu, dWv = k.mgp_uv_bwd(d['X'], rows_axis, d['U'], d['V'], d['dU'], d['dV'], 3.0)
        return dict(dWu=dWu, dWv=dWv)

    def softmax(k, d):
        if is_twin(k):
            P = d['P'].clone().requires_grad_()
            Ps = softmax_relu(P)
            (Ps * d['dPs']).sum().backward()
            return dict(Ps=Ps.detach(), dP=P.grad)
        Ps = k.mgp_softmax_fwd(d['P'])
        return dict(Ps=Ps, dP=k.mgp_softmax_bwd(d['P'], Ps, d['dPs']))

    xi = (1, 2, 4, 1)
    D0 = make()['P']
    D0 = D0 - D0.t()
    pos = tuple(int(v) for v in (D0 > 0).nonzero()[-1])                    # an entry that passes the relu: its gradient is not masked
    case(Case(f'mgp_uv_fwd_{tag}', make, uv_fwd, dict(U='rows', V='rows'), dict(X=('X', xi, False), Wu=('Wu', (1, 2), True))))
    case(Case(f'mgp_uv_bwd_{tag}', make, uv_bwd, dict(dWu='reduce', dWv='reduce'), dict(dU=('dU', (1, 2, 3), True), X=('X', xi, True), U=('U', (1, 2, 3), True))))
    # P - P^T is dense in both indices: P[n, m] reaches rows n and m of Ps, and rows AND columns n and m of dP (no row of dP stays clear)
    case(Case(f'mgp_softmax_{tag}', make, softmax, dict(Ps='rows', dP='rows'), dict(P=('P', pos, False), dPs=('dPs', pos, False)), coverage=False,
              tols=dict(dP=nf.GRAD_TOL)))


_mgp_cases(2)
_mgp_cases(3)
MGP_SOFTMAX = ['mgp_softmax_rows_axis2', 'mgp_softmax_rows_axis3']


def _mixed_fusion_case(want_dA):
    n = 10
    D = n * n

    def make():
        g = torch.Generator().manual_seed(n)
        A, P = torch.rand(n, n, generator=g), torch.softmax(torch.randn(n, n, generator=g), -1)
        WA, WP = (torch.randn(D, D, generator=g) * (1.0 / D) ** 0.5 for _ in range(2))
        bA, bP = (torch.randn(D, generator=g) * 0.1 for _ in range(2))
        return dict(A=A, P=P, WA=WA, WP=WP, bA=bA, bP=bP, dG=torch.randn(n, n, generator=g))

    def run(k, d):
        if is_twin(k):                                                      # the reference's own expression (STC_GNN.py:246-261) and its autograd
            leaves = {n_: d[n_].clone().requires_grad_() for n_ in ('A', 'P', 'WA', 'WP', 'bA', 'bP')}
            gate = torch.sigmoid(leaves['WA'] @ leaves['A'].reshape(D) + leaves['bA'] + leaves['WP'] @ leaves['P'].reshape(D) + leaves['bP']).reshape(n, n)
            G = gate * leaves['A'] + (1 - gate) * leaves['P']
            (G * d['dG']).sum().backward()
            out = dict(gate=gate.detach(), G=G.detach(), dWA=leaves['WA'].grad, dWP=leaves['WP'].grad, db=leaves['bA'].grad, dP=leaves['P'].grad)
            if want_dA:
                out['dA'] = leaves['A'].grad
            return out
        gate, G = k.mixed_fusion_fwd(d['WA'], d['bA'], d['WP'], d['bP'], d['A'], d['P'])
        dWA, dWP, db, dP, dA = k.mixed_fusion_bwd(d['WA'], d['WP'], d['A'], d['P'], gate, d['dG'], want_dA)
        out = dict(gate=gate, G=G, dWA=dWA, dWP=dWP, db=db, dP=dP)
        if want_dA:
            out['dA'] = dA
        return out

    kinds = dict(gate='rows', G='rows', dWA='reduce', dWP='reduce', db='reduce', dP='rows', dA='rows')
    tols = dict(dWA=nf.GRAD_TOL, dWP=nf.GRAD_TOL, db=nf.GRAD_TOL, dP=nf.GRAD_TOL, dA=nf.GRAD_TOL)
    # every gate reads all of A and P (W_A vec(A)): a poison there is a table poison; dG and a bias are elementwise
    sites = dict(A=('A', (2, 3), True), P=('P', (4, 5), True), dG=('dG', (2, 3), False), bias=('bA', (23,), False))
    case(Case('mixed_fusion_dA' if want_dA else 'mixed_fusion', make, run, kinds, sites, tols=tols, coverage=False))


_mixed_fusion_case(True)
_mixed_fusion_case(False)

GPU_ONLY_FORMS = RUNSCALE_GPU
CPU_CASES = [n for n in CASES if n not in GPU_ONLY_FORMS]


# ============================================================================================================== CPU part
@pytest.mark.parametrize('name,site', _ids(CPU_CASES))
def test_contract_on_the_cpu_twin(name, site, monkeypatch):
    """The twin in float32 as the code under test against its float64 run: poison placement, reach and self-checks of every case."""
    c = CASES[name]
    k = EM
    if name in RUNSCALE_CPU:                                               # the operand format emulated per wave: twelve nodes share a wave's sums
        k = EmulatedKernels(operand_format='f16x2')
        monkeypatch.setattr(k, 'GRAD_WAVES', 4, raising=False)
    c.check(k, on_cpu, site)


def test_control_fmaxf_relu_masks_the_nan():
    """Negative control for part A: the softmax restatement with fmaxf semantics (the kernel before this contract) turns a NaN in P into 0."""
    c = CASES['mgp_softmax_rows_axis2']
    fmax_relu = lambda D: torch.where(torch.isnan(D), torch.zeros_like(D), torch.relu(D))          # fmaxf(d, 0): the non-NaN operand

    def broken(k, d):
        P = d['P'].clone().requires_grad_()
        Ps = softmax_relu(P, relu=fmax_relu)
        (Ps * d['dPs']).sum().backward()
        return dict(Ps=Ps.detach(), dP=P.grad.nan_to_num(0.0))

    c.check(EM, on_cpu, 'P')                                              # (the honest restatement passes)
    with pytest.raises(nf.ContractFailure) as e:
        c.check(EM, on_cpu, 'P', run=broken)
    assert e.value.part == 'A'


def test_control_zero_weight_block_mates_break_containment():
    """Negative control for part B: a CSR product that multiplies explicit zeros for its whole 4-row block, claiming a spread unit of "none"."""
    c = CASES['csr_spmm_f32_F85']

    def blocked(k, d):
        n, (B, _, F) = d['rowptr'].numel() - 1, d['X'].shape
        dense = torch.zeros(n, n, dtype=d['X'].dtype)
        rows = torch.repeat_interleave(torch.arange(n), (d['rowptr'][1:] - d['rowptr'][:-1]).long())
        dense[rows, d['colidx'].long()] = d['val'].to(d['X'].dtype)
        Y = torch.empty(B, n, F, dtype=d['X'].dtype)
        for blk in nf.blocks_of(n, 4):
            cols = sorted(set(int(j) for r in blk for j in d['colidx'][d['rowptr'][r]:d['rowptr'][r + 1]]))
            Y[:, blk] = 2.0 * torch.einsum('rc,bcf->brf', dense[blk][:, cols], d['X'][:, cols]) if cols else 0.0
        return dict(Y=Y)

    with pytest.raises(nf.ContractFailure) as e:
        c.check(EM, on_cpu, 'X', run=blocked)
    assert e.value.part == 'B'
    blocked_case = Case('control', c.make, c.run, c.kinds, c.sites, spread=lambda c_, name, bad: nf.spread_groups(bad, 1, nf.blocks_of(33, 4)))
    blocked_case.check(EM, on_cpu, 'X', run=blocked)                      # ... and with the 4-row block declared, the same product passes


GATE_INPUTS = [0.0, 2.0 ** -130, 0.25 - 2.0 ** -26, 0.25, 0.25 + 2.0 ** -25, 16.0, 88.0, 104.0, 1e30, float('inf')]


def _gate_values():
    v = torch.tensor(GATE_INPUTS, dtype=torch.float32)
    return torch.cat([v, -v, torch.tensor([NAN])])                         # 21 pre-activations; 0.25 is the seam of stc_tanh (polynomial / exp2 form)


def _check_gate(got, fn, tag):
    x = _gate_values()
    want = fn(x.double())
    got = got.detach().cpu().double()
    fin = torch.isfinite(x)
    assert torch.isfinite(got[fin]).all() and float((got[fin] - want[fin]).abs().max() / want[fin].abs().max()) < nf.F32_TOL, tag
    inf = torch.isinf(x)
    assert torch.equal(got[inf], want[inf]), (tag, got[inf])               # +-Inf: exactly 1 / 0 (sigmoid), +-1 (tanh)
    assert torch.isnan(got[-1]), tag


def _gate_functions(k, to):
    x = _gate_values()
    n, h = x.numel(), 4
    G = x.view(n, 1).repeat(1, 2 * h)
    H, Xt = torch.ones(n, h), torch.zeros(n, 1)
    U, R, Ci = (to(torch.full(s, NAN)) for s in ((n, h), (n, h), (n, 1 + h)))
    k.gru_gates_fwd(to(G), to(Xt), to(H), U, R, Ci)
    for j in range(h):
        _check_gate(U[:, j], torch.sigmoid, 'update gate')
        _check_gate(R[:, j], torch.sigmoid, 'reset gate')
        _check_gate(Ci[:, 1 + j], torch.sigmoid, 'R * H with H = 1')
    Cand, Hn = to(torch.full((n, h), NAN)), to(torch.full((n, h), NAN))
    k.gru_blend_fwd(to(G[:, :h].contiguous()), to(torch.ones(n, h)), to(H), Cand, Hn)
    for j in range(h):
        _check_gate(Cand[:, j], torch.tanh, 'candidate')
        _check_gate(Hn[:, j], torch.tanh, 'new state with U = 1')
    # one fused epilogue: the gates of stc_cell_gates_fwd_f32 on zero slabs, the pre-activation is the bias (32 columns: 21 values, then zeros)
    nodes, C, L, K = 50, 32, 32, 2
    bias = torch.zeros(2 * 16)
    bias[:n] = x
    Zs = [torch.zeros(nodes, C, L) for _ in range(K)]
    Tc = torch.eye(C).repeat(K, 1, 1)
    W = torch.randn(K * K * L, 32, generator=torch.Generator().manual_seed(1))
    Uf, Rf, Cf = (to(torch.full(s, NAN)) for s in ((nodes, C, 16), (nodes, C, 16), (nodes, C, L)))
    k.cell_gates_fwd([to(z) for z in Zs], to(Tc), to(W), to(bias), to(torch.ones(nodes, C, 16)), Uf, Rf, Cf)
    both = torch.cat([Uf, Rf], -1).reshape(nodes * C, 32)
    for row in (0, nodes * C // 2, nodes * C - 1):
        _check_gate(both[row, :n], torch.sigmoid, 'fused epilogue')


def test_gate_functions_on_the_cpu_twin():
    _gate_functions(EM, lambda t: t)


# ============================================================================================================== module level (tools/probes/nan_robustness.py as tests)
MODULE_FAMILIES = {'c32': (32, 2), 'c64': (64, 2), 'c32k3': (32, 3), 'small': (5, 2)}


def _module_case(family):
    C, K = MODULE_FAMILIES[family]
    H, W, B, T, horizon = 12, 20, 2, 3, 2
    torch.manual_seed(0)
    graph = CsrGraph.queen_grid(H, W, normalize=True)
    model = M.STCGNN(H * W, C, K, K, 1, 16, 2, horizon, graph_mode='csr-fixed')
    g = torch.Generator().manual_seed(C + K)
    X = (torch.rand(B, T, H * W, C, generator=g) < 0.3).float()
    X[0, 1, 7, 3] = NAN                                                    # sample 0 only
    Y = (torch.rand(B, horizon, H * W, C, generator=g) < 0.3).float()
    return model, graph, X, Y, torch.softmax(torch.randn(C, C, generator=g), -1)


def _plain_loss(y_pred, y_true):
    """Squared error + the per-sample Dice term of the reference's loss: plain arithmetic, a NaN goes through (the BCE term of
    ``combo_loss`` refuses predictions outside [0, 1] instead of handing them on)."""
    B = y_pred.shape[0]
    num = 2 * (y_pred * y_true).reshape(B, -1).sum(-1)
    den = (y_pred + y_true).reshape(B, -1).sum(-1)
    return ((y_pred - y_true) ** 2).mean() + torch.mean(1 - num / den)


def _module_run(model, graph, X, Y, Gc, dev):
    model = model.to(dev)
    model.zero_grad(set_to_none=True)
    yhat = model(X_seq=X.to(dev), As=graph, Ac=Gc.to(dev))
    loss = _plain_loss(yhat, Y.to(dev))
    loss.backward()
    return yhat.detach().cpu(), float(loss.detach()), {k_: p.grad.detach().cpu() for k_, p in model.named_parameters()}


_TWIN_RUNS = {}


def _twin_run(family, monkeypatch):
    if family not in _TWIN_RUNS:
        monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
        _TWIN_RUNS[family] = _module_run(*_module_case(family), 'cpu')
    return _TWIN_RUNS[family]


@pytest.mark.parametrize('family', list(MODULE_FAMILIES))
def test_module_on_the_cpu_twin_flags_the_poisoned_sample(family, monkeypatch):
    """A NaN in sample 0 of X_seq through the host schedule on the CPU twin: NaN loss, every parameter gradient non-finite, sample 1 finite."""
    yhat, loss, grads = _twin_run(family, monkeypatch)
    assert loss != loss or abs(loss) == float('inf')
    assert not torch.isfinite(yhat[0]).all() and torch.isfinite(yhat[1]).all()
    assert all(not torch.isfinite(g).all() for g in grads.values()), [k_ for k_, g in grads.items() if torch.isfinite(g).all()]


def _generator_case():
    torch.manual_seed(5)
    gen = M.MGP_Gen(num_nodes=12, num_categories=4, hidden_dim=8)
    with torch.no_grad():
        gen.params_S['Wu'][1, 2] = NAN                                       # one projection weight of the spatial branch
    g = torch.Generator().manual_seed(1)
    X = (torch.rand(3, 4, 12, 4, generator=g) < 0.3).float()
    return gen, X, torch.rand(12, 12, generator=g), torch.rand(4, 4, generator=g)


def test_generator_torch_path_hands_a_nan_weight_on():
    """The module's own torch path (what the kernels replace): a NaN projection weight gives a NaN spatial graph and a NaN loss."""
    gen, X, As, Ac = _generator_case()
    Gs, Gc = gen(X, As, Ac)
    assert torch.isnan(Gs).all() and torch.isfinite(Gc).all() and torch.isnan(Gs.sum() + Gc.sum())


# ============================================================================================================== GPU part
@pytest.fixture(scope='module')
def hip():
    from stc_hip._lib import HipKernels
    return HipKernels()


def _timed(hip, fn):
    from stc_hip._lib import KernelTimer
    hip.timer = t = KernelTimer()
    try:
        fn()
    finally:
        hip.timer = None
    return set(t.summary())


_PLAIN = [n for n in CPU_CASES if n not in NODE_CASES + FUSED_CASES + PLANAR_CASES + ONE_LAUNCH_CASES + RUNSCALE_CPU + MGP_SOFTMAX + SMALL_F32_FORMAT_CASES + FIRST_STEP_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize('name,site', _ids(_PLAIN))
def test_contract_on_the_kernels(hip, monkeypatch, name, site):
    """Aggregation forms, node helpers, elementwise kernels, head, Adam, learned-graph front end, MixedFusion."""
    monkeypatch.setattr(hip, 'patch_min_items', 0, raising=False)          # (small launches go to the row-blocked kernel by default)
    c = CASES[name]
    if name in FORM_KERNEL:                                                # the case runs the form it is about
        assert _timed(hip, lambda: c.run(hip, on_gpu(c.operands))) == {FORM_KERNEL[name]}
    c.check(hip, on_gpu, site)


@pytest.mark.gpu
@pytest.mark.parametrize('name,site', _ids(MGP_SOFTMAX))
def test_mgp_softmax_hands_non_finite_values_on(hip, name, site):
    """stc_mgp_softmax_fwd/bwd_f32: a NaN or Inf in P (or in dPs) comes out as in torch's softmax(relu(P - P^T)) and its autograd -- with fmaxf
    as relu and max the graph came out finite (this test failed before the kernels took a NaN-propagating relu / max and the mask !(d <= 0))."""
    CASES[name].check(hip, on_gpu, site)


@pytest.fixture(params=['default', 'fp32-mfma', 'generic-only'])
def node_path(request, hip):
    hip.set_dispatch_level({'default': 0, 'fp32-mfma': 1, 'generic-only': 2}[request.param])
    yield request.param
    hip.set_dispatch_level(0)


@pytest.fixture(params=['default', 'fp32-mfma'])
def fused_path(request, hip):
    hip.set_dispatch_level({'default': 0, 'fp32-mfma': 1}[request.param])
    yield request.param
    hip.set_dispatch_level(0)


@pytest.fixture(params=['f16x2', 'bf16x3'])
def operand_format(request, hip, monkeypatch):
    from stc_hip import _lib
    monkeypatch.setattr(hip, 'operand_format', {'f16x2': _lib.FMT_F16X2, 'bf16x3': _lib.FMT_BF16X3}[request.param], raising=False)
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize('name,site', _ids(NODE_CASES))
def test_contract_on_the_node_kernels(hip, node_path, name, site):
    """stc_bdg_node_fwd/bwd_f32 at all three dispatch levels: node-local, no spread unit."""
    CASES[name].check(hip, on_gpu, site)


@pytest.mark.gpu
@pytest.mark.parametrize('name,site', _ids(FUSED_CASES))
def test_contract_on_the_fused_cell_kernels(hip, fused_path, name, site):
    CASES[name].check(hip, on_gpu, site)


@pytest.mark.gpu
@pytest.mark.parametrize('name,site', _ids(PLANAR_CASES + ONE_LAUNCH_CASES + SMALL_F32_FORMAT_CASES + FIRST_STEP_CASES))
def test_contract_on_the_planar_cell_kernels(hip, operand_format, name, site):
    """Planar gates forward / backward, the one-launch backward (plain and accumulate forms), the two-launch C = 64 backward, the order-3 planar
    kernels (gates backward with accumulate_x) and the first-step forms, both operand formats."""
    c = CASES[name]
    if name in ONE_LAUNCH_CASES and not hip.cell_bwd_planar_supported(32, 16):
        pytest.fail('the one-launch backward is part of the library')
    c.check(hip, on_gpu, site)


@pytest.mark.gpu
@pytest.mark.parametrize('name,site', _ids(RUNSCALE_GPU))
def test_runscale_stop_path(hip, monkeypatch, name, site):
    """fp16 x 2 backward kernels (one-launch C = 32, two-launch C = 64, order 3), 8-9 nodes per wave, one node's gradient non-finite in the middle
    of a wave (RunScale::node: a non-finite maximum gives the node the smallest scale, ends no pass and moves no reference): every other node's
    gradient planes are bit-identical to the clean run, accumulated planes received their addend exactly once, dW / db are non-finite (part D)."""
    from stc_hip import _lib
    monkeypatch.setattr(hip, 'operand_format', _lib.FMT_F16X2, raising=False)
    CASES[name].check(hip, on_gpu, site)


@pytest.mark.gpu
def test_gate_functions_on_the_kernels(hip):
    _gate_functions(hip, lambda t: t.cuda())


def _pad_columns(hip, dt, which):
    nodes, C, L, Lw, Ho, K = 50, 32, 32 if dt == 'bf16' else 20, 17, 32, 2      # (the bf16 kernels take slabs of 16 or 32 columns)
    d = _node_operands(nodes, C, L, Lw, Ho, K, seed=nodes + L + Lw)
    if dt == 'bf16':
        d['Zs'], d['dY'] = [z.to(torch.bfloat16) for z in d['Zs']], d['dY'].to(torch.bfloat16)
        run = CASES['bdg_node_fwd_bf16' if which == 'fwd' else 'bdg_node_bwd_bf16'].run
    else:
        run = _node_fwd if which == 'fwd' else (lambda k, o: _node_bwd(k, o, want_dT=False))
    r = 23
    clean = run(hip, on_gpu(d))
    got = run(hip, on_gpu(nf.poisoned(d, ('Zs', 1), (r, 4, 18), NAN)))
    others = [i for i in range(nodes) if i != r]
    for name in clean:
        if name in ('dW', 'db'):
            continue                                                       # sums over the nodes: one unit
        assert torch.isfinite(clean[name]).all(), name
        assert torch.equal(nf.bits(got[name])[others], nf.bits(clean[name])[others]), name


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_nan_in_the_pad_columns_stays_in_its_node_f32(hip, node_path, which):
    """Slabs of L = 20 columns (bf16: 32) with Lw = 17 used: the host writes zeros into the pad columns and the header asks for finite values there.  A NaN
    there is outside the contract for its own node (the matrix-core paths multiply it by a zero weight row) -- what is pinned is that it stays in
    that node: every other node's rows equal the clean run bit for bit.  All three dispatch levels."""
    _pad_columns(hip, 'f32', which)


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_nan_in_the_pad_columns_stays_in_its_node_bf16(hip, which):
    _pad_columns(hip, 'bf16', which)


def _flag(t):
    return not bool(torch.isfinite(t).all())


@pytest.mark.gpu
@pytest.mark.parametrize('family', list(MODULE_FAMILIES))
def test_module_hands_a_nan_sample_on_like_the_twin(family, monkeypatch):
    """tools/probes/nan_robustness.py's cases as assertions: a NaN in sample 0 of X_seq.  Loss non-finite; every parameter gradient flagged exactly
    where the CPU twin's run of the same schedule flags it; sample 1 of yhat finite and within the forward bound of the twin; sample 0 non-finite
    wherever the twin's is."""
    yhat_w, loss_w, grads_w = _twin_run(family, monkeypatch)
    monkeypatch.setattr(ops, '_kernels', None)
    yhat, loss, grads = _module_run(*_module_case(family), 'cuda')
    assert not (abs(loss) < float('inf')) and not (abs(loss_w) < float('inf'))
    for k_ in grads_w:
        assert _flag(grads[k_]) == _flag(grads_w[k_]), k_
    assert torch.isfinite(yhat[1]).all()
    err = float((yhat[1].double() - yhat_w[1].double()).abs().max() / yhat_w[1].double().abs().max())
    assert err < nf.F32_TOL, err
    assert not bool((~torch.isfinite(yhat_w[0]) & torch.isfinite(yhat[0])).any())


@pytest.mark.gpu
def test_generator_kernels_hand_a_nan_weight_on(monkeypatch):
    """dense-learned: a NaN in one MGP_Gen projection weight.  Gs and the loss are non-finite on the kernel path as on the module's own torch path
    (toggled as in tests/test_mgp_front.py) -- with fmaxf in stc_mgp_softmax_fwd_f32 the kernel path handed on a finite, uniform graph."""
    gen, X, As, Ac = _generator_case()
    gen, X, As, Ac = gen.cuda(), X.cuda(), As.cuda(), Ac.cuda()
    calls = []
    real = ops.mgp_front
    monkeypatch.setattr(ops, 'mgp_front', lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])

    def run():
        gen.zero_grad(set_to_none=True)
        Gs, Gc = gen(X, As, Ac)
        loss = Gs.sum() + Gc.sum()
        loss.backward()
        return Gs.detach().cpu(), Gc.detach().cpu(), float(loss.detach()), {k_: p.grad.detach().cpu() for k_, p in gen.named_parameters()}

    Gs, Gc, loss, grads = run()
    assert calls == [2, 3]
    monkeypatch.setattr(ops, 'mgp_front_supported', lambda *a: False)
    Gs_t, Gc_t, loss_t, grads_t = run()
    assert torch.isnan(Gs_t).all() and loss_t != loss_t                    # the reference behaviour
    assert not bool((~torch.isfinite(Gs_t) & torch.isfinite(Gs)).any()) and loss != loss
    assert not bool((~torch.isfinite(Gc_t) & torch.isfinite(Gc)).any())
    for k_ in grads_t:
        assert not bool((~torch.isfinite(grads_t[k_]) & torch.isfinite(grads[k_])).any()), k_
