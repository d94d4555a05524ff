"""Helpers of tests/test_shape_lattice.py: every shape the library's own predicates accept, and one parity run per shape.

The table is not a list.  A FAMILY declares a BOX -- a finite range per dimension -- and the family's points are exactly the points of the box
that the library's predicate accepts, asked through ``_lib.load_library()`` (no device needed).  Only the box bounds and the node counts are
written out here.  In this code base almost every accepted point is separate machine code (the node and cell kernels are templates over
(C, Ho, L, K, ...), the few-category kernels change tile geometry with 16 / C, the generic kernel with 32 / C), so a point nobody listed is code
nobody has run.

    family        entry points                                                      predicate
    mfma_node     stc_bdg_node_fwd/bwd_f32, dispatch levels 0 and 1                 the matrix-core kernels' shape set (= the fused cell kernels':
                                                                                    stc_cell_fused_supported) and the entry point's own size checks
    generic_node  stc_bdg_node_fwd/bwd_f32, dispatch level 2                        the entry point's size checks (a call with nodes = 0 runs them only)
    fused_cell    stc_cell_gates_fwd/blend_fwd/gates_bwd/cand_bwd_f32               stc_cell_fused_supported
    planar        stc_cell_gates_fwd/bwd_planar_f32 + node_post on planes           stc_cell_planar_supported and stc_bdg_node_post_supported
    one_launch    stc_cell_bwd_planar_f32                                           stc_cell_bwd_planar_supported
    planar_k      the four stc_cell_*_planar_k_f32                                  stc_cell_planar_k_supported
    first_step    stc_cell_gates_fwd_first_f32 / stc_cell_bwd_first_f32             stc_cell_first_supported
    post          stc_bdg_node_post_fwd/bwd_f32 on interleaved rows                 stc_bdg_node_post_supported
    small_cell    stc_cell_small_fwd/bwd_f32                                        stc_cell_small_supported
    mix_dt        stc_mix_dt_f32 and the packed node route (ops._packed_spans)      stc_mix_dt_supported
    bf16_node     stc_bdg_node_fwd/bwd_bf16                                         stc_bdg_node_bf16_supported
    bf16_planar   stc_cell_gates_fwd/bwd_planar_bf16, stc_bdg_node_post_bwd_bf16    stc_cell_planar_bf16_supported
    bf16_one_launch  stc_cell_bwd_planar_bf16                                       stc_cell_bwd_planar_bf16_supported
    cheby         stc_cheby_dense_fwd/bwd_f32                                       n <= 128, K <= STC_MAX_K (the entry point's STC_REQUIRE limits)
    fusion        stc_mixed_fusion_fwd/bwd_f32                                      HipKernels.mixed_fusion_supported (ops.mixed_fusion_supported on the GPU)

Node counts: the smallest size at which the tiling can still go wrong -- more than one tile with a ragged last one: 2 * max(1, 32 // C) + 1 for
the generic kernel, 2 * (16 // C) + 1 for the packed and the few-category kernels (those at batch 2), 5 where one wave owns one node.

References are float64: the node forward is ONE einsum (STC_GNN.py:38-45 on pre-aggregated slabs, pad columns carrying no weight) and its
backward torch autograd of that line; the few-category cells are ``oracle.stc_oracle.stc_cell`` with autograd; pieces with no one-line expression
(the fused and planar prologues / epilogues, mix_dT) are the CPU twin run on float64 tensors; the mixed fusion is float64 autograd of the
reference's expression.  The order-3 planar set, the first-step forms and the bf16 set run the body of their existing hand-picked test at the
lattice's shapes (same reference, same assertions).  Bounds: no new numbers -- each family imports the bound of its existing hand-picked test and the same ``rel_err``.
"""
import zlib

import pytest
import torch

from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, _lib, ops
from stc_hip.graph import csr_operand, dense_operand
from tests.conftest import rel_err
from tests.test_hip_kernels import FUSION_GRAD, TOL                          # the fp32 kernels against their twin; test_mixed_fusion's gradient bound
from tests.test_small_cell import TOL as SMALL_TOL, _buffers, _graph, _inputs, _run, _split_params
from tests.test_small_dense_order3 import FWD_CELL, GRAD_CELL, _dense_graphs, _step

EM = EmulatedKernels()
H16 = 16
CINS = [1, 2, 3, 4, 16]
TWIN_IS_REFERENCE = 1e-12         # two float64 computations of one expression: a condition, not a measurement
MAX_K = _lib.MAX_K                # STC_MAX_K of include/stc_hip.h (tests/test_abi.py holds the header and the bindings together)
OK, EUNSUPPORTED = 0, -4


def row_width(cin, h=H16):
    """Columns of an interleaved cell row: cin + h rounded up to 4 floats."""
    return cin + h + (-(cin + h)) % 4


# ---- the boxes ----------------------------------------------------------------------------------------------------------------------------------
#: the generic kernel's four shape classes (L, Lw, Ho, Ks, Kc): Ks != Kc with L % 4 != 0; Lw < L; the highest order with an odd Ho; the bench width
GENERIC_CLASSES = [(17, 17, 16, 3, 2), (20, 17, 32, 2, 2), (6, 5, 3, MAX_K, MAX_K), (32, 32, 32, 2, 2)]

#: family -> the box the family is run on: a finite range per dimension (an argument a family's kernels fix -- hidden width 16, order 2 -- is no
#: dimension of its box: ``DEFAULTS``)
BOXES = {
    'mfma_node': dict(C=[16, 32, 64], L=[20, 32], Ho=[16, 32], K=[1, 2, 3], pad=[0, 3]),
    'generic_node': dict(C=list(range(1, 34)) + [48, 63, 64], cls=list(range(len(GENERIC_CLASSES)))),
    'fused_cell': dict(K=[1, 2, 3], C=[16, 32, 64], cin=[1, 2, 3, 4, 13, 16]),
    'planar': dict(C=[32, 64], cin=CINS),
    'one_launch': dict(C=[32, 64], cin=CINS),
    'planar_k': dict(C=[32, 64], cin=CINS, K=[2, 3]),
    'first_step': dict(C=[32, 64], cin=CINS),
    'post': dict(C=[32, 64], cin=CINS),
    'small_cell': dict(C=list(range(1, 17)), cin=CINS, K=[2, 3]),
    'mix_dt': dict(C=list(range(1, 17)), L=[20, 32], Ho=[16, 32], K=[1, 2, 3]),
    'bf16_node': dict(C=[16, 32, 64], L=[16, 20, 32], Ho=[16, 32], K=[1, 2, 3]),      # (16: the bf16 kernels' own narrow row, tests/test_bf16_kernels.py)
    'bf16_planar': dict(C=[16, 32, 64], cin=CINS),
    'bf16_one_launch': dict(C=[16, 32, 64], cin=CINS),
    'cheby': dict(n=[1, 2, 63, 64, 65, 127, 128], K=list(range(1, MAX_K + 1))),
    'fusion': dict(n=[2, 6, 34, 62, 128]),
}
DEFAULTS = dict(h=H16, K=2, pad=0)
#: family -> the MARGIN: per argument of the predicate, values beyond the box on each side (and the arguments the box fixes, freed).  The library
#: must decline every point of box + margin that is not a point of the box: a predicate that widens -- a hidden width of 32, an order 3 on the planar
#: forms, a C of 48 -- turns the CPU suite red until the box, and with it the GPU runs, grow
_HS, _KS = [8, 32], [1, 3, MAX_K]
MARGINS = {
    'mfma_node': dict(C=[8, 48, 128], L=[16, 24, 36], Ho=[8, 48], K=[MAX_K], h=_HS),
    'generic_node': dict(),                                   # (takes every size up to its LDS limit: nothing to decline)
    'fused_cell': dict(K=[MAX_K], C=[8, 48, 128], cin=[0, 17], h=_HS),
    'planar': dict(C=[16, 48, 128], K=_KS, h=_HS),
    'one_launch': dict(C=[16, 48, 128], h=_HS),
    'planar_k': dict(C=[16, 48, 128], K=[1, MAX_K], h=_HS),
    'first_step': dict(C=[16, 48, 128], h=_HS),
    'post': dict(C=[16, 48, 128], cin=[8], K=_KS, h=_HS),
    'small_cell': dict(C=[0, 17, 32], cin=[0, 5, 8, 17], K=[1, MAX_K], h=_HS),
    'mix_dt': dict(C=[0, 17, 32], L=[16, 24, 36], Ho=[8, 48], K=[MAX_K]),
    'bf16_node': dict(C=[8, 48, 128], L=[24, 36], Ho=[8, 48], K=[MAX_K]),
    'bf16_planar': dict(C=[8, 48, 128], K=_KS, h=_HS),
    'bf16_one_launch': dict(C=[8, 48, 128], cin=[0, 5, 8], h=_HS),
    'cheby': dict(),                                          # (limits, not a predicate: held to STC_ELIMIT in tests/test_shape_lattice.py)
    'fusion': dict(n=[1, 3, 5]),
}


def _sizes_ok(lib, C, L, Lw, Ho, Ks, Kc):
    """The size checks of stc_bdg_node_fwd_f32 and nothing else: with nodes = 0 the entry point returns after them (no pointer is read)."""
    return lib.stc_bdg_node_fwd_f32(None, Ks, None, Kc, None, None, None, 0, C, L, Lw, Ho, None) == OK


def _full(p):
    return dict(DEFAULTS, **p)


#: family -> predicate(lib, point) at dispatch level 0; every argument of the library's predicate comes from the point (``DEFAULTS`` where the box fixes it)
ACCEPTS = {
    'mfma_node': lambda lib, p: bool(lib.stc_cell_fused_supported(p['K'], p['K'], p['C'], p['L'], p['h'])) and p['Ho'] in (H16, 2 * H16)
                                and _sizes_ok(lib, p['C'], p['L'], p['L'] - p['pad'], p['Ho'], p['K'], p['K']),
    'generic_node': lambda lib, p: _sizes_ok(lib, p['C'], *GENERIC_CLASSES[p['cls']]),
    'fused_cell': lambda lib, p: bool(lib.stc_cell_fused_supported(p['K'], p['K'], p['C'], row_width(p['cin'], p['h']), p['h'])),
    'planar': lambda lib, p: bool(lib.stc_cell_planar_supported(p['K'], p['K'], p['C'], p['h']))
                             and bool(lib.stc_bdg_node_post_supported(p['K'], p['K'], p['C'], row_width(p['cin'], p['h']), p['h'])),
    'one_launch': lambda lib, p: bool(lib.stc_cell_bwd_planar_supported(p['C'], p['h'])),
    'planar_k': lambda lib, p: bool(lib.stc_cell_planar_k_supported(p['K'], p['C'], p['h'])),
    'first_step': lambda lib, p: bool(lib.stc_cell_first_supported(p['C'], p['h'])),
    'post': lambda lib, p: bool(lib.stc_bdg_node_post_supported(p['K'], p['K'], p['C'], row_width(p['cin'], p['h']), p['h'])),
    'small_cell': lambda lib, p: bool(lib.stc_cell_small_supported(p['K'], p['K'], p['C'], p['cin'], p['h'])),
    'mix_dt': lambda lib, p: bool(lib.stc_mix_dt_supported(p['K'], p['K'], p['C'], p['L'], p['Ho'])),
    'bf16_node': lambda lib, p: bool(lib.stc_bdg_node_bf16_supported(p['K'], p['K'], p['C'], p['L'], p['Ho'])),
    'bf16_planar': lambda lib, p: bool(lib.stc_cell_planar_bf16_supported(p['K'], p['K'], p['C'], p['h'])),
    'bf16_one_launch': lambda lib, p: bool(lib.stc_cell_bwd_planar_bf16_supported(p['C'], p['cin'] + p['h'], p['h'])),
    'cheby': lambda lib, p: 1 <= p['n'] <= 128 and 1 <= p['K'] <= MAX_K,
    'fusion': lambda lib, p: bool(_lib.HipKernels.mixed_fusion_supported(None, p['n'] * p['n'])),       # (the size rule; the operands' own: asked on the GPU)
}
FAMILIES = tuple(BOXES)


def _product(dims):
    pts = [{}]
    for dim, values in dims.items():
        pts = [dict(p, **{dim: v}) for p in pts for v in values]
    return pts


def margin_points(family):
    """Box + margin, every argument free, as full points (the defaults filled in)."""
    dims = {d: list(v) for d, v in BOXES[family].items()}
    for d, v in MARGINS[family].items():
        base = dims[d] if d in dims else [DEFAULTS[d]]
        dims[d] = base + [x for x in v if x not in base]
    return [_full(p) for p in _product(dims)]


def box_points(family):
    return _product(BOXES[family])


def accepted(family, lib=None):
    """The points of the family's box that the library's predicate accepts, at dispatch level 0."""
    lib = lib or _lib.load_library()
    assert lib.stc_set_dispatch_level(0) == OK
    return [p for p in box_points(family) if ACCEPTS[family](lib, _full(p))]


LATTICE = {family: accepted(family) for family in FAMILIES}


def point_id(p):
    return '-'.join(f'{k}{v}' for k, v in p.items())


def points(family):
    """pytest parameters of a family: one per accepted point."""
    return [pytest.param(p, id=point_id(p)) for p in LATTICE[family]]


def seed_of(family, p):
    return zlib.crc32(repr((family, sorted(p.items()))).encode())


def node_shape(family, p):
    """(nodes, C, L, Lw, Ho, Ks, Kc) of a point of a node family."""
    if family == 'generic_node':
        return (2 * max(1, 32 // p['C']) + 1, p['C'], *GENERIC_CLASSES[p['cls']])
    if family == 'mix_dt':
        return (2 * (16 // p['C']) + 1, p['C'], p['L'], p['L'] - 3 if p['L'] == 20 else p['L'], p['Ho'], p['K'], p['K'])      # (L = 20: 1 + 16 columns, padded)
    return (5, p['C'], p['L'], p['L'] - p['pad'], p['Ho'], p['K'], p['K'])


# ---- float64 references ---------------------------------------------------------------------------------------------------------------------------
def node_forward(Zs, Tc, W, b, Lw):
    """Y = b + sum_{n, c, c', l} Z_n[v, c', l] T_c[c', d] W[(n, c, l), o] (STC_GNN.py:38-45 on pre-aggregated slabs; columns l >= Lw carry no weight)."""
    Ks, Kc = len(Zs), Tc.shape[0]
    Y = torch.einsum('nvpl,cpd,nclo->vdo', torch.stack([z[..., :Lw] for z in Zs]), Tc, W.view(Ks, Kc, Lw, W.shape[1]))
    return Y if b is None else Y + b


def node_operands(nodes, C, L, Lw, Ho, Ks, Kc, seed):
    """The conventions of tests/test_hip_kernels.py: T_0 = I and the other T_c random (not symmetric), W scaled by the root of its fan-in, 7.0 in
    the pad columns."""
    g = torch.Generator().manual_seed(seed)
    Zs = [torch.randn(nodes, C, L, generator=g) for _ in range(Ks)]
    for z in Zs:
        z[..., Lw:] = 7.0
    Tc = torch.randn(Kc, C, C, generator=g) / C ** 0.5
    Tc[0] = torch.eye(C)
    W = torch.randn(Ks * Kc * Lw, Ho, generator=g) / (Ks * Kc * Lw) ** 0.5
    return dict(Zs=Zs, Tc=Tc, W=W, b=torch.randn(Ho, generator=g), dY=torch.randn(nodes, C, Ho, generator=g), Lw=Lw)


_NODE_REF = {}


def node_reference(key, d):
    """Float64 forward (with the bias) and torch autograd's backward of ``node_forward`` for the operands ``d``: computed once per ``key``, shared,
    never modified."""
    if key not in _NODE_REF:
        Zs = [z.double().requires_grad_() for z in d['Zs']]
        Tc, W, b = (d[n].double().requires_grad_() for n in ('Tc', 'W', 'b'))
        Y = node_forward(Zs, Tc, W, b, d['Lw'])
        Y.backward(d['dY'].double())
        _NODE_REF[key] = dict(Y=Y.detach(), dZ=[z.grad for z in Zs], dW=W.grad, db=b.grad, dT=Tc.grad)
    return _NODE_REF[key]


def d64(v):
    return None if v is None else ([d64(t) for t in v] if isinstance(v, (list, tuple)) else v.double())


def e64(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float64)


def cu(v):
    return None if v is None else ([cu(t) for t in v] if isinstance(v, (list, tuple)) else v.cuda())


def nan(*shape):
    return torch.full(shape, float('nan')).cuda()


def close(got, want, bound, what):
    err = rel_err(got, want)
    print(f'{what}: {err:.3e} (bound {bound:.1e})')
    assert torch.isfinite(got.float()).all(), f'{what}: a non-finite result (an output the launch did not write?)'
    assert err < bound, f'{what}: relative error {err:.3e} >= {bound:.1e}'


def formats(hip):
    """The kernel set on both operand formats the binding can select: the default one and the view heavy graphs get."""
    other = hip.for_graph(float('inf'))
    return [hip] if other is hip else [hip, other]


class at_level:
    """The process-wide dispatch ceiling for the length of a ``with`` block."""
    def __init__(self, hip, level):
        self.hip, self.level = hip, level

    def __enter__(self):
        self.hip.set_dispatch_level(self.level)

    def __exit__(self, *exc):
        self.hip.set_dispatch_level(0)


# ---- node kernels: matrix-core (levels 0, 1), generic (level 2) -----------------------------------------------------------------------------------
def check_node_backward(tag, d, ref, dZ, dW, db, dT, bound=TOL):
    Lw, L = d['Lw'], d['Zs'][0].shape[-1]
    for n, (a, w) in enumerate(zip(dZ, ref['dZ'])):
        close(a, w, bound, f'{tag} dZ[{n}]')
        if Lw < L:
            assert float(a[..., Lw:].abs().max()) == 0.0, f'{tag} dZ[{n}]: a pad column has a gradient'
    close(dW, ref['dW'], bound, f'{tag} dW')
    if db is not None:
        close(db, ref['db'], bound, f'{tag} db')
    if dT is not None:
        assert float(dT[0].abs().max()) == 0.0, f'{tag}: dT[0] is not exactly zero (T_0 = I is a constant)'
        if dT.shape[0] > 1:
            close(dT[1:], ref['dT'][1:], bound, f'{tag} dT[1:]')


def run_node(hip, family, p, level):
    """Forward with and without bias, backward with and without dT, the weight gradient a second time."""
    run_node_shape(hip, node_shape(family, p), seed_of(family, p), (family, point_id(p)), f'{family} {point_id(p)} level {level}', level)


#: the gates convolution of a cell with a 32-column input at hidden width 32 (Ks = Kc = 2): L = 32 + 32, Ho = 2 x 32.  Outside ``GENERIC_CLASSES``
#: because the generic backward takes it for few categories only: W^T and the dW accumulators fill 130 KiB of the LDS, the tile shrinks to what
#: fits beside them (csrc/stc_node.hip ``fit_bwd``) -- one node of up to 21 categories, 15 when dT_c is wanted too
HIDDEN32_GATES = (64, 64, 64, 2, 2)


def run_node_shape(hip, shape, seed, key, tag, level):
    nodes, C, L, Lw, Ho, Ks, Kc = shape
    d = node_operands(*shape, seed=seed)
    ref = node_reference(key, d)
    Zs, Tc, W, dY = cu(d['Zs']), cu(d['Tc']), cu(d['W']), cu(d['dY'])
    with at_level(hip, level):
        for b in (d['b'], None):
            Y = nan(nodes, C, Ho)
            hip.bdg_node_fwd(Zs, Tc, W, cu(b), Y)
            close(Y, ref['Y'] if b is not None else ref['Y'] - d['b'].double(), TOL, f'{tag} Y bias={b is not None}')
        for want_dT in (True, False):
            dZ = [nan(nodes, C, L) for _ in range(Ks)]
            dW, db, dT = nan(*W.shape), nan(Ho), nan(Kc, C, C) if want_dT else None
            hip.bdg_node_bwd(Zs, Tc, W, dY, dZ, dW, db, dT)
            check_node_backward(f'{tag} dT={want_dT}', d, ref, dZ, dW, db, dT)
            dW2 = nan(*W.shape)
            hip.bdg_node_bwd(Zs, Tc, W, dY, dZ, dW2, None, dT)
            assert torch.equal(dW, dW2), f'{tag}: dW differs on a second call'


def twin_node(family, p):
    """CPU: the float64 twin against the float64 reference expression at a node point (the packed route: through ``ops._packed_spans`` and the
    block-diagonal category graph, as ``ops._bdg_forward`` launches it)."""
    shape = node_shape(family, p)
    nodes, C, L, Lw, Ho, Ks, Kc = shape
    d = node_operands(*shape, seed=seed_of(family, p))
    ref = node_reference((family, point_id(p)), d)
    Zs, Tc, W, b, dY = d64(d['Zs']), d64(d['Tc']), d64(d['W']), d64(d['b']), d64(d['dY'])
    if family == 'mix_dt':
        Y, dZ, dW, db = packed_node(EM, Zs, Tc, W, b, dY, lambda *s: e64(*s))
        dT = e64(Kc, C, C)
        EM.mix_dT(Zs, W, dY, dT)
    else:
        Y, dZ, dW, db, dT = e64(nodes, C, Ho), [e64(nodes, C, L) for _ in range(Ks)], e64(*W.shape), e64(Ho), e64(Kc, C, C)
        EM.bdg_node_fwd(Zs, Tc, W, b, Y)
        EM.bdg_node_bwd(Zs, Tc, W, dY, dZ, dW, db, dT)
    close(Y, ref['Y'], TWIN_IS_REFERENCE, 'twin Y')
    dT[0].zero_()                                                          # (T_0 = I is a constant of the kernels' contract: the twin's first block carries no meaning)
    check_node_backward('twin', d, ref, dZ, dW, db, dT, TWIN_IS_REFERENCE)


# ---- stc_mix_dt_f32 and the packed node route ----------------------------------------------------------------------------------------------------
def packed_node(k, Zs, Tc, W, b, dY, new):
    """The node convolution of few categories as ``ops._bdg_forward`` / ``ops._bdg_backward_slabs`` launch it: floor(16 / C) nodes per row tile as
    one node with a block-diagonal category graph, the remainder one node per tile in a launch of its own, their parameter gradients added."""
    R, C, L = Zs[0].shape
    Ho, Ks = W.shape[1], len(Zs)
    Y, dZ, dW, db = new(R, C, Ho), [new(R, C, L) for _ in range(Ks)], None, None
    for lo, n, q in ops._packed_spans(R, 16 // C):
        rows = lambda t: t[lo:lo + n].view(n // q, q * C, t.shape[-1])
        Tq = Tc if q == 1 else ops._block_diag(Tc, q)
        k.bdg_node_fwd([rows(z) for z in Zs], Tq, W, b, rows(Y))
        dW_i, db_i = new(*W.shape), new(Ho)
        k.bdg_node_bwd([rows(z) for z in Zs], Tq, W, rows(dY), [rows(z) for z in dZ], dW_i, db_i, None)
        dW, db = (dW_i, db_i) if dW is None else (dW + dW_i, db + db_i)
    return Y, dZ, dW, db


def run_mix_dt(hip, p):
    shape = node_shape('mix_dt', p)
    nodes, C, L, Lw, Ho, K, _ = shape
    d = node_operands(*shape, seed=seed_of('mix_dt', p))
    ref = node_reference(('mix_dt', point_id(p)), d)
    tag = f'mix_dt {point_id(p)}'
    Zs, Tc, W, dY = cu(d['Zs']), cu(d['Tc']), cu(d['W']), cu(d['dY'])
    want = e64(K, C, C)                                            # (as tests/test_hip_kernels.py: the float64 twin is the exact side)
    EM.mix_dT(d64(d['Zs']), d64(d['W']), d64(d['dY']), want)
    got = nan(K, C, C)
    hip.mix_dT(Zs, W, dY, got)
    assert float(got[0].abs().max()) == 0.0, f'{tag}: dT[0] is not exactly zero'
    if K > 1:
        close(got[1:], want[1:], TOL, f'{tag} dT[1:] against the twin')
        close(got[1:], ref['dT'][1:], TOL, f'{tag} dT[1:] against autograd')
    again = nan(K, C, C)
    hip.mix_dT(Zs, W, dY, again)
    assert torch.equal(got, again), f'{tag}: dT differs on a second call'
    for level in (0, 1):
        with at_level(hip, level):
            Y, dZ, dW, db = packed_node(hip, Zs, Tc, W, cu(d['b']), dY, nan)
            close(Y, ref['Y'], TOL, f'{tag} packed Y level {level}')
            check_node_backward(f'{tag} packed level {level}', d, ref, dZ, dW, db, None)
            again = packed_node(hip, Zs, Tc, W, cu(d['b']), dY, nan)
            assert torch.equal(dW, again[2]), f'{tag}: packed dW differs on a second call'


# ---- fused cell kernels ------------------------------------------------------------------------------------------------------------------------
def fused_operands(p, nodes=5):
    K, C, cin = p['K'], p['C'], p['cin']
    Lw, L = cin + H16, row_width(cin)
    g = torch.Generator().manual_seed(seed_of('fused_cell', p))
    rnd = lambda *s: torch.randn(*s, generator=g)
    Zs = [rnd(nodes, C, L) for _ in range(K)]
    for z in Zs[1:]:
        z[..., Lw:] = 7.0
    Zs[0][..., Lw:] = 0.0                                          # (the pad columns of the concatenated input are zeros: the forward copies them out)
    Tc = rnd(K, C, C) / C ** 0.5
    Tc[0] = torch.eye(C)
    fan = (K * K * Lw) ** 0.5
    return dict(Zs=Zs, Tc=Tc, H=rnd(nodes, C, H16), Wg=rnd(K * K * Lw, 2 * H16) / fan, bg=rnd(2 * H16), Wc=rnd(K * K * Lw, H16) / fan, bc=rnd(H16),
                dCand=rnd(nodes, C, L), dU=rnd(nodes, C, H16), U=torch.rand(nodes, C, H16, generator=g), R=torch.rand(nodes, C, H16, generator=g),
                owed=rnd(nodes, C, H16), Cand=torch.tanh(rnd(nodes, C, H16)), dHn=rnd(nodes, C, H16), Lw=Lw, L=L, nodes=nodes)


def fused_twin(d):
    """Everything ``run_fused`` compares, from the twin on float64 tensors."""
    nodes, K, C, L, cin = d['nodes'], len(d['Zs']), d['Tc'].shape[1], d['L'], d['Lw'] - H16
    t = {n: d64(v) for n, v in d.items() if n not in ('Lw', 'L', 'nodes')}
    plane = lambda: e64(nodes, C, H16)
    w = dict(U=plane(), R=plane(), Ci=e64(nodes, C, L), Cand=plane(), Hn=plane(), Cand0=plane(), Hn0=plane())
    EM.cell_gates_fwd(t['Zs'], t['Tc'], t['Wg'], t['bg'], t['H'], w['U'], w['R'], w['Ci'])
    EM.cell_blend_fwd(t['Zs'], t['Tc'], t['Wc'], t['bc'], w['U'], t['H'], w['Cand'], w['Hn'])
    EM.cell_blend_fwd(t['Zs'], t['Tc'], t['Wc'], None, w['U'], t['H'], w['Cand0'], w['Hn0'])
    # gates backward: the dU form with a gradient already owed to H, and the Cand form (dH_in = dHnew, both blend products formed inside)
    w.update(gdZ=[e64(nodes, C, L) for _ in range(K)], gdW=e64(*t['Wg'].shape), gdb=e64(2 * H16), dXt=e64(nodes, C, cin), dH=t['owed'].clone())
    EM.cell_gates_bwd(t['Zs'], t['Tc'], t['Wg'], t['dCand'], t['dU'], t['H'], t['U'], t['R'], w['dH'], w['gdZ'], w['gdW'], w['gdb'], w['dXt'], w['dH'])
    w.update(g4dZ=[e64(nodes, C, L) for _ in range(K)], g4dW=e64(*t['Wg'].shape), g4db=e64(2 * H16), dH4=plane())
    EM.cell_gates_bwd(t['Zs'], t['Tc'], t['Wg'], t['dCand'], None, t['H'], t['U'], t['R'], t['owed'], w['g4dZ'], w['g4dW'], w['g4db'], None, w['dH4'], Cand=t['Cand'])
    w.update(cdZ=[e64(nodes, C, L) for _ in range(K)], cdW=e64(*t['Wc'].shape), cdb=e64(H16))
    EM.cell_cand_bwd(t['Zs'], t['Tc'], t['Wc'], t['dHn'], t['U'], t['Cand'], w['cdZ'], w['cdW'], w['cdb'])
    return w


def twin_fused(p):
    """CPU: the twin's fused forward and candidate backward in float64 against the node reference expression with the gate math of
    STC_GNN.py:69-78 written out, differentiated by torch autograd."""
    d = fused_operands(p)
    w = fused_twin(d)
    cin, Lw, L = d['Lw'] - H16, d['Lw'], d['L']
    t = {n: d64(v) for n, v in d.items() if n not in ('Lw', 'L', 'nodes')}
    U, R = torch.sigmoid(node_forward(t['Zs'], t['Tc'], t['Wg'], t['bg'], Lw)).split(H16, -1)
    close(w['U'], U, TWIN_IS_REFERENCE, 'twin U')
    close(w['R'], R, TWIN_IS_REFERENCE, 'twin R')
    close(w['Ci'], torch.cat([t['Zs'][0][..., :cin], R * t['H'], torch.zeros(*R.shape[:2], L - Lw, dtype=R.dtype)], -1), TWIN_IS_REFERENCE, 'twin CandIn')
    for bc, cand, hn in ((t['bc'], 'Cand', 'Hn'), (None, 'Cand0', 'Hn0')):
        Cand = torch.tanh(node_forward(t['Zs'], t['Tc'], t['Wc'], bc, Lw))
        close(w[cand], Cand, TWIN_IS_REFERENCE, 'twin ' + cand)
        close(w[hn], (1.0 - U) * t['H'] + U * Cand, TWIN_IS_REFERENCE, 'twin ' + hn)
    # candidate backward: d/d(Z, W, b) of <dHnew, (1 - U) H + U tanh(pre)> at the point where tanh(pre) = Cand, i.e. dY = dHnew U (1 - Cand^2)
    Zs, Wc, bc = [z.clone().requires_grad_() for z in t['Zs']], t['Wc'].clone().requires_grad_(), t['bc'].clone().requires_grad_()
    node_forward(Zs, t['Tc'], Wc, bc, Lw).backward(t['dHn'] * t['U'] * (1 - t['Cand'] ** 2))
    for n in range(len(Zs)):
        close(w['cdZ'][n], Zs[n].grad, TWIN_IS_REFERENCE, f'twin cand dZ[{n}]')
    close(w['cdW'], Wc.grad, TWIN_IS_REFERENCE, 'twin cand dW')
    close(w['cdb'], bc.grad, TWIN_IS_REFERENCE, 'twin cand db')

    # gates backward, with the gates the forward gives for these slabs: autograd of the gate math (STC_GNN.py:69-78) through the convolution.  The
    # state enters twice -- as columns of the slabs (their gradient: dZ) and directly, in R * H and the blend (its gradient: dH); dXt is a copy
    nodes, K, C = d['nodes'], len(t['Zs']), t['Tc'].shape[1]
    U0, R0 = w['U'], w['R']
    for form in ('dU', 'Cand'):
        dZ, dW, db, dXt = [e64(nodes, C, L) for _ in range(K)], e64(*t['Wg'].shape), e64(2 * H16), e64(nodes, C, cin)
        Zs, Wg, bg, H = [z.clone().requires_grad_() for z in t['Zs']], t['Wg'].clone().requires_grad_(), t['bg'].clone().requires_grad_(), t['H'].clone().requires_grad_()
        Ug, Rg = torch.sigmoid(node_forward(Zs, t['Tc'], Wg, bg, Lw)).split(H16, -1)
        through_reset = (t['dCand'][..., cin:Lw] * (Rg * H)).sum()
        if form == 'dU':                                           # dU given, a gradient already owed to H accumulated in place
            dH = t['owed'].clone()
            EM.cell_gates_bwd(t['Zs'], t['Tc'], t['Wg'], t['dCand'], t['dU'], t['H'], U0, R0, dH, dZ, dW, db, dXt, dH)
            ((t['dU'] * Ug).sum() + through_reset).backward()
            want_dH = H.grad + t['owed']
            assert torch.equal(dXt, t['dCand'][..., :cin])
        else:                                                      # Cand given: dH_in is the new state's gradient, both blend products formed inside
            dH = e64(nodes, C, H16)
            EM.cell_gates_bwd(t['Zs'], t['Tc'], t['Wg'], t['dCand'], None, t['H'], U0, R0, t['owed'], dZ, dW, db, None, dH, Cand=t['Cand'])
            ((t['owed'] * ((1.0 - Ug) * H + Ug * t['Cand'])).sum() + through_reset).backward()
            want_dH = H.grad
        for n in range(K):
            close(dZ[n], Zs[n].grad, TWIN_IS_REFERENCE, f'twin gates({form}) dZ[{n}]')
        close(dW, Wg.grad, TWIN_IS_REFERENCE, f'twin gates({form}) dW')
        close(db, bg.grad, TWIN_IS_REFERENCE, f'twin gates({form}) db')
        close(dH, want_dH, TWIN_IS_REFERENCE, f'twin gates({form}) dH')


_FUSED_TWIN = {}


def run_fused(hip, p, level):
    """The four fused entry points at one point, in the forms tests/test_hip_kernels.py runs them."""
    d = fused_operands(p)
    key = point_id(p)
    if key not in _FUSED_TWIN:
        _FUSED_TWIN[key] = fused_twin(d)
    w = _FUSED_TWIN[key]
    nodes, K, C, L, Lw = d['nodes'], p['K'], p['C'], d['L'], d['Lw']
    cin = Lw - H16
    tag = f'fused {key} level {level}'
    g = {n: cu(v) for n, v in d.items() if n not in ('Lw', 'L', 'nodes')}
    plane = lambda: nan(nodes, C, H16)
    pads_zero = lambda ts, what: all(float(t[..., Lw:].abs().max()) == 0.0 for t in ts) if L > Lw else True
    with at_level(hip, level):
        assert hip.cell_fused_supported(K, K, C, L, H16)
        U, R, Ci = plane(), plane(), nan(nodes, C, L)
        hip.cell_gates_fwd(g['Zs'], g['Tc'], g['Wg'], g['bg'], g['H'], U, R, Ci)
        for a, n in ((U, 'U'), (R, 'R'), (Ci, 'Ci')):
            close(a, w[n], TOL, f'{tag} {n}')
        assert pads_zero([Ci], 'CandIn') and torch.equal(Ci[..., :cin].cpu(), d['Zs'][0][..., :cin]), f'{tag}: CandIn pad / input columns'
        Uw = cu(w['U'].float())
        for bc, cand, hn in ((g['bc'], 'Cand', 'Hn'), (None, 'Cand0', 'Hn0')):
            Cand, Hn = plane(), plane()
            hip.cell_blend_fwd(g['Zs'], g['Tc'], g['Wc'], bc, Uw, g['H'], Cand, Hn)
            # (the twin blends with its float64 U, the kernel with U rounded to fp32: 6e-8 of the state, against a bound of 1e-5)
            close(Cand, w[cand], TOL, f'{tag} {cand}')
            close(Hn, w[hn], TOL, f'{tag} {hn}')
        # gates backward, dU form, a gradient owed to H accumulated in place
        dZ, dW, db, dXt, dH = [nan(nodes, C, L) for _ in range(K)], nan(*d['Wg'].shape), nan(2 * H16), nan(nodes, C, cin), g['owed'].clone()
        hip.cell_gates_bwd(g['Zs'], g['Tc'], g['Wg'], g['dCand'], g['dU'], g['H'], g['U'], g['R'], dH, dZ, dW, db, dXt, dH)
        for n in range(K):
            close(dZ[n], w['gdZ'][n], TOL, f'{tag} gates dZ[{n}]')
        assert pads_zero(dZ, 'gates dZ'), f'{tag}: a pad column of the gates backward has a gradient'
        close(dW, w['gdW'], TOL, f'{tag} gates dW')
        close(db, w['gdb'], TOL, f'{tag} gates db')
        close(dH, w['dH'], TOL, f'{tag} gates dH')
        assert torch.equal(dXt.cpu(), d['dCand'][..., :cin]), f'{tag}: dXt is not the input columns of dCandIn'
        dW2, dH2 = nan(*d['Wg'].shape), nan(nodes, C, H16)                       # nothing owed: dH_in = NULL; db, dXt not wanted
        hip.cell_gates_bwd(g['Zs'], g['Tc'], g['Wg'], g['dCand'], g['dU'], g['H'], g['U'], g['R'], None, dZ, dW2, None, None, dH2)
        assert torch.equal(dW, dW2), f'{tag}: gates dW differs on a second call'
        close(dH2, w['dH'] - d['owed'].double(), TOL, f'{tag} gates dH, nothing owed')
        # Cand form
        dZ, dW, db, dH4 = [nan(nodes, C, L) for _ in range(K)], nan(*d['Wg'].shape), nan(2 * H16), plane()
        hip.cell_gates_bwd(g['Zs'], g['Tc'], g['Wg'], g['dCand'], None, g['H'], g['U'], g['R'], g['owed'], dZ, dW, db, None, dH4, dH_in_scaled=True, Cand=g['Cand'])
        for n in range(K):
            close(dZ[n], w['g4dZ'][n], TOL, f'{tag} gates(Cand) dZ[{n}]')
        close(dW, w['g4dW'], TOL, f'{tag} gates(Cand) dW')
        close(db, w['g4db'], TOL, f'{tag} gates(Cand) db')
        close(dH4, w['dH4'], TOL, f'{tag} gates(Cand) dH')
        # candidate backward
        dZ, dW, db = [nan(nodes, C, L) for _ in range(K)], nan(*d['Wc'].shape), nan(H16)
        hip.cell_cand_bwd(g['Zs'], g['Tc'], g['Wc'], g['dHn'], g['U'], g['Cand'], dZ, dW, db)
        for n in range(K):
            close(dZ[n], w['cdZ'][n], TOL, f'{tag} cand dZ[{n}]')
        assert pads_zero(dZ, 'cand dZ'), f'{tag}: a pad column of the candidate backward has a gradient'
        close(dW, w['cdW'], TOL, f'{tag} cand dW')
        close(db, w['cdb'], TOL, f'{tag} cand db')
        dW2 = nan(*d['Wc'].shape)
        hip.cell_cand_bwd(g['Zs'], g['Tc'], g['Wc'], g['dHn'], g['U'], g['Cand'], dZ, dW2, None)
        assert torch.equal(dW, dW2), f'{tag}: cand dW differs on a second call'


# ---- planar forms ----------------------------------------------------------------------------------------------------------------------------------
def planar_operands(family, p, nodes=5):
    C, cin = p['C'], p['cin']
    Lw, K = cin + H16, 2
    g = torch.Generator().manual_seed(seed_of(family, p))
    rnd = lambda *s: torch.randn(*s, generator=g)
    Tc = rnd(K, C, C) / C ** 0.5
    Tc[0] = torch.eye(C)
    fan = (K * K * Lw) ** 0.5
    plane = lambda: rnd(nodes, C, H16)
    return dict(X=rnd(nodes, C, cin), SX=rnd(nodes, C, cin), H=torch.tanh(plane()), SH=plane(), Tc=Tc, Wg=rnd(K * K * Lw, 2 * H16) / fan, bg=rnd(2 * H16),
                Wc=rnd(K * K * Lw, H16) / fan, bc=rnd(H16), dRH=plane(), Cand=torch.tanh(plane()), dHn=plane(), dA=plane(), dB=plane(),
                U=torch.sigmoid(plane()), R=torch.sigmoid(plane()), dBm=plane())


def twin_planar(p, nodes=5):
    """CPU: the planar twins in float64 against the expression on interleaved rows [Xt | H], [S.Xt | S.H]: gates forward, gates backward (autograd of
    the gate math through the convolution, the state's direct share apart) and the post-aggregation pair A, Bm with its backward -- the pieces the
    one-launch backward, the first-step forms and the planar runs on the GPU are compared with."""
    C, cin = p['C'], p['cin']
    wide, Lw = cin == H16, cin + H16
    t = {n: d64(v) for n, v in planar_operands('planar', p, nodes).items()}
    plane = lambda: e64(nodes, C, H16)
    leaf = lambda v: v.clone().requires_grad_()
    X, SX, Hc, SH, Wg, bg, H = (leaf(t[n]) for n in ('X', 'SX', 'H', 'SH', 'Wg', 'bg', 'H'))      # (Hc: the state as columns of the rows; H: its direct use)
    Ug, Rg = torch.sigmoid(node_forward([torch.cat([X, Hc], -1), torch.cat([SX, SH], -1)], t['Tc'], Wg, bg, Lw)).split(H16, -1)
    U_w, R_w, RH_w = plane(), plane(), plane()
    EM.cell_gates_fwd_planar(t['X'], t['H'], t['SX'], t['SH'], t['Tc'], t['Wg'], t['bg'], U_w, R_w, RH_w)
    for a, b, n in ((U_w, Ug, 'U'), (R_w, Rg, 'R'), (RH_w, Rg * H, 'RH')):
        close(a, b.detach(), TWIN_IS_REFERENCE, f'twin planar {n}')
    dZ = [plane() if (wide or i >= 2) else None for i in range(4)]
    dW, db, dH = e64(*t['Wg'].shape), e64(2 * H16), plane()
    EM.cell_gates_bwd_planar(t['X'], t['H'], t['SX'], t['SH'], t['Tc'], t['Wg'], t['dRH'], t['Cand'], U_w, R_w, t['dHn'], dZ, dW, db, dH)
    ((t['dRH'] * (Rg * H)).sum() + (t['dHn'] * ((1.0 - Ug) * H + Ug * t['Cand'])).sum()).backward()
    for i, v in enumerate((X, SX, Hc, SH)):
        if dZ[i] is not None:
            close(dZ[i], v.grad, TWIN_IS_REFERENCE, f'twin planar gates dZ[{i}]')
    for a, b, n in ((dW, Wg.grad, 'dW'), (db, bg.grad, 'db'), (dH, H.grad, 'dH')):
        close(a, b, TWIN_IS_REFERENCE, f'twin planar gates {n}')
    # post-aggregation pair on rows [Xt | R*H]: A = the convolution's slab-0 blocks (with the bias), Bm = its slab-1 blocks; Y = A + S.Bm
    rows, Wc, bc = leaf(torch.cat([t['X'], RH_w], -1)), leaf(t['Wc']), leaf(t['bc'])
    blocks = Wc.view(2, 2, Lw, H16)
    A = node_forward([rows], t['Tc'], blocks[0].reshape(2 * Lw, H16), bc, Lw)
    Bm = node_forward([rows], t['Tc'], blocks[1].reshape(2 * Lw, H16), None, Lw)
    lead, second = (t['X'], RH_w) if wide else (RH_w, t['X'])
    A_w, B_w, dX_w, dX2_w, dWc_w, dbc_w = plane(), plane(), plane(), plane(), e64(*t['Wc'].shape), e64(H16)
    EM.node_post_fwd(lead, t['Tc'], t['Wc'], t['bc'], A_w, B_w, X2=second)
    EM.node_post_bwd(lead, t['Tc'], t['Wc'], t['dA'], t['dB'], dX_w, dWc_w, dbc_w, X2=second, dX2=dX2_w if wide else None)
    close(A_w, A.detach(), TWIN_IS_REFERENCE, 'twin post A')
    close(B_w, Bm.detach(), TWIN_IS_REFERENCE, 'twin post Bm')
    ((t['dA'] * A).sum() + (t['dB'] * Bm).sum()).backward()
    if wide:
        close(dX_w, rows.grad[..., :cin], TWIN_IS_REFERENCE, 'twin post dX')
        close(dX2_w, rows.grad[..., cin:], TWIN_IS_REFERENCE, 'twin post dX2')
    else:
        close(dX_w, rows.grad[..., cin:], TWIN_IS_REFERENCE, 'twin post d(R*H)')
    close(dWc_w, Wc.grad, TWIN_IS_REFERENCE, 'twin post dW')
    close(dbc_w, bc.grad, TWIN_IS_REFERENCE, 'twin post db')


def run_planar(hip, p, nodes=5):
    """Gates forward / backward on planes and the post-aggregation pair with a planar input, both operand formats, against the twin on float64."""
    C, cin = p['C'], p['cin']
    wide = cin == H16
    d = planar_operands('planar', p, nodes)
    t = {n: d64(v) for n, v in d.items()}
    plane64 = lambda: e64(nodes, C, H16)
    U_w, R_w, RH_w = plane64(), plane64(), plane64()
    EM.cell_gates_fwd_planar(t['X'], t['H'], t['SX'], t['SH'], t['Tc'], t['Wg'], t['bg'], U_w, R_w, RH_w)
    dZ_w = [plane64() if (wide or i >= 2) else None for i in range(4)]
    dW_w, db_w, dH_w = e64(*d['Wg'].shape), e64(2 * H16), plane64()
    EM.cell_gates_bwd_planar(t['X'], t['H'], t['SX'], t['SH'], t['Tc'], t['Wg'], t['dRH'], t['Cand'], U_w, R_w, t['dHn'], dZ_w, dW_w, db_w, dH_w)
    A_w, B_w, dX_w, dX2_w, dWc_w, dbc_w = plane64(), plane64(), plane64(), plane64(), e64(*d['Wc'].shape), e64(H16)
    lead, second = (t['X'], RH_w) if wide else (RH_w, t['X'])       # (the 16-wide plane leads; a narrow input plane rides second)
    EM.node_post_fwd(lead, t['Tc'], t['Wc'], t['bc'], A_w, B_w, X2=second)
    EM.node_post_bwd(lead, t['Tc'], t['Wc'], t['dA'], t['dB'], dX_w, dWc_w, dbc_w, X2=second, dX2=dX2_w if wide else None)
    g = {n: cu(v) for n, v in d.items()}
    Uc, Rc, RHc = cu(U_w.float()), cu(R_w.float()), cu(RH_w.float())
    plane = lambda: nan(nodes, C, H16)
    for k in formats(hip):
        tag = f'planar {point_id(p)} format {k.operand_format}'
        assert k.cell_planar_supported(2, 2, C, H16)
        U, R, RH = plane(), plane(), plane()
        k.cell_gates_fwd_planar(g['X'], g['H'], g['SX'], g['SH'], g['Tc'], g['Wg'], g['bg'], U, R, RH)
        for a, w, n in ((U, U_w, 'U'), (R, R_w, 'R'), (RH, RH_w, 'RH')):
            close(a, w, TOL, f'{tag} {n}')
        dZ = [plane() if (wide or i >= 2) else None for i in range(4)]
        dW, db, dH = nan(*d['Wg'].shape), nan(2 * H16), plane()
        k.cell_gates_bwd_planar(g['X'], g['H'], g['SX'], g['SH'], g['Tc'], g['Wg'], g['dRH'], g['Cand'], Uc, Rc, g['dHn'], dZ, dW, db, dH)
        for i, (a, w) in enumerate(zip(dZ, dZ_w)):
            assert (a is None) == (w is None)
            if a is not None:
                close(a, w, TOL, f'{tag} gates dZ[{i}]')
        close(dW, dW_w, TOL, f'{tag} gates dW')
        close(db, db_w, TOL, f'{tag} gates db')
        close(dH, dH_w, TOL, f'{tag} gates dH')
        dZf, dW2 = [plane() if (wide or i >= 2) else None for i in range(4)], nan(*d['Wg'].shape)      # dH = None: the share folded into the H plane's gradient
        k.cell_gates_bwd_planar(g['X'], g['H'], g['SX'], g['SH'], g['Tc'], g['Wg'], g['dRH'], g['Cand'], Uc, Rc, g['dHn'], dZf, dW2, None, None)
        assert torch.equal(dW, dW2), f'{tag}: gates dW differs on a second call'
        close(dZf[2], dZ_w[2] + dH_w, TOL, f'{tag} gates dZ[2] with the state share folded in')
        assert torch.equal(dZf[3], dZ[3])
        A, Bm = plane(), plane()
        lead_c, second_c = (g['X'], RHc) if wide else (RHc, g['X'])
        k.node_post_fwd(lead_c, g['Tc'], g['Wc'], g['bc'], A, Bm, X2=second_c)
        close(A, A_w, TOL, f'{tag} post A')
        close(Bm, B_w, TOL, f'{tag} post Bm')
        if k.cell_planar_post_fused(C):            # the same pair from the gates launch itself (candidate projection as its second stage)
            U2, R2, RH2, A2, B2 = (plane() for _ in range(5))
            k.cell_gates_fwd_planar(g['X'], g['H'], g['SX'], g['SH'], g['Tc'], g['Wg'], g['bg'], U2, R2, RH2, post=(g['Wc'], g['bc'], A2, B2))
            assert torch.equal(U2, U) and torch.equal(RH2, RH), f'{tag}: the fused second stage changes U / RH'
            close(A2, A_w, TOL, f'{tag} fused post A')
            close(B2, B_w, TOL, f'{tag} fused post Bm')
        dX, dX2, dWc, dbc = plane(), plane() if wide else None, nan(*d['Wc'].shape), nan(H16)
        k.node_post_bwd(lead_c, g['Tc'], g['Wc'], g['dA'], g['dB'], dX, dWc, dbc, X2=second_c, dX2=dX2)
        close(dX, dX_w, TOL, f'{tag} post dX')
        if wide:
            close(dX2, dX2_w, TOL, f'{tag} post dX2')
        close(dWc, dWc_w, TOL, f'{tag} post dW')
        close(dbc, dbc_w, TOL, f'{tag} post db')
        dWc2 = nan(*d['Wc'].shape)
        k.node_post_bwd(lead_c, g['Tc'], g['Wc'], g['dA'], g['dB'], dX, dWc2, None, X2=second_c, dX2=dX2)
        assert torch.equal(dWc, dWc2), f'{tag}: post dW differs on a second call'


def run_one_launch(hip, p, nodes=5):
    """stc_cell_bwd_planar_f32 with and without biases, both operand formats, against the twin on float64; the weight gradients a second time."""
    C, cin = p['C'], p['cin']
    wide = cin == H16
    d = planar_operands('one_launch', p, nodes)
    t = {n: d64(v) for n, v in d.items()}
    names = ('X', 'H', 'SX', 'SH', 'Tc', 'Wg', 'Wc', 'U', 'R', 'Cand', 'dHn', 'dBm')
    dZ_w = [e64(nodes, C, H16) if (wide or i >= 2) else None for i in range(4)]
    dWg_w, dbg_w, dWc_w, dbc_w = e64(*d['Wg'].shape), e64(2 * H16), e64(*d['Wc'].shape), e64(H16)
    EM.cell_bwd_planar(*[t[n] for n in names], dZ_w, dWg_w, dbg_w, dWc_w, dbc_w)
    operands = [cu(d[n]) for n in names]
    for k in formats(hip):
        tag = f'one-launch {point_id(p)} format {k.operand_format}'
        assert k.cell_bwd_planar_supported(C, H16)
        for bias in (True, False):
            dZ = [nan(nodes, C, H16) if (wide or i >= 2) else None for i in range(4)]
            dWg, dWc = nan(*d['Wg'].shape), nan(*d['Wc'].shape)
            dbg, dbc = (nan(2 * H16), nan(H16)) if bias else (None, None)
            k.cell_bwd_planar(*operands, dZ, dWg, dbg, dWc, dbc)
            for i, (a, w) in enumerate(zip(dZ, dZ_w)):
                assert (a is None) == (w is None)
                if a is not None:
                    close(a, w, TOL, f'{tag} dZ[{i}]')
            close(dWg, dWg_w, TOL, f'{tag} dWg')
            close(dWc, dWc_w, TOL, f'{tag} dWc')
            if bias:
                close(dbg, dbg_w, TOL, f'{tag} dbg')
                close(dbc, dbc_w, TOL, f'{tag} dbc')
            else:
                dWg2, dWc2 = nan(*d['Wg'].shape), nan(*d['Wc'].shape)
                k.cell_bwd_planar(*operands, dZ, dWg2, None, dWc2, None)
                assert torch.equal(dWg, dWg2) and torch.equal(dWc, dWc2), f'{tag}: the weight gradients differ on a second call'


def run_post(hip, p, nodes=5):
    """stc_bdg_node_post_fwd/bwd_f32 on interleaved rows [Xt | H | pad] against the twin on float64; 7.0 in the pad columns."""
    C, cin = p['C'], p['cin']
    Lw, L, K = cin + H16, row_width(cin), 2
    g = torch.Generator().manual_seed(seed_of('post', p))
    rnd = lambda *s: torch.randn(*s, generator=g)
    X = rnd(nodes, C, L)
    X[..., Lw:] = 7.0
    Tc = rnd(K, C, C) / C ** 0.5
    Tc[0] = torch.eye(C)
    W, b, dA, dB = rnd(K * K * Lw, H16) / (K * K * Lw) ** 0.5, rnd(H16), rnd(nodes, C, H16), rnd(nodes, C, H16)
    A_w, B_w, dX_w, dW_w, db_w = e64(nodes, C, H16), e64(nodes, C, H16), e64(nodes, C, L), e64(*W.shape), e64(H16)
    EM.node_post_fwd(X.double(), Tc.double(), W.double(), b.double(), A_w, B_w)
    EM.node_post_bwd(X.double(), Tc.double(), W.double(), dA.double(), dB.double(), dX_w, dW_w, db_w)
    tag = f'post {point_id(p)}'
    assert hip.node_post_supported(K, K, C, L, H16)
    A, Bm = nan(nodes, C, H16), nan(nodes, C, H16)
    hip.node_post_fwd(cu(X), cu(Tc), cu(W), cu(b), A, Bm)
    close(A, A_w, TOL, f'{tag} A')
    close(Bm, B_w, TOL, f'{tag} Bm')
    dX, dW, db = nan(nodes, C, L), nan(*W.shape), nan(H16)
    hip.node_post_bwd(cu(X), cu(Tc), cu(W), cu(dA), cu(dB), dX, dW, db)
    close(dX, dX_w, TOL, f'{tag} dX')
    close(dW, dW_w, TOL, f'{tag} dW')
    close(db, db_w, TOL, f'{tag} db')
    if L > Lw:
        assert float(dX[..., Lw:].abs().max()) == 0.0, f'{tag}: a pad column has a gradient'
    dW2 = nan(*W.shape)
    hip.node_post_bwd(cu(X), cu(Tc), cu(W), cu(dA), cu(dB), dX, dW2, None)
    assert torch.equal(dW, dW2), f'{tag}: dW differs on a second call'


# ---- few-category cell kernels ------------------------------------------------------------------------------------------------------------------
#: (dense graph, biases, splits) per point: a sparse and a dense graph, with and without biases, splits = 1 and one split form; order 3 with a dense
#: graph runs in the split form only, as the library requires (there ``splits = 1`` is the split form on one workgroup)
SMALL_FORMS = [(False, True, 1), (False, False, 2), (True, True, 1), (True, False, 2)]
SMALL_BATCH = 2


def small_operands(p, bias, dtype=torch.float32):
    """The operand conventions of tests/test_small_cell.py (``_inputs``: a row-stochastic category graph and its Chebyshev stack, weights at the
    pre-activation spread of the model) from the point's seed; the same float32 draws whatever ``dtype`` they are handed over in."""
    N = 2 * (16 // p['C']) + 1
    return N, _inputs(SMALL_BATCH, N, p['C'], p['cin'], seed=seed_of('small_cell', p) % (1 << 31), dtype=dtype, bias=bias, K=p['K'])


def small_graph(p, N, dense):
    return _graph(N, seed=seed_of('small_cell', p) % (1 << 31) + 1, dense=dense)


_SMALL_REF = {}


def small_reference(p, dense, bias, dtype=torch.float32):
    """``oracle.stc_oracle.stc_cell`` in float64 and its autograd: the gates, the candidate, the new state and every gradient; once per case
    (``dtype``: the one the operands were drawn and scaled in -- float32 for the library, float64 for the twin)."""
    key = (point_id(p), dense, bias, dtype)
    if key not in _SMALL_REF:
        N, t = small_operands(p, bias, dtype)
        Gs = small_graph(p, N, dense).to_dense().double()
        leaves = {n: t[n].double().requires_grad_(True) for n in ('X', 'H', 'Wg', 'Wc') + (('bg', 'bc') if bias else ())}
        pre = []

        def conv(X, Gs_, Gc_, W, b, Ks, Kc):               # (the oracle's own convolution, its pre-activations kept: gates first, candidate second)
            pre.append(O.bdg_dif(X, Gs_, Gc_, W, b, Ks, Kc))
            return pre[-1]
        Hnew = O.stc_cell(Gs, t['Gc'].double(), leaves['X'], leaves['H'], leaves['Wg'], leaves.get('bg'), leaves['Wc'], leaves.get('bc'), p['K'], p['K'], conv=conv)
        Hnew.backward(t['dHnew'].double())
        u, r = torch.sigmoid(pre[0].detach()).split(H16, -1)
        _SMALL_REF[key] = dict(Hnew=Hnew.detach(), U=u, R=r, Cand=torch.tanh(pre[1].detach()), **{'d' + n: v.grad for n, v in leaves.items()})
    return _SMALL_REF[key]


def small_step(k, p, dense, bias, splits, dev, dtype=torch.float32):
    """One cell step through kernel set ``k`` (the library, or the twin on float64 tensors): plain CPU tensors, the parameter-gradient rows summed."""
    N, t = small_operands(p, bias, dtype)
    C, cin, K = p['C'], p['cin'], p['K']
    graph = small_graph(p, N, dense)
    buf, P = _buffers(SMALL_BATCH, N, C, cin, dtype, k, K=K)
    to = lambda v: (v.to(dtype) if v.is_floating_point() else v).to(dev)
    if dense and K == 3:
        assert dtype == torch.float32
        op, f2, b2 = _dense_graphs(graph.to_dense(), dev)
        got = _step(k, op, f2, b2, t, buf, P, splits, dev)
        fill = 0.0
    else:
        op = dense_operand(graph.to_dense().to(dev)) if dense else csr_operand(graph, torch.device(dev))
        got = _run(k, op, t, buf, P, to, splits=splits)
        fill = 0.125                                                # (``_run`` starts every partial row there: the launch adds to it)
    dWg, dbg, dWc, dbc, rest = _split_params(got['dP'], cin, K=K)
    assert bool((rest == fill).all()), 'the columns beyond the parameters were written'
    start = fill * got['dP'].shape[0]
    got.update(dWg=dWg - start, dbg=dbg - start, dWc=dWc - start, dbc=dbc - start)
    return got


def check_small(tag, got, want, bias, fwd_bound, grad_bound):
    for n in ('U', 'R', 'Cand', 'Hnew'):
        close(got[n], want[n], fwd_bound, f'{tag} {n}')
    for n in ('dX', 'dH', 'dWg', 'dWc') + (('dbg', 'dbc') if bias else ()):
        close(got[n], want[n], grad_bound, f'{tag} {n}')
    if not bias:
        assert float(got['dbg'].abs().max()) == 0.0 and float(got['dbc'].abs().max()) == 0.0, f'{tag}: an absent bias has a gradient'


def run_small(hip, p):
    C, cin, K = p['C'], p['cin'], p['K']
    N = 2 * (16 // C) + 1
    assert hip.cell_small_supported(K, K, C, cin, H16, N)
    for dense, bias, splits in SMALL_FORMS:
        tag = f'small {point_id(p)} dense={dense} bias={bias} splits={splits}'
        # the hand-picked test of the form: tests/test_small_dense_order3.py for a dense graph at order 3, tests/test_small_cell.py otherwise
        fwd_bound, grad_bound = (FWD_CELL, GRAD_CELL) if (dense and K == 3) else (SMALL_TOL, SMALL_TOL)
        got = small_step(hip, p, dense, bias, splits, 'cuda')
        check_small(tag, got, small_reference(p, dense, bias), bias, fwd_bound, grad_bound)
        if bias:
            again = small_step(hip, p, dense, bias, splits, 'cuda')
            assert torch.equal(got['dP'], again['dP']), f'{tag}: the parameter-gradient rows differ on a second call'


def twin_small(p):
    """CPU: the twin on float64 tensors against the float64 oracle cell, sparse and dense graph (the dense form of order 3 exists in the library
    only: its twin is the sparse form on the same matrix)."""
    for dense, bias, splits in SMALL_FORMS:
        if dense and p['K'] == 3:
            continue
        got = small_step(EM, p, dense, bias, 1, 'cpu', torch.float64)
        check_small(f'twin small {point_id(p)} dense={dense}', got, small_reference(p, dense, bias, torch.float64), bias, TWIN_IS_REFERENCE, TWIN_IS_REFERENCE)


# ---- riders --------------------------------------------------------------------------------------------------------------------------------------
def run_cheby(hip, p):
    """stc_cheby_dense_fwd/bwd_f32 against the twin on float64 (the recurrence T_k = 2 G T_{k-1} - T_{k-2} and its autograd)."""
    n, K = p['n'], p['K']
    g = torch.Generator().manual_seed(seed_of('cheby', p))
    G = torch.randn(n, n, generator=g) / n ** 0.5
    dT = torch.randn(K, n, n, generator=g)
    G64 = G.double().requires_grad_()
    T64 = torch.stack(O.cheby_poly(G64, K)[:K])
    T_w, dG_w = e64(K, n, n), e64(n, n)
    EM.cheby_dense_fwd(G.double(), K, T_w)
    EM.cheby_dense_bwd(G.double(), T_w, dT.double().clone(), dG_w)
    tag = f'cheby {point_id(p)}'
    close(T_w, T64.detach(), TWIN_IS_REFERENCE, f'{tag} twin T')
    if K > 1:
        T64.backward(dT.double())
        close(dG_w, G64.grad, TWIN_IS_REFERENCE, f'{tag} twin dG')
    T = nan(K, n, n)
    hip.cheby_dense_fwd(cu(G), K, T)
    close(T, T_w, TOL, f'{tag} T')
    dG = nan(n, n)
    hip.cheby_dense_bwd(cu(G), cu(T_w.float()), cu(dT.clone()), dG)
    if K > 1:
        close(dG, dG_w, TOL, f'{tag} dG')
    else:
        assert float(dG.abs().max()) == 0.0, f'{tag}: T_0 = I has no gradient'



def run_fusion(p):
    """stc_mixed_fusion_fwd/bwd_f32 through ``ops.mixed_fusion`` against float64 autograd of the reference's own expression (STC_GNN.py:246-261), as
    test_mixed_fusion has it.  The float64 side runs as plain torch on the device, and forms no (n^2, n^2) gradient (2 GiB each at n = 128): autograd
    gives the pre-activation's gradient dz, and the gradient of a weight matrix that enters as W @ x is the outer product of dz and x, compared
    block of rows by block of rows under the same max-norm ``rel_err``."""
    n = p['n']
    D = n * n
    g = torch.Generator(device='cuda').manual_seed(seed_of('fusion', p))
    rnd = lambda *s: torch.randn(*s, generator=g, device='cuda')
    A, P = torch.rand(n, n, generator=g, device='cuda'), torch.softmax(rnd(n, n), -1)
    WA, WP = rnd(D, D) * (1.0 / D) ** 0.5, rnd(D, D) * (1.0 / D) ** 0.5
    bA, bP, R = rnd(D) * 0.1, rnd(D) * 0.1, rnd(n, n)
    ref = [t.double().requires_grad_(i not in (2, 4)) for i, t in enumerate((A, P, WA, bA, WP, bP))]
    z = ref[2] @ ref[0].reshape(D) + ref[3] + ref[4] @ ref[1].reshape(D) + ref[5]
    z.retain_grad()
    a = torch.sigmoid(z).reshape(n, n)
    Gref = a * ref[0] + (1 - a) * ref[1]
    (Gref * R.double()).sum().backward()
    dz = z.grad
    ref[2] = ref[4] = None                                          # (the float64 copies of the weights are not needed beyond this point)
    dev = [t.requires_grad_() for t in (A, P, WA, bA, WP, bP)]
    assert ops.mixed_fusion_supported(*dev), f'fusion n={n}: the predicate declines a point of the box'
    G = ops.mixed_fusion(*dev)
    (G * R).sum().backward()
    close(G.detach(), Gref.detach(), TOL, f'fusion n={n} G')
    for name, i in (('dA', 0), ('dP', 1), ('dbA', 3), ('dbP', 5)):
        close(dev[i].grad, ref[i].grad, FUSION_GRAD, f'fusion n={n} {name}')
    for name, i, x in (('dWA', 2, A), ('dWP', 4, P)):
        x64, got, worst = x.detach().double().reshape(1, D), dev[i].grad, 0.0
        assert bool(torch.isfinite(got).all()), f'fusion n={n} {name}: a non-finite gradient'
        for lo in range(0, D, 2048):
            worst = max(worst, float((got[lo:lo + 2048].double() - dz[lo:lo + 2048, None] * x64).abs().max()))
        err = worst / float(dz.abs().max() * x64.abs().max())          # (max |dz x^T| = max |dz| max |x|)
        print(f'fusion n={n} {name}: {err:.3e} (bound {FUSION_GRAD:.1e})')
        assert err < FUSION_GRAD, f'fusion n={n} {name}: relative error {err:.3e} >= {FUSION_GRAD:.1e}'
