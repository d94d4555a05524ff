"""Guard bands around every kernel operand: where a launch writes and reads, the minimum alignment and scratch the ABI allows, and the
maxima nobody reads back (include/stc_hip.h promises each; the value-parity tests assert none).

The harness is device-agnostic: it runs a kernel set ``k`` (``HipKernels`` on the GPU, ``EmulatedKernels`` on the CPU) twice per case --
once on plain torch allocations, once on BANDED operands -- and compares.

``Bands.band(t)`` places an operand of ``t``'s shape inside one larger flat allocation:
  * the view starts at a byte offset = 16 (mod 128): legal by the header ("16-byte aligned") and nothing more -- torch's own allocations
    are 512-byte aligned, so no other test runs below 128;
  * margins of at least max(1024 elements, two rows of the operand) on either side (row = product of all dimensions but the first), so
    that a write one whole row off still lands in a margin of the test's own allocation: the failure mode is an assertion, never a fault;
  * INPUT margins hold quiet NaN: a read past the operand that reaches arithmetic -- even times a zero weight -- shows as a non-finite
    result (a read that a select masks does not show, and is harmless);
  * OUTPUT / in-out margins hold a fixed non-NaN bit pattern and are compared as integer bits after the launch and a synchronize; the
    interior is NaN wherever the header says "overwritten".
Scratch: the instance's ``_get_workspace`` is replaced by one that hands out a banded uint8 view of EXACTLY the requested byte count (the
production one never passes less than 1 MiB), and the three fronts that allocate their own scratch and results (mixed fusion, the MGP
front, graph_grad / mix_grad without ``into=``) see a ``torch`` whose ``empty`` / ``empty_like`` band what they return -- no production
caller changes.

NOT banded, on purpose: the integer index arrays (rowptr, colidx, the row-block / patch / two-ring plan tables, patch_idx).  A garbage index
read from a margin would turn into a wild address, and this file must never be able to cause a fault.  The float tables that travel with a
host-built plan (blk_vals, patch_val, t1 / t2 value bits) stay plain with their plan.

Per case: every margin (operands and scratch) keeps its bits; the interior of every 'in' operand -- ``const`` in the header -- keeps its
bits too (the one operand the header declares consumed, dT of stc_cheby_dense_bwd_f32, is 'io'); every result the header says is written is finite; the results equal, bit
for bit, the same launch on plain tensors (no kernel may choose its path by alignment above 16 bytes; the dW / db / dTc sums are
fixed-order); the results are within the family's existing tolerance of the CPU twin run in float64 (``TOL`` / ``BTOL`` / ``BOUND`` of the
family's own test file -- no new numbers).

Coverage: ``test_every_entry_point_has_a_banded_case`` walks ``_lib``'s ctypes table; every entry that takes a device buffer must be named
by a case here or by ``NO_BANDED_CASE`` below with its reason.  On the GPU each case also asserts that the entries it names were launched.
``NO_BANDED_CASE`` is empty today.  Two things a case does not compare, by the header's own words: stc_cheby_dense_bwd_f32's dT is scratch that
the launch destroys (margins checked, final content not compared), and dTc[0] of the node backward / stc_mix_dt_f32 is WRITTEN as zero (T_0 = I is
a constant) where the twin's first matrix is the plain product -- compared from dTc[1:] on, dTc[0] == 0 asserted.  The fronts that allocate their
own results are banded through the substituted ``torch``; each case states how many such buffers it expects (``fronts=``) and fails when another
number was banded, and a front that allocates through any other torch factory raises.
"""
import importlib
import math
import pkgutil

import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, _lib
from stc_hip.graph import csr_operand, full_pattern
from tests.conftest import rel_err
from tests.test_bf16_kernels import BTOL
from tests.test_grad_scale import BOUND
from tests.test_hip_kernels import TOL

#: entry points with a device buffer that CANNOT or MUST NOT be banded, and the technical reason (none today)
NO_BANDED_CASE = {}

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_PATTERN = {1: 0x5A, 2: 0x4B4B, 4: 0x4B4B4B4B, 8: 0x4B4B4B4B4B4B4B4B}       # non-NaN in every float format of that size
MIN_MARGIN = 1024


class Bands:
    """The banded allocations of one run and their margin snapshots."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.items = []                  # (name, integer view of the flat allocation, start, numel, margin bits before the launch)

    def band(self, shape, dtype, kind, name, margin=None):
        """An uninitialised contiguous view of ``shape`` inside a larger flat allocation; ``kind``: 'in' (NaN margins) or 'out' (bit pattern)."""
        shape = tuple(shape)
        es = torch.empty(0, dtype=dtype).element_size()
        n = math.prod(shape)
        row = math.prod(shape[1:]) if len(shape) > 1 else 1
        m = max(MIN_MARGIN, 2 * row) if margin is None else margin
        flat = torch.empty(2 * m + n + 256 // es, dtype=dtype, device=self.device)
        shift = (16 - (flat.data_ptr() + m * es)) % 128
        assert shift % es == 0
        start = m + shift // es
        bits = flat.view(_BITS[es])
        if kind == 'in' and dtype.is_floating_point:
            flat.fill_(float('nan'))
        else:
            bits.fill_(_PATTERN[es])
        view = flat[start:start + n].view(shape)
        assert (n == 0 or view.data_ptr() % 128 == 16) and view.is_contiguous() and start >= m and bits.numel() - start - n >= m
        self.items.append([name, bits, start, n, None])
        return view

    def snapshot(self):
        for it in self.items:
            if it[4] is None:
                it[4] = (it[1][:it[2]].clone(), it[1][it[2] + it[3]:].clone())

    def violations(self):
        """Names of the allocations whose margins changed (call after a synchronize)."""
        bad = []
        for name, bits, start, n, snap in self.items:
            if not (torch.equal(bits[:start], snap[0]) and torch.equal(bits[start + n:], snap[1])):
                bad.append(name)
        return bad


class _BandingTorch:
    """``torch`` as the fronts that allocate their own results and scratch see it during a banded run: ``empty`` / ``empty_like`` return
    banded views (NaN interior, so that a result or scratch word read before it is written shows), everything else is torch's."""

    def __init__(self, bands):
        self._bands = bands

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=torch.float32, device=None, **other):
        assert not other, f'torch.empty({other}): not banded'
        size = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else size
        assert torch.device(device).type == self._bands.device.type
        t = self._bands.band(size, dtype, 'out', f'front-allocated{size}')
        if dtype.is_floating_point:
            t.fill_(float('nan'))
        return t

    def empty_like(self, t):
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)

    def _unbanded(self, *a, **kw):
        raise AssertionError('a front allocates through a torch factory the harness does not band: teach _BandingTorch about it')

    zeros = zeros_like = ones = full = full_like = empty_strided = rand = randn = _unbanded


class Case:
    """One launch (or a front's few launches) on operands described by ``make() -> {name: (role, value)}``:
         'in'   input tensor (NaN margins)                'out'  overwritten result: the value gives shape / dtype, the interior starts as NaN
         'io'   in / out tensor with initial values       'idx'  integer index array or plan table: moved to the device, never banded
         'arg'  anything else, passed through
    a value may be a list / tuple (of tensors or None).  ``call(k, t)`` runs it on kernel set ``k`` with ``t.<name>`` realised; what it
    returns (tensors a front allocated itself) is compared as well.  ``entries``: the C entry points the case launches on the GPU."""

    def __init__(self, id, entries, make, call, tol=TOL, level=0, fmt=None, cpu=False, check=None, unwritten=(), bitwise=True, twin=True, patch=False, reduce=None, tols=None, fronts=0, zeros=False):
        self.id, self.entries, self.make, self.call = id, frozenset(entries), make, call
        self.tol, self.level, self.fmt, self.cpu, self.check = tol, level, fmt, cpu, check
        self.unwritten, self.bitwise, self.twin, self.patch = frozenset(unwritten), bitwise, twin, patch
        self.tols = tols or {}                # name -> its own bound against the twin where the family's test has one (default: tol)
        self.fronts = fronts                  # buffers the fronts allocate themselves during the call: each must have been banded
        self.zeros = zeros                    # nodes == 0: every result is memset -- exactly its own floats, all zero
        self.reduce = reduce or {}            # name -> the part of a result that the twin defines (applied to both sides)


class _Ops:
    pass


def _map(value, fn):
    if isinstance(value, (list, tuple)):
        return type(value)(_map(v, fn) for v in value)
    return None if value is None else fn(value)


def _realise(spec, mode, device, bands=None):
    """The operands of one run: mode 'plain' (torch allocations on ``device``), 'banded', or 'twin' (CPU, fp32 widened to float64)."""
    t = _Ops()
    # bf16 storage: the family's bound (BTOL) is against the fp32 twin on the same bf16-valued inputs, so its fp32 parameters are not widened
    leaves = [x for _, v in spec.values() for x in (v if isinstance(v, (list, tuple)) else [v]) if isinstance(x, torch.Tensor)]
    widen = not any(x.dtype == torch.bfloat16 for x in leaves)
    for name, (role, value) in spec.items():
        def one(v, role=role, name=name):
            if role == 'arg' or not isinstance(v, torch.Tensor):
                return v
            if mode == 'twin':
                w = v.double() if (widen and v.dtype == torch.float32) else v.clone()
                return torch.full_like(w, float('nan')) if role == 'out' else w
            if role == 'idx':
                return v.to(device)
            if mode == 'plain':
                return torch.full(v.shape, float('nan'), dtype=v.dtype, device=device) if role == 'out' else v.to(device).clone()
            b = bands.band(v.shape, v.dtype, 'in' if role == 'in' else 'out', name)
            b.fill_(float('nan')) if role == 'out' else b.copy_(v)
            return b
        setattr(t, name, _map(value, one))
    return t


def _flat(spec, t, returned):
    """[(name, role, tensor)] of every tensor operand of a run, front-allocated results included."""
    out = []
    for name, (role, _) in spec.items():
        v = getattr(t, name)
        vs = v if isinstance(v, (list, tuple)) else [v]
        out += [(f'{name}[{i}]' if len(vs) > 1 else name, role, x) for i, x in enumerate(vs) if isinstance(x, torch.Tensor)]
    if returned is not None:
        rs = returned if isinstance(returned, (list, tuple)) else [returned]
        out += [(f'returned[{i}]', 'out', x) for i, x in enumerate(rs) if isinstance(x, torch.Tensor)]
    return out


def _bits(x):
    return x.contiguous().view(_BITS[x.element_size()])


def run_case(case, k, device, monkeypatch, twin=None):
    """Run ``case`` on kernel set ``k``: plain, banded, and (``twin``: a CPU kernel set) in float64; returns the list of findings (empty = pass)."""
    device = torch.device(device)
    on_gpu = device.type == 'cuda'
    spec = case.make()
    launched = []
    if on_gpu:
        real_launch = k._launch
        monkeypatch.setattr(k, '_launch', lambda name, *a, **kw: (launched.append(name), real_launch(name, *a, **kw))[1])
        if case.fmt is not None:
            monkeypatch.setattr(k, 'operand_format', {'f16x2': _lib.FMT_F16X2, 'bf16x3': _lib.FMT_BF16X3}[case.fmt], raising=False)
        if case.patch:
            monkeypatch.setattr(k, 'patch_min_items', 0, raising=False)
        k.set_dispatch_level(case.level)
    findings = []
    try:
        plain = _realise(spec, 'plain', device)
        plain_ret = case.call(k, plain)
        bands = Bands(device)
        banded = _realise(spec, 'banded', device, bands)
        if on_gpu:
            def scratch(dev, nbytes):                       # exactly what the workspace query asks for; margins wide enough for an under-reporting query
                return bands.band((nbytes,), torch.uint8, 'out', f'workspace({nbytes})', margin=min(max(4096, nbytes), 1 << 24))
            monkeypatch.setattr(k, '_get_workspace', scratch, raising=False)
            monkeypatch.setattr(_lib, 'torch', _BandingTorch(bands))
        bands.snapshot()
        const = [(name, x, _bits(x).clone()) for name, role, x in _flat(spec, banded, None) if role == 'in']    # const operands: their bits before the launch
        try:
            banded_ret = case.call(k, banded)
            if on_gpu:
                torch.cuda.synchronize()
        finally:
            if on_gpu:
                monkeypatch.setattr(_lib, 'torch', torch)
        bands.snapshot()                                    # (front-allocated buffers: banded during the call, nothing ran before they existed)
    finally:
        if on_gpu:
            k.set_dispatch_level(0)
    findings += [f'margin of {name} changed' for name in bands.violations()]
    findings += [f'input {name} was modified by the launch' for name, x, before in const if not torch.equal(_bits(x), before)]
    got, ref = _flat(spec, banded, banded_ret), _flat(spec, plain, plain_ret)
    assert [g[0] for g in got] == [r[0] for r in ref]
    want = None
    if twin is not None and case.twin:
        tw = _realise(spec, 'twin', 'cpu')
        want = _flat(spec, tw, case.call(twin, tw))
    for i, (name, role, x) in enumerate(got):
        if role not in ('out', 'io'):
            continue
        base = name.split('[')[0]
        if base in case.unwritten or name in case.unwritten:
            continue
        if x.numel() == 0:
            continue
        if case.zeros and not bool((x == 0).all()):
            findings.append(f'{name}: not all zero after a launch over zero nodes')
            continue
        if not bool(torch.isfinite(x.float() if x.dtype != torch.float64 else x).all()):
            findings.append(f'{name}: non-finite result on banded operands')
            continue
        if case.bitwise and not torch.equal(_bits(x), _bits(ref[i][2])):
            findings.append(f'{name}: differs from the launch on plain tensors (rel {rel_err(x.double(), ref[i][2].double()):.2e})')
        elif not case.bitwise and rel_err(x.double(), ref[i][2].double()) >= case.tol:
            findings.append(f'{name}: differs from the launch on plain tensors beyond {case.tol}')
        if want is not None and name.startswith('returned') is False:
            part = case.reduce.get(base, lambda v: v)
            bound = case.tols.get(base, case.tol)
            e = rel_err(part(x.double()), part(want[i][2].double()))
            if not e < bound:
                findings.append(f'{name}: {e:.2e} from the float64 twin (bound {bound})')
    if case.check is not None:
        findings += case.check(banded, banded_ret) or []
    n_fronts = sum(it[0].startswith('front-allocated') for it in bands.items)
    if on_gpu and n_fronts != case.fronts:
        findings.append(f'{n_fronts} front-allocated buffers were banded, the case expects {case.fronts}: a front allocates in a way the harness does not see')
    if on_gpu and not case.entries <= set(launched):
        findings.append(f'launched {sorted(set(launched))}, the case names {sorted(case.entries)}')
    return findings


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
NODES = (1, 3, 13, 50, 4500)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _mix(g, K, C):
    Tc = torch.randn(K, C, C, generator=g) / C ** 0.5
    Tc[0] = torch.eye(C)
    return Tc


def _random_csr(n_rows, n_cols, density, seed):
    """CSR with an empty second and an empty LAST row."""
    g = _g(seed)
    mask = torch.rand(n_rows, n_cols, generator=g) < density
    mask[n_rows - 1] = False
    if n_rows > 2:
        mask[1] = False
    vals = torch.randn(n_rows, n_cols, generator=g) * mask
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(mask.sum(1), 0)
    return rowptr.to(torch.int32), mask.nonzero()[:, 1].to(torch.int32).contiguous(), vals[mask].contiguous()


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


# ---- aggregations -------------------------------------------------------------------------------------------------------------------------
def _spmm_csr(n_rows, n_cols, F, B, beta, dt, inplace):
    def make():
        rp, ci, val = _random_csr(n_rows, n_cols, 0.3, n_rows + F)
        g = _g(F)
        X, Y0 = torch.randn(B, n_cols, F, generator=g).to(dt), torch.randn(B, n_rows, F, generator=g).to(dt)
        spec = dict(rp=('idx', rp), ci=('idx', ci), val=('in', val), X=('in', X))
        if inplace:
            spec['Y'] = ('io', Y0)
        else:
            spec['Y'] = ('out', Y0)
            if beta:
                spec['Y0'] = ('in', Y0)
        return spec

    def call(k, t):
        y0 = t.Y if inplace else getattr(t, 'Y0', None)
        k.csr_spmm(t.rp, t.ci, t.val, n_rows, n_cols, t.X, y0, t.Y, 2.0 if beta else 1.0, beta)
    return make, call


for dt, tag, tol in ((torch.float32, 'f32', TOL), (torch.bfloat16, 'bf16', BTOL)):
    for n_rows, n_cols, F, B, beta, inplace in ((37, 37, 85 if tag == 'f32' else 88, 2, 0.0, False), (37, 50, 1024, 1, -1.0, False),
                                                (37, 37, 160, 2, -1.0, True), (5, 7, 3 if tag == 'f32' else 8, 1, 0.0, False)):
        case(f'csr_spmm_{tag}-{n_rows}x{n_cols}-F{F}-beta{beta}{"-inplace" if inplace else ""}', {f'stc_csr_spmm_{tag}'},
             *_spmm_csr(n_rows, n_cols, F, B, beta, dt, inplace), tol=tol, cpu=(F == 85))


def _grid_graph(H, W, permute=None):
    graph = CsrGraph.queen_grid(H, W, normalize=True, permute_seed=permute)
    if permute is not None:
        graph = graph.with_locality()[0]
    return graph


def _banded_matrix(n, hw, seed):
    """A banded random matrix with an empty fourth and an empty LAST row; n % 4 != 0 gives the row-blocked kernels a ragged last block."""
    g = _g(seed)
    i = torch.arange(n)
    M = ((i[:, None] - i[None, :]).abs() <= hw) & (torch.rand(n, n, generator=g) < 0.7)
    M[3] = False
    M[n - 1] = False
    return CsrGraph.from_dense(torch.randn(n, n, generator=g) * M)


def _spmm_plan(graph_fn, F, B, beta, dt, inplace, side='fwd'):
    def make():
        graph = graph_fn()
        n = graph.n
        g = _g(F + n)
        X, Y0 = torch.randn(B, n, F, generator=g).to(dt), torch.randn(B, n, F, generator=g).to(dt)
        spec = dict(graph=('arg', graph), X=('in', X), Y=('io' if inplace else 'out', Y0))
        if beta and not inplace:
            spec['Y0'] = ('in', Y0)
        return spec

    def call(k, t):
        op = csr_operand(t.graph, t.X.device)
        y0 = t.Y if inplace else getattr(t, 'Y0', None)
        k.csr_spmm(getattr(op, side + '_rowptr'), getattr(op, side + '_colidx'), getattr(op, side + '_val'), op.n, op.n, t.X, y0, t.Y,
                   2.0 if beta else 1.0, beta, plan=getattr(op, side + '_plan'))
    return make, call


for dt, tag, tol in ((torch.float32, 'f32', TOL), (torch.bfloat16, 'bf16', BTOL)):
    for n, F, B, beta, inplace in ((37, 64, 2, 0.0, False), (203, 1024, 1, -1.0, True), (77, 16, 2, -1.0, False), (30, 2048, 1, 0.0, False)):
        case(f'bcsr_spmm_{tag}-n{n}-F{F}-beta{beta}{"-inplace" if inplace else ""}', {f'stc_bcsr_spmm_{tag}'},
             *_spmm_plan(lambda n=n, F=F: _banded_matrix(n, 4, n + F), F, B, beta, dt, inplace), tol=tol, cpu=(n == 37 and tag == 'f32'))
    # every arm of the row-blocked ladder (csrc/stc_spmm_gather.h launch_gather.  fp32 rows: float4 per lane 1 / 2 / 4, pipelined gather for beta = 0 and
    # whole column blocks, old loop otherwise; bf16 rows of <= 512, <= 1024, more columns), at the smallest shape with a ragged block
    for F, beta in ((512, 0.0), (320, 0.0), (1024, 0.0), (1280, -1.0)) if tag == 'f32' else ((512, 0.0), (1024, 0.0), (2048, 0.0)):
        case(f'bcsr_spmm_{tag}-n37-F{F}-beta{beta}-ladder', {f'stc_bcsr_spmm_{tag}'},
             *_spmm_plan(lambda F=F: _banded_matrix(37, 4, 37 + F), F, 2, beta, dt, False), tol=tol)
    Fp = 256 if tag == 'f32' else 512
    for (H, W, permute), B, beta, inplace, side in (((17, 41, None), 2, 0.0, False, 'fwd'), ((17, 41, None), 1, -1.0, True, 'bwd'),
                                                    ((40, 40, 7), 1, -1.0, False, 'fwd'), ((40, 40, 7), 1, 0.0, False, 'bwd')):
        case(f'patch_spmm_{tag}-{H}x{W}{"-renumbered" if permute else ""}-{side}-beta{beta}{"-inplace" if inplace else ""}', {f'stc_patch_spmm_{tag}'},
             *_spmm_plan(lambda H=H, W=W, permute=permute: _grid_graph(H, W, permute), Fp, B, beta, dt, inplace, side), tol=tol, patch=True)


def _dense_agg(n, F, B, beta):
    def make():
        g = _g(n + F)
        S = torch.softmax(torch.randn(n, n, generator=g), -1)
        X, Y0 = torch.randn(B, n, F, generator=g), torch.randn(B, n, F, generator=g)
        return dict(S=('in', S.reshape(-1)), X=('in', X), Y=('io', Y0))

    def call(k, t):
        rp, ci = full_pattern(n, t.X.device)
        k.csr_spmm(rp, ci, t.S, n, n, t.X, t.Y if beta else None, t.Y, 2.0 if beta else 1.0, beta)
    return make, call


for n, F, B, beta in ((37, 7, 1, 0.0), (37, 7, 2, -1.0), (100, 100, 3, -1.0), (100, 100, 1, 0.0)):
    case(f'dense_agg-n{n}-F{F}-beta{beta}', {'stc_dense_agg_f32'}, *_dense_agg(n, F, B, beta))


def _sddmm(n, F, B, accumulate):
    def make():
        rp, ci, _ = _random_csr(n, n, 0.4, n + F)
        g = _g(n)
        return dict(rp=('idx', rp), ci=('idx', ci), A=('in', torch.randn(B, n, F, generator=g)), Bm=('in', torch.randn(B, n, F, generator=g)),
                    out=('io' if accumulate else 'out', torch.randn(ci.numel(), generator=g)))

    def call(k, t):
        k.csr_sddmm(t.rp, t.ci, n, n, t.A, t.Bm, t.out, 2.0, accumulate)
    return make, call


for n, F, B in ((33, 85, 2), (50, 256, 3), (12, 7, 1)):
    for accumulate in (False, True):
        # out[j] is one wave's sum, written once: reproducible, compared bit for bit
        case(f'sddmm-n{n}-F{F}-{"acc" if accumulate else "write"}', {'stc_csr_sddmm_f32'}, *_sddmm(n, F, B, accumulate), cpu=(n == 12))


def _state_planes(g, B, n, C, h=16, dt=torch.float32):
    rnd = lambda: torch.randn(B, n, C, h, generator=g)
    return rnd, (lambda: torch.sigmoid(rnd()).to(dt)), (lambda: torch.tanh(rnd()).to(dt))


def _spmm_sum(H, W, B, C, n_add, dual, blend, dt, strided=False, alpha=1.0):
    h = 16

    def make():
        graph = _grid_graph(H, W)
        rnd, unit, tanh = _state_planes(_g(H * W + n_add), B, graph.n, C, h, dt)
        spec = dict(graph=('arg', graph), X=('in', rnd().to(dt)), Y=('out', rnd().to(dt)), adds=('in', [rnd().to(dt) for _ in range(n_add)]))
        if strided:                                         # an addend that is columns [16, 32) of rows of 32 floats, scaled
            spec['wide'] = ('in', torch.randn(B, graph.n, C, 2 * h, generator=_g(5)))
        if dual:
            spec['X2'] = ('in', rnd().to(dt))
        if blend:
            spec.update(U=('in', unit()), Cand=('in', tanh()), dY=('out', rnd().to(dt)))
        return spec

    def call(k, t):
        op = csr_operand(t.graph, t.X.device)
        adds = [(a, 0) for a in t.adds] + ([(t.wide, h, -1.0)] if strided else [])
        kw = dict(alpha=alpha) if dt == torch.float32 else {}
        (k if dt == torch.float32 else k.bf16).spmm_sum(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, op.bwd_plan[:3], t.X, getattr(t, 'X2', None), adds, t.Y,
                                                        blend=(t.U, t.Cand, t.dY) if blend else None, **kw)
    return make, call


for dt, tag, tol in ((torch.float32, 'f32', TOL), (torch.bfloat16, 'bf16', BTOL)):
    for H, W, B, C, n_add, dual, blend in ((5, 5, 2, 32, 3, True, True), (4, 7, 1, 64, 5, False, False), (1, 1, 1, 32, 2, False, True), (9, 33, 1, 32, 0, True, True)):
        case(f'spmm_sum_{tag}-{H}x{W}-C{C}-add{n_add}{"-dual" if dual else ""}{"-blend" if blend else ""}', {f'stc_spmm_sum_{tag}'},
             *_spmm_sum(H, W, B, C, n_add, dual, blend, dt), tol=tol, cpu=(H == 5 and tag == 'f32'))
    # C = 128: rows of 2048 columns, the widest arm of both dispatch ladders
    case(f'spmm_sum_{tag}-4x7-C128-add2-blend', {f'stc_spmm_sum_{tag}'}, *_spmm_sum(4, 7, 1, 128, 2, False, True, dt), tol=tol)
case('spmm_sum_f32-4x7-strided-addend-alpha2', {'stc_spmm_sum_f32'}, *_spmm_sum(4, 7, 2, 32, 1, False, False, torch.float32, strided=True, alpha=2.0))


def _copy_checks(names_cols):
    """Column slices of wider rows: everything outside the columns a launch owns keeps the bits it had (9.0)."""
    def check(t, _):
        bad = []
        for name, own in names_cols.items():
            buf = getattr(t, name)
            keep = [c for c in range(buf.shape[-1]) if c not in own]
            if keep and not bool((buf[..., keep] == 9.0).all()):
                bad.append(f'{name}: columns outside {sorted(own)[0]}..{sorted(own)[-1]} changed')
        return bad
    return check


def _spmm_blend(H, W, B, C, dt, copies, blocked=True):
    h = 16

    def make():
        graph = _grid_graph(H, W)
        n = graph.n
        rnd, unit, tanh = _state_planes(_g(H * W + C), B, n, C, h, dt)
        spec = dict(graph=('arg', graph), Bm=('in', rnd().to(dt)), A=('in', rnd().to(dt)), U=('in', unit()), Hp=('in', tanh()),
                    Cand=('out', rnd().to(dt)), Hnew=('out', rnd().to(dt)))
        if copies == 'pair':
            spec.update(c0=('io', torch.full((B * n, C, 32), 9.0)), c1=('io', torch.full((B * n, C, 32), 9.0)))
        if copies == 'side':
            spec.update(c0=('io', torch.full((B * n, C, 20), 9.0)), side=('in', torch.randn(B * n, C, 1, generator=_g(3))))
        return spec

    def call(k, t):
        op = csr_operand(t.graph, t.Bm.device)
        kw = {}
        if copies == 'pair':
            kw = dict(copies=[(t.c0, 16), (t.c1, 0)])
        if copies == 'side':
            kw = dict(copies=[(t.c0, 1)], side=t.side)
        (k if dt == torch.float32 else k.bf16).spmm_blend_fwd(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, op.fwd_plan[:3] if blocked else None, t.Bm, t.A, t.U, t.Hp, t.Cand, t.Hnew, **kw)
    # side: columns [0, 1) from side, [1, 17) the state, pad [17, 20) zeroed -- the launch owns the whole row
    check = _copy_checks({'c0': range(16, 32), 'c1': range(0, 16)}) if copies == 'pair' else None
    return dict(make=make, call=call, check=check)


for H, W, B, C, copies in ((5, 5, 2, 32, 'pair'), (4, 7, 3, 32, 'side'), (3, 3, 1, 64, None), (1, 1, 1, 32, None), (9, 33, 1, 32, 'pair')):
    case(f'spmm_blend_f32-{H}x{W}-C{C}-{copies}', {'stc_spmm_blend_fwd_f32'}, **_spmm_blend(H, W, B, C, torch.float32, copies), cpu=(H == 4))
# the other pieces-per-lane arms of the launch ladder: rows of 320 float4 (C = 80, the widest) on the row-blocked kernel, and 320, 256, 128 and 64 on
# the wave-per-row kernel (no row-block plan)
for C, blocked in ((80, True), (80, False), (64, False), (32, False), (16, False)):
    case(f'spmm_blend_f32-5x5-C{C}-{"blocked" if blocked else "csr"}', {'stc_spmm_blend_fwd_f32'}, **_spmm_blend(5, 5, 2, C, torch.float32, None, blocked))
for H, W, B, C in ((5, 5, 2, 32), (4, 7, 1, 64), (1, 1, 1, 32)):
    case(f'spmm_blend_bf16-{H}x{W}-C{C}', {'stc_spmm_blend_fwd_bf16'}, **_spmm_blend(H, W, B, C, torch.bfloat16, None), tol=BTOL)
case('spmm_blend_f32-4x7-C128-None', {'stc_spmm_blend_fwd_f32'}, **_spmm_blend(4, 7, 1, 128, torch.float32, None))          # C = 128: the widest arm
case('spmm_blend_bf16-4x7-C128', {'stc_spmm_blend_fwd_bf16'}, **_spmm_blend(4, 7, 1, 128, torch.bfloat16, None), tol=BTOL)


def _ring2(kind, H, W, B, dual=False, n_add=1):
    C, h = 32, 16

    def make():
        graph = _grid_graph(H, W)
        rnd, unit, tanh = _state_planes(_g(H * W + n_add), B, graph.n, C, h)
        spec = dict(graph=('arg', graph))
        if kind == 'sum':
            spec.update(X=('in', rnd()), adds=('in', [rnd() for _ in range(n_add)]), U=('in', unit()), Cand=('in', tanh()), Y=('out', rnd()), Z=('out', rnd()))
        elif kind == 'blend':
            spec.update(Bm=('in', rnd()), A=('in', rnd()), U=('in', unit()), Hp=('in', tanh()), Cand=('out', rnd()), Hnew=('out', rnd()), SHnew=('out', rnd()))
        else:
            spec.update(X=('in', rnd()), adds=('in', [rnd() for _ in range(n_add)]), V=('out', rnd()), Z=('out', rnd()))
        if dual:
            spec['X2'] = ('in', rnd())
        return spec

    def call(k, t):
        op = csr_operand(t.graph, (t.X if kind != 'blend' else t.Bm).device)
        x2 = getattr(t, 'X2', None)
        if kind == 'sum':
            k.ring2_sum(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, op.bwd_ring2, t.X, x2, t.adds, t.U, t.Cand, t.Y, t.Z)
        elif kind == 'blend':
            k.ring2_blend(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, op.fwd_ring2, t.Bm, t.A, t.U, t.Hp, t.Cand, t.Hnew, t.SHnew)
        else:                                               # the order-3 forward recurrence: V = S.X, Z = 2 S.V - X (+ further addends)
            k.ring2_chain(op.fwd_rowptr, op.fwd_colidx, op.fwd_val, op.fwd_ring2, t.X, x2, 1.0, [], t.V, 2.0, [(t.X, -1.0)] + [(a, 1.0) for a in t.adds], t.Z)
    return make, call


for H, W, B in ((9, 33, 1), (12, 20, 2)):
    case(f'ring2_sum-{H}x{W}', {'stc_ring2_sum_f32'}, *_ring2('sum', H, W, B, dual=(H == 12), n_add=3 if H == 12 else 0), cpu=(H == 9))
    case(f'ring2_blend-{H}x{W}', {'stc_ring2_blend_f32'}, *_ring2('blend', H, W, B))
    case(f'ring2_chain-{H}x{W}', {'stc_ring2_chain_f32'}, *_ring2('chain', H, W, B, dual=(H == 9), n_add=2 if H == 12 else 0))


# ---- node kernels -------------------------------------------------------------------------------------------------------------------------
LEVELS = {0: 'default', 1: 'fp32-mfma', 2: 'generic'}


def _node(nodes, C, L, Lw, Ho, K, backward, want_dT=False, dt=torch.float32):
    def make():
        g = _g(nodes + C + L + Ho + K)
        Zs = [torch.randn(nodes, C, L, generator=g) for _ in range(K)]
        for z in Zs:
            z[..., Lw:] = 7.0                               # garbage in the pad columns must not matter
        W = torch.randn(K * K * Lw, Ho, generator=g) / (K * K * Lw) ** 0.5
        spec = dict(Zs=('in', [z.to(dt) for z in Zs]), Tc=('in', _mix(g, K, C)), W=('in', W))
        if not backward:
            spec.update(b=('in', torch.randn(Ho, generator=g)), Y=('out', torch.empty(nodes, C, Ho, dtype=dt)))
        else:
            spec.update(dY=('in', torch.randn(nodes, C, Ho, generator=g).to(dt)), dZs=('out', [torch.empty(nodes, C, L, dtype=dt) for _ in range(K)]),
                        dW=('out', torch.empty_like(W)), db=('out', torch.empty(Ho)))
            if want_dT:
                spec['dTc'] = ('out', torch.empty(K, C, C))
        return spec

    def call(k, t):
        if not backward:
            k.bdg_node_fwd(t.Zs, t.Tc, t.W, t.b, t.Y)
        elif dt == torch.bfloat16:
            k.bdg_node_bwd_bf16(t.Zs, t.Tc, t.W, t.dY, t.dZs, t.dW, t.db)
        else:
            k.bdg_node_bwd(t.Zs, t.Tc, t.W, t.dY, t.dZs, t.dW, t.db, getattr(t, 'dTc', None))
    return make, call


for level, lname in LEVELS.items():
    for nodes in NODES:
        for C, L, Lw, Ho, K in ((32, 32, 32, 32, 2), (32, 20, 17, 16, 2)) + (((5, 20, 17, 32, 2),) if level == 2 else ()):
            sid = f'{lname}-nodes{nodes}-C{C}-L{L}-Lw{Lw}-Ho{Ho}-K{K}'
            case(f'node_fwd-{sid}', {'stc_bdg_node_fwd_f32'}, *_node(nodes, C, L, Lw, Ho, K, False), level=level, cpu=(nodes == 13 and level == 0))
            # dTc[0] is WRITTEN as zero (T_0 = I is a constant: header, stc_mix_dt_f32 / tests/test_hip_kernels.py), the twin's first matrix is the plain product
            case(f'node_bwd-{sid}', {'stc_bdg_node_bwd_f32'}, *_node(nodes, C, L, Lw, Ho, K, True, want_dT=(L == 32)), level=level, cpu=(nodes == 13 and level == 2),
                 reduce=dict(dTc=lambda v: v[1:]), check=(lambda t, _: [] if not hasattr(t, 'dTc') or not t.dTc.is_cuda or float(t.dTc[0].abs().max()) == 0.0 else ['dTc[0] is not zero']))
for nodes in NODES:
    for C, L, Lw, Ho, K in ((32, 32, 32, 32, 2), (64, 16, 16, 16, 3), (32, 32, 17, 16, 2)):
        sid = f'nodes{nodes}-C{C}-L{L}-Lw{Lw}-Ho{Ho}-K{K}'
        # against the twin with the hardware path's rounding points (the twin's own bf16 methods; tests/test_bf16_kernels.py bounds dW by 2e-3, the rest by 2^-7)
        case(f'node_fwd_bf16-{sid}', {'stc_bdg_node_fwd_bf16'}, *_node(nodes, C, L, Lw, Ho, K, False, dt=torch.bfloat16), tol=BTOL)
        case(f'node_bwd_bf16-{sid}', {'stc_bdg_node_bwd_bf16'}, *_node(nodes, C, L, Lw, Ho, K, True, dt=torch.bfloat16), tol=BTOL)


def _post(nodes, C, form, backward):
    """form: 'rows32' / 'rows20' (interleaved rows, Lw = 32 / 17 of 20), 'planar' (X + X2, 16 + 16), 'narrow' (16-wide plane + cin = 3)."""
    Ho, K = 16, 2
    L, Lw = {'rows32': (32, 32), 'rows20': (20, 17), 'planar': (32, 32), 'narrow': (20, 19)}[form]

    def make():
        g = _g(nodes + C + L)
        rnd = lambda *s: torch.randn(*s, generator=g)
        spec = dict(Tc=('in', _mix(g, K, C)), W=('in', rnd(K * K * Lw, Ho) / (K * K * Lw) ** 0.5))
        if form.startswith('rows'):
            X = rnd(nodes, C, L)
            X[..., Lw:] = 7.0 if backward else 0.0
            spec['X'] = ('in', X)
        else:
            spec.update(X=('in', rnd(nodes, C, 16)), X2=('in', rnd(nodes, C, 16 if form == 'planar' else 3)))
        if not backward:
            spec.update(b=('in', rnd(Ho)), A=('out', torch.empty(nodes, C, Ho)), Bm=('out', torch.empty(nodes, C, Ho)))
        else:
            spec.update(dA=('in', rnd(nodes, C, Ho)), dB=('in', rnd(nodes, C, Ho)), dX=('out', torch.empty(nodes, C, L if form.startswith('rows') else 16)),
                        dW=('out', torch.empty(K * K * Lw, Ho)), db=('out', torch.empty(Ho)))
            if form == 'planar':
                spec['dX2'] = ('out', torch.empty(nodes, C, 16))
        return spec

    def call(k, t):
        x2 = getattr(t, 'X2', None)
        if not backward:
            k.node_post_fwd(t.X, t.Tc, t.W, t.b, t.A, t.Bm, X2=x2)
        else:
            k.node_post_bwd(t.X, t.Tc, t.W, t.dA, t.dB, t.dX, t.dW, t.db, X2=x2, dX2=getattr(t, 'dX2', None))
    return make, call


for nodes in NODES:
    for C, form in ((32, 'rows32'), (32, 'rows20'), (32, 'planar'), (64, 'planar'), (32, 'narrow'), (64, 'narrow')):
        case(f'post_fwd-nodes{nodes}-C{C}-{form}', {'stc_bdg_node_post_fwd_f32'}, *_post(nodes, C, form, False), cpu=(nodes == 13 and form == 'narrow'))
        for fmt in (('f16x2', 'bf16x3') if (C == 64 and form in ('planar', 'narrow')) else (None,)):
            case(f'post_bwd-nodes{nodes}-C{C}-{form}{"-" + fmt if fmt else ""}', {'stc_bdg_node_post_bwd_f32'}, *_post(nodes, C, form, True), fmt=fmt)


# ---- fused cell kernels on interleaved rows -------------------------------------------------------------------------------------------------
def _fused(kind, nodes, C, cin, K, copies=None):
    h = 16
    Lw = cin + h
    L = Lw + (-Lw) % 4

    def make():
        g = _g(nodes + C + cin + K)
        rnd = lambda *s: torch.randn(*s, generator=g)
        Zs = [rnd(nodes, C, L) for _ in range(K)]
        Zs[0][..., Lw:] = 0.0
        Ho = h if kind in ('blend', 'cand_bwd') else 2 * h
        spec = dict(Zs=('in', Zs), Tc=('in', _mix(g, K, C)), W=('in', rnd(K * K * Lw, Ho) / (K * K * Lw) ** 0.5))
        plane = lambda: torch.empty(nodes, C, h)
        if kind == 'gates':
            spec.update(b=('in', rnd(Ho)), H=('in', rnd(nodes, C, h)), U=('out', plane()), Rg=('out', plane()), CandIn=('out', torch.empty(nodes, C, L)))
        elif kind == 'blend':
            spec.update(b=('in', rnd(Ho)), U=('in', torch.sigmoid(rnd(nodes, C, h))), H=('in', rnd(nodes, C, h)), Cand=('out', plane()), Hnew=('out', plane()))
            if copies == 'pair':
                spec.update(c0=('io', torch.full((nodes, C, 32), 9.0)), c1=('io', torch.full((nodes, C, 32), 9.0)))
            if copies == 'side':
                spec.update(c0=('io', torch.full((nodes, C, 20), 9.0)), side=('in', rnd(nodes, C, 1)))
        else:
            spec.update(dZs=('out', [torch.empty(nodes, C, L) for _ in range(K)]), dW=('out', torch.empty(K * K * Lw, Ho)), db=('out', torch.empty(Ho)),
                        U=('in', torch.sigmoid(rnd(nodes, C, h))), Cand=('in', torch.tanh(rnd(nodes, C, h))), dHnew=('in', rnd(nodes, C, h)))
            if kind == 'gates_bwd':
                spec.update(dCandIn=('in', rnd(nodes, C, L)), H=('in', rnd(nodes, C, h)), Rg=('in', torch.sigmoid(rnd(nodes, C, h))),
                            dXt=('out', torch.empty(nodes, C, cin)), dH=('out', plane()))
        return spec

    def call(k, t):
        if kind == 'gates':
            k.cell_gates_fwd(t.Zs, t.Tc, t.W, t.b, t.H, t.U, t.Rg, t.CandIn)
        elif kind == 'blend':
            kw = dict(copies=[(t.c0, 16), (t.c1, 0)]) if copies == 'pair' else dict(copies=[(t.c0, 1)], side=t.side) if copies == 'side' else {}
            k.cell_blend_fwd(t.Zs, t.Tc, t.W, t.b, t.U, t.H, t.Cand, t.Hnew, **kw)
        elif kind == 'cand_bwd':
            k.cell_cand_bwd(t.Zs, t.Tc, t.W, t.dHnew, t.U, t.Cand, t.dZs, t.dW, t.db)
        else:                                               # the Cand form: dH_in is the new state's gradient
            k.cell_gates_bwd(t.Zs, t.Tc, t.W, t.dCandIn, None, t.H, t.U, t.Rg, t.dHnew, t.dZs, t.dW, t.db, t.dXt, t.dH, dH_in_scaled=True, Cand=t.Cand)
    check = _copy_checks({'c0': range(16, 32), 'c1': range(0, 16)}) if copies == 'pair' else None
    return dict(make=make, call=call, check=check)


for level in (0, 1):
    for nodes in NODES:
        for C, cin, K in ((32, 16, 2), (32, 1, 2)) + (((16, 16, 3), (64, 1, 2)) if nodes == 13 else ()):
            sid = f'{LEVELS[level]}-nodes{nodes}-C{C}-cin{cin}-K{K}'
            case(f'cell_gates_fwd-{sid}', {'stc_cell_gates_fwd_f32'}, **_fused('gates', nodes, C, cin, K), level=level, cpu=(nodes == 3 and level == 0))
            case(f'cell_gates_bwd-{sid}', {'stc_cell_gates_bwd_f32'}, **_fused('gates_bwd', nodes, C, cin, K), level=level)
            case(f'cell_cand_bwd-{sid}', {'stc_cell_cand_bwd_f32'}, **_fused('cand_bwd', nodes, C, cin, K), level=level)
            copies = 'pair' if cin == 16 else 'side'
            case(f'cell_blend_fwd-{sid}-{copies}', {'stc_cell_blend_fwd_f32'}, **_fused('blend', nodes, C, cin, K, copies), level=level, cpu=(nodes == 3 and level == 0))


# ---- planar cell kernels (K = 2), both operand formats --------------------------------------------------------------------------------------
def _amax_rows(planes):
    """What a forward launch leaves for ``planes``: (len, 256) floats whose row maxima are the plane maxima (here: slot 0)."""
    a = torch.zeros(len(planes), 256)
    for i, p in enumerate(planes):
        a[i, 0] = p.abs().max() if p.numel() else 0.0
    return a


def _planar(kind, nodes, C, cin, acc=False, fold=False, dt=torch.float32, with_amax=False):
    h, K = 16, 2
    Lw = cin + h
    wide = cin == h

    def make():
        g = _g(nodes + C + cin)
        rnd = lambda *s: torch.randn(*s, generator=g)
        pl = lambda *s: rnd(*s).to(dt)
        X, SX, H, SH = pl(nodes, C, cin), pl(nodes, C, cin), torch.tanh(rnd(nodes, C, h)).to(dt), pl(nodes, C, h)
        spec = dict(X=('in', X), H=('in', H), SX=('in', SX), SH=('in', SH), Tc=('in', _mix(g, K, C)), Wg=('in', rnd(4 * Lw, 2 * h) / (4 * Lw) ** 0.5))
        new = lambda *s: torch.empty(*s, dtype=dt)
        if kind == 'gates_fwd':
            spec.update(bg=('in', rnd(2 * h)), U=('out', new(nodes, C, h)), Rg=('out', new(nodes, C, h)), RH=('out', new(nodes, C, h)))
            if C in (32, 64):
                spec.update(Wc=('in', rnd(4 * Lw, h) / (4 * Lw) ** 0.5), bc=('in', rnd(h)), A=('out', new(nodes, C, h)), Bm=('out', new(nodes, C, h)))
            return spec
        spec.update(U=('in', torch.sigmoid(rnd(nodes, C, h)).to(dt)), Rg=('in', torch.sigmoid(rnd(nodes, C, h)).to(dt)), Cand=('in', torch.tanh(rnd(nodes, C, h)).to(dt)),
                    dHnew=('in', pl(nodes, C, h)), dWg=('out', torch.empty(4 * Lw, 2 * h)), dbg=('out', torch.empty(2 * h)))
        grads = [pl(nodes, C, h) if (wide or i >= 2) else None for i in range(4)]
        spec['dZs'] = ('io' if acc else 'out', grads)
        if with_amax:
            spec['amax'] = ('in', _amax_rows((X, SX, H, SH) if wide else (H, SH, X, SX)))
        if kind == 'gates_bwd':
            spec['dRH'] = ('in', pl(nodes, C, h))
            if not fold:
                spec['dH'] = ('out', new(nodes, C, h))
        else:
            spec.update(Wc=('in', rnd(4 * Lw, h) / (4 * Lw) ** 0.5), dBm=('in', pl(nodes, C, h)), dWc=('out', torch.empty(4 * Lw, h)), dbc=('out', torch.empty(h)))
        return spec

    def call(k, t):
        kk = k if dt == torch.float32 else k.bf16
        amax = dict(act_amax=t.amax) if with_amax else {}
        if kind == 'gates_fwd':
            kk.cell_gates_fwd_planar(t.X, t.H, t.SX, t.SH, t.Tc, t.Wg, t.bg, t.U, t.Rg, t.RH, post=(t.Wc, t.bc, t.A, t.Bm) if hasattr(t, 'Wc') else None)
        elif kind == 'gates_bwd':
            kk.cell_gates_bwd_planar(t.X, t.H, t.SX, t.SH, t.Tc, t.Wg, t.dRH, t.Cand, t.U, t.Rg, t.dHnew, t.dZs, t.dWg, t.dbg, getattr(t, 'dH', None), **amax)
        else:
            acc_kw = dict(accumulate_x=acc and wide, accumulate_h=acc) if dt == torch.float32 else {}
            kk.cell_bwd_planar(t.X, t.H, t.SX, t.SH, t.Tc, t.Wg, t.Wc, t.U, t.Rg, t.Cand, t.dHnew, t.dBm, t.dZs, t.dWg, t.dbg, t.dWc, t.dbc, **acc_kw, **amax)
    return make, call


for fmt in ('f16x2', 'bf16x3'):
    for nodes in NODES:
        for C, cin in ((32, 16), (32, 1), (32, 3), (64, 16), (64, 1), (64, 3)):
            if nodes not in (13, 4500) and (C, cin) not in ((32, 16), (32, 3), (64, 16)):
                continue
            sid = f'{fmt}-nodes{nodes}-C{C}-cin{cin}'
            amax = fmt == 'f16x2'
            case(f'planar_gates_fwd-{sid}', {'stc_cell_gates_fwd_planar_f32'}, *_planar('gates_fwd', nodes, C, cin), fmt=fmt, cpu=(nodes == 3 and cin == 3 and fmt == 'f16x2'))
            case(f'planar_gates_bwd-{sid}', {'stc_cell_gates_bwd_planar_f32'}, *_planar('gates_bwd', nodes, C, cin, fold=(cin == 3), with_amax=amax), fmt=fmt)
            if C == 32:                                     # stc_cell_bwd_planar_supported: the fp32 one-launch backward is built for C = 32, h = 16 only (header)
                # (tests/test_grad_scale.py: the one-launch backward under either format, BOUND against the float64 twin)
                case(f'planar_cell_bwd-{sid}', {'stc_cell_bwd_planar_f32'}, *_planar('cell_bwd', nodes, C, cin, with_amax=amax), fmt=fmt, tol=BOUND,
                     cpu=(nodes == 3 and cin == 3 and fmt == 'f16x2'))
                case(f'planar_cell_bwd-{sid}-accumulate', {'stc_cell_bwd_planar_f32'}, *_planar('cell_bwd', nodes, C, cin, acc=True, with_amax=amax), fmt=fmt, tol=BOUND)

for nodes in NODES:
    for C, cin in ((32, 16), (64, 16), (32, 3), (64, 1)):
        sid = f'nodes{nodes}-C{C}-cin{cin}'
        bf = torch.bfloat16
        case(f'planar_gates_fwd_bf16-{sid}', {'stc_cell_gates_fwd_planar_bf16'}, *_planar('gates_fwd', nodes, C, cin, dt=bf), tol=BTOL)
        case(f'planar_gates_bwd_bf16-{sid}', {'stc_cell_gates_bwd_planar_bf16'}, *_planar('gates_bwd', nodes, C, cin, dt=bf, fold=(cin == 16)), tol=BTOL)
        if C == 32 or cin == 16:
            case(f'planar_cell_bwd_bf16-{sid}', {'stc_cell_bwd_planar_bf16'}, *_planar('cell_bwd', nodes, C, cin, dt=bf), tol=BTOL)


def _post_bf16(nodes, C, narrow):
    def make():
        g = _g(nodes + C)
        bf = torch.bfloat16
        pl = lambda *s: torch.randn(*s, generator=g).to(bf)
        w2 = 3 if narrow else 16
        Lw = 16 + w2
        spec = dict(X=('in', pl(nodes, C, 16)), X2=('in', pl(nodes, C, w2)), Tc=('in', _mix(g, 2, C)), W=('in', torch.randn(4 * Lw, 16, generator=g) / (4 * Lw) ** 0.5),
                    dA=('in', pl(nodes, C, 16)), dB=('in', pl(nodes, C, 16)), dX=('out', pl(nodes, C, 16)), dW=('out', torch.empty(4 * Lw, 16)), db=('out', torch.empty(16)))
        if not narrow:
            spec['dX2'] = ('out', pl(nodes, C, 16))
        return spec

    def call(k, t):
        k.bf16.node_post_bwd(t.X, t.Tc, t.W, t.dA, t.dB, t.dX, t.dW, t.db, X2=t.X2, dX2=getattr(t, 'dX2', None))
    return make, call


for nodes in NODES:
    for C, narrow in ((32, False), (64, False), (32, True)):
        case(f'post_bwd_bf16-nodes{nodes}-C{C}{"-narrow" if narrow else ""}', {'stc_bdg_node_post_bwd_bf16'}, *_post_bf16(nodes, C, narrow), tol=BTOL)


# ---- planar cell kernels of order 3 -------------------------------------------------------------------------------------------------------------
def _planar_k(kind, nodes, cin, fold=False, with_amax=False):
    C, h, K = 32, 16, 3
    Lw = cin + h
    wide = cin == h

    def make():
        g = _g(nodes + cin + 3)
        rnd = lambda *s: torch.randn(*s, generator=g)
        Zx, Zh = [rnd(nodes, C, cin) for _ in range(K)], [rnd(nodes, C, h) for _ in range(K)]
        Ho = 2 * h if kind.startswith('gates') else h
        spec = dict(Zx=('in', Zx), Zh=('in', Zh), Tc=('in', _mix(g, K, C)), W=('in', rnd(K * K * Lw, Ho) / (K * K * Lw) ** 0.5))
        plane = lambda: torch.empty(nodes, C, h)
        if kind == 'gates_fwd':
            spec.update(b=('in', rnd(Ho)), U=('out', plane()), Rg=('out', plane()), RH=('out', plane()))
        elif kind == 'cand_fwd':
            spec.update(b=('in', rnd(Ho)), U=('in', torch.sigmoid(rnd(nodes, C, h))), H=('in', rnd(nodes, C, h)), Cand=('out', plane()), Hnew=('out', plane()))
        else:
            spec.update(U=('in', torch.sigmoid(rnd(nodes, C, h))), Cand=('in', torch.tanh(rnd(nodes, C, h))), dHnew=('in', rnd(nodes, C, h)),
                        dZh=('out', [plane() for _ in range(K)]), dW=('out', torch.empty(K * K * Lw, Ho)), db=('out', torch.empty(Ho)))
            acc = kind == 'gates_bwd' and fold and wide
            spec['dZx'] = ('io' if acc else 'out', [rnd(nodes, C, cin) if wide else None for _ in range(K)])
            if with_amax:
                spec['amax'] = ('in', _amax_rows(Zx + Zh if wide else Zh + Zx))
            if kind == 'gates_bwd':
                spec.update(dRH=('in', rnd(nodes, C, h)), Rg=('in', torch.sigmoid(rnd(nodes, C, h))))
                if not fold:
                    spec['dH'] = ('out', plane())
        return spec

    def call(k, t):
        amax = dict(act_amax=t.amax) if with_amax else {}
        if kind == 'gates_fwd':
            k.cell_gates_fwd_planar_k(t.Zx, t.Zh, t.Tc, t.W, t.b, t.U, t.Rg, t.RH)
        elif kind == 'cand_fwd':
            k.cell_cand_fwd_planar_k(t.Zx, t.Zh, t.Tc, t.W, t.b, t.U, t.H, t.Cand, t.Hnew)
        elif kind == 'gates_bwd':
            k.cell_gates_bwd_planar_k(t.Zx, t.Zh, t.Tc, t.W, t.dRH, t.Cand, t.U, t.Rg, t.dHnew, t.dZx, t.dZh, t.dW, t.db, getattr(t, 'dH', None),
                                      accumulate_x=fold and wide, **amax)
        else:
            k.cell_cand_bwd_planar_k(t.Zx, t.Zh, t.Tc, t.W, t.dHnew, t.U, t.Cand, t.dZx, t.dZh, t.dW, t.db, **amax)
    return make, call


for fmt in ('f16x2', 'bf16x3'):
    for nodes in NODES:
        for cin in (16, 3):
            sid = f'{fmt}-nodes{nodes}-cin{cin}'
            amax = fmt == 'f16x2'
            case(f'planar_k_gates_fwd-{sid}', {'stc_cell_gates_fwd_planar_k_f32'}, *_planar_k('gates_fwd', nodes, cin), fmt=fmt)
            case(f'planar_k_cand_fwd-{sid}', {'stc_cell_cand_fwd_planar_k_f32'}, *_planar_k('cand_fwd', nodes, cin), fmt=fmt)
            case(f'planar_k_gates_bwd-{sid}', {'stc_cell_gates_bwd_planar_k_f32'}, *_planar_k('gates_bwd', nodes, cin, fold=(nodes % 2 == 1), with_amax=amax), fmt=fmt,
                 cpu=(nodes == 3 and fmt == 'f16x2'))
            case(f'planar_k_cand_bwd-{sid}', {'stc_cell_cand_bwd_planar_k_f32'}, *_planar_k('cand_bwd', nodes, cin, with_amax=amax), fmt=fmt)


# ---- helpers: gate / blend math, head, concat / split / axpy, the category graph's Chebyshev set -----------------------------------------------
def _gru(kind, rows, cin, h=16):
    pad = (-(cin + h)) % 4

    def make():
        g = _g(rows + cin)
        rnd = lambda *s: torch.randn(*s, generator=g)
        unit = lambda: torch.sigmoid(rnd(rows, h))
        new = lambda w: torch.empty(rows, w)
        if kind == 'gates_fwd':
            return dict(G=('in', rnd(rows, 2 * h)), Xt=('in', rnd(rows, cin)), H=('in', rnd(rows, h)), U=('out', new(h)), Rg=('out', new(h)), CandIn=('out', new(cin + h + pad)))
        if kind == 'gates_bwd':
            return dict(dCandIn=('in', rnd(rows, cin + h + pad)), dU=('in', rnd(rows, h)), H=('in', rnd(rows, h)), U=('in', unit()), Rg=('in', unit()),
                        dG=('out', new(2 * h)), dXt=('out', new(cin)), dH=('io', rnd(rows, h)))
        if kind == 'blend_fwd':
            return dict(Cpre=('in', rnd(rows, h)), U=('in', unit()), H=('in', rnd(rows, h)), Cand=('out', new(h)), Hnew=('out', new(h)))
        if kind == 'blend_bwd_bf16':
            bf = torch.bfloat16
            return dict(dHnew=('in', rnd(rows, h).to(bf)), U=('in', unit().to(bf)), Cand=('in', torch.tanh(rnd(rows, h)).to(bf)), dCpre=('out', new(h).to(bf)))
        return dict(dHnew=('in', rnd(rows, h)), U=('in', unit()), H=('in', rnd(rows, h)), Cand=('in', torch.tanh(rnd(rows, h))),
                    dCpre=('out', new(h)), dU=('out', new(h)), dH=('out', new(h)))

    def call(k, t):
        if kind == 'gates_fwd':
            k.gru_gates_fwd(t.G, t.Xt, t.H, t.U, t.Rg, t.CandIn)
        elif kind == 'gates_bwd':                            # dH_in aliases dH: the gradient the state is already owed
            k.gru_gates_bwd(t.dCandIn, t.dU, t.H, t.U, t.Rg, t.dG, t.dXt, t.dH, dH_in=t.dH)
        elif kind == 'blend_fwd':
            k.gru_blend_fwd(t.Cpre, t.U, t.H, t.Cand, t.Hnew)
        elif kind == 'blend_bwd_bf16':
            k.bf16.gru_blend_bwd(t.dHnew, t.U, None, t.Cand, t.dCpre, None, None)
        else:
            k.gru_blend_bwd(t.dHnew, t.U, t.H, t.Cand, t.dCpre, t.dU, t.dH)
    return make, call


for rows, cin in ((1, 1), (13, 3), (50 * 5, 16), (4500, 1)):
    case(f'gru_gates_fwd-rows{rows}-cin{cin}', {'stc_gru_gates_fwd_f32'}, *_gru('gates_fwd', rows, cin), cpu=(rows == 13))
    case(f'gru_gates_bwd-rows{rows}-cin{cin}', {'stc_gru_gates_bwd_f32'}, *_gru('gates_bwd', rows, cin), cpu=(rows == 13))
    case(f'gru_blend_fwd-rows{rows}', {'stc_gru_blend_fwd_f32'}, *_gru('blend_fwd', rows, cin))
    case(f'gru_blend_bwd-rows{rows}', {'stc_gru_blend_bwd_f32'}, *_gru('blend_bwd', rows, cin))
    case(f'gru_blend_bwd_bf16-rows{rows}', {'stc_gru_blend_bwd_bf16'}, *_gru('blend_bwd_bf16', rows, cin), tol=BTOL)


def _head(shape, backward, dt):
    h = 16

    def make():
        g = _g(sum(shape))
        rnd = lambda *s: torch.randn(*s, generator=g)
        H, w, b = rnd(*shape, h).to(dt), rnd(h) / 4, rnd(1)
        if not backward:
            return dict(H=('in', H), w=('in', w), b=('in', b), y=('out', torch.empty(*shape)))
        y = torch.sigmoid(H.float() @ w + b)
        return dict(H=('in', H), w=('in', w), y=('in', y), dy=('in', rnd(*shape)), dH=('out', torch.empty(*shape, h, dtype=dt)), dwb=('out', torch.empty(h + 1)))

    def call(k, t):
        if not backward:
            k.head_fwd(t.H, t.w, t.b, t.y)
        else:
            k.head_bwd(t.H, t.w, t.y, t.dy, t.dH, t.dwb)
    return make, call


for dt, tag in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
    for shape in ((1,), (3, 7), (2, 3, 50, 5), (1, 6, 777, 4), (1, 300000)):
        sid = 'x'.join(map(str, shape))
        case(f'head_fwd_{tag}-{sid}', {f'stc_head_fwd_{tag}'}, *_head(shape, False, dt), cpu=(shape == (3, 7)))          # (y is fp32 for both storage types: TOL)
        # the family's own bounds (test_output_head / test_output_head_bf16): y and fp32 dH within TOL, dwb within 2e-5 (= BOUND), bf16 dH rows within BTOL
        case(f'head_bwd_{tag}-{sid}', {f'stc_head_bwd_{tag}'}, *_head(shape, True, dt), tol=TOL if tag == 'f32' else BTOL, tols=dict(dwb=BOUND), cpu=(shape == (3, 7)))


def _cat(kind, rows, a, b):
    pad = (-(a + b)) % 4

    def make():
        g = _g(rows + a + b)
        rnd = lambda *s: torch.randn(*s, generator=g)
        if kind == 'concat2':
            return dict(A=('in', rnd(rows, a)), Bm=('in', rnd(rows, b)), out=('out', torch.empty(rows, a + b + pad)))
        if kind == 'axpy':
            return dict(x=('in', rnd(rows, a)), y=('io', rnd(rows, a)))
        # split with every addend form: addA read in place from rows of a + b + pad floats, addB aliasing B (accumulate in place), second addends
        return dict(src=('in', rnd(rows, a + b + pad)), addA=('in', rnd(rows, a + b + pad)), A=('out', torch.empty(rows, a)), Bm=('io', rnd(rows, b)),
                    addA2=('in', rnd(rows, a)), addB2=('in', rnd(rows, b)))

    def call(k, t):
        if kind == 'concat2':
            k.concat2(t.A, t.Bm, t.out)
        elif kind == 'axpy':
            k.axpy(-1.0, t.x, t.y)
        else:
            k.split2(t.src, t.A, t.Bm, addA=t.addA, addB=t.Bm, addA_ld=a + b + pad, addA2=t.addA2, addB2=t.addB2)
    return make, call


for rows, a, b in ((1, 1, 16), (13 * 32, 3, 16), (50 * 5, 16, 16), (4500 * 32, 1, 16)):
    for kind in ('concat2', 'split2', 'axpy'):
        case(f'{kind}-rows{rows}-{a}+{b}', {f'stc_{kind}_f32'}, *_cat(kind, rows, a, b), cpu=(rows == 1))


def _cheby(n, K, backward):
    def make():
        g = _g(n * 10 + K)
        G = torch.randn(n, n, generator=g) / n ** 0.5
        if not backward:
            return dict(G=('in', G), T=('out', torch.empty(K, n, n)))
        T = torch.empty(K, n, n)
        EmulatedKernels().cheby_dense_fwd(G, K, T)
        # dT is scratch that the launch destroys (header): an in / out operand whose final content is whatever the kernel left -- margins only
        return dict(G=('in', G), T=('in', T), dT=('io', torch.randn(K, n, n, generator=g)), dG=('out', torch.empty(n, n)))

    def call(k, t):
        if not backward:
            k.cheby_dense_fwd(t.G, K, t.T)
        else:
            k.cheby_dense_bwd(t.G, t.T, t.dT, t.dG)
    return make, call


for n, K in ((3, 1), (5, 2), (32, 4), (64, 3), (128, 3)):
    case(f'cheby_fwd-n{n}-K{K}', {'stc_cheby_dense_fwd_f32'}, *_cheby(n, K, False), cpu=(n == 5))
    case(f'cheby_bwd-n{n}-K{K}', {'stc_cheby_dense_bwd_f32'}, *_cheby(n, K, True), unwritten=('dT',), cpu=(n == 5))


# ---- fronts without a CPU twin: Adam, the MGP front, mixed fusion -- float64 references written out here ---------------------------------------
def _adam(n):
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4)

    def make():
        g = _g(n)
        rnd = lambda: torch.randn(n, generator=g)
        return dict(p=('io', rnd()), g=('in', rnd()), m=('io', 0.1 * rnd()), v=('io', 0.01 * rnd().abs()), step=('in', torch.tensor([3.0])))

    def call(k, t):
        before = [x.double().cpu() for x in (t.p, t.g, t.m, t.v)]
        k.adam(t.p, t.g, t.m, t.v, t.step, **hyper)
        t.before = before

    def check(t, _):
        p, g, m, v = t.before
        b1, b2 = hyper['beta1'], hyper['beta2']
        g = g + hyper['weight_decay'] * p
        m = m + (1 - b1) * (g - m)
        v = b2 * v + (1 - b2) * g * g
        p = p - hyper['lr'] / (1 - b1 ** 3) * m / (v.sqrt() / math.sqrt(1 - b2 ** 3) + hyper['eps'])
        errs = dict(p=rel_err(t.p, p), m=rel_err(t.m, m), v=rel_err(t.v, v))
        return [f'adam.{n_}: {e:.2e} from float64' for n_, e in errs.items() if not e < TOL]
    return dict(make=make, call=call, check=check)


for n in (4, 1028, 300004):
    case(f'adam-n{n}', {'stc_adam_f32'}, **_adam(n), twin=False)


def _mgp(B, T, N, C, rows_axis, h=8):
    alpha = 2.0

    def make():
        g = _g(B + T + N + C)
        X = torch.rand(B, T, N, C, generator=g)
        F = C if rows_axis == 2 else N
        R = N if rows_axis == 2 else C
        rnd = lambda *s: torch.randn(*s, generator=g)
        return dict(X=('in', X), Wu=('in', rnd(F, h) / F ** 0.5), Wv=('in', rnd(F, h) / F ** 0.5), dU=('in', rnd(R, B * T, h)), dV=('in', rnd(R, B * T, h)),
                    dPs=('in', rnd(R, R)))

    def call(k, t):
        U, V = k.mgp_uv_fwd(t.X, rows_axis, t.Wu, t.Wv, alpha)
        dWu, dWv = k.mgp_uv_bwd(t.X, rows_axis, U, V, t.dU, t.dV, alpha)
        R = U.shape[0]
        P = (U.reshape(R, -1) @ V.reshape(R, -1).t()).contiguous()
        Ps = k.mgp_softmax_fwd(P)
        dP = k.mgp_softmax_bwd(P, Ps, t.dPs)
        return U, V, dWu, dWv, Ps, dP

    def check(t, ret):
        U, V, dWu, dWv, Ps, dP = ret
        X = t.X.double().cpu()
        x = (X.reshape(-1, *X.shape[2:]) if rows_axis == 2 else X.reshape(-1, *X.shape[2:]).transpose(1, 2)).requires_grad_(False)      # (K, R, F)
        Wu, Wv = t.Wu.double().cpu().requires_grad_(True), t.Wv.double().cpu().requires_grad_(True)
        Ur, Vr = torch.tanh(alpha * x @ Wu).transpose(0, 1), torch.tanh(alpha * x @ Wv).transpose(0, 1)                               # (R, K, h)
        (Ur * t.dU.double().cpu()).sum().add((Vr * t.dV.double().cpu()).sum()).backward()
        P = (U.double().cpu().reshape(U.shape[0], -1) @ V.double().cpu().reshape(U.shape[0], -1).t()).requires_grad_(True)
        Psr = torch.softmax(torch.relu(P - P.t()), -1)
        (Psr * t.dPs.double().cpu()).sum().backward()
        errs = dict(U=rel_err(U, Ur), V=rel_err(V, Vr), dWu=rel_err(dWu, Wu.grad), dWv=rel_err(dWv, Wv.grad), Ps=rel_err(Ps, Psr), dP=rel_err(dP, P.grad))
        return [f'mgp.{n_}: {e:.2e} from float64' for n_, e in errs.items() if not e < TOL]
    return dict(make=make, call=call, check=check)


for B, T, N, C, axis in ((2, 3, 100, 5, 2), (2, 3, 100, 5, 3), (1, 1, 37, 3, 2), (3, 2, 13, 16, 3)):
    case(f'mgp_front-{B}x{T}x{N}x{C}-rows_axis{axis}', {'stc_mgp_uv_fwd_f32', 'stc_mgp_uv_bwd_f32', 'stc_mgp_softmax_fwd_f32', 'stc_mgp_softmax_bwd_f32'},
         **_mgp(B, T, N, C, axis), twin=False, fronts=6)        # U, V, the uv partials, Ps, rowdot, dP


def _mixed_fusion(n, want_dA, want_dW):
    D = n * n

    def make():
        g = _g(D)
        rnd = lambda *s: torch.randn(*s, generator=g)
        return dict(WA=('in', rnd(D, D) / D ** 0.5), bA=('in', rnd(D)), WP=('in', rnd(D, D) / D ** 0.5), bP=('in', rnd(D)), A=('in', rnd(n, n)), P=('in', rnd(n, n)),
                    dG=('in', rnd(n, n)))

    def call(k, t):
        gate, G = k.mixed_fusion_fwd(t.WA, t.bA, t.WP, t.bP, t.A, t.P)
        return (gate, G) + tuple(k.mixed_fusion_bwd(t.WA, t.WP, t.A, t.P, gate, t.dG, want_dA, want_dW))

    def check(t, ret):
        gate, G, dWA, dWP, db, dP, dA = ret
        d = lambda x: x.double().cpu()
        leaves = {n_: d(getattr(t, n_)).requires_grad_(True) for n_ in ('WA', 'bA', 'WP', 'A', 'P')}
        gr = torch.sigmoid(leaves['WA'] @ leaves['A'].reshape(-1) + leaves['bA'] + leaves['WP'] @ leaves['P'].reshape(-1) + d(t.bP)).view(n, n)
        Gr = gr * leaves['A'] + (1 - gr) * leaves['P']
        (Gr * d(t.dG)).sum().backward()
        errs = dict(gate=rel_err(gate, gr), G=rel_err(G, Gr), db=rel_err(db, leaves['bA'].grad), dP=rel_err(dP, leaves['P'].grad))
        if want_dA:
            errs['dA'] = rel_err(dA, leaves['A'].grad)
        if want_dW:
            errs.update(dWA=rel_err(dWA, leaves['WA'].grad), dWP=rel_err(dWP, leaves['WP'].grad))
        return [f'mixed_fusion.{n_}: {e:.2e} from float64' for n_, e in errs.items() if not e < TOL]
    return dict(make=make, call=call, check=check)


for n, want_dA, want_dW in ((10, True, True), (10, False, True), (10, True, False), (2, True, True), (6, False, True)):
    case(f'mixed_fusion-D{n * n}{"-dA" if want_dA else ""}{"-dW" if want_dW else ""}', {'stc_mixed_fusion_fwd_f32', 'stc_mixed_fusion_bwd_f32'},
         **_mixed_fusion(n, want_dA, want_dW), twin=False, fronts=5 + want_dA + 2 * want_dW)      # gate, G, db, dP, scratch (+ dA, + dW_A, dW_P)


# ---- small graphs: one cell step per launch, and the gradient products of learned graphs ----------------------------------------------------------
def _param_rows():
    """stc_cell_small_param_rows(): from the library where it is built (no GPU needed), else the twin's figure."""
    try:
        return int(_lib.load_library().stc_cell_small_param_rows())
    except _lib.StcError:
        return EmulatedKernels.cell_small_param_rows


def _small_cell(B, N, C, cin, K, splits, bias):
    """Forward then backward of one cell step.  dparams has EXACTLY batch * splits * stc_cell_small_param_rows() rows of EXACTLY the parameter count
    (params_ld exact), zero on entry; which row of a sample's group a partial lands in is the kernel's business: compared per sample."""
    from tests.test_small_cell import _graph, _inputs
    rows = _param_rows()

    def make():
        t = _inputs(B, N, C, cin, seed=3 * N + C + cin, bias=bias, K=K)
        new = lambda *s: torch.empty(*s)
        zgw = 32 if cin == 16 else 20
        spec = dict(graph=('arg', _graph(N, seed=N + cin)))
        spec.update({n: ('in', t[n]) for n in ('X', 'H', 'Tc', 'Wg', 'Wc', 'dHnew') + (('bg', 'bc') if bias else ())})
        spec.update({n: ('out', new(B, N, C, 16)) for n in ('U', 'R', 'Cand', 'Hnew', 'RH', 'dH')})
        spec.update(Zg=('out', new(B, N * C, zgw)), Zc=('out', new(B, N * C, 16)), dX=('out', new(B, N, C, cin)),
                    dP=('io', torch.zeros(B * splits * rows, EmulatedKernels.cell_small_params(K, K, cin))))
        if K == 3:
            spec.update(Zg2=('out', new(B, N * C, zgw)), Zc2=('out', new(B, N * C, 16)))
        return spec

    def call(k, t):
        op = csr_operand(t.graph, t.H.device)
        dt = t.H.dtype
        f3 = b3 = {}
        if K == 3:
            g2 = t.graph.second_order(t.H.device)
            f3 = dict(graph2=(g2['fwd2_rowptr'], g2['fwd2_colidx'], g2['fwd2_val'].to(dt)), Zg2=t.Zg2, Zc2=t.Zc2)
            b3 = dict(f3, graph2=(g2['bwd2_rowptr'], g2['bwd2_colidx'], g2['bwd2_val'].to(dt)))
        bg, bc = getattr(t, 'bg', None), getattr(t, 'bc', None)
        k.cell_small_fwd(op.fwd_rowptr, op.fwd_colidx, op.fwd_val.to(dt), t.X, t.H, t.Tc, t.Wg, bg, t.Wc, bc, t.U, t.R, t.Cand, t.Hnew, t.RH, t.Zg, t.Zc,
                         splits=splits, **f3)
        k.cell_small_bwd(op.bwd_rowptr, op.bwd_colidx, op.bwd_val.to(dt), t.X, t.H, t.Tc, t.Wg, t.Wc, t.U, t.R, t.Cand, t.RH, t.Zg, t.Zc, t.dHnew,
                         t.dX, False, t.dH, False, t.dP, bias, bias, splits=splits, **b3)
    return dict(make=make, call=call, reduce=dict(dP=lambda v: v.view(B, splits * rows, -1).sum(1)))


for K in (2, 3):
    for B, N, C, cin, splits, bias in ((3, 100, 5, 1, 1, True), (3, 100, 5, 16, 4, True), (2, 37, 8, 3, 4, False), (1, 10, 16, 4, 1, True), (2, 7, 1, 2, 1, False),
                                       (2, 33, 7, 16, 4, True)):
        case(f'cell_small-K{K}-B{B}-N{N}-C{C}-cin{cin}-splits{splits}{"" if bias else "-nobias"}', {'stc_cell_small_fwd_f32', 'stc_cell_small_bwd_f32'},
             **_small_cell(B, N, C, cin, K, splits, bias), cpu=(N == 7))


GUARD = 16          # doubles between and around the blocks of a shared partial buffer


def _grad_product(kind, cells, B, N, C, wa, wb, sel, chunks):
    """One product written into ITS block of a (chunks, total) float64 buffer that also holds a neighbour's block and guard columns (a non-zero
    chunk_stride: total doubles between consecutive chunks); everything outside the block keeps its bits in every chunk."""
    size = N * N if kind == 'graph' else C * wa * C * wb
    other = 50
    total = GUARD + other + GUARD + size + GUARD

    def make():
        g = _g(cells * N + wa)
        A, Bm = torch.randn(cells, B, N * C, wa, generator=g), torch.randn(cells, B, N * C, wa if kind == 'graph' else wb, generator=g)
        return dict(A=('in', A), Bm=('in', Bm), part=('io', torch.full((chunks, total), 9.0, dtype=torch.float64)))

    def call(k, t):
        (k.graph_grad if kind == 'graph' else k.mix_grad)(t.A, t.Bm, *sel, N, into=(t.part, GUARD + other + GUARD))

    def check(t, _):
        keep = torch.ones(total, dtype=torch.bool)
        keep[GUARD + other + GUARD:GUARD + other + GUARD + size] = False
        return [] if bool((t.part[:, keep.to(t.part.device)] == 9.0).all()) else ['the neighbouring block or a guard column of the partial buffer changed']
    own = lambda v: v[:, GUARD + other + GUARD:GUARD + other + GUARD + size].sum(0)
    return dict(make=make, call=call, check=check, reduce=dict(part=own))


for cells, B, N, C, wa, wb, sel, chunks in ((9, 4, 100, 5, 32, 32, (0, 1, 9), 7), (6, 3, 100, 5, 32, 16, (1, 2, 3), 96), (4, 2, 37, 8, 20, 32, (0, 3, 2), 3),
                                            (3, 2, 12, 3, 20, 16, (2, 1, 1), 1), (2, 1, 130, 1, 32, 32, (0, 1, 2), 5)):
    sid = f'cells{cells}-B{B}-N{N}-C{C}-{wa}x{wb}-chunks{chunks}'
    # tests/test_small_cell.py test_graph_gradient_products: 1e-6 of the float64 product
    case(f'graph_grad-{sid}', {'stc_graph_grad_f32'}, **_grad_product('graph', cells, B, N, C, wa, wb, sel, chunks), tol=1e-6, cpu=(N == 12))
    case(f'mix_grad-{sid}', {'stc_mix_grad_f32'}, **_grad_product('mix', cells, B, N, C, wa, wb, sel, chunks), tol=1e-6, cpu=(N == 12))


def _mix_dt(nodes, C, L, Lw, Ho, K):
    def make():
        g = _g(nodes + 10 * C + K)
        Zs = [torch.randn(nodes, C, L, generator=g) for _ in range(K)]
        for z in Zs:
            z[..., Lw:] = 7.0
        return dict(Zs=('in', Zs), W=('in', torch.randn(K * K * Lw, Ho, generator=g)), dY=('in', torch.randn(nodes, C, Ho, generator=g)), dTc=('out', torch.empty(K, C, C)))

    def call(k, t):
        k.mix_dT(t.Zs, t.W, t.dY, t.dTc)
    return dict(make=make, call=call, reduce=dict(dTc=lambda v: v[1:]),
                check=lambda t, _: [] if float(t.dTc[0].abs().max()) == 0.0 else ['dTc[0] is not zero'])


for nodes, C, L, Lw, Ho, K in ((1, 16, 32, 32, 32, 2), (3, 5, 20, 17, 32, 3), (13, 5, 32, 32, 16, 2), (50, 7, 32, 32, 32, 2), (9, 11, 20, 18, 16, 2), (4500, 5, 20, 17, 32, 3),
                               (3200, 5, 32, 32, 16, 3), (7, 8, 32, 32, 32, 2)):
    case(f'mix_dt-nodes{nodes}-C{C}-L{L}-Lw{Lw}-Ho{Ho}-K{K}', {'stc_mix_dt_f32'}, **_mix_dt(nodes, C, L, Lw, Ho, K), cpu=(nodes == 13))


# ---- nodes == 0: sizes of zero elements are legal; the parameter gradients are memset -- exactly nW / Ho / nT floats, between intact margins ----------
_ZERO = dict(zeros=True, twin=False)
for level in LEVELS:
    case(f'zero_nodes-node_bwd-{LEVELS[level]}', (), *_node(0, 32, 32, 32, 32, 2, True, want_dT=True), level=level, **_ZERO)
    case(f'zero_nodes-node_bwd-{LEVELS[level]}-padded', (), *_node(0, 32, 20, 17, 16, 2, True), level=level, **_ZERO)
case('zero_nodes-node_bwd-generic-C5', (), *_node(0, 5, 20, 17, 32, 2, True, want_dT=True), level=2, **_ZERO)
case('zero_nodes-node_bwd_bf16', (), *_node(0, 32, 32, 32, 32, 2, True, dt=torch.bfloat16), **_ZERO)
for form in ('rows32', 'rows20', 'planar', 'narrow'):
    case(f'zero_nodes-post_bwd-{form}', (), *_post(0, 32, form, True), **_ZERO)
case('zero_nodes-post_bwd_bf16', (), *_post_bf16(0, 32, False), **_ZERO)
for kind in ('gates_bwd', 'cand_bwd'):
    f = _fused(kind, 0, 32, 16, 2)
    case(f'zero_nodes-cell_{kind}', (), f['make'], f['call'], **_ZERO)
for cin in (16, 3):
    case(f'zero_nodes-planar_gates_bwd-cin{cin}', (), *_planar('gates_bwd', 0, 32, cin), **_ZERO)
    case(f'zero_nodes-planar_cell_bwd-cin{cin}', (), *_planar('cell_bwd', 0, 32, cin), **_ZERO)
    case(f'zero_nodes-planar_cell_bwd_bf16-cin{cin}', (), *_planar('cell_bwd', 0, 32, cin, dt=torch.bfloat16), **_ZERO)
    case(f'zero_nodes-planar_k_gates_bwd-cin{cin}', (), *_planar_k('gates_bwd', 0, cin), **_ZERO)
    case(f'zero_nodes-planar_k_cand_bwd-cin{cin}', (), *_planar_k('cand_bwd', 0, cin), **_ZERO)
m = _mix_dt(0, 5, 20, 17, 32, 3)
case('zero_nodes-mix_dt', (), m['make'], m['call'], **_ZERO)
case('zero_nodes-head_bwd', (), *_head((0,), True, torch.float32), **_ZERO)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
EM = EmulatedKernels()
_BY_ID = {c.id: c for c in CASES}
assert len(_BY_ID) == len(CASES)


@pytest.fixture(scope='module')
def hip():
    return _lib.HipKernels()


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [c.id for c in CASES])
def test_banded_launch(hip, cid, monkeypatch):
    findings = run_case(_BY_ID[cid], hip, 'cuda', monkeypatch, twin=EM)
    assert not findings, findings


@pytest.mark.parametrize('cid', [c.id for c in CASES if c.cpu])
def test_harness_passes_the_cpu_twin(cid, monkeypatch):
    """The same cases through ``EmulatedKernels`` on banded CPU tensors: the harness itself raises no finding."""
    assert run_case(_BY_ID[cid], EM, 'cpu', monkeypatch, twin=EM) == []


def test_banded_views_are_what_the_docstring_says():
    for shape, dt in (((5, 7, 3), torch.float32), ((4500, 32, 16), torch.bfloat16), ((0, 32, 16), torch.float32), ((96, 300), torch.float64), ((777,), torch.uint8)):
        b = Bands('cpu')
        v = b.band(shape, dt, 'in', 'x')
        w = b.band(shape, dt, 'out', 'y')
        b.snapshot()
        for t in (v, w):
            assert t.shape == shape and t.is_contiguous() and (t.numel() == 0 or t.data_ptr() % 128 == 16)
        _, bits, start, n, _ = b.items[0]
        es = v.element_size()
        assert min(start, bits.numel() - start - n) >= max(1024, 2 * math.prod(shape[1:]))
        if dt.is_floating_point:
            flat = bits.view(dt)
            assert bool(torch.isnan(flat[:start].float()).all()) and bool(torch.isnan(flat[start + n:].float()).all())
            out = b.items[1][1].view(dt)
            assert bool(torch.isfinite(out[:b.items[1][2]].double()).all())
        assert b.violations() == []
        w.fill_(1)
        v.fill_(1)
        assert b.violations() == []                         # the interior is the operand's
        b.items[1][1][b.items[1][2] - 1] += 1               # one element before the view
        assert b.violations() == ['y']
        b.items[0][1][b.items[0][2] + n] = 0                # one element after
        assert b.violations() == ['x', 'y']


# ---- maxima nobody reads back: exact, so no tolerance -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('n_amax', [1, 7, 256])
def test_spmm_sum_leaves_max_abs_y(hip, n_amax):
    """``spmm_sum(..., amax=)``: the maximum over the slots is max |Y| bit for bit; a slot no wave used stays zero, none exceeds the maximum."""
    B, C, h = 2, 32, 16
    graph = _grid_graph(9, 33)
    op = csr_operand(graph, torch.device('cuda'))
    g = _g(n_amax)
    X, add = torch.randn(B, graph.n, C, h, generator=g).cuda(), torch.randn(B, graph.n, C, h, generator=g)
    add[-1, -1, -1, -1] = 77.0                              # the launch's maximum sits in its last row
    bands = Bands('cuda')
    Y, amax = bands.band(X.shape, torch.float32, 'out', 'Y'), bands.band((n_amax,), torch.float32, 'out', 'amax')
    Y.fill_(float('nan'))
    amax.zero_()
    bands.snapshot()
    hip.spmm_sum(op.bwd_rowptr, op.bwd_colidx, op.bwd_val, op.bwd_plan[:3], X, None, [(add.cuda(), 0)], Y, amax=amax)
    torch.cuda.synchronize()
    assert bands.violations() == []
    top = Y.abs().max()
    assert float(top) >= 70.0 and torch.equal(amax.max(), top)
    assert bool(((amax >= 0) & (amax <= top)).all())


@pytest.mark.gpu
@pytest.mark.parametrize('nodes', [13, 4500])
@pytest.mark.parametrize('cin', [16, 3])
@pytest.mark.parametrize('launch', ['gates', 'gates_k', 'cand_k'])
def test_forward_launches_leave_the_plane_maxima(hip, monkeypatch, launch, cin, nodes):
    """act_amax of the three forward launches (fp16 x 2 format): row i holds max |plane i| exactly, in the documented order -- the X-side planes first
    for a wide input, the H-side planes first for a narrow one; planes scaled 1, 3, 5, .. so that a swapped row shows, each plane's maximum in its
    LAST node; nothing outside the rows the launch owns is touched.  A launch owns ALL rows of its buffer -- the header gives act_amax as exactly
    (4, STC_ACT_AMAX_SLOTS) at order 2 and (2 K, STC_ACT_AMAX_SLOTS) at order K, wide and narrow input alike, and the front refuses any other shape --
    so "the rows beyond" are the margin behind the buffer: a launch that wrote a seventh row at K = 3, or row 2 K at any order, changes it."""
    monkeypatch.setattr(hip, 'operand_format', _lib.FMT_F16X2, raising=False)
    C, h = 32, 16
    K = 2 if launch == 'gates' else 3
    g = _g(nodes + cin + K)
    rnd = lambda *s: torch.randn(*s, generator=g)
    xs, hs = [rnd(nodes, C, cin) for _ in range(K)], [torch.tanh(rnd(nodes, C, h)) for _ in range(K)]
    order = (xs + hs) if cin == h else (hs + xs)           # the header's row order (K = 2: xs = (X, S.X), hs = (H, S.H))
    for i, p in enumerate(order):
        p.mul_(2 * i + 1)
        p[-1, -1, -1] = 1.5 * float(p.abs().max())
    Lw = cin + h
    Ho = h if launch == 'cand_k' else 2 * h
    Tc, W, b = _mix(g, K, C).cuda(), (rnd(K * K * Lw, Ho) / (K * K * Lw) ** 0.5).cuda(), rnd(Ho).cuda()
    bands = Bands('cuda')
    act = bands.band((2 * K, 256), torch.float32, 'out', 'act_amax')
    act.zero_()
    outs = [bands.band((nodes, C, h), torch.float32, 'out', f'out{i}') for i in range(3)]
    bands.snapshot()
    cx, ch = [p.cuda() for p in xs], [p.cuda() for p in hs]
    if launch == 'gates':
        hip.cell_gates_fwd_planar(cx[0], ch[0], cx[1], ch[1], Tc, W, b, *outs, act_amax=act)
    elif launch == 'gates_k':
        hip.cell_gates_fwd_planar_k(cx, ch, Tc, W, b, *outs, act_amax=act)
    else:
        hip.cell_cand_fwd_planar_k(cx, ch, Tc, W, b, torch.sigmoid(rnd(nodes, C, h)).cuda(), ch[0], outs[0], outs[1], act_amax=act)
    torch.cuda.synchronize()
    assert bands.violations() == []
    for i, p in enumerate(order):
        top = p.abs().max().cuda()
        assert torch.equal(act[i].max(), top), (i, float(act[i].max()), float(top))
        assert bool(((act[i] >= 0) & (act[i] <= top)).all())


def _room_after(t, extra):
    """Whether ``extra`` more elements exist behind ``t`` in its own allocation."""
    return t.untyped_storage().nbytes() >= (t.storage_offset() + t.numel() + extra) * t.element_size()


class _Overrunning(EmulatedKernels):
    """Negative controls: a twin whose csr_spmm writes one row too many and whose bdg_node_fwd reads one row past Z[0] with a zero weight."""

    def csr_spmm(self, rowptr, colidx, val, n_rows, n_cols, X, Y0, Y, alpha, beta, plan=None):
        super().csr_spmm(rowptr, colidx, val, n_rows, n_cols, X, Y0, Y, alpha, beta, plan=plan)
        F = Y.shape[-1]
        if _room_after(Y, F):
            torch.as_strided(Y, (F,), (1,), Y.storage_offset() + Y.numel()).fill_(1.0)

    def bdg_node_fwd(self, Zs, Tc, W, bias, Y):
        super().bdg_node_fwd(Zs, Tc, W, bias, Y)
        row = Zs[0].shape[1] * Zs[0].shape[2]
        if _room_after(Zs[0], row):
            past = torch.as_strided(Zs[0], (row,), (1,), Zs[0].storage_offset() + Zs[0].numel())
            Y[-1, 0, 0] += 0.0 * past.sum().to(Y.dtype)


def test_negative_control_write_one_row_too_far(monkeypatch):
    c = next(c for c in CASES if c.id.startswith('csr_spmm_f32') and c.cpu)
    assert run_case(c, EM, 'cpu', monkeypatch) == []
    assert run_case(c, _Overrunning(), 'cpu', monkeypatch) == ['margin of Y changed']


def test_negative_control_read_past_an_input_with_zero_weight(monkeypatch):
    c = next(c for c in CASES if c.id.startswith('node_fwd') and c.cpu)
    assert run_case(c, EM, 'cpu', monkeypatch) == []
    assert run_case(c, _Overrunning(), 'cpu', monkeypatch) == ['Y: non-finite result on banded operands']


class _Clobbering(EmulatedKernels):
    """Negative control: a twin whose csr_spmm uses its const operand X as scratch (scales it in place and back: the result is right, one
    element of X ends one ulp off)."""

    def csr_spmm(self, rowptr, colidx, val, n_rows, n_cols, X, Y0, Y, alpha, beta, plan=None):
        super().csr_spmm(rowptr, colidx, val, n_rows, n_cols, X, Y0, Y, alpha, beta, plan=plan)
        first = X.view(-1)[:1]
        first.copy_(torch.nextafter(first, torch.full_like(first, float('inf'))))


def test_negative_control_a_const_operand_is_written(monkeypatch):
    c = next(c for c in CASES if c.id.startswith('csr_spmm_f32') and c.cpu)
    assert run_case(c, _Clobbering(), 'cpu', monkeypatch) == ['input X was modified by the launch']


def _takes_device_buffers(argtypes):
    """More pointer arguments than the trailing stream."""
    return sum(a in (_lib._p, _lib._pp, _lib._pi, _lib._pf) for a in argtypes) >= 2


def test_every_entry_point_has_a_banded_case():
    import tests                                    # every tests/test_*_guard_bands.py appends its cases to CASES on import: also when this file is run alone
    for m in pkgutil.iter_modules(tests.__path__):
        if m.name.startswith('test_') and m.name.endswith('_guard_bands'):
            importlib.import_module(f'tests.{m.name}')
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in set(ids) if ids.count(i) > 1)
    named = set().union(*[c.entries for c in CASES])
    assert named <= set(_lib._ABI), named - set(_lib._ABI)
    assert not named & set(NO_BANDED_CASE)
    missing = [name for name, (_, argtypes) in _lib._ABI.items()
               if _takes_device_buffers(argtypes) and name != 'stc_last_error' and name not in named and name not in NO_BANDED_CASE]
    assert not missing, f'entry points without a banded case (add one, or list it in NO_BANDED_CASE with the reason): {missing}'
