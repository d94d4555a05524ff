"""Launch geometry: every kernel that loops over a capped or residency-sized grid, run past its first trip against float64 (tests/launch_trips.py
holds the table, the sizes and the checker; DESIGN.md, "Launch geometry").

CPU: the table is closed over csrc/ (a scan finds every use of ``gridDim.x`` and every ``persistent_grid`` call site), every cap text is pinned,
every case's size is two full trips and a ragged one by the table's own numbers, and the checker reports two fake operators that go wrong past the
first trip.

GPU, per 'case' row.  Elementwise kernels: (a) every output pre-filled with NaN comes back finite, (b) the one large launch is BITWISE the
concatenation of launches over slices under half a trip (an element's result does not depend on the grid; no tolerance), (c) a float64 restatement at
the bound of the kernel's existing parity test, evaluated per trip region.  Adam: the UPDATE against float64, at three times the error torch's own
float32 Adam has on the same inputs.  The learned-graph front end through ``ops.mgp_front`` at the bound rule of tests/test_mgp_front.py.  The output
head at the hidden widths whose template arms no other test wraps.  The forward matrix-core forms at twice the device's residency ceiling, in the
per-node norm of tests/test_grad_scale.py.
"""
import math
import os

import pytest
import torch

from oracle.kernel_emul import EmulatedKernels
from stc_hip._lib import _ptr
from tests import launch_trips as LT
from tests.launch_trips import ROWS, check_launch, geometry_problems, log_parity, regions, rel, slices
from tests.test_grad_scale import per_node_err
from tests.test_hip_kernels import TOL
from tests.test_mgp_front import _reference as mgp_reference

EM = EmulatedKernels()
NOISE_FACTOR = 3.0            # over the reference's own float32 noise: the rule of tests/test_mgp_front.py and tests/test_scale_sweep.py
HEAD_DWB = 2e-5               # test_output_head's bound on dw | db
AXPY = 1e-7                  # test_axpy_concat_split's bound on y + a x (one fused rounding)
BF16_ULP = 2.0 ** -7          # tests/test_bf16_kernels.py: one bf16 ulp, checked as 2^-7 relative


def _case_rows():
    return [r for r in ROWS if r.status == 'case']


# ---- CPU: the table -------------------------------------------------------------------------------------------------------------------------------
def test_every_grid_stride_kernel_and_persistent_call_site_is_a_row():
    found, keys = LT.scan(), LT.table_keys()
    assert ('?' not in {k for _, k in found}), f'the scan could not name: {sorted(f for f in found if f[1] == "?")}'
    assert not found - keys, f'no row of tests/launch_trips.py for {sorted(found - keys)}: decide case / covered_by / exempt'
    assert not keys - found, f'rows the scan of csrc/ no longer finds: {sorted(keys - found)}'


def test_the_scan_misses_a_deleted_row_and_a_new_kernel(tmp_path):
    """The closure test's own controls: a table without a row, and a source tree with a grid-stride kernel nobody listed."""
    fewer = tuple(r for r in ROWS if r.kernel != 'axpy_kernel')
    assert ('stc_gates.hip', 'axpy_kernel') in LT.scan() - LT.table_keys(fewer)
    (tmp_path / 'new.hip').write_text('template <int N>\n__global__ __launch_bounds__(256) void fresh_kernel(float* y, long long n) {\n'
                                      '    for (long long i = blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = 0.f;\n}\n'
                                      'int launch() { int grid; return stc::persistent_grid<kern>("hipFuncSetAttribute(fresh site)", 256, 0, 1, 5, 4, INT_MAX, &grid); }\n')
    assert LT.scan(str(tmp_path)) == {('new.hip', 'fresh_kernel'), ('new.hip', 'fresh site')}


@pytest.mark.parametrize('row', ROWS, ids=lambda r: f'{r.kernel}{"@" + r.site.replace(" ", "-") if r.site else ""}')
def test_cap_text_is_where_the_row_says(row):
    for file, text in LT.pins(row):
        with open(os.path.join(LT.CSRC, file)) as f:
            assert text in f.read(), (f'{file} no longer holds "{text}": the cap of {row.kernel} ({row.entry}) moved -- revisit the row of tests/launch_trips.py '
                                      f'(per_trip = {row.trip(row.sizes[0]) if row.sizes else row.per_trip} {row.unit}) and the sizes of its cases')


def test_every_cap_text_names_one_place():
    """A cap text that another launch of the file shares would stay green when its own site moves: each occurs once (``EW_CAP`` is the one
    function ``ew_grid``, which its rows share on purpose)."""
    for row in ROWS:
        with open(os.path.join(LT.CSRC, row.file)) as f:
            assert f.read().count(row.cap) == 1, f'{row.kernel} / {row.site}: "{row.cap}" does not occur exactly once in {row.file}'
    caps = [(r.file, r.cap) for r in ROWS if r.cap != LT.EW_CAP]
    assert len(caps) == len(set(caps)), 'two rows pin the same text'


def test_a_moved_cap_constant_fails_the_pin(tmp_path, monkeypatch):
    """Control: a scratch copy of a source with its cap constant changed is reported under the row's name."""
    with open(os.path.join(LT.CSRC, 'stc_adam.hip')) as f:
        (tmp_path / 'stc_adam.hip').write_text(f.read().replace('256 * 8 ? 256 * 8', '256 * 16 ? 256 * 16'))
    monkeypatch.setattr(LT, 'CSRC', str(tmp_path))
    with pytest.raises(AssertionError, match='adam_kernel'):
        test_cap_text_is_where_the_row_says(ROWS[0])


def test_rows_are_well_formed():
    ids = set()
    for r in ROWS:
        assert r.status in LT.STATUSES and r.kernel and r.entry and r.cap, r
        assert (r.file, r.kernel, r.site) not in ids, f'two rows for {r.kernel} / {r.site}'
        ids.add((r.file, r.kernel, r.site))
        if r.status == 'case':
            assert r.sizes and r.per_trip is not None, f'{r.kernel}: a case row needs sizes and items per trip'
        elif r.status == 'covered_by':
            path, _, name = r.covered_by.partition('::')
            with open(os.path.join(LT.REPO, path)) as f:
                assert f'def {name}(' in f.read(), f'{r.kernel}: {r.covered_by} does not exist'
            assert r.why and r.params, f'{r.kernel}: covered_by needs the case and the argument why it takes two trips'
        else:
            assert len(r.why) > 40, f'{r.kernel}: an exemption needs a reason a reader can check'


@pytest.mark.parametrize('row,size', [(r, s) for r in _case_rows() for s in r.sizes], ids=lambda v: getattr(v, 'kernel', None) or getattr(v, 'id', None))
def test_every_case_takes_two_full_trips_and_a_ragged_one(row, size):
    assert not geometry_problems(row, size), f'{row.kernel} at {size.id} ({size.items} {row.unit}): {geometry_problems(row, size)}'


def test_the_geometry_check_has_teeth():
    adam = ROWS[0]
    ok = adam.sizes[0]
    assert not geometry_problems(adam, ok)
    for items, word in ((LT.ADAM_TRIP + 5 * 1024 + 300, 'full trips'), (2 * LT.ADAM_TRIP + 300, 'whole workgroup'), (2 * LT.ADAM_TRIP + 5 * 1024, 'splits no lane'),
                        (2 * LT.ADAM_TRIP + 5 * 1024 + 512, 'unroll'), (2 * LT.ADAM_TRIP + 5 * 1024 + 900, 'unroll')):
        msgs = geometry_problems(adam, LT.Size('x', items, ok.block, unroll=ok.unroll))
        assert any(word in m for m in msgs), (items, msgs)
    assert LT.ADAM_N == 16798896 and LT.trips(LT.ADAM_N // 4, LT.ADAM_TRIP, 1024) == (2, 5, 300)       # piece 0 full, 44 lanes of piece 1
    assert LT.mfma_nodes(256) == 16685
    assert regions(10, 4) == [('first', 0, 4), ('second', 4, 8), ('ragged', 8, 10)] and regions(3, 4) == [('first', 0, 3)]


# ---- CPU: negative controls of the checker ---------------------------------------------------------------------------------------------------------
class _FakeOperator:
    """y = 2 x + 1 over a 'launch' of rows lo..hi whose grid covers ``trip`` rows per trip."""
    trip, rows = 64, 2 * 64 + 3 * 8 + 5

    def __init__(self, fault=None):
        self.fault = fault
        self.x = torch.randn(self.rows, 3, generator=torch.Generator().manual_seed(7))

    def run(self, lo, hi):
        x, y = self.x[lo:hi], torch.full((hi - lo, 3), float('nan'))
        n = hi - lo
        if self.fault == 'first-trip-only':
            n = min(n, self.trip)                                     # everything past the first trip stays unwritten
            y[:n] = 2 * x[:n] + 1
        elif self.fault == 'stale-inputs':
            y[:] = 2 * x[torch.arange(n) % self.trip] + 1             # the later trips re-read the first trip's inputs
        else:
            y[:] = 2 * x + 1
        return dict(y=y)

    def problems(self):
        return check_launch(self.run, self.rows, self.trip, ref=dict(y=2 * self.x.double() + 1), bound=1e-6)


def test_the_checker_passes_a_correct_operator():
    assert _FakeOperator().problems() == []


def test_the_checker_reports_an_operator_that_writes_the_first_trip_only():
    found = _FakeOperator('first-trip-only').problems()
    assert any(p.startswith('(a)') and 'row 64' in p for p in found), found
    assert not any('first trip' in p for p in found if p.startswith('(c)')), found           # and it says WHERE: the first trip is right


def test_the_checker_reports_an_operator_that_reuses_the_first_trips_inputs():
    found = _FakeOperator('stale-inputs').problems()
    assert not any(p.startswith('(a)') for p in found), found                                # every element is written and finite: only (b), (c) can see it
    assert any(p.startswith('(b)') and 'row 64' in p for p in found), found
    assert {p.split(',')[1].split()[0] for p in found if p.startswith('(c)')} == {'second', 'ragged'}, found


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip():
    from stc_hip._lib import HipKernels
    k = HipKernels()
    yield k
    k.set_dispatch_level(0)


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device='cuda')


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


def _cut(t, lo, hi):
    return {k: v[lo:hi] for k, v in t.items()}


def _f64(t):
    return {k: v.double() for k, v in t.items()}


def _nan64(like, *shape):
    return torch.full(shape, float('nan'), dtype=torch.float64, device=like.device)


def _rows_case(spec):
    rows, a, b, pad = spec['rows'], spec['a'], spec['b'], spec['pad']
    return rows, a, b, pad, a + b + pad


def _gates(hip, spec):
    """(inputs, {name: (launch, twin)}) of the two gate kernels on rows [Xt | H | pad]."""
    rows, cin, h, pad, L = _rows_case(spec)
    g = _gen(rows + cin)
    t = dict(G=_randn(g, rows, 2 * h), Xt=_randn(g, rows, cin), H=_randn(g, rows, h), dCi=_randn(g, rows, L), dU=_randn(g, rows, h), owed=_randn(g, rows, h))
    t['U'], t['R'] = torch.sigmoid(_randn(g, rows, h)), torch.sigmoid(_randn(g, rows, h))

    def fwd(k, s, new):
        n = len(s['H'])
        o = dict(U=new(n, h), Rg=new(n, h), CandIn=new(n, L))
        k.gru_gates_fwd(s['G'], s['Xt'], s['H'], o['U'], o['Rg'], o['CandIn'])
        return o

    def bwd(k, s, new):
        n = len(s['H'])
        o = dict(dG=new(n, 2 * h), dXt=new(n, cin), dH=new(n, h))
        k.gru_gates_bwd(s['dCi'], s['dU'], s['H'], s['U'], s['R'], o['dG'], o['dXt'], o['dH'], dH_in=s['owed'])
        return o
    return t, dict(gates_fwd=(fwd, TOL), gates_bwd=(bwd, TOL))                 # test_gru_gates_and_blend's bound


def _cat_split(hip, spec):
    rows, a, b, pad, L = _rows_case(spec)
    g = _gen(rows + a + 1)
    t = dict(A=_randn(g, rows, a), B=_randn(g, rows, b), src=_randn(g, rows, L), owedA=_randn(g, rows, a), owedB=_randn(g, rows, b))

    def concat(k, s, new):
        o = dict(out=new(len(s['A']), L))
        k.concat2(s['A'], s['B'], o['out'])
        return o

    def split(k, s, new):                                              # in place: the halves already hold a gradient (clones)
        o = dict(A=s['owedA'].clone(), B=s['owedB'].clone())
        k.split2(s['src'], o['A'], o['B'], addA=o['A'], addB=o['B'])
        return o

    def split_plain(k, s, new):
        o = dict(A=new(len(s['src']), a), B=new(len(s['src']), b))
        k.split2(s['src'], o['A'], o['B'])
        return o

    # test_axpy_concat_split holds these to ``torch.equal``: copies, and ONE float32 addition per element where a half is already owed a gradient
    pad0 = lambda s: torch.zeros(len(s['A']), pad, device=s['A'].device)
    return t, dict(concat2=(concat, lambda s: dict(out=torch.cat([s['A'], s['B'], pad0(s)], -1))),
                   split2_in_place=(split, lambda s: dict(A=s['src'][:, :a] + s['owedA'], B=s['src'][:, a:a + b] + s['owedB'])),
                   split2=(split_plain, lambda s: dict(A=s['src'][:, :a], B=s['src'][:, a:a + b])))


def _blend(hip, n):
    g = _gen(n)
    t = dict(Cpre=2 * _randn(g, n), U=torch.sigmoid(_randn(g, n)), H=_randn(g, n), dHn=_randn(g, n))
    t['Cand'] = torch.tanh(_randn(g, n))

    def fwd(k, s, new):
        o = dict(Cand=new(len(s['H'])), Hnew=new(len(s['H'])))
        k.gru_blend_fwd(s['Cpre'], s['U'], s['H'], o['Cand'], o['Hnew'])
        return o

    def bwd(k, s, new):
        o = dict(dCpre=new(len(s['H'])), dU=new(len(s['H'])), dH=new(len(s['H'])))
        k.gru_blend_bwd(s['dHn'], s['U'], s['H'], s['Cand'], o['dCpre'], o['dU'], o['dH'])
        return o
    return t, dict(blend_fwd=(fwd, TOL), blend_bwd=(bwd, TOL))


def _axpy(hip, n):
    g = _gen(n + 1)
    t = dict(x=_randn(g, n), y=_randn(g, n))

    def run(k, s, new):
        o = dict(y=s['y'].clone())
        k.axpy(-1.5, s['x'], o['y'])
        return o
    return t, dict(axpy=(run, AXPY))


#: id -> (builder, its size argument, items per row, whether the float4 form must run).  A builder returns the operands and, per launch,
#: (launch, rule): the rule is the bound of the kernel's existing parity test against the twin in float64, or -- where that test asks for
#: ``torch.equal`` -- the float32 expression the result must equal exactly.
ELEMENTWISE = {
    'gates-scalar': (_gates, LT.SCALAR_ROWS, 20, False),
    'gates-vector': (_gates, LT.VECTOR_ROWS, 8, True),
    'concat-split-scalar': (_cat_split, LT.SCALAR_ROWS, 20, False),
    'concat-split-vector': (_cat_split, LT.VECTOR_ROWS, 8, True),
    'blend-scalar': (_blend, LT.FLAT_SCALAR_N, 1, False),
    'blend-vector': (_blend, LT.FLAT_VECTOR_N, 0.25, True),
    'axpy': (_axpy, LT.FLAT_SCALAR_N, 1, False),
}


def _exactly(name, got, want):
    return None if torch.equal(got, want) else f'{int((got != want).sum())} elements differ from the float32 expression (exact: copies and single additions)'


def _flat_parts(n, trip, vec):
    """Slices of a flat operand that keep the launch's arm: float4 form -- starts and lengths multiples of 4; scalar form -- an odd length, so that no
    slice has a length the float4 form takes (its starts then leave the 16-byte grid after the first, which the scalar form does not mind)."""
    if vec:
        return slices(n, int(trip / 2) - 4)
    width = (int(trip / 2) - 8) | 1
    parts = [(lo, min(n, lo + width)) for lo in range(0, n, width)]
    assert all((hi - lo) % 4 or lo % 4 for lo, hi in parts)
    return parts


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(ELEMENTWISE))
def test_elementwise_kernels_past_the_first_trip(hip, case):
    build, spec, items_per_row, vec = ELEMENTWISE[case]
    covered = [r for r in _case_rows() if any(s.id == case for s in r.sizes)]
    assert covered and all((r.unit == 'float4s') == vec for r in covered), f'{case}: no row of the table, or the wrong arm'
    t, launches = build(hip, spec)
    rows = len(next(iter(t.values())))
    trip_rows = LT.EW_TRIP / items_per_row
    assert int(rows * items_per_row) == covered[0].sizes[0].items
    flat = isinstance(spec, int)
    parts = _flat_parts(rows, trip_rows, vec) if flat else None
    t64 = _f64(t)
    problems = []
    for name, (launch, rule) in launches.items():
        if callable(rule):
            ref, bound, judge = rule(t), None, _exactly
        else:
            ref, bound, judge = launch(EM, t64, lambda *s: _nan64(next(iter(t.values())), *s)), rule, None
        problems += check_launch(lambda lo, hi: launch(hip, _cut(t, lo, hi), _nan), rows, trip_rows, ref=ref, bound=bound, judge=judge, parts=parts,
                                 what=f'{case} {name}.')
    assert not problems, '\n'.join(problems)


@pytest.mark.gpu
def test_bf16_blend_backward_past_the_first_trip(hip):
    n, bf = LT.BF16_BLEND_N, torch.bfloat16
    g = _gen(n)
    dHn, U, Cand = _randn(g, n).to(bf), torch.sigmoid(_randn(g, n)).to(bf), torch.tanh(_randn(g, n)).to(bf)

    def run(lo, hi):
        out = _nan(hi - lo, dtype=bf)
        hip.bf16.gru_blend_bwd(dHn[lo:hi], U[lo:hi], None, Cand[lo:hi], out, None, None)
        return dict(dCpre=out)

    want = (dHn.double() * U.double() * (1 - Cand.double() ** 2))

    def one_ulp(name, got, ref):                                       # tests/test_bf16_kernels.py::assert_one_ulp, against float64 rounded to bf16 once
        w = ref.to(bf).double()
        diff = (got.double() - w).abs()
        floor = 4e-6 * float(w.abs().max())
        if not bool((diff <= w.abs() * BF16_ULP + floor).all()):
            return f'beyond one bf16 ulp: max difference {float(diff.max()):.3e}'
        return None if float((diff > 0).double().mean()) <= 0.05 else f'{float((diff > 0).double().mean()):.3f} of the elements differ'
    trip = 8 * LT.BF16_BLEND_TRIP
    problems = check_launch(run, n, trip, ref=dict(dCpre=want), judge=one_ulp, parts=slices(n, trip // 2 - 8, step=8), what='blend_bwd_bf16 ')
    assert not problems, '\n'.join(problems)


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------------------
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def _adam64(p, g, m, v, t, wd):
    """The float64 formulas of tests/test_guard_bands.py::_adam at step t: (p, m, v, g')."""
    b1, b2 = HYPER['beta1'], HYPER['beta2']
    g = g + wd * p
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    return p - HYPER['lr'] / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + HYPER['eps']), m, v, g


def _adam_excess(new, old, want, g1):
    """Per element, what the three bounds of the update are multiples of: (|p - p64| - 2^-23 |p64|)+ / |dp64|, |m - m64| / (|g'| + |m_old|),
    |v - v64| / |v64| (an element whose denominator is zero must be exact)."""
    p64, m64, v64 = want
    out = {}
    for name, err, den in (('p', ((new[0].double() - p64).abs() - 2.0 ** -23 * p64.abs()).clamp_min(0), (p64 - old[0].double()).abs()),
                           ('m', (new[1].double() - m64).abs(), g1.abs() + old[1].double().abs()),
                           ('v', (new[2].double() - v64).abs(), v64.abs())):
        assert bool((err[den == 0] == 0).all()), f'adam.{name}: an element with nothing to compare against is not exact'
        out[name] = torch.where(den > 0, err / den.clamp_min(1e-300), torch.zeros_like(err))
    return out


@pytest.fixture(scope='module')
def adam_inputs():
    n = LT.ADAM_N
    g = _gen(n)
    return dict(p=_randn(g, n), g=_randn(g, n), m=0.1 * _randn(g, n), v=0.01 * _randn(g, n).abs())


@pytest.mark.gpu
@pytest.mark.parametrize('weight_decay', [0.0, 1e-4])
@pytest.mark.parametrize('t', [1, 3, 1000])
def test_adam_update_past_the_first_trip(hip, adam_inputs, t, weight_decay, monkeypatch):
    from stc_hip.optim import Adam
    d, n = adam_inputs, LT.ADAM_N
    trip = 4 * LT.ADAM_TRIP
    step = torch.tensor([float(t)], device='cuda')
    old = (d['p'], d['m'], d['v'])

    def run(lo, hi):
        o = dict(p=d['p'][lo:hi].clone(), m=d['m'][lo:hi].clone(), v=d['v'][lo:hi].clone())
        hip.adam(o['p'], d['g'][lo:hi], o['m'], o['v'], step, weight_decay=weight_decay, **HYPER)
        return o
    # (a), (b): finite, and bitwise the launches over slices under half a trip (starts on 16-byte boundaries; the clones keep them)
    problems = check_launch(run, n, trip, parts=slices(n, trip // 2 - 4), what=f'adam t={t} wd={weight_decay} ')
    assert not problems, '\n'.join(problems)
    got = run(0, n)
    *want, g1 = _adam64(d['p'].double(), d['g'].double(), d['m'].double(), d['v'].double(), t, weight_decay)
    # the yardstick: torch's own float32 Adam (capturable: the step count on the device, as the kernel has it) on the same inputs
    ref_p = torch.nn.Parameter(d['p'].clone())
    ref_p.grad = d['g'].clone()
    ref = torch.optim.Adam([ref_p], lr=HYPER['lr'], betas=(HYPER['beta1'], HYPER['beta2']), eps=HYPER['eps'], weight_decay=weight_decay, capturable=True, foreach=False)
    ref.state[ref_p] = dict(step=torch.tensor(float(t - 1), device='cuda'), exp_avg=d['m'].clone(), exp_avg_sq=d['v'].clone())
    ref.step()
    st = ref.state[ref_p]
    assert float(st['step']) == t
    noise = {k: float(x.max()) for k, x in _adam_excess((ref_p.data, st['exp_avg'], st['exp_avg_sq']), old, want, g1).items()}
    ours = _adam_excess((got['p'], got['m'], got['v']), old, want, g1)
    failures = []
    for name in ('p', 'm', 'v'):
        c = NOISE_FACTOR * noise[name]
        assert noise[name] <= c          # (true by construction -- the bound is a multiple of this very figure -- and tests nothing: kept as the statement
                                         # that the yardstick is measured with the same three quantities, on the same inputs, as the kernel)
        for region, lo, hi in regions(n, trip):
            err = float(ours[name][lo:hi].max())
            log_parity(f'adam t={t} wd={weight_decay} {name} {region}', err, noise[name], NOISE_FACTOR, c)
            print(f'adam t={t} wd={weight_decay} {name} {region}: kernel {err:.3e}, torch float32 {noise[name]:.3e}, bound {c:.3e}')
            if not err <= c:
                failures.append(f'{name}, {region} trip: {err:.3e} > {NOISE_FACTOR:g} x {noise[name]:.3e}')
    assert not failures, '\n'.join(failures)
    if t == 3:                                                         # the same update through the optimizer class
        monkeypatch.setattr(Adam, 'LARGE_BYTES', 1 << 20)
        p = torch.nn.Parameter(d['p'].clone())
        p.grad = d['g'].clone()
        opt = Adam([p], lr=HYPER['lr'], betas=(HYPER['beta1'], HYPER['beta2']), eps=HYPER['eps'], weight_decay=weight_decay)
        opt.state[p] = dict(step=torch.tensor(2.0, device='cuda'), exp_avg=d['m'].clone(), exp_avg_sq=d['v'].clone())
        assert opt._ours(opt.param_groups[0], p)
        opt.step()
        assert float(opt.state[p]['step']) == 3
        for name, a in (('p', p.data), ('m', opt.state[p]['exp_avg']), ('v', opt.state[p]['exp_avg_sq'])):
            assert torch.equal(a, got[name]), f'stc_hip.optim.Adam: {name} differs from the kernel called directly'


# ---- learned-graph front end ------------------------------------------------------------------------------------------------------------------------
def _mgp_operands(s):
    g = torch.Generator().manual_seed(s['B'] * 1000 + s['N'])
    X = (torch.rand(s['B'], s['T'], s['N'], s['C'], generator=g) < 0.3).float()
    F, R = (s['C'], s['N']) if s['rows_axis'] == 2 else (s['N'], s['C'])
    Wu, Wv = (torch.randn(F, s['h'], generator=g) * (2.0 / (F + s['h'])) ** 0.5 for _ in range(2))
    return X.cuda(), Wu.cuda(), Wv.cuda(), torch.randn(R, R, generator=g).cuda(), R


@pytest.mark.gpu
@pytest.mark.parametrize('spec', [LT.MGP_NODES, LT.MGP_CATEGORIES], ids=['mgp-nodes', 'mgp-categories'])
def test_mgp_front_past_the_first_trip(hip, spec):
    """``ops.mgp_front`` with gradients against ``_reference`` of tests/test_mgp_front.py in float64, that file's bound rule unchanged: nodes -- the uv
    forward's outputs and the softmax backward's entries both take two trips and a ragged third; categories -- the uv forward's outputs."""
    from stc_hip import ops
    X, Wu, Wv, W, R = _mgp_operands(spec)
    axis = spec['rows_axis']
    a64, b64 = Wu.double().requires_grad_(), Wv.double().requires_grad_()
    want = mgp_reference(X.double(), a64, b64, 3, axis == 3)
    (want * W.double()).sum().backward()
    a32, b32 = Wu.clone().requires_grad_(), Wv.clone().requires_grad_()
    want32 = mgp_reference(X, a32, b32, 3, axis == 3)
    (want32 * W).sum().backward()
    fwd_noise, grad_noise = rel(want32, want), max(rel(a32.grad, a64.grad), rel(b32.grad, b64.grad))
    fwd_bound, grad_bound = max(1e-5, NOISE_FACTOR * fwd_noise), max(2e-5, NOISE_FACTOR * grad_noise)
    a, b = Wu.clone().requires_grad_(), Wv.clone().requires_grad_()
    assert ops.mgp_front_supported(X, a, b)
    got = ops.mgp_front(X, a, b, axis, 3.0)
    (got * W).sum().backward()
    errs = dict(Ps=rel(got, want.detach()), dWu=rel(a.grad, a64.grad), dWv=rel(b.grad, b64.grad))
    for name, err in errs.items():
        noise, bound = (fwd_noise, fwd_bound) if name == 'Ps' else (grad_noise, grad_bound)
        log_parity(f'mgp_front {spec["B"]}x{spec["T"]}x{spec["N"]}x{spec["C"]} h={spec["h"]} {name}', err, noise, NOISE_FACTOR, bound)
        print(f'mgp_front axis {axis} {name}: {err:.3e}, torch float32 {noise:.3e}, bound {bound:.3e}')
    assert got.shape == (R, R) and bool(torch.isfinite(got).all()) and errs['Ps'] < fwd_bound, (errs, fwd_bound)
    assert errs['dWu'] < grad_bound and errs['dWv'] < grad_bound, (errs, grad_bound)


@pytest.mark.gpu
@pytest.mark.parametrize('spec', [LT.MGP_NODES, LT.MGP_CATEGORIES], ids=['mgp-nodes', 'mgp-categories'])
def test_mgp_uv_forward_past_the_first_trip(hip, spec):
    X, Wu, Wv, _, R = _mgp_operands(spec)
    axis, alpha = spec['rows_axis'], 3.0
    per_row = spec['B'] * spec['T'] * spec['h']

    def run(lo, hi):
        # the binding allocates U, V itself (torch.empty): the entry point is called on NaN-filled buffers this test owns, with the binding's arguments
        part = (X[:, :, lo:hi, :] if axis == 2 else X[..., lo:hi]).contiguous()
        K, rows, F, ks, rs, fs = hip._mgp_strides(part, axis)
        U, V = _nan(rows, K, spec['h']), _nan(rows, K, spec['h'])
        hip._launch('stc_mgp_uv_fwd_f32', part, _ptr(part), ks, rs, fs, _ptr(Wu), _ptr(Wv), alpha, _ptr(U), _ptr(V), K, rows, F, spec['h'])
        if (lo, hi) == (0, R):                                         # and the binding hands out the same bits
            U2, V2 = hip.mgp_uv_fwd(part, axis, Wu, Wv, alpha)
            assert torch.equal(U, U2) and torch.equal(V, V2)
        return dict(U=U, V=V)

    x = (X if axis == 2 else X.transpose(2, 3)).double()               # (B, T, R, F)
    ref = {n: torch.tanh(alpha * torch.matmul(x, w.double())).flatten(0, 1).transpose(0, 1).contiguous() for n, w in (('U', Wu), ('V', Wv))}
    problems = check_launch(run, R, LT.MGP_TRIP / per_row, ref=ref, bound=TOL, parts=slices(R, int(LT.MGP_TRIP / per_row / 2) - 1, step=1), what='mgp_uv_fwd ')
    assert not problems, '\n'.join(problems)


@pytest.mark.gpu
def test_mgp_softmax_backward_entries_past_the_first_trip(hip):
    """The entries of stc_mgp_softmax_bwd_f32 at R^2 = two trips and a ragged third, against float64 autograd of softmax(relu(P - P^T)) per trip region
    of the rows.  An entry reads its transposed partner and two row dots, so no slice of the launch is a launch: (b) is the same bits twice."""
    R = LT.MGP_NODES['N']
    g = _gen(R)
    P, dPs = 3 * _randn(g, R, R), _randn(g, R, R)
    Ps = hip.mgp_softmax_fwd(P)
    p64 = P.double().requires_grad_()
    want_Ps = torch.softmax(torch.relu(p64 - p64.t()), -1)
    (want_Ps * dPs.double()).sum().backward()
    p32 = P.clone().requires_grad_()
    (torch.softmax(torch.relu(p32 - p32.t()), -1) * dPs).sum().backward()
    assert rel(Ps, want_Ps.detach()) < TOL
    Ps_in = want_Ps.detach().float()
    rowdot, dP = _nan(R), _nan(R, R)                                   # (the binding allocates both with torch.empty: NaN-filled buffers of the test's own)
    hip._launch('stc_mgp_softmax_bwd_f32', P, _ptr(P), _ptr(Ps_in), _ptr(dPs), _ptr(rowdot), _ptr(dP), R)
    assert bool(torch.isfinite(dP).all()) and bool(torch.isfinite(rowdot).all())
    assert torch.equal(dP, hip.mgp_softmax_bwd(P, Ps_in, dPs))
    failures = []
    for region, lo, hi in regions(R, LT.MGP_TRIP / R):
        noise = rel(p32.grad[lo:hi], p64.grad[lo:hi])
        bound = max(2e-5, NOISE_FACTOR * noise)
        err = rel(dP[lo:hi], p64.grad[lo:hi])
        log_parity(f'mgp_softmax_bwd R={R} dP {region}', err, noise, NOISE_FACTOR, bound)
        if not err < bound:
            failures.append(f'dP, {region} trip (rows {lo}..{hi}): {err:.3e} >= {bound:.3e}')
    assert not failures, '\n'.join(failures)


# ---- output head -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('h', LT.HEAD_WIDTHS)
def test_output_head_past_the_first_trip(hip, h):
    rows, lpr = LT.head_rows(h), LT.head_lpr(h)
    fwd_trip, bwd_trip = LT.EW_TRIP // lpr, LT.HEAD_PARTS * LT.EW_THREADS // lpr
    g = _gen(h)
    H, w, b, dy = _randn(g, rows, h), 0.5 * _randn(g, h), _randn(g, 1), _randn(g, rows)
    y64, dH64, dwb64 = _nan64(H, rows), _nan64(H, rows, h), _nan64(H, h + 1)
    EM.head_fwd(H.double(), w.double(), b.double(), y64)
    y_in = y64.float()
    EM.head_bwd(H.double(), w.double(), y_in.double(), dy.double(), dH64, dwb64)

    def fwd(lo, hi):
        y = _nan(hi - lo)
        hip.head_fwd(H[lo:hi], w, b, y)
        return dict(y=y)

    kept = {}

    def bwd(lo, hi):
        dH, dwb = _nan(hi - lo, h), _nan(h + 1)
        hip.head_bwd(H[lo:hi], w, y_in[lo:hi], dy[lo:hi], dH, dwb)
        kept.setdefault((lo, hi), dwb)
        return dict(dH=dH)
    parts = slices(rows, bwd_trip // 2 - 1, step=1)                    # under half a BACKWARD trip: a quarter of a forward one
    problems = check_launch(fwd, rows, fwd_trip, ref=dict(y=y64), bound=TOL, parts=parts, what=f'head h={h} ')
    problems += check_launch(bwd, rows, bwd_trip, ref=dict(dH=dH64), bound=TOL, parts=parts, what=f'head h={h} ')
    assert not problems, '\n'.join(problems)
    dwb = kept[(0, rows)]
    assert bool(torch.isfinite(dwb).all()) and rel(dwb, dwb64) < HEAD_DWB, rel(dwb, dwb64)
    again = _nan(h + 1)
    hip.head_bwd(H, w, y_in, dy, _nan(rows, h), again)
    assert torch.equal(dwb, again)                                     # fixed-order reduction over the partial rows of every trip


# ---- forward matrix-core forms: two trips at any occupancy ---------------------------------------------------------------------------------------
C32, H16, K2 = 32, 16, 2


def _device_nodes():
    nodes = LT.mfma_nodes(torch.cuda.get_device_properties(0).multi_processor_count)
    assert nodes >= 2 * LT.MAX_WAVES_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count + 5
    return nodes


@pytest.fixture(scope='module')
def node_case():
    """Operands of the node convolution at C = 32, L = 32, Ho = 16, K = 2 (the conventions of tests/test_hip_kernels.py) and the CPU twin's results, once."""
    nodes, L = _device_nodes(), 32
    g = torch.Generator().manual_seed(nodes)
    Zs = [torch.randn(nodes, C32, L, generator=g) for _ in range(K2)]
    Tc = torch.randn(K2, C32, C32, generator=g) / C32 ** 0.5
    Tc[0] = torch.eye(C32)
    W, b = torch.randn(K2 * K2 * L, H16, generator=g) / (K2 * K2 * L) ** 0.5, torch.randn(H16, generator=g)
    Y, A, Bm = (torch.empty(nodes, C32, H16) for _ in range(3))
    EM.bdg_node_fwd(Zs, Tc, W, b, Y)
    EM.node_post_fwd(Zs[0], Tc, W, b, A, Bm)
    return dict(nodes=nodes, Zs=[z.cuda() for z in Zs], Tc=Tc.cuda(), W=W.cuda(), b=b.cuda(), Y=Y, A=A, Bm=Bm)


def _per_node(got, want, bound, what, within=False):
    """``within``: the bound itself passes -- the one-ulp rule is |a - b| <= 2^-7 |b| (tests/test_bf16_kernels.py::assert_one_ulp), and in the per-node
    norm one ulp of a node whose maximum is a power of two (2.0 -> 2.015625) is EXACTLY 2^-7 of that maximum."""
    assert bool(torch.isfinite(got.float()).all()), f'{what}: a non-finite result (a node no trip reached?)'
    err = per_node_err(got.float(), want.float())
    print(f'{what}: per-node error {err:.3e} (bound {bound:.1e})')
    assert err <= bound if within else err < bound, f'{what}: per-node error {err:.3e} beyond {bound:.1e}'


LEVELS = {'default': 0, 'fp32-mfma': 1, 'generic-only': 2}


@pytest.fixture(scope='module')
def node_forward_by_level(hip, node_case):
    """Y of stc_bdg_node_fwd_f32 under each dispatch ceiling, once."""
    c, out = node_case, {}
    for path, level in LEVELS.items():
        hip.set_dispatch_level(level)
        try:
            out[path] = _nan(c['nodes'], C32, H16)
            hip.bdg_node_fwd(c['Zs'], c['Tc'], c['W'], c['b'], out[path])
        finally:
            hip.set_dispatch_level(0)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('path,next_path', [('default', 'fp32-mfma'), ('fp32-mfma', 'generic-only')])
def test_node_forward_at_twice_the_residency(hip, node_case, node_forward_by_level, path, next_path):
    c, Y = node_case, node_forward_by_level[path]
    _per_node(Y, c['Y'], TOL, f'node forward [{path}] at {c["nodes"]} nodes')
    # that the launch took the form its row names: the entry point falls through to the next path without a word where a form declines (an LDS
    # limit, an alignment), and the case would pass on the generic kernel.  The shape is in the matrix-core set, and the three forms do not
    # share their arithmetic (two fp16 pieces per operand / fp32 matrix cores / fmaf chains): a launch that fell through has the next form's bits
    assert hip.cell_fused_supported(K2, K2, C32, 32, H16), 'C = 32, L = 32, K = 2 left the matrix-core shape set'
    assert not torch.equal(Y, node_forward_by_level[next_path]), f'[{path}] returns the bits of [{next_path}]: the launch fell through to that form'


@pytest.mark.gpu
def test_post_aggregation_forward_at_twice_the_residency(hip, node_case):
    c = node_case
    A, Bm = _nan(c['nodes'], C32, H16), _nan(c['nodes'], C32, H16)
    assert hip.node_post_supported(K2, K2, C32, 32, H16)
    hip.node_post_fwd(c['Zs'][0], c['Tc'], c['W'], c['b'], A, Bm)         # (this entry point has the one form: where it declines the call raises, no other path runs)
    _per_node(A, c['A'], TOL, 'node_post_fwd A')
    _per_node(Bm, c['Bm'], TOL, 'node_post_fwd Bm')


@pytest.mark.gpu
def test_bf16_node_forward_at_twice_the_residency(hip):
    nodes, L, bf = _device_nodes(), 32, torch.bfloat16
    g = torch.Generator().manual_seed(nodes + 1)
    Zs = [torch.randn(nodes, C32, L, generator=g).to(bf) for _ in range(K2)]
    Tc = torch.softmax(torch.randn(K2, C32, C32, generator=g), -1)          # (the operands of tests/test_bf16_kernels.py::_node_inputs_bf16)
    Tc[0] = torch.eye(C32)
    W, b = torch.randn(K2 * K2 * L, H16, generator=g) * 0.2, torch.randn(H16, generator=g)
    assert hip.node_bf16_supported(K2, K2, C32, L, H16)
    want = torch.empty(nodes, C32, H16, dtype=bf)
    EM.bdg_node_fwd_bf16(Zs, Tc, W, b, want)
    got = _nan(nodes, C32, H16, dtype=bf)
    hip.bdg_node_fwd_bf16([z.cuda() for z in Zs], Tc.cuda(), W.cuda(), b.cuda(), got)
    _per_node(got, want, BF16_ULP, 'bf16 node forward', within=True)


@pytest.mark.gpu
def test_bf16_gates_forward_at_twice_the_residency(hip):
    nodes, bf, h = _device_nodes(), torch.bfloat16, H16
    kb = hip.bf16
    assert kb.cell_planar_supported(K2, K2, C32, h)
    g = torch.Generator().manual_seed(nodes + 2)
    rnd = lambda *s: torch.randn(*s, generator=g)
    X, SX, H, SH = (rnd(nodes, C32, h).to(bf) for _ in range(4))
    Tc = rnd(K2, C32, C32) / C32 ** 0.5
    Tc[0] = torch.eye(C32)
    Wg, bg = rnd(K2 * K2 * 2 * h, 2 * h) / (4 * 2 * h) ** 0.5, rnd(2 * h)
    want = [torch.empty(nodes, C32, h) for _ in range(3)]
    EM.cell_gates_fwd_planar(X.float(), H.float(), SX.float(), SH.float(), Tc, Wg, bg, *want)
    got = [_nan(nodes, C32, h, dtype=bf) for _ in range(3)]
    kb.cell_gates_fwd_planar(X.cuda(), H.cuda(), SX.cuda(), SH.cuda(), Tc.cuda(), Wg.cuda(), bg.cuda(), *got)
    for name, a, w in zip(('U', 'R', 'R*H'), got, want):
        _per_node(a, w.to(bf), BF16_ULP, f'bf16 gates forward {name}', within=True)
