"""Helpers of tests/test_cell_graph_trace.py: the launches of ``ops.stc_cell_graph`` as data.

``Traced`` wraps a kernel set and logs every launch the cell-graph executor makes through it: the method's name and its arguments and keywords,
encoded recursively -- a tensor as (buffer number by first appearance of its storage, storage offset, shape, stride, dtype), ``None``, numbers,
bools and strings as they are.  The capability questions (``*_supported``, ``ring2_fits``), ``act_amax_buffer`` and plain attributes pass
through unlogged; ``for_graph`` and ``bf16`` return wrapped sets that share the log.  Every numbered storage is kept alive until the log is
dropped, so no address comes back under a second number.

``CASES`` are forward + backward runs of the executor (``_SMALL`` off) whose traces tests/cell_graph_traces.json pins: per case and kernel set
the launch names of each direction and a SHA-256 over the canonical JSON of the full encoding.  The fixture is recorded from a checkout that is
known good -- ``python tests/launch_trace.py --record cpu|gpu`` uses public entry points only, so the same file runs there -- and is never
regenerated from the code it checks.  ``--bits FILE`` writes a SHA-256 of every array a case returns (states, parameter gradients): two
checkouts computed the same bits when their files are equal.
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'cell_graph_traces.json')
_UNLOGGED = ('act_amax_buffer', 'ring2_fits')

FANOUT_SCHEDULE = [(1, ('ext', 0), ('ext', 2))] + [(0, ('cell', 0), ('ext', 2))] * 7 + [(0, ('cell', 3), ('cell', 0))]
FANOUT_OUTPUTS = list(range(1, 9))


class Traced:
    def __init__(self, inner, log=None, held=None, overrides=None):
        self.__dict__.update(_inner=inner, _log=[] if log is None else log, _held={} if held is None else held, _overrides=overrides or {})

    def _wrap(self, inner):
        return Traced(inner, self._log, self._held, self._overrides)

    def _encode(self, a):
        if isinstance(a, torch.Tensor):
            st = a.untyped_storage()
            number = self._held.setdefault(st.data_ptr(), (len(self._held), st))[0]
            return ['tensor', number, a.storage_offset(), list(a.shape), list(a.stride()), str(a.dtype)]
        if isinstance(a, (list, tuple)):
            return [self._encode(v) for v in a]
        if isinstance(a, dict):
            return {str(k): self._encode(v) for k, v in sorted(a.items())}
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        return f'<{type(a).__name__}>'

    @property
    def bf16(self):
        return self._wrap(self._inner.bf16)

    def for_graph(self, row_sum_bound):
        return self._wrap(self._inner.for_graph(row_sum_bound))

    def __getattr__(self, name):
        if name in self._overrides:
            return self._overrides[name]
        attr = getattr(self._inner, name)
        if not callable(attr) or name.endswith('_supported') or name in _UNLOGGED:
            return attr

        def launch(*args, **kw):
            self._log.append([name, self._encode(args), self._encode(kw)])
            return attr(*args, **kw)
        return launch


def _general_inputs(schedule, C, K, grid, B, dev, dtype):
    import STC_GNN as M
    from stc_hip import CsrGraph
    N, h = grid[0] * grid[1], 16
    graph = CsrGraph.queen_grid(*grid, normalize=True)
    pair = M._graphs(graph, torch.softmax(torch.randn(C, C), -1).to(dev), K, K)
    cells = (M.STC_Cell(N, C, K, K, h, h).to(dev), M.STC_Cell(N, C, K, K, 1, h).to(dev))     # parameter set 0 = wide, 1 = narrow
    ext = [torch.rand(B, N, C, w).to(dev).to(dtype) for w in (1, h, h)]                      # as tests/test_module_parity._general_schedule
    params = [p for c in cells for p in (c.gates.W, c.gates.b, c.candi.W, c.candi.b)]
    return pair, ext, [tuple(params[:4]), tuple(params[4:])], params


def run_case(name, kind):
    """One case on kernel set ``kind`` ('cpu': the emulated twin, 'gpu': the HIP library).  Returns (forward launches, backward launches,
    {name: array}) with the launches in ``Traced``'s encoding."""
    import STC_GNN as M
    from stc_hip import CsrGraph, ops
    case = CASES[name]
    K, grid, B = case['K'], case.get('grid', (4, 5)), case.get('B', 2)
    dev = 'cpu' if kind == 'cpu' else 'cuda'
    dtype = torch.bfloat16 if case.get('bf16') else torch.float32
    if kind == 'cpu':
        from oracle.kernel_emul import EmulatedKernels
        inner, C = EmulatedKernels(case.get('fmt')), 8 if grid == (16, 16) else 4
    else:
        from stc_hip._lib import HipKernels
        inner, C = HipKernels(), case.get('C', 32)
    k = Traced(inner, overrides={'cell_bwd_planar_supported': lambda *a: False} if case.get('two_launch') else None)
    switches = dict(_kernels=k, _SMALL=False, _PLANAR=case.get('planar', True), _POST_AGG=case.get('post_agg', True))
    before = {n: getattr(ops, n) for n in switches}
    for n, v in switches.items():
        setattr(ops, n, v)
    try:
        torch.manual_seed(77)
        if case['sched'] == 'model':
            graph = CsrGraph.queen_grid(*grid, normalize=True)
            model = M.STCGNN(grid[0] * grid[1], C, K, K, 1, 16, 2, 2, graph_mode='csr-fixed').to(dev)
            pair = M._graphs(graph, torch.softmax(torch.randn(C, C), -1).to(dev), K, K)
            X = torch.rand(B, 3, grid[0] * grid[1], C, 1).to(dev)
            Rw = torch.randn(2, B, grid[0] * grid[1], C).to(dev)
            states = model._run_cell_graph(pair, X)
            assert states is not None, 'the model did not take the cell-graph path'
            out, params = model._head(states), dict(model.named_parameters())
        else:
            schedule, outputs = {'general': (None, None), 'fanout': (FANOUT_SCHEDULE, FANOUT_OUTPUTS)}[case['sched']]
            if schedule is None:
                from tests.test_module_parity import GENERAL_OUTPUTS as outputs, GENERAL_SCHEDULE as schedule
            pair, ext, stacks, flat = _general_inputs(schedule, C, K, grid, B, dev, dtype)
            Rw = torch.randn(len(outputs), B, grid[0] * grid[1], C, 16).to(dev)
            out = ops.stc_cell_graph(pair.spatial, pair.Tc, K, schedule, outputs, ext, stacks)
            params = {f'{i // 4}.{"Wg bg Wc bc".split()[i % 4]}': p for i, p in enumerate(flat)}
        n_fwd = len(k._log)
        (out.float() * Rw).sum().backward()
        arrays = {'out': out.detach(), **{f'd{n}': p.grad for n, p in params.items() if p.grad is not None}}
        return k._log[:n_fwd], k._log[n_fwd:], {n: t.float().cpu().numpy() for n, t in arrays.items()}
    finally:
        for n, v in before.items():
            setattr(ops, n, v)


def summary(launches):
    """What the fixture keeps of one direction: the launch names and the hash of the full encoding."""
    blob = json.dumps(launches, sort_keys=True, separators=(',', ':'))
    return {'names': [l[0] for l in launches], 'sha256': hashlib.sha256(blob.encode()).hexdigest()}


_G = dict(sched='general')
CASES = {
    'general-k2-one-launch': dict(_G, K=2),
    'general-k2-two-launch': dict(_G, K=2, two_launch=True),
    'general-k2-rows-post': dict(_G, K=2, planar=False),
    'general-k2-rows-slabs': dict(_G, K=2, planar=False, post_agg=False),
    'general-k3': dict(_G, K=3),
    'general-k3-rows': dict(_G, K=3, planar=False),
    'general-k2-bf16': dict(_G, K=2, bf16=True),
    'general-k2-one-launch-f16x2': dict(_G, K=2, fmt='f16x2', only='cpu'),     # (the HIP library runs this format by default)
    'general-k3-f16x2': dict(_G, K=3, fmt='f16x2', only='cpu'),
    'general-k2-c64': dict(_G, K=2, C=64, only='gpu'),                        # the two-launch backward as the library itself chooses it
    'ring2-k2': dict(_G, K=2, grid=(16, 16), B=1),
    'ring2-k3': dict(_G, K=3, grid=(16, 16), B=1),
    'fanout-k2-two-launch': dict(sched='fanout', K=2, two_launch=True),
    'fanout-k3': dict(sched='fanout', K=3),
    'fanout-k2-bf16': dict(sched='fanout', K=2, bf16=True),
    'model-k2': dict(sched='model', K=2),
    'model-k3': dict(sched='model', K=3),
}


def cases_of(kind):
    return [n for n, c in CASES.items() if c.get('only', kind) == kind]


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--record', choices=['cpu', 'gpu'], help='run every case of this kernel set and write its half of the fixture')
    ap.add_argument('--out', default=FIXTURE, help='fixture file to update (default: the committed one)')
    ap.add_argument('--bits', help='also write "case array sha256" lines of every returned array to this file')
    ap.add_argument('--commit', default='', help='the commit the record is taken at (kept in the fixture)')
    a = ap.parse_args(argv)
    if not a.record:
        ap.error('--record cpu|gpu')
    fixture = json.load(open(a.out)) if os.path.exists(a.out) else {}
    half, lines = {'recorded_at': a.commit}, []
    for name in cases_of(a.record):
        fwd, bwd, arrays = run_case(name, a.record)
        half[name] = {'forward': summary(fwd), 'backward': summary(bwd)}
        lines += [f'{name} {n} {hashlib.sha256(arr.tobytes()).hexdigest()}' for n, arr in sorted(arrays.items())]
        print(f'{name}: {len(fwd)} forward, {len(bwd)} backward launches', flush=True)
    fixture[a.record] = half
    with open(a.out, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')
    if a.bits:
        with open(a.bits, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'stc-gnn_amd')]
    main(sys.argv[1:])
