"""A/B of ``graph_mode='csr-category-learned'`` in one process (numbers: profiles/r16/INDEX.md).

Per shape, three configurations of the eager train step (forward + ComboLoss + backward + Adam), in alternating order, ``--repeats`` timed repeats
of ``--calls`` steps each:
  (a) the mode: the cell-graph executor with ``learn_Tc`` (PLANAR cells, two dT_c launches per cell);
  (b) the mode with ``ops._DTC = False``: one autograd node per cell -- how this training ran before the kernels existed;
  (c) ``'csr-fixed'`` given the same frozen ``Gc``: what the learning itself costs.
Shapes: a 100 x 100 queen grid, C = 32, 4 samples, T = 9 + 3; the metric shape (224 x 224, C = 32) at ``--metric-batch`` samples.
Per configuration: median and spread of the step, peak memory, C entry points launched per step; for (a) also the two kernels' microseconds per
launch and achieved TB/s on their algorithmic bytes (HIP events around each launch, ``_lib.KernelTimer``).

    python tools/probes/gc_learned_ab.py [--skip-metric] [--json out/gc_learned_ab.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, 'stc-gnn_amd')]
import torch          # noqa: E402

import STC_GNN as M          # noqa: E402
from stc_hip import CsrGraph, ops          # noqa: E402
from stc_hip._lib import KernelTimer          # noqa: E402
from stc_hip.loss import ComboLoss          # noqa: E402
from stc_hip.optim import Adam as StcAdam          # noqa: E402

med = lambda v: sorted(v)[len(v) // 2]
DTC = ('stc_cell_dtc_gates_planar_f32', 'stc_cell_dtc_cand_planar_f32')


class Config:
    def __init__(self, tag, graph, C, B, T, horizon, mode, dtc, state=None):
        self.tag, self.dtc, self.graph = tag, dtc, graph
        torch.manual_seed(0)
        self.model = M.STCGNN(graph.n, C, 2, 2, 1, 16, 2, horizon, graph_mode=mode).cuda()
        if state is not None:
            self.model.load_state_dict(state, strict=False)
        g = torch.Generator().manual_seed(1)
        self.X = (torch.rand(B, T, graph.n, C, generator=g) < 0.1635).float().cuda()
        self.Y = (torch.rand(B, horizon, graph.n, C, generator=g) < 0.1635).float().cuda()
        self.Ac = torch.softmax(torch.randn(C, C, generator=g), -1).cuda()
        self.loss = ComboLoss()
        self.opt = StcAdam(self.model.parameters(), lr=2e-3, weight_decay=1e-4, capturable=True)

    def step(self):
        ops._DTC = self.dtc
        try:
            self.opt.zero_grad(set_to_none=True)
            loss = self.loss(self.model(X_seq=self.X, As=self.graph, Ac=self.Ac), self.Y)
            loss.backward()
            self.opt.step()
        finally:
            ops._DTC = True
        return loss


def entry_points(call):
    k, log = ops.kernels(), []
    inner = k._launch
    k._launch = lambda name, *a, **kw: (log.append(name), inner(name, *a, **kw))[1]
    try:
        call()
        torch.cuda.synchronize()
    finally:
        del k._launch
    return log


def shape(name, H, W, C, B, T, horizon, a):
    graph = CsrGraph.queen_grid(H, W, normalize=True)
    learned = Config('a: csr-category-learned', graph, C, B, T, horizon, 'csr-category-learned', True)
    per_cell = Config('b: the same, ops._DTC off', graph, C, B, T, horizon, 'csr-category-learned', False, learned.model.state_dict())
    fixed = Config('c: csr-fixed, frozen Gc', graph, C, B, T, horizon, 'csr-fixed', True, learned.model.state_dict())
    with torch.no_grad():
        fixed.Ac = learned.model.mix_graph_pair(learned.X, learned.Ac)
    configs, rows = [learned, per_cell, fixed], []
    for c in configs:
        for _ in range(2):
            c.step()
        torch.cuda.synchronize()
    times = {c.tag: [] for c in configs}
    for r in range(a.repeats):
        for c in (configs if r % 2 == 0 else configs[::-1]):         # alternating order
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                c.step()
            torch.cuda.synchronize()
            times[c.tag].append(1e3 * (time.perf_counter() - t0) / a.calls)
    for c in configs:
        torch.cuda.reset_peak_memory_stats()
        names = entry_points(c.step)
        peak = torch.cuda.max_memory_allocated() / 2 ** 20
        ms = times[c.tag]
        row = dict(shape=name, grid=[H, W], C=C, batch=B, T=T, horizon=horizon, config=c.tag, step_ms=ms, step_ms_median=med(ms), spread_ms=max(ms) - min(ms),
                   peak_MiB=peak, entry_points_per_step=len(names), dtc_launches=sum(names.count(n) for n in DTC))
        if c is learned:
            k = ops.kernels()
            k.timer = KernelTimer(only=DTC)
            try:
                for _ in range(3):
                    c.step()
                summary = k.timer.summary()
            finally:
                k.timer = None
            row['kernels'] = {n: dict(launches=s['launches'], us_per_launch=1e3 * s['ms'] / s['launches'], TBps=s['bytes'] / (1e9 * s['ms']))
                              for n, s in summary.items()}
        rows.append(row)
        print(f'{name} {c.tag:32s} {med(ms):9.2f} ms (spread {max(ms) - min(ms):.2f}), peak {peak:9.0f} MiB, {len(names)} entry points per step'
              + ''.join(f'; {n.replace("stc_cell_", "").replace("_planar_f32", "")} {v["us_per_launch"]:.1f} us x{v["launches"]} {v["TBps"]:.2f} TB/s'
                        for n, v in row.get('kernels', {}).items()), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--metric-batch', type=int, default=2)
    ap.add_argument('--skip-metric', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    rows = shape('grid100', 100, 100, 32, 4, 9, 3, a)
    if not a.skip_metric:
        torch.cuda.empty_cache()
        rows += shape('metric', 224, 224, 32, a.metric_batch, 9, 3, a)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
