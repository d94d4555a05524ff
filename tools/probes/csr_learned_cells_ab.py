"""A/B of ``graph_mode='csr-learned'`` with ``csr_cells='fused'`` against ``'per-cell'`` at C = 32 in one process (numbers: profiles/r17/INDEX.md).

Per shape, two configurations of the eager train step (forward + ComboLoss + backward + Adam) built from the same seed, in alternating order,
``--repeats`` timed repeats of ``--calls`` steps each:
  (a) ``'fused'``: the cell-graph executor as one autograd node -- PLANAR cells, per cell one ``stc_graph_grad_csr_pairs_f32`` launch, two dT_c
      launches and, for a narrow input, one ``stc_cell_dsx_narrow_planar_f32`` launch;
  (b) ``'per-cell'``: one autograd node per cell, value gradients from ``stc_csr_sddmm_f32`` -- the default.
Shapes: a 100 x 100 queen grid, C = 32, 4 samples, rank 16, T = 9 + 3; the 224 x 224 grid, C = 32, at the first of ``--metric-batches`` samples at which
both configurations fit (an allocator refusal moves on to the next, smaller count).
Per configuration: median and spread of the step, peak memory, C entry points launched per step; for (a) also the two new kernels' microseconds per
launch and achieved TB/s on their algorithmic bytes (HIP events around each launch, ``_lib.KernelTimer``).

    python tools/probes/csr_learned_cells_ab.py [--skip-metric] [--json out/csr_learned_cells_ab.json]
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
NEW = ('stc_graph_grad_csr_pairs_f32', 'stc_cell_dsx_narrow_planar_f32')
RANK = 16


class Config:
    def __init__(self, tag, graph, C, B, T, horizon, cells, state=None):
        self.tag, self.graph = tag, graph
        torch.manual_seed(0)
        self.model = M.STCGNN(graph.n, C, 2, 2, 1, 16, 2, horizon, graph_mode='csr-learned', fusion_rank=RANK, spatial_graph=graph, csr_cells=cells).cuda()
        if state is not None:
            self.model.load_state_dict(state)
        g = torch.Generator().manual_seed(1)
        self.X = (torch.rand(B, T, graph.n, C, generator=g) < 0.1635).float().cuda()
        self.Y = (torch.rand(B, horizon, graph.n, C, generator=g) < 0.1635).float().cuda()
        self.Ac = torch.softmax(torch.randn(C, C, generator=g), -1).cuda()
        self.loss = ComboLoss()
        self.opt = StcAdam(self.model.parameters(), lr=2e-3, weight_decay=1e-4, capturable=True)

    def step(self):
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss(self.model(X_seq=self.X, As=self.graph, Ac=self.Ac), self.Y)
        loss.backward()
        self.opt.step()
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
    fused = Config("a: csr_cells='fused'", graph, C, B, T, horizon, 'fused')
    per_cell = Config("b: csr_cells='per-cell'", graph, C, B, T, horizon, 'per-cell', fused.model.state_dict())
    configs, rows = [fused, per_cell], []
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
        row = dict(shape=name, grid=[H, W], C=C, batch=B, T=T, horizon=horizon, rank=RANK, config=c.tag, step_ms=ms, step_ms_median=med(ms),
                   spread_ms=max(ms) - min(ms), peak_MiB=peak, entry_points_per_step=len(names), new_launches={n: names.count(n) for n in NEW},
                   sddmm_launches=names.count('stc_csr_sddmm_f32'))
        if c is fused:
            k = ops.kernels()
            k.timer = KernelTimer(only=NEW)
            try:
                for _ in range(3):
                    c.step()
                summary = k.timer.summary()
            finally:
                k.timer = None
            row['kernels'] = {n: dict(launches=s['launches'], us_per_launch=1e3 * s['ms'] / s['launches'], TBps=s['bytes'] / (1e9 * s['ms']))
                              for n, s in summary.items()}
        rows.append(row)
        print(f'{name} B={B} {c.tag:28s} {med(ms):9.2f} ms (spread {max(ms) - min(ms):.2f}), peak {peak:9.0f} MiB, {len(names)} entry points per step '
              f'({row["sddmm_launches"]} sddmm, {sum(row["new_launches"].values())} new)'
              + ''.join(f'; {n.replace("stc_", "").replace("_f32", "")} {v["us_per_launch"]:.1f} us x{v["launches"]} {v["TBps"]:.2f} TB/s'
                        for n, v in row.get('kernels', {}).items()), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--metric-batches', type=int, nargs='+', default=[8, 4, 2, 1])
    ap.add_argument('--skip-metric', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    rows = shape('grid100', 100, 100, 32, 4, 9, 3, a)
    if not a.skip_metric:
        for B in a.metric_batches:
            torch.cuda.empty_cache()
            try:
                rows += shape('metric', 224, 224, 32, B, 9, 3, a)
                break
            except torch.OutOfMemoryError:
                print(f'metric B={B}: does not fit in both configurations', flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
