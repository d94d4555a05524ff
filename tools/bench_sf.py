#!/usr/bin/env python3
"""SF-shape train step (config 3 of BASELINE.json: B=32, T=9+3, N=100, C=5, h=16, K=2, 2 layers) on one MI355X.
--order 3: the same model at Chebyshev order 3 (the reference's ``Main.py -K 3``); with --mode dense-learned --graph: learned dense graphs
on the few-category cell kernels' order-3 dense form where the kernel set has it.  --repeats R times the step loop R times (their spread is
the run-to-run noise of one process); --json adds one JSON line with every repeat.
--mode dense-learned: the reference's full model incl. MGP_Gen/MixedFusion (2e8 parameters, Adam over 800 MB);
--mode csr-fixed: encoder/decoder/head only on the fixed 10x10 queen grid (22 033 parameters).
--infer: the forward alone under ``torch.no_grad()`` (evaluation: no loss, no optimizer; --graph captures that forward); the JSON line then
carries ``infer``, ``peak_bytes`` (peak allocation of the timed loops above what was allocated before them, after warm-up) and a ``checksum`` of the prediction.
Prints ms/step and samples/s (reference on 8 CPU cores: 67 samples/s fwd+bwd, ~30 with Adam)."""
import argparse
import json
import os
import sys
import time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'stc-gnn_amd')):
    sys.path.insert(0, p)
import torch
import STC_GNN as M
from stc_hip import CsrGraph, ops
from stc_hip.loss import ComboLoss

ap = argparse.ArgumentParser()
ap.add_argument('--mode', default='csr-fixed')
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--order', type=int, default=2, help='Chebyshev order of both graphs (Main.py -K)')
ap.add_argument('--repeats', type=int, default=1, help='time the loop of --steps steps this many times')
ap.add_argument('--json', action='store_true', help='also print one JSON line (ms per step of every repeat, their median and spread)')
ap.add_argument('--graph', action='store_true', help='capture the whole train step in a HIP graph and replay it')
ap.add_argument('--fused-adam', action='store_true', help='torch.optim.Adam(fused=True): one multi-tensor kernel per step instead of ~10 passes')
ap.add_argument('--infer', action='store_true', help='time the forward alone under torch.no_grad(): no loss, no optimizer')
ap.add_argument('--profile', action='store_true', help='print the kernels of 3 steps by GPU time (torch.profiler)')
ap.add_argument('--fusion-rank', type=int, default=None, help="dense-learned: MixedFusion(N, rank=R), rank-R factors in place of the two Linear(N^2, N^2) layers")
ap.add_argument('--grid', type=int, nargs=2, metavar=('H', 'W'), default=[10, 10], help='the queen grid (default: the SF shape, 10 x 10)')
ap.add_argument('--categories', type=int, default=5, help='incident categories C (default: the SF shape, 5)')
a = ap.parse_args()
dev = torch.device('cuda')
torch.manual_seed(0)
(GH, GW), C = a.grid, a.categories
B, T, N, h, K, layers, hor = 32, 9, GH * GW, 16, a.order, 2, 3
model = M.STCGNN(N, C, K, K, 1, h, layers, hor, graph_mode=a.mode, **({} if a.fusion_rank is None else {'fusion_rank': a.fusion_rank})).to(dev)
X = (torch.rand(B, T, N, C, device=dev) < 0.1635).float()
Y = (torch.rand(B, hor, N, C, device=dev) < 0.1635).float()
if a.mode == 'csr-fixed':
    As = CsrGraph.queen_grid(GH, GW, normalize=True, device=dev)
else:
    As = CsrGraph.queen_grid(GH, GW, normalize=False).to_dense().to(dev)
Ac = torch.rand(C, C, device=dev)
crit = ComboLoss()
opt = None if a.infer else torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=1e-4, capturable=a.graph, **({'fused': True} if a.fused_adam else {}))


def train_step():
    opt.zero_grad(set_to_none=True)
    loss = crit(model(X_seq=X, As=As, Ac=Ac), Y)
    loss.backward()
    opt.step()
    return loss


def infer_step():
    with torch.no_grad():
        return model(X_seq=X, As=As, Ac=Ac)


step = infer_step if a.infer else train_step


small_calls = []                             # whether the cells run on the few-category kernels (stc_hip/small.py) or the general path
_small_graph = ops.stc_small_graph
ops.stc_small_graph = lambda *args, **kw: (small_calls.append(1), _small_graph(*args, **kw))[1]
for _ in range(3):
    step()
torch.cuda.synchronize()
if a.graph:
    # static inputs X, Y; grads live in the graph's private pool (set_to_none=True recreates them at each replay); --infer: the static prediction
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = step()
    eager_step, step = step, (lambda: (graph.replay(), static_loss)[1])
    torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
allocated_before = torch.cuda.memory_allocated()
times = []
for _ in range(max(1, a.repeats)):
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) / a.steps)
dt = sorted(times)[len(times) // 2]
peak_bytes = torch.cuda.max_memory_allocated() - allocated_before
result = dict(infer=True, peak_bytes=peak_bytes, checksum=float(loss.double().sum())) if a.infer else dict(loss=float(loss.detach()))      # (--infer: `loss` is the prediction)
print(f'SF shape {a.mode}{" K=3" if K == 3 else ""}{" hipGraph" if a.graph else ""}{" fused-adam" if a.fused_adam else ""}{" no_grad forward" if a.infer else ""}: {1e3 * dt:.2f} ms/step, {B / dt:.1f} samples/s, '
      + (f'peak {peak_bytes / 2 ** 20:.1f} MiB, checksum {result["checksum"]:.6f}, ' if a.infer else f'loss {result["loss"]:.4f}, ')
      + f'{sum(p.numel() for p in model.parameters())} parameters', flush=True)
if a.json:
    print(json.dumps(dict(shape='sf', mode=a.mode, order=K, batch=B, **({} if a.fusion_rank is None else dict(fusion_rank=a.fusion_rank, grid=[GH, GW], categories=C)), hip_graph=a.graph, fused_adam=a.fused_adam, steps=a.steps, ms_per_step=1e3 * dt,
                          repeats_ms=[1e3 * t for t in times], spread_ms=1e3 * (max(times) - min(times)), samples_per_s=B / dt,
                          cells_on_small_graph_kernels=bool(small_calls), **result)), flush=True)
if a.profile:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            step()
        torch.cuda.synchronize()
    print(prof.key_averages().table(sort_by='cuda_time_total', row_limit=22, max_name_column_width=60), flush=True)
