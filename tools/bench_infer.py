#!/usr/bin/env python3
"""Forward-only (evaluation / forecasting) step of the csr-fixed metric configuration: the model bench.py trains, run under torch.no_grad().

    python tools/bench_infer.py --steps 10 --warmup 3            (shape arguments as bench.py: --grid --categories --hidden --order --layers --obs --pred
                                                                   --batch-per-gpu)

Prints ONE JSON line: ms_per_forward (mean of the timed steps, between two synchronizes), samples_per_s, peak_allocated_bytes (torch's peak over
the timed steps, model, graph and input included; peak_above_inputs_bytes: without them), samples_per_gpu, and est_max_samples_per_gpu = how many
samples the device's memory holds at the measured bytes per sample (peak above the inputs + the input window, both linear in the batch) -- derived
from the measurement, not probed by filling the device.  Uses nothing but the public module, so it measures any commit of this repository.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, 'stc-gnn_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--grid', type=int, default=224, help='H = W of the queen grid (N = grid^2)')
    ap.add_argument('--categories', type=int, default=32)
    ap.add_argument('--hidden', type=int, default=16)
    ap.add_argument('--order', type=int, default=2, help='Chebyshev order Ks = Kc')
    ap.add_argument('--layers', type=int, default=2)
    ap.add_argument('--obs', type=int, default=18)
    ap.add_argument('--pred', type=int, default=6)
    ap.add_argument('--batch-per-gpu', type=int, default=8)
    a = ap.parse_args()

    import torch
    import STC_GNN as M
    from stc_hip import CsrGraph

    if not torch.cuda.is_available():
        raise SystemExit('bench_infer.py needs the MI355X (no CPU path)')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    N, C, B = a.grid * a.grid, a.categories, a.batch_per_gpu
    graph = CsrGraph.queen_grid(a.grid, a.grid, normalize=True, device=dev)
    Gc = torch.softmax(torch.randn(C, C, generator=torch.Generator().manual_seed(7)), -1).to(dev)
    torch.manual_seed(42)
    model = M.STCGNN(N, C, a.order, a.order, 1, a.hidden, a.layers, a.pred, graph_mode='csr-fixed').to(dev).eval()
    X = (torch.rand(B, a.obs, N, C, generator=torch.Generator().manual_seed(1000)) < 0.1635).float().to(dev)

    with torch.no_grad():
        for _ in range(max(1, a.warmup)):
            y = model(X_seq=X, As=graph, Ac=Gc)
        torch.cuda.synchronize(dev)
        del y
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            y = model(X_seq=X, As=graph, Ac=Gc)
        torch.cuda.synchronize(dev)
        seconds = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated(dev)
    total = torch.cuda.get_device_properties(dev).total_memory
    per_sample = (peak - before + X.numel() * X.element_size()) / B
    fixed = before - X.numel() * X.element_size()                      # model, graph operands, workspaces
    ms = 1e3 * seconds / a.steps
    print(json.dumps(dict(metric='forward-only csr-fixed STC-GNN step (no_grad)', ms_per_forward=ms, samples_per_s=B / (ms * 1e-3), samples_per_gpu=B,
                          peak_allocated_bytes=peak, peak_above_inputs_bytes=peak - before, device_total_bytes=total,
                          est_max_samples_per_gpu=int((total - fixed) // per_sample), steps=a.steps, warmup=a.warmup, checksum=float(y.double().sum()),
                          shape=dict(N=N, C=C, hidden=a.hidden, order=a.order, layers=a.layers, obs=a.obs, pred=a.pred), device=torch.cuda.get_device_name(dev))))


if __name__ == '__main__':
    main()
