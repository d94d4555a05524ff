"""Same-process A/B of ``MixedFusion(n, rank=r)`` alone, forward + backward: the torch ops (``fusion._FUSED = False``) against the fused HIP
kernels (``csrc/stc_mixed_fusion_lr.hip``).

Shapes (n, r): (100, 16) the SF grid, (240, 16) CHI, (300, 16) NYC, (300, 64) the highest rank; A a 0/1 prior at rate 0.3, P a softmax of
normals, every parameter and A, P wanting a gradient; each eager and as HIP-graph replays; three repeats.  Prints, per combination, the GPU
kernels and memory copies of one eager call and of one replay (torch.profiler) and the microseconds per call (host clock around a loop of calls, one synchronize
at its end: eager figures include the host side of the launches, replays do not), then one JSON line with everything.

    python tools/probes/mixed_fusion_lr_ab.py [--repeats 3] [--shapes 100x16 240x16 300x16 300x64] [--calls 200]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, 'stc-gnn_amd')]
import torch          # noqa: E402
from torch.profiler import ProfilerActivity, profile          # noqa: E402

import STC_GNN as M          # noqa: E402
from stc_hip import fusion as F          # noqa: E402

SHAPES = ['100x16', '240x16', '300x16', '300x64']


def timed(call, calls, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        out.append(1e6 * (time.perf_counter() - t0) / calls)
    return out


def gpu_launches(call):
    """Kernels and memory copies / sets of one call, as the profiler's device-side events."""
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200, help='calls per timed loop')
    ap.add_argument('--shapes', nargs='+', default=SHAPES, help='n x r pairs, e.g. 100x16')
    a = ap.parse_args()
    dev = torch.device('cuda')
    rows = []
    for name in a.shapes:
        n, r = (int(v) for v in name.split('x'))
        torch.manual_seed(n + r)
        mod = M.MixedFusion(n, rank=r).to(dev)
        A = (torch.rand(n, n, device=dev) < 0.3).float().requires_grad_()
        P = torch.softmax(torch.randn(n, n, device=dev), -1).requires_grad_()
        R = torch.randn(n, n, device=dev)
        leaves = [A, P, *mod.parameters()]

        def call():
            for t in leaves:
                t.grad = None
            G = mod(A, P)
            G.backward(R)
            return G

        for fused in (False, True):
            F._FUSED = fused
            for _ in range(3):
                checksum = float(call().detach().double().sum())
            launches = gpu_launches(call)
            eager = timed(call, a.calls, a.repeats)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    call()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                call()
            replay_launches = gpu_launches(graph.replay)
            replay = timed(graph.replay, a.calls, a.repeats)
            del graph
            med = lambda v: sorted(v)[len(v) // 2]
            row = dict(n=n, rank=r, route='fused' if fused else 'torch', checksum=checksum, gpu_launches=launches, replay_gpu_launches=replay_launches,
                       eager_us=eager, eager_us_median=med(eager), replay_us=replay, replay_us_median=med(replay))
            rows.append(row)
            print(f'n {n:4d} rank {r:3d} {row["route"]:5s}: {launches:3d} GPU launches per eager call, {replay_launches:3d} per replay; eager {med(eager):8.1f} us (spread {max(eager) - min(eager):.1f}), '
                  f'replay {med(replay):8.1f} us (spread {max(replay) - min(replay):.1f}); sum(G) {checksum:.6f}', flush=True)
        del mod, A, P, R, leaves
        torch.cuda.empty_cache()
    F._FUSED = True
    print(json.dumps(dict(probe='mixed_fusion_lr_ab', repeats=a.repeats, calls=a.calls, rows=rows)), flush=True)


if __name__ == '__main__':
    main()
