"""Same-process A/B of ``ComboLoss`` alone, forward + backward: the torch ops (``loss._FUSED = False``) against the fused HIP kernels.

Shapes: the SF shape (32, 3, 100, 5) and the metric shape (8, 6, 50176, 32), each as the model hands the prediction over -- a
(horizon, B, N, C) tensor seen through ``transpose(0, 1)`` -- and as a contiguous tensor; each eager and as HIP-graph replays; three repeats.
Prints, per combination, the GPU kernels and memory copies of one eager call (torch.profiler) and the microseconds per call (host clock around a
loop of calls, one synchronize at its end: eager figures include the host side of the launches, replays do not), then one JSON line with everything.

    python tools/probes/combo_loss_ab.py [--repeats 3] [--shapes sf metric]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, 'stc-gnn_amd')]
import torch          # noqa: E402
from torch.profiler import ProfilerActivity, profile          # noqa: E402

from stc_hip import loss as L          # noqa: E402

SHAPES = {'sf': ((32, 3, 100, 5), 300), 'metric': ((8, 6, 50176, 32), 10)}          # (B, horizon, N, C), calls per timed loop


def operands(shape, layout, dev):
    g = torch.Generator().manual_seed(0)
    p = torch.rand(*shape, generator=g).clamp(0.01, 0.99)
    y = (torch.rand(*shape, generator=g) < 0.1635).float().to(dev)
    if layout == 'transposed':
        p = p.transpose(0, 1).contiguous().to(dev).transpose(0, 1)
    else:
        p = p.to(dev)
    return p.requires_grad_(), y


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
    ap.add_argument('--shapes', nargs='+', default=list(SHAPES), choices=list(SHAPES))
    a = ap.parse_args()
    dev = torch.device('cuda')
    crit = L.ComboLoss()
    rows = []
    for name in a.shapes:
        shape, calls = SHAPES[name]
        for layout in ('transposed', 'contiguous'):
            p, y = operands(shape, layout, dev)

            def call():
                p.grad = None
                loss = crit(p, y)
                loss.backward()
                return loss

            for fused in (False, True):
                L._FUSED = fused
                for _ in range(3):
                    value = float(call().detach())
                launches = gpu_launches(call)
                eager = timed(call, calls, a.repeats)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        call()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    call()
                replay = timed(graph.replay, calls, a.repeats)
                del graph
                med = lambda v: sorted(v)[len(v) // 2]
                row = dict(shape=name, dims=list(shape), layout=layout, route='fused' if fused else 'torch', loss=value, gpu_launches=launches,
                           eager_us=eager, eager_us_median=med(eager), replay_us=replay, replay_us_median=med(replay))
                rows.append(row)
                print(f'{name:6s} {layout:10s} {row["route"]:5s}: {launches:3d} GPU launches per call; eager {med(eager):9.1f} us (spread {max(eager) - min(eager):.1f}), '
                      f'replay {med(replay):9.1f} us (spread {max(replay) - min(replay):.1f}); loss {value:.6f}', flush=True)
            del p, y
            torch.cuda.empty_cache()
    L._FUSED = True
    print(json.dumps(dict(probe='combo_loss_ab', repeats=a.repeats, rows=rows)), flush=True)


if __name__ == '__main__':
    main()
