"""One-process measurements of ``graph_mode='csr-learned'`` (``csrc/stc_mgp_csr.hip``, ``stc_hip.learned``):

1. the spatial branch of the generator alone (``learned.mgp_csr_front``: U / V, score, softmax), forward + backward, the HIP kernels against the
   torch route (``learned.csr._FUSED = False``), eager and as HIP-graph replays, with the GPU launches of one call (torch.profiler's device-side
   events) and the C entry points launched;
2. a whole train step (forward, ComboLoss, backward, Adam) on the synthetic 32 x 32 grid with 8 categories (N = 1 024), ``csr-learned`` at rank 16
   against ``dense-learned`` at rank 16, eager;
3. one forward + backward of the ``csr-learned`` model at 2 samples on growing queen grids up to 224 x 224 (the general per-cell path), with the
   step time and the peak of torch's allocator: the largest grid that fits.

Prints one line per measurement, then one JSON line with everything.  No time here is a pass / fail number.

    python tools/probes/mgp_csr_ab.py [--repeats 3] [--calls 20] [--grids 64 128 176 224]"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, 'stc-gnn_amd')]
import torch          # noqa: E402
from torch.profiler import ProfilerActivity, profile          # noqa: E402

import STC_GNN as M          # noqa: E402
from stc_hip import CsrGraph, learned, ops          # noqa: E402
from stc_hip import data as sdata          # noqa: E402
from stc_hip.graph import csr_pattern          # noqa: E402
from stc_hip.learned import csr as L          # noqa: E402
from stc_hip.loss import ComboLoss          # noqa: E402
from stc_hip.trainer import Trainer          # noqa: E402

med = lambda v: sorted(v)[len(v) // 2]


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
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def entry_points(call):
    """The C entry points one call launches, in order."""
    k, log = ops.kernels(), []
    inner = k._launch
    k._launch = lambda name, *a, **kw: (log.append(name), inner(name, *a, **kw))[1]
    try:
        call()
        torch.cuda.synchronize()
    finally:
        del k._launch
    return log


def branch(H, W, C, B, T, h, a, routes):
    dev = torch.device('cuda')
    graph = CsrGraph.queen_grid(H, W, normalize=True)
    pat = csr_pattern(graph, dev)
    torch.manual_seed(H + C)
    X = (torch.rand(B, T, H * W, C, device=dev) < 0.1635).float()
    Wu, Wv = (torch.nn.init.xavier_normal_(torch.empty(C, h, device=dev)).requires_grad_() for _ in range(2))
    R = torch.randn(graph.nnz, device=dev)

    def call():
        Wu.grad = Wv.grad = None
        Ps = learned.mgp_csr_front(X, Wu, Wv, pat, 3.0)
        Ps.backward(R)
        return Ps

    rows = []
    for fused in routes:
        L._FUSED = fused
        for _ in range(3):
            checksum = float(call().detach().double().sum())
        names = entry_points(call)
        launches = gpu_launches(call)
        eager = timed(call, a.calls, a.repeats)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                call()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        replay_launches = gpu_launches(g.replay)
        replay = timed(g.replay, a.calls, a.repeats)
        del g
        row = dict(section='branch', grid=[H, W], N=H * W, nnz=graph.nnz, C=C, K=B * T, h=h, KH=B * T * h, route='kernels' if fused else 'torch', checksum=checksum,
                   entry_points=names, gpu_launches=launches, replay_gpu_launches=replay_launches, eager_us=eager, eager_us_median=med(eager),
                   replay_us=replay, replay_us_median=med(replay))
        rows.append(row)
        print(f'branch {H}x{W} C={C} KH={B * T * h} {row["route"]:7s}: {launches:3d} GPU launches per eager call, {replay_launches:3d} per replay; '
              f'eager {med(eager):9.1f} us (spread {max(eager) - min(eager):.1f}), replay {med(replay):9.1f} us (spread {max(replay) - min(replay):.1f}); '
              f'entry points {" ".join(n.replace("stc_", "") for n in names)}; sum(Ps) {checksum:.4f}', flush=True)
    L._FUSED = True
    del X, Wu, Wv, R
    torch.cuda.empty_cache()
    return rows


def train_steps(a):
    rows = []
    H, W, C = 32, 32, 8
    base = dict(device='cuda:0', H=H, W=W, C=C, batch_size=8, obs_len=9, pred_len=3, split_ratio=[6, 1, 1], model='STC-GNN', cheby_order=2, hidden_dim=16,
                nn_layers=2, learn_rate=2e-3, decay_rate=1e-4, num_epochs=1, time_slice=4, city='SYN', fusion_rank=16, output_dir=tempfile.mkdtemp(prefix='mgp_csr_ab_'))
    for mode in ('csr-learned', 'dense-learned'):
        data = sdata.synthetic_incidents(H, W, C, 60, sparse_graph=mode == 'csr-learned')
        loaders = sdata.get_data_loader(base, data, base['obs_len'], base['pred_len'], base['split_ratio'])
        torch.manual_seed(0)
        trainer = Trainer(dict(base), data, graph_mode=mode)
        x, y = next(iter(loaders['train']))
        trainer.model.train()
        for _ in range(2):
            loss = float(trainer._step(x, y))
        torch.cuda.reset_peak_memory_stats()
        ms = [t / 1e3 for t in timed(lambda: trainer._step(x, y), max(2, a.calls // 4), a.repeats)]
        n_param = sum(p.numel() for p in trainer.model.parameters())
        row = dict(section='train_step', mode=mode, N=H * W, C=C, batch=int(x.shape[0]), rank=16, parameters=n_param, loss=loss, step_ms=ms, step_ms_median=med(ms),
                   peak_GB=torch.cuda.max_memory_allocated() / 2 ** 30)
        rows.append(row)
        print(f'train step {mode:13s} N={H * W} C={C} batch {x.shape[0]} rank 16: {med(ms):8.2f} ms eager (spread {max(ms) - min(ms):.2f}), '
              f'{n_param / 1e6:.1f} M parameters, peak {row["peak_GB"]:.2f} GB, loss {loss:.4f}', flush=True)
        del trainer, loaders, data
        torch.cuda.empty_cache()
    return rows


def largest_grid(a):
    rows = []
    dev = torch.device('cuda')
    C, T, horizon, B = 8, 9, 3, 2
    for side in a.grids:
        try:
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            graph = CsrGraph.queen_grid(side, side, normalize=True)
            torch.manual_seed(side)
            model = M.STCGNN(side * side, C, 2, 2, 1, 16, 2, horizon, graph_mode='csr-learned', fusion_rank=16, spatial_graph=graph).to(dev)
            X = (torch.rand(B, T, side * side, C, device=dev) < 0.1635).float()
            Y = (torch.rand(B, horizon, side * side, C, device=dev) < 0.1635).float()
            Ac = torch.softmax(torch.randn(C, C, device=dev), -1)
            crit = ComboLoss()

            def step():
                model.zero_grad(set_to_none=True)
                loss = crit(model(X_seq=X, As=graph, Ac=Ac), Y)
                loss.backward()
                return loss

            loss = float(step().detach())
            ms = [t / 1e3 for t in timed(step, 2, 2)]
            row = dict(section='largest_grid', grid=[side, side], N=side * side, nnz=graph.nnz, C=C, batch=B, fits=True, loss=loss, step_ms=ms, step_ms_median=med(ms),
                       peak_GB=torch.cuda.max_memory_allocated() / 2 ** 30)
            print(f'general path {side}x{side} (N = {side * side}, nnz = {graph.nnz}) C={C} at {B} samples: forward + backward {med(ms):9.1f} ms, '
                  f'peak {row["peak_GB"]:.2f} GB, loss {loss:.4f}', flush=True)
            del model, X, Y, graph
        except torch.cuda.OutOfMemoryError as e:
            row = dict(section='largest_grid', grid=[side, side], N=side * side, fits=False, error=str(e)[:200])
            print(f'general path {side}x{side}: does not fit ({str(e)[:120]})', flush=True)
        rows.append(row)
        if not row['fits']:
            break
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20, help='calls per timed loop')
    ap.add_argument('--grids', type=int, nargs='+', default=[64, 128, 176, 224], help='sides of the queen grids of section 3')
    a = ap.parse_args()
    rows = []
    for section in (lambda: branch(32, 32, 8, 4, 9, 16, a, (False, True)),            # the synthetic grid of section 2: KH = 576
                    lambda: branch(100, 100, 5, 16, 9, 16, a, (False, True)),        # 10 000 nodes, the flagship's rows: KH = 2 304
                    lambda: branch(224, 224, 5, 16, 9, 16, a, (True,)),              # the flagship grid: the torch route's (nnz, KH) gathers are 3.7 GB each there
                    lambda: train_steps(a), lambda: largest_grid(a)):
        try:
            rows += section()
        except (RuntimeError, ValueError, TypeError, AttributeError, KeyError) as e:      # a section that fails is reported, the others still run
            if 'HIP error' in str(e) or 'illegal memory' in str(e):
                raise                                                    # never go on after a device fault
            print(f'section failed: {type(e).__name__}: {str(e)[:300]}', flush=True)
            rows.append(dict(section='failed', error=f'{type(e).__name__}: {str(e)[:300]}'))
    print(json.dumps(dict(probe='mgp_csr_ab', repeats=a.repeats, calls=a.calls, device=torch.cuda.get_device_name(0), rows=rows)), flush=True)


if __name__ == '__main__':
    main()
