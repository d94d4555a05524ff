"""One-process measurements of ``graph_mode='csr-learned'`` (``csrc/stc_mgp_csr.hip``, ``stc_hip.learned``):

1. the spatial branch of the generator alone (``learned.mgp_csr_front``: U / V, score, softmax), forward + backward, the HIP kernels against the
   torch route (``learned.csr._FUSED = False``), eager and as HIP-graph replays, with the GPU launches of one call (torch.profiler's device-side
   events) and the C entry points launched;
2. a whole train step (forward, ComboLoss, backward, Adam) on the synthetic 32 x 32 grid with 8 categories (N = 1 024), ``csr-learned`` at rank 16
   against ``dense-learned`` at rank 16, eager;
3. one forward + backward of the ``csr-learned`` model at 2 samples on growing queen grids up to 224 x 224 (the general per-cell path), with the
   step time and the peak of torch's allocator: the largest grid that fits.

With ``--cells per-cell fused`` it runs these INSTEAD (``STCGNN(csr_cells=...)``: one autograd node per cell against the few-category cell
executor with the value gradient sampled at the stored entries, ``stc_graph_grad_csr_f32``):

4. the whole train step of the ``csr-learned`` trainer, the named routes alternating in one process, eager and as HIP-graph replays, at
   ``-synthetic 32 32 8`` (batch 8), 64 x 64 x 8 and 90 x 90 x 8 (2 samples; 64 800 rows per sample: the largest the cell kernels take), with the C
   entry points and GPU launches of a step and the allocator's peak;
5. ``stc_graph_grad_csr_f32`` alone against ``stc_csr_sddmm_f32`` on the same stacked operands, one (planes, N, F) call each: the planes of the
   16-column cells of such a step (15 cells x batch, F = 8 x 32).

Prints one line per measurement, then one JSON line with everything.  No time here is a pass / fail number.

    python tools/probes/mgp_csr_ab.py [--repeats 3] [--calls 20] [--grids 64 128 176 224] [--cells per-cell fused]"""
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


CELL_SHAPES = ((32, 32, 8, 8), (64, 64, 8, 2), (90, 90, 8, 2))          # H, W, C, batch


def cells_ab(a):
    """Section 4: the whole train step per route of ``a.cells``, alternating."""
    from stc_hip import _lib
    rows = []
    for H, W, C, B in CELL_SHAPES:
        base = dict(device='cuda:0', H=H, W=W, C=C, batch_size=B, obs_len=9, pred_len=3, split_ratio=[6, 1, 1], model='STC-GNN', cheby_order=2, hidden_dim=16,
                    nn_layers=2, learn_rate=2e-3, decay_rate=1e-4, num_epochs=1, time_slice=4, city='SYN', fusion_rank=16, output_dir=tempfile.mkdtemp(prefix='mgp_csr_ab_'))
        data = sdata.synthetic_incidents(H, W, C, 60, sparse_graph=True)
        loaders = sdata.get_data_loader(base, data, base['obs_len'], base['pred_len'], base['split_ratio'])
        x, y = (t.cuda() for t in next(iter(loaders['train'])))
        trainers, info = {}, {}
        for route in a.cells:
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            torch.manual_seed(0)
            t = trainers[route] = Trainer(dict(base, csr_cells=route), data, graph_mode='csr-learned', hip_graph=True)
            t.model.train()
            for _ in range(2):
                loss = float(t._step(x, y))
            names = entry_points(lambda: t._step(x, y))
            launches = gpu_launches(lambda: t._step(x, y))
            eager_peak = (torch.cuda.max_memory_allocated() - before) / 2 ** 30
            for _ in range(3):                                        # two warm-up steps on the capture stream, then the capture
                t._graphed_step(x, y)
            replay_launches = gpu_launches(lambda: t._graphed_step(x, y))
            info[route] = dict(loss=loss, entry_points=len(names), cell_launches=sum(n.startswith('stc_cell_small') for n in names),
                               sddmm=names.count('stc_csr_sddmm_f32'), graph_grad_csr=names.count('stc_graph_grad_csr_f32'), gpu_launches=launches,
                               replay_gpu_launches=replay_launches, eager_peak_GB=eager_peak)
        eager, replay = {r: [] for r in a.cells}, {r: [] for r in a.cells}
        calls = max(2, a.calls // 4)
        for _ in range(a.repeats):                                    # the routes alternate: clock and cache drift hit both alike
            for route, t in trainers.items():
                eager[route] += [u / 1e3 for u in timed(lambda: t._step(x, y), calls, 1)]
                replay[route] += [u / 1e3 for u in timed(lambda: t._graphed_step(x, y), calls, 1)]
        for route in a.cells:
            row = dict(section='cells_ab', grid=[H, W], N=H * W, C=C, batch=B, rows_per_sample=H * W * C, route=route, eager_ms=eager[route],
                       eager_ms_median=med(eager[route]), replay_ms=replay[route], replay_ms_median=med(replay[route]), **info[route])
            rows.append(row)
            print(f'train step {H}x{W}x{C} batch {B} {route:8s}: eager {med(eager[route]):8.2f} ms (spread {max(eager[route]) - min(eager[route]):.2f}), replay '
                  f'{med(replay[route]):8.2f} ms (spread {max(replay[route]) - min(replay[route]):.2f}); {info[route]["entry_points"]} entry points '
                  f'({info[route]["cell_launches"]} cell, {info[route]["sddmm"]} sddmm, {info[route]["graph_grad_csr"]} graph_grad_csr), {info[route]["gpu_launches"]} GPU '
                  f'launches eager, {info[route]["replay_gpu_launches"]} replayed; peak {info[route]["eager_peak_GB"]:.2f} GB eager; loss {info[route]["loss"]:.4f}', flush=True)
        del trainers, loaders, data
        torch.cuda.empty_cache()
    return rows


def sampled_kernel_ab(a):
    """Section 5: the sampled graph product, new kernel against one stc_csr_sddmm_f32 call over the same planes."""
    rows, k, dev = [], ops.kernels(), torch.device('cuda')
    for H, W, C, B in CELL_SHAPES:
        graph = CsrGraph.queen_grid(H, W, normalize=True)
        d, N, cells, w = graph.on(dev), H * W, 15, 32
        torch.manual_seed(H)
        A, Bm = (torch.randn(cells, B, N * C, w, device=dev) for _ in range(2))
        out = torch.zeros(graph.nnz, device=dev)
        new = lambda: k.graph_grad_csr(d['fwd_rowptr'], d['fwd_colidx'], A, Bm, 0, 1, cells, N)
        old = lambda: k.csr_sddmm(d['fwd_rowptr'], d['fwd_colidx'], N, N, A.view(cells * B, N, C * w), Bm.view(cells * B, N, C * w), out, 1.0, False)
        got = new()
        old()
        err = float((got - out.double()).abs().max() / got.abs().max())
        t_new, t_old = [], []
        for _ in range(a.repeats):
            t_new += timed(new, a.calls, 1)
            t_old += timed(old, a.calls, 1)
        chunks = k.graph_grad_csr_chunks(cells * B, N, graph.nnz)
        rows.append(dict(section='sampled_kernel', grid=[H, W], N=N, nnz=graph.nnz, planes=cells * B, F=C * w, chunks=chunks, graph_grad_csr_us=t_new,
                         graph_grad_csr_us_median=med(t_new), sddmm_us=t_old, sddmm_us_median=med(t_old), difference=err))
        print(f'sampled product {H}x{W} nnz={graph.nnz} planes={cells * B} F={C * w}: graph_grad_csr ({chunks} chunks, + its sum) {med(t_new):8.1f} us (spread '
              f'{max(t_new) - min(t_new):.1f}), csr_sddmm {med(t_old):8.1f} us (spread {max(t_old) - min(t_old):.1f}); they differ by {err:.1e}', flush=True)
        del A, Bm
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--cells', nargs='+', choices=['per-cell', 'fused'], default=None, help='sections 4 and 5 instead: the train step on these cell routes, alternating')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20, help='calls per timed loop')
    ap.add_argument('--grids', type=int, nargs='+', default=[64, 128, 176, 224], help='sides of the queen grids of section 3')
    a = ap.parse_args()
    rows = []
    sections = (lambda: branch(32, 32, 8, 4, 9, 16, a, (False, True)),                # the synthetic grid of section 2: KH = 576
                lambda: branch(100, 100, 5, 16, 9, 16, a, (False, True)),            # 10 000 nodes, the flagship's rows: KH = 2 304
                lambda: branch(224, 224, 5, 16, 9, 16, a, (True,)),                  # the flagship grid: the torch route's (nnz, KH) gathers are 3.7 GB each there
                lambda: train_steps(a), lambda: largest_grid(a))
    if a.cells:
        sections = (lambda: cells_ab(a), lambda: sampled_kernel_ab(a))
    for section in sections:
        try:
            rows += section()
        except (RuntimeError, ValueError, TypeError, AttributeError, KeyError) as e:      # a section that fails is reported, the others still run
            if 'HIP error' in str(e) or 'illegal memory' in str(e):
                raise                                                    # never go on after a device fault
            print(f'section failed: {type(e).__name__}: {str(e)[:300]}', flush=True)
            rows.append(dict(section='failed', error=f'{type(e).__name__}: {str(e)[:300]}'))
    print(json.dumps(dict(probe='mgp_csr_ab', repeats=a.repeats, calls=a.calls, cells=a.cells, device=torch.cuda.get_device_name(0), rows=rows)), flush=True)


if __name__ == '__main__':
    main()
