"""Probe: stc_graph_grad_f32, tile per wave (form 1) against blocked (form 2), launch alone into a preallocated partial buffer.

    python tools/probes/graph_grad_forms.py [--out FILE] [--repeats 3]

768 planes (24 cells x batch 32) of N x F, N in {64, 100, 128, 196, 256, 300}, F = 256 (C = 8) and 160 (C = 5), at 256 chunks (the rule of samples
up to SMALL_STAGED_ROWS rows) and at ``HipKernels.graph_grad_chunks``.  Warm: back-to-back launches between two device events; cold: one launch
at a time after a 512 MB write that evicts the operands from L2 and the Infinity Cache.  The forms alternate inside every repeat; per
configuration the median of the repeats and their spread (max - min) are printed, and the bits of the two forms' partials are compared.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'stc-gnn_amd')]

import torch  # noqa: E402
from stc_hip._lib import HipKernels  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    hip, dev = HipKernels(), torch.device('cuda')
    cells, batch, w = 24, 32, 32
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    rows = []
    for C in (8, 5):
        for N in (64, 100, 128, 196, 256, 300):
            g = torch.Generator(device=dev).manual_seed(N + C)
            A, Bm = (torch.randn(cells, batch, N * C, w, generator=g, device=dev) for _ in range(2))
            for chunks in sorted({256, hip.graph_grad_chunks(cells * batch, N, N * C, dev)}):
                part = {f: torch.empty(chunks, N * N, dtype=torch.float64, device=dev) for f in (1, 2)}

                def launch(form):
                    hip.graph_grad(A, Bm, 0, 1, cells, N, into=(part[form], 0))

                def timed(form, cold):
                    hip.set_graph_grad_form(form)
                    launch(form)
                    n = 5 if cold else args.iters
                    total = 0.0
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    if not cold:
                        ev[0].record()
                        for _ in range(n):
                            launch(form)
                        ev[1].record()
                        torch.cuda.synchronize()
                        return ev[0].elapsed_time(ev[1]) * 1e3 / n
                    for _ in range(n):
                        flush.fill_(1)
                        ev[0].record()
                        launch(form)
                        ev[1].record()
                        torch.cuda.synchronize()
                        total += ev[0].elapsed_time(ev[1]) * 1e3
                    return total / n

                t = {(f, c): [] for f in (1, 2) for c in (False, True)}
                for _ in range(args.repeats):
                    for cold in (False, True):
                        for f in (1, 2):
                            t[f, cold].append(timed(f, cold))
                hip.set_graph_grad_form(0)
                row = dict(N=N, F=C * w, planes=cells * batch, chunks=chunks, same_bits=bool(torch.equal(part[1], part[2])))
                for (f, cold), v in t.items():
                    row[f'form{f}_{"cold" if cold else "warm"}_us'] = round(statistics.median(v), 1)
                    row[f'form{f}_{"cold" if cold else "warm"}_spread_us'] = round(max(v) - min(v), 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del A, Bm
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(json.dumps(r) for r in rows) + '\n')


if __name__ == '__main__':
    main()
