"""Time one memory read with top_k=None (ops.dense_read: full softmax + read-out) beside the top-k read (ops.affinity_topk
+ one ops.readout_sparse per object) on the same bank and queries: (10 000, 8 160) with 1 and 5 objects, (50 000,
32 400) with 1 object.  Prints one JSON line per shape (milliseconds, median of --iters after --warmup).

    python tools/dense_read_bench.py [--iters 5] [--warmup 2] [--top_k 30]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd')]

import torch  # noqa: E402

from deva.hip import ops  # noqa: E402
from workload import synth  # noqa: E402

SHAPES = ((10000, 8160, 1), (10000, 8160, 5), (50000, 32400, 1))


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--top_k', type=int, default=30)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    for n, hw, nobj in SHAPES:
        mk, ms, qk, qe = synth.affinity_inputs(n, hw, seed=1)
        n_long = n // 5  # a long-term segment in front of the working memory, as in a running clip
        rows = mk.t().contiguous().to(dev)
        shr = ms.reshape(-1).contiguous().to(dev)
        kl, sl, kw, sw = rows[:n_long].contiguous(), shr[:n_long].contiguous(), rows[n_long:].contiguous(), shr[n_long:].contiguous()
        vals = torch.randn(nobj, n, 512, device=dev)
        vl = [v[:n_long].contiguous() for v in vals]
        vw = [v[n_long:].contiguous() for v in vals]
        qkd, qed = qk.to(dev), qe.to(dev)
        out = torch.empty((nobj, 512, hw), device=dev)
        fix = torch.zeros(n, dtype=torch.int64, device=dev)
        del mk, qk, qe, vals

        def dense():
            ops.dense_read(kl, sl, n_long, kw, sw, n - n_long, qkd, qed, vl, vw, out, fix)

        def topk():
            idx, w = ops.affinity_topk(kl, sl, n_long, kw, sw, n - n_long, qkd, qed, args.top_k, fix)
            for o in range(nobj):
                ops.readout_sparse(idx, w, vl[o], n_long, vw[o], out[o])

        t_dense = _time(dense, args.iters, args.warmup)
        t_topk = _time(topk, args.iters, args.warmup)
        gflop_scores = 2 * 4 * 64 * n * hw / 1e9
        gflop_readout = 2 * 512 * n * hw * nobj / 1e9
        print(json.dumps({'n': n, 'hw': hw, 'objects': nobj, 'dense_ms': round(t_dense, 3), 'top_k': args.top_k,
                          'topk_ms': round(t_topk, 3), 'dense_gflop': round(gflop_scores + gflop_readout, 1),
                          'dense_tflops': round((gflop_scores + gflop_readout) / t_dense, 1)}), flush=True)
        del kl, sl, kw, sw, vl, vw, out, fix, rows, shr, qkd, qed
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
