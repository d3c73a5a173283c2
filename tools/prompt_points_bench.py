"""Choice of the prompt points of an automatic detection frame: `detections.forward_prompt_points` (csrc/prompts.hip:
three launches, one pinned copy of 8 P + 4 bytes, one event wait) against the reference's statement
(automatic_sam.py:69-82) in ATen on the same device, its boolean-index copy and `.cpu()` included.

    python tools/prompt_points_bench.py [--rounds 7] [--calls 200] [--out FILE.md]

Forward masks are those of tests/prompt_case.py at 1080 x 1920 and 480 x 854, int64 as `estimate_forward_mask` returns
them; grids of 32 and 64 points per side.  Both forms end with their points on the host, so a host clock around
`--calls` consecutive calls measures whole calls; the two forms run in alternating rounds on the same mask: median,
minimum and maximum of the per-call time over the rounds.  The first pass reads the mask once: its bytes over the fused
call's time is reported as what it is, a whole-call rate that includes two more launches, the copy and the wait."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import prompt_case as PC  # noqa: E402
from deva.inference import detections as D  # noqa: E402


def aten_points(forward_mask, n):
    """the reference's lines in ATen on the mask's device -> host fp32 [K,2]"""
    fg = (forward_mask > 0).float()[None, None]
    low = F.interpolate(fg, scale_factor=1 / 16, mode='bilinear', antialias=True)
    offset = 1 / (2 * n)
    side = torch.linspace(offset, 1 - offset, n, device=forward_mask.device)
    grid = torch.stack([side[None, :].repeat(n, 1), side[:, None].repeat(1, n)], dim=-1)[None]
    labels = F.grid_sample(low, grid * 2 - 1, align_corners=False).view(-1)
    return grid.view(-1, 2)[labels < 0.01].cpu().numpy()


def per_call_us(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()                                                        # (ends with its points on the host: synchronised)
    return (time.perf_counter() - t0) / calls * 1e6


def spread(ts):
    return f'{statistics.median(ts):.1f} (min {min(ts):.1f}, max {max(ts):.1f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('prompt_points_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    lines = [f'{torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds of {args.calls} calls, microseconds per call, '
             'median (min, max)', '',
             '| mask | points | kept | fused call | ATen call | ratio | mask bytes / fused call | same points |',
             '|---|---|---|---|---|---|---|---|']
    for (h, w), seed in (((1080, 1920), 3), ((480, 854), 4)):
        mask = PC.forward_mask(h, w, seed).to(dev)
        for n in (32, 64):
            fused = lambda: D.forward_prompt_points(mask, n)        # noqa: E731
            aten = lambda: aten_points(mask, n)                     # noqa: E731
            a, b = fused(), aten()                                  # warm-up of both, and the results side by side
            same = a.shape == b.shape and bool(np.array_equal(a, b))
            t_fused, t_aten = [], []
            for _ in range(args.rounds):
                t_fused.append(per_call_us(fused, args.calls))
                t_aten.append(per_call_us(aten, args.calls))
            f, r = statistics.median(t_fused), statistics.median(t_aten)
            lines.append(f'| {h} x {w} int64 | {n * n} | {len(a)} | {spread(t_fused)} | {spread(t_aten)} | {r / f:.1f}x | '
                         f'{h * w * 8 / f / 1e3:.0f} GB/s | {"yes" if same else f"NO ({len(a)} / {len(b)})"} |')
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
