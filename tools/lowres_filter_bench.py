"""The proposal filter and the best-mask choice from low-resolution logits (`ProposalFilter.add_lowres`,
`lowres.select_masks`, csrc/lowres/lowres.hip) against the route they replace, in one process on the same inputs.

    python tools/lowres_filter_bench.py [--rounds 5] [--batches 16] [--batch 192] [--out FILE.md]

A frame is `--batches` batches of `--batch` low-resolution planes (256 x 256, the generator of tests/lowres_case.py made
steep enough that planes pass the stability drop; four distinct batches, cycled), at 1080 x 1920 and at 480 x 854.
  full   the route before: ATen's two `F.interpolate` calls on the device (256 -> 1024, crop, -> the frame), then
         `flt.add` on the frame-sized fp32 planes
  lowres `flt.add_lowres` on the low-resolution planes
Both end with the same `flt.finish()`.  The text-prompted side is 16 boxes x 3 candidates: the two interpolations and
`ops.box_mask_select` against `lowres.select_masks`.  Alternating rounds, device events around each side, median, minimum
and maximum over the rounds.  The kernels alone -- the batch passes without `finish`, and the materialising kernel -- are
timed the same way and set against what they must do: the pixels they evaluate (live planes once, stored planes twice),
the lane-operations that takes (`LANE_OPS` per pixel, counted in the tile path's inner loop) against the fp32 vector
rate, and the bytes they must move (256 KB read per evaluated plane, one byte written per stored pixel) against HBM."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import lowres_case as LC  # noqa: E402
from deva.hip import lowres, ops  # noqa: E402
from deva.inference.proposals import ProposalFilter  # noqa: E402

HBM = 8e12            # bytes / s
VALU = 256 * 64 * 2.4e9   # fp32 lane-operations / s: 256 CUs x 4 SIMDs x 16 lanes, one operation per lane and clock at 2.4 GHz
LANE_OPS = 64         # vector operations per output pixel of the tile path: 1129 vector instructions in the binarise kernel, 16 pixels a step
LOW, M = (256, 256), 1024
SIZES = [(1080, 1920), (480, 854)]


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def spread(ts):
    return f'{statistics.median(ts):.2f} (min {min(ts):.2f}, max {max(ts):.2f})'


def alternate(rounds, **sides):
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            times[k].append(timed(fn)[0])
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', type=int, default=16)
    ap.add_argument('--batch', type=int, default=192)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lowres_filter_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    distinct = []
    for seed in range(4):
        low = torch.from_numpy(LC.smooth_logits(seed, args.batch, LOW, scale=60.0)).to(dev)
        iou = torch.from_numpy(np.random.default_rng(seed).uniform(0.80, 1.0, args.batch).astype(np.float32)).to(dev)
        distinct.append((low, iou))
    batches = [distinct[i % 4] for i in range(args.batches)]
    lines = ['| size | what | full route, ms | low-resolution route, ms | ratio |', '|---|---|---|---|---|']
    notes = []
    for size in SIZES:
        input_size = lowres.sam_input_size(*size, M)
        flt = ProposalFilter(*size, capacity=4096)

        def full_batches():
            flt.reset()
            for low, iou in batches:
                flt.add(LC.aten_chain(low, M, input_size, size).contiguous(), iou)

        def lowres_batches():
            flt.reset()
            for low, iou in batches:
                flt.add_lowres(low, iou, input_size, model_size=M)

        def frame(fill):
            fill()
            return flt.finish()

        _, a = timed(lambda: frame(full_batches))                    # warm-up of both, and the results side by side
        _, b = timed(lambda: frame(lowres_batches))
        stored = int(flt._state.host[1])
        live = sum(int((iou > 0.88).sum()) for _, iou in batches)
        agree = float((a.masks == b.masks).float().mean()) if a.masks.shape == b.masks.shape else float('nan')
        t = alternate(args.rounds, full=lambda: frame(full_batches), lowres=lambda: frame(lowres_batches))
        k = alternate(args.rounds, full=full_batches, lowres=lowres_batches)
        out = torch.empty((args.batch,) + size, device=dev)
        u = alternate(args.rounds, full=lambda: LC.aten_chain(distinct[0][0], M, input_size, size),
                      lowres=lambda: lowres.upsample_logits(distinct[0][0], input_size, size, model_size=M, out=out))
        tag = f'{size[0]} x {size[1]}'
        for what, tt in ((f'frame: {args.batches} x {args.batch} planes, finish included', t), ('the batch passes alone', k),
                         (f'{args.batch} planes materialised (ATen: two interpolations)', u)):
            med = {s: statistics.median(v) for s, v in tt.items()}
            lines.append(f'| {tag} | {what} | {spread(tt["full"])} | {spread(tt["lowres"])} | {med["full"] / med["lowres"]:.2f}x |')
        pixels = (live + stored) * size[0] * size[1]
        ms = statistics.median(k['lowres'])
        moved = (live + stored) * LOW[0] * LOW[1] * 4 + stored * size[0] * size[1]
        notes.append(f'- {tag}: {live} live and {stored} stored planes of {args.batches * args.batch}, {b.masks.shape[0]} kept; the kept planes of '
                     f'both routes have the same shape: {a.masks.shape == b.masks.shape}, equal bytes: {agree:.6f}.  The batch passes evaluate '
                     f'{pixels / 1e9:.2f} G pixels in {ms:.2f} ms = {pixels / ms / 1e6:.0f} G pixels/s; at {LANE_OPS} lane-operations a pixel that '
                     f'is {100 * pixels * LANE_OPS / (ms * 1e-3) / VALU:.0f} % of the fp32 vector rate; they must move {moved / 1e6:.0f} MB '
                     f'= {100 * moved / (ms * 1e-3) / HBM:.1f} % of HBM in that time (the full route moves at least '
                     f'{(args.batches * args.batch * 12 + live * 4 + stored * 5) * size[0] * size[1] / 1e9:.1f} GB).')
        # the text-prompted side: 16 boxes x 3 candidates
        cand = distinct[0][0][:48].view(16, 3, *LOW).contiguous()
        scores = distinct[0][1][:48].view(16, 3).contiguous()
        planes = torch.empty((16,) + size, dtype=torch.uint8, device=dev)

        def full_select():
            logits = LC.aten_chain(cand.view(48, *LOW), M, input_size, size).view(16, 3, *size)
            return ops.box_mask_select(logits, scores, 0.0, out=planes)

        s = alternate(args.rounds, full=full_select,
                      lowres=lambda: lowres.select_masks(cand, scores, input_size, size, model_size=M, out=planes))
        med = {side: statistics.median(v) for side, v in s.items()}
        lines.append(f'| {tag} | 16 boxes x 3 candidates to byte planes | {spread(s["full"])} | {spread(s["lowres"])} | '
                     f'{med["full"] / med["lowres"]:.2f}x |')
        del flt, out, planes
        torch.cuda.empty_cache()
    text = '\n'.join(lines + [''] + notes) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
