"""The overlap of D x G COCO run-length masks: `deva.hip.rle.intersections` (csrc/rle_overlap/rle_overlap.hip) against what
a user has without it.

    python tools/rle_overlap_bench.py [--rounds 7] [--shape 0|1] [--out FILE.md]

Workload: blob masks (tests/overlap_case.py `small_blobs`: a few discs and holes in a window of the mask's own) as
compressed COCO strings, 64 x 64 of them at 1080 x 1920 and 20 x 5 at 480 x 854.  Every timing of a whole call is a host
clock around the call and a device synchronise, after a warm-up, in alternating rounds: median, minimum and maximum.

  intersections  the whole call: both sides parsed and checked on the host, their run arrays and boxes built, two uploads,
                 two launches.  The tables stay on the device.
  (a) ATen       `rle.decode` of both sides to float32 planes, then the plane product `dt @ gt.T` on the device (exact:
                 every partial sum is an integer below 2^24).
  (b) pairs      `rle.decode` of both sides, the masks of a side laid into one label plane (ATen; where masks of one side
                 overlap the later one wins, so this route answers for disjoint masks only and is not compared), then
                 `pair_metrics.pair_counts`, which also matches boundaries: it is the only device route there was.
  (c) numpy      tests/overlap_case.py `statement` on the host: planes from the counts, the product in 2^18-pixel pieces.
  kernels alone  ten calls of `deva_overlap_intersections` (the scan and the pair pass) queued behind a delay kernel
                 between two device events, so that no host time lies between them: per call.  Each launch's own time is
                 read from a kernel trace of this tool (`rocprofv3 --kernel-trace --stats -- python tools/rle_overlap_bench.py
                 --rounds 1 --shape 0`); the events cannot separate two launches of one call."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import overlap_case as OC  # noqa: E402
from deva.hip import pair_metrics, rle, rle_overlap  # noqa: E402
from deva.inference.frame_results import coco_strings  # noqa: E402

QUEUED = 10
SHAPES = ((1080, 1920, 64, 64, 150), (480, 854, 20, 5, 60))     # H, W, D, G, the blobs' radius


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ts):
    return f'{statistics.median(ts):.3f} (min {min(ts):.3f}, max {max(ts):.3f})'


def as_strings(all_counts, h, w):
    texts = coco_strings(np.concatenate([np.asarray(c, dtype=np.int64) for c in all_counts]), [len(c) for c in all_counts])
    return [{'size': [h, w], 'counts': t} for t in texts]


def aten_route(dt, gt):
    a, b = rle.decode(dt, dtype=torch.float32), rle.decode(gt, dtype=torch.float32)
    a, b = a.flatten(1), b.flatten(1)
    return (a @ b.T).to(torch.int32), a.sum(1).to(torch.int32), b.sum(1).to(torch.int32)


def pairs_route(dt, gt):
    planes = []
    for side in (gt, dt):
        stack = rle.decode(side, dtype=torch.uint8).to(torch.int32)
        ids = torch.arange(1, stack.shape[0] + 1, dtype=torch.int32, device=stack.device).view(-1, 1, 1)
        planes.append((stack * ids).amax(0).contiguous())
    return pair_metrics.pair_counts(planes[0], planes[1], list(range(1, len(gt) + 1)), list(range(1, len(dt) + 1)))


def kernels_alone(dt, gt, h, w, dev, sleep_cycles):
    """-> ms per call of the library (both launches)"""
    parsed = [rle.parse_checked(side, (h, w)) for side in (dt, gt)]
    sides = [rle_overlap._side(p, 0, int(p.per_mask.size), k, True) for k, p in enumerate(parsed)]
    sides = [s._replace(device=s.host.to(dev)) for s in sides]
    scratch = torch.empty(sides[1].words - sides[1].n - 1, dtype=torch.int32, device=dev)
    inter = torch.empty((sides[0].n, sides[1].n), dtype=torch.int32, device=dev)
    area_d, area_g = torch.empty(sides[0].n, dtype=torch.int32, device=dev), torch.empty(sides[1].n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda._sleep(sleep_cycles)
    start.record()
    for _ in range(QUEUED):
        rle_overlap._launch(sides[0], sides[1], h, w, scratch, inter, area_d, area_g, stream)
    stop.record()
    if start.query():
        raise RuntimeError('kernels_alone: the delay was over before the launches were queued; the timing would hold host time')
    stop.synchronize()
    return start.elapsed_time(stop) / QUEUED, sides


def shape_rows(h, w, n_d, n_g, radius, rounds, dev, sleep_cycles):
    counts_d, counts_g = OC.small_blobs(h, w, n_d, seed=1, radius=radius), OC.small_blobs(h, w, n_g, seed=2, radius=radius)
    dt, gt = as_strings(counts_d, h, w), as_strings(counts_g, h, w)
    got = [t.cpu().numpy() for t in rle.intersections(dt, gt)]                       # warm-up, and the comparison of the routes
    aten = [t.cpu().numpy() for t in aten_route(dt, gt)]
    t_numpy, want = [], None
    for _ in range(min(rounds, 2)):
        t0 = time.perf_counter()
        want = OC.statement(counts_d, counts_g, h, w, direct=False)
        t_numpy.append((time.perf_counter() - t0) * 1e3)
    equal = all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(got, aten, want))
    pairs_route(dt, gt)
    t_ours, t_aten, t_pairs, t_kernels = [], [], [], []
    for _ in range(rounds):
        t_ours.append(wall(lambda: rle.intersections(dt, gt))[0])
        t_aten.append(wall(lambda: aten_route(dt, gt))[0])
        t_pairs.append(wall(lambda: pairs_route(dt, gt))[0])
        t_kernels.append(kernels_alone(dt, gt, h, w, dev, sleep_cycles)[0])
    runs = sum(len(c) for c in counts_d) + sum(len(c) for c in counts_g)
    tag = f'{h} x {w}, {n_d} x {n_g}'
    ours = statistics.median(t_ours)
    return [f'| {tag}: `rle.intersections`, {runs} runs in all, {int(np.count_nonzero(want[0]))} of {n_d * n_g} pairs overlap | {spread(t_ours)} |',
            f'| {tag}: (a) `rle.decode` of both sides + the plane product in ATen | {spread(t_aten)}: {statistics.median(t_aten) / ours:.1f}x |',
            f'| {tag}: (b) `rle.decode` + label planes + `pair_metrics.pair_counts` (disjoint masks only; boundaries too) | {spread(t_pairs)}: '
            f'{statistics.median(t_pairs) / ours:.1f}x |',
            f'| {tag}: (c) the numpy statement on the host | {spread(t_numpy)}: {statistics.median(t_numpy) / ours:.1f}x |',
            f'| {tag}: same integers from `intersections`, (a) and (c) | {"yes" if equal else "NO"} |',
            f'| {tag}: `deva_overlap_intersections` alone (scan + pair pass), per call | {spread(t_kernels)} |']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--shape', type=int, default=None, help='0 or 1: that row of SHAPES alone (for a kernel trace of one shape)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('rle_overlap_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    # ~40 ms of delay: the host enqueues ten calls well inside it
    torch.cuda._sleep(1000000)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(20000000)
    b.record()
    b.synchronize()
    sleep_cycles = int(20000000 / a.elapsed_time(b) * 40)
    lines = [f'{torch.cuda.get_device_name(0)}; blob masks as compressed COCO strings; {args.rounds} alternating rounds', '',
             '| | ms, median (min, max) |', '|---|---|']
    for h, w, n_d, n_g, radius in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        lines += shape_rows(h, w, n_d, n_g, radius, args.rounds, dev, sleep_cycles)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
