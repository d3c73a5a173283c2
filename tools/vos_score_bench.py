"""The DAVIS counts of a scored frame: `vos_metrics.boundary_counts` (csrc/vos_metrics/boundary_counts.hip, two launches,
seven integers per object) and a whole `VideoObjectScorer.add_frame`, against the two statements a user would otherwise
run for the same records: ATen on the device (one boolean plane per object, the boundary map by slicing, a `conv2d` with
the disk as kernel compared with 0) and numpy on the host (tests/vos_case.py: the per-object statement of the public
toolkits).  Neither baseline is the code under test.

    python tools/vos_score_bench.py [--rounds 7] [--calls 50] [--out FILE.md]

480 x 854 with 3 objects (radius 8) and 1080 x 1920 with 10 objects (radius 18); uint8 ground truth and the int16 channel
plane, the scorer's own forms.  Device forms: device events around `--calls` consecutive calls, the forms in alternating
rounds on the same tensors; median, minimum and maximum over the rounds.  The host form: a host clock.  The least traffic
of the pass over the planes is what it must move: the two planes in (1 + 2 bytes a pixel) and the two word planes out
(16 bytes a pixel); the disk search reads those 16 bytes once more and then only around boundary pixels.  `add_frame` is
timed with a host clock around `--calls` frames and one wait for the last records (it does not synchronise itself).
The kernels' own times come from a kernel trace of a run of this script (`--rounds 2 --calls 20`)."""
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

import vos_case as VC  # noqa: E402
from deva.hip import vos_metrics  # noqa: E402
from deva.inference.vos_quality import VideoObjectScorer  # noqa: E402

ROOF = 8e12
SHAPES = ((480, 854, 3), (1080, 1920, 10))


def spread(ts, digits=1):
    return f'{statistics.median(ts):.{digits}f} (min {min(ts):.{digits}f}, max {max(ts):.{digits}f})'


def event_us(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls * 1e3


class _Result:
    def __init__(self, index, channel_ids):
        self.index, self.channel_ids = index, channel_ids


def aten_counts(gt, pred, ids, disk):
    """the per-object statement in ATen -> int64 [n,7]"""
    g = gt.unsqueeze(0) == ids.view(-1, 1, 1)
    p = pred.unsqueeze(0) == ids.view(-1, 1, 1)

    def bmap(s):
        b = torch.zeros_like(s)
        b[:, :, :-1] |= s[:, :, :-1] ^ s[:, :, 1:]
        b[:, :-1, :] |= s[:, :-1, :] ^ s[:, 1:, :]
        b[:, :-1, :-1] |= s[:, :-1, :-1] ^ s[:, 1:, 1:]
        return b

    def dilated(b):
        r = disk.shape[-1] // 2
        return F.conv2d(b.unsqueeze(1).float(), disk, padding=r)[:, 0] > 0
    bg, bp = bmap(g), bmap(p)
    fields = ((g & p), g, p, bg, bp, bg & dilated(bp), bp & dilated(bg))
    return torch.stack([f.sum(dim=(1, 2)) for f in fields], dim=1)


def table(args, dev, h, w, n):
    gt, pred, ids = VC.case(h, w, n, 5)
    pred = np.where(np.isin(pred, ids), pred, 0)              # a tracker's output holds only its own ids
    radius = vos_metrics.boundary_radius(h, w)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    channel_ids = np.concatenate([[0], ids])
    index = (np.searchsorted(ids, pred) + 1) * (pred != 0)
    lut = np.concatenate([[65535], np.arange(n)]).astype(np.uint16)
    gt_d, index_d, lut_d, ids_d = up(gt.astype(np.uint8)), up(index.astype(np.int16)), up(lut), up(ids.astype(np.int32))
    gt64, pred64, ids64 = up(gt), up(pred), up(ids)
    scratch = torch.empty(vos_metrics.boundary_scratch_bytes(h, w), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 8), dtype=torch.uint32, device=dev)
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    disk = up((yy * yy + xx * xx <= radius * radius).astype(np.float32))[None, None]

    fast = lambda: vos_metrics.boundary_counts(gt_d, index_d, ids_d, radius=radius, pred_lut=lut_d, scratch=scratch, out=out,  # noqa: E731
                                               validate=False)
    aten = lambda: aten_counts(gt64, pred64, ids64, disk)     # noqa: E731
    host = lambda: VC.counts(gt, pred, ids, radius)           # noqa: E731

    want = host()
    same = np.array_equal(fast().cpu().numpy(), want) and np.array_equal(aten().cpu().numpy(), want[:, :7].astype(np.int64))
    boundary = int(want[:, 3].sum() + want[:, 4].sum())

    scorer = VideoObjectScorer()
    result = _Result(index_d, channel_ids)

    def add_frames(calls):
        scorer.start_video('bench', ids.tolist())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            scorer.add_frame(result, gt_d)
        enqueue = (time.perf_counter() - t0) / calls * 1e6
        scorer._frames[-1].event.synchronize()
        total = (time.perf_counter() - t0) / calls * 1e6
        scorer._frames = None
        return enqueue, total

    t = {k: [] for k in ('fast', 'aten', 'host', 'enqueue', 'add')}
    for fn in (fast, aten):
        event_us(fn, 3)                                          # warm-up of every form
    add_frames(3)
    for _ in range(args.rounds):
        t['fast'].append(event_us(fast, args.calls))
        t['aten'].append(event_us(aten, max(args.calls // 10, 2)))
        e, a = add_frames(args.calls)
        t['enqueue'].append(e)
        t['add'].append(a)
    for _ in range(min(args.rounds, 3)):
        t0 = time.perf_counter()
        host()
        t['host'].append((time.perf_counter() - t0) * 1e6)
    px = h * w
    f = statistics.median(t['fast'])
    plan = vos_metrics.boundary_plan(h, w, n, radius)
    least = (1 + 2 + 16) * px
    return [f'{h} x {w}, {n} objects, radius {radius} ({plan.label_grid} + {plan.match_grid} workgroups of {plan.block}, '
            f'{plan.lds_bytes} B of LDS, {boundary} boundary pixels on the two sides); {args.rounds} alternating rounds of '
            f'{args.calls} calls, microseconds per call, median (min, max); all forms give the same records: '
            f'{"yes" if same else "NO"}', '',
            '| form | per call | least traffic of the pass over the planes | rate | of the 8 TB/s roof |', '|---|---|---|---|---|',
            f'| boundary_counts, uint8 + channel plane | {spread(t["fast"])} | {least / 1e6:.1f} MB (1 + 2 in, 16 out B / pixel) | '
            f'{least / f / 1e3:.0f} GB/s | {least / f * 1e6 / ROOF:.3f} |',
            f'| add_frame, whole (host clock, records on the host) | {spread(t["add"])} | | | |',
            f'| add_frame, until it returns (host clock) | {spread(t["enqueue"])} | | | |',
            f'| ATen one-hot planes + conv2d with the disk on the device | {spread(t["aten"])} | | | |',
            f'| numpy statement on the host | {spread(t["host"], 0)} | | | |',
            f'| ratios to boundary_counts | ATen {statistics.median(t["aten"]) / f:.0f}x, numpy {statistics.median(t["host"]) / f:.0f}x | | | |',
            '']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('vos_score_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    lines = [torch.cuda.get_device_name(0), '']
    for h, w, n in SHAPES:
        lines += table(args, dev, h, w, n)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
