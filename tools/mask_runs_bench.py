"""Mask planes on the device to COCO run lengths: `deva.hip.mask_runs.encode` (csrc/mask_runs/mask_runs.hip) against
what a user has without it.

    python tools/mask_runs_bench.py [--rounds 7] [--masks 64] [--out FILE.md]

Workload: `--masks` planes of seeded blobs with holes and specks (tests/rle_case.py `blobs`: eight distinct ones, cycled) at
1080 x 1920 and 480 x 854, as uint8 planes and as float32 logits (+-4 around a threshold of 0).  Every timing of a whole
call is a host clock around the call and a device synchronise, after a warm-up, in alternating rounds: median, minimum
and maximum.

  encode        the whole call: the count pass and its scans, the 8-byte read of the total, the write pass, the copies
                of `n` and `bounds` to pinned memory, the counts and strings on the host.
  host route    `planes.cpu()`, `rle_case.counts_of` per plane (vectorised numpy), `coco_strings` over all of them.
  ATen route    uint8 only, on the device: the planes transposed to column-major, compared with their copy shifted by
                one position, `nonzero`; then the same host arithmetic as `encode`.
  kernels alone ten calls of each library entry point queued behind a delay kernel between two device events, so that
                no host time lies between them: per call.  For the count pass also the bytes of its least traffic (every
                plane element read once, 12 bytes written per segment) per second against the rate a float4 copy reaches
                on this part (6.29 TB/s measured, 8.0 TB/s by the data sheet)."""
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

import rle_case as LC  # noqa: E402
from deva.hip import mask_runs  # noqa: E402
from deva.inference.frame_results import coco_strings, rle_counts  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
QUEUED = 10


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ts):
    return f'{statistics.median(ts):.3f} (min {min(ts):.3f}, max {max(ts):.3f})'


def host_route(planes, threshold):
    host = planes.cpu().numpy()
    ones = host != 0 if threshold is None else host > threshold
    each = [LC.counts_of(m) for m in ones]
    texts = coco_strings(np.concatenate([np.asarray(c, dtype=np.int64) for c in each]), [len(c) for c in each])
    return [{'size': list(host.shape[1:]), 'counts': t} for t in texts]


def aten_route(planes):
    n, h, w = planes.shape
    flat = (planes != 0).transpose(1, 2).reshape(n, h * w)
    before = torch.zeros_like(flat)
    before[:, 1:] = flat[:, :-1]
    where = (flat != before).nonzero()                       # (synchronises: its size)
    per_mask = torch.bincount(where[:, 0], minlength=n).cpu().numpy()
    counts, lengths = rle_counts(np.concatenate([[0], per_mask]), where[:, 1].cpu().numpy(), h * w)
    return [{'size': [h, w], 'counts': t} for t in coco_strings(counts, lengths)]


def kernels_alone(planes, threshold, sleep_cycles):
    """-> (ms per count call, ms per write call)"""
    counted = mask_runs.count(planes, threshold, stats=True)
    total = int(counted.total.cpu())
    bounds = torch.empty(total, dtype=torch.int32, device=planes.device)
    out = {'n': counted.n, 'base': counted.base, 'total': counted.total, 'stats': counted.stats, 'scratch': counted.scratch}
    times = []
    for call in (lambda: mask_runs.count(planes, threshold, stats=True, out=out), lambda: mask_runs.write(counted, bounds)):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda._sleep(sleep_cycles)
        start.record()
        for _ in range(QUEUED):
            call()
        stop.record()
        if start.query():
            raise RuntimeError('kernels_alone: the delay was over before the launches were queued; the timing would hold host time')
        stop.synchronize()
        times.append(start.elapsed_time(stop) / QUEUED)
    return times[0], times[1], total


def size_rows(h, w, k, rounds, dev, sleep_cycles):
    distinct = np.stack([LC.blobs(h, w, seed, specks=0.0005) for seed in range(8)])
    bytes_ = torch.from_numpy(distinct[np.arange(k) % 8]).to(dev)
    logits = torch.where(bytes_ != 0, 4.0, -4.0).to(torch.float32)
    lines = []
    for name, planes, threshold, size_of in (('uint8', bytes_, None, 1), ('float32', logits, 0.0, 4)):
        got = mask_runs.encode(planes, threshold=threshold)              # warm-up, and the comparison of the routes
        equal = got == host_route(planes, threshold) and (threshold is not None or got == aten_route(planes))
        t_encode, t_host, t_aten, t_count, t_write = [], [], [], [], []
        for _ in range(rounds):
            t_encode.append(wall(lambda: mask_runs.encode(planes, threshold=threshold))[0])
            t_host.append(wall(lambda: host_route(planes, threshold))[0])
            if threshold is None:
                t_aten.append(wall(lambda: aten_route(planes))[0])
            c, wr, total = kernels_alone(planes, threshold, sleep_cycles)
            t_count.append(c)
            t_write.append(wr)
        tag = f'{h} x {w}, {name}'
        plan = mask_runs.runs_plan(k, (h, w))
        least = k * h * w * size_of + plan.scratch_bytes
        rate = least / (statistics.median(t_count) * 1e-3)
        lines += [f'| {tag}: `encode`, {k} masks, {total} boundaries, {sum(len(r["counts"]) for r in got)} characters | {spread(t_encode)} |',
                  f'| {tag}: host route (`planes.cpu()`, numpy counts per plane, `coco_strings`) | {spread(t_host)}: '
                  f'{statistics.median(t_host) / statistics.median(t_encode):.1f}x |']
        if t_aten:
            lines.append(f'| {tag}: ATen route on the device (transpose, compare with the shifted copy, `nonzero`) | {spread(t_aten)}: '
                         f'{statistics.median(t_aten) / statistics.median(t_encode):.1f}x |')
        lines += [f'| {tag}: same strings on all routes | {"yes" if equal else "NO"} |',
                  f'| {tag}: `deva_runs_count` alone (stats, count, two scans), {least / 1e6:.1f} MB of least traffic | {spread(t_count)}: '
                  f'{rate / 1e12:.2f} TB/s, {100 * rate / HBM_MEASURED:.0f}% of the measured copy rate, {100 * rate / HBM_SPEC:.0f}% of the data sheet |',
                  f'| {tag}: `deva_runs_write` alone, {plan.scratch_bytes / 1e6:.1f} MB of scratch read | {spread(t_write)} |']
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--masks', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('mask_runs_bench: needs the GPU (a CPU timing says nothing about it)')
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
    lines = [f'{torch.cuda.get_device_name(0)}; {args.masks} planes of blobs with holes and specks; {args.rounds} alternating rounds',
             '', '| | ms, median (min, max) |', '|---|---|']
    for h, w in ((1080, 1920), (480, 854)):
        lines += size_rows(h, w, args.masks, args.rounds, dev, sleep_cycles)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
