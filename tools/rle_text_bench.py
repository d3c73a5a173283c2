"""The text of COCO run lengths coded and parsed on the device (csrc/rle_text/rle_text.hip) against the host path of the
same calls, in one process.

    python tools/rle_text_bench.py [--rounds 7] [--out FILE.md]

Workloads, the shapes of tools/mask_runs_bench.py, tools/rle_decode_bench.py and tools/rle_overlap_bench.py: 64 planes or
masks of blobs (tests/rle_case.py `blobs`, eight distinct ones repeated) at 1080 x 1920 and at 480 x 854; for the overlap
64 x 64 blob masks at 1080 x 1920 and 20 x 5 at 480 x 854 (tests/overlap_case.py `small_blobs`).  Every timing of a whole
call is a host clock around the call and a device synchronise, after a warm-up, in alternating rounds (host path, device
path, host path, ...): median, minimum and maximum.  The yardstick is the host path measured in the same run; it is the
code of the commit before this library, whose recorded figures stand beside it.  No ratio is asserted.

  encode         `rle.encode(planes)` with text='host' and text='device'
  decode         `rle.decode(masks)` with parse='host' and parse='device'
  intersections  `rle.intersections(dt, gt)` with parse='host' and parse='device'
  kernels alone  ten calls of the library's launcher queued behind a delay kernel between two device events, so that no
                 host time lies between them: per call."""
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
import rle_case as LC  # noqa: E402
from deva.hip import mask_runs, rle, rle_text  # noqa: E402
from deva.inference.frame_results import coco_strings  # noqa: E402

QUEUED = 10
SIZES = ((1080, 1920, 64), (480, 854, 64))
OVERLAPS = ((1080, 1920, 64, 64, 150), (480, 854, 20, 5, 60))
RECORDED = {'encode': '13.6 ms', 'decode': '6.2 ms', 'intersections': '2.5 ms'}   # the commit before, 64 at 1080 x 1920 (README)


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


def queued(call, sleep_cycles):
    """-> ms per call of `call`, ten of them queued behind the delay"""
    call()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda._sleep(sleep_cycles)
    start.record()
    for _ in range(QUEUED):
        call()
    stop.record()
    if start.query():
        raise RuntimeError('queued: the delay was over before the launches were queued; the timing would hold host time')
    stop.synchronize()
    return start.elapsed_time(stop) / QUEUED


def two_paths(host, device, rounds):
    """alternating rounds -> (times of the host path, times of the device path, the results are equal)"""
    def same(a, b):
        if isinstance(a, torch.Tensor):
            return torch.equal(a, b)
        return all(same(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else a == b
    equal = same(host(), device())                                # warm-up, and the comparison
    t_host, t_device = [], []
    for _ in range(rounds):
        t_host.append(wall(host)[0])
        t_device.append(wall(device)[0])
    return t_host, t_device, equal


def rows(tag, name, recorded, t_host, t_device, equal):
    ratio = statistics.median(t_host) / statistics.median(t_device)
    note = f'; recorded before: {recorded}' if recorded else ''
    return [f'| {tag}: `rle.{name}`, host path{note} | {spread(t_host)} |',
            f'| {tag}: `rle.{name}`, device path | {spread(t_device)}: host / device = {ratio:.2f} |',
            f'| {tag}: `rle.{name}`: the same result on both paths | {"yes" if equal else "NO"} |']


def size_rows(h, w, k, rounds, dev, sleep_cycles):
    first = (h, w) == SIZES[0][:2]
    distinct = np.stack([LC.blobs(h, w, seed, specks=0.0005) for seed in range(8)])
    planes = torch.from_numpy(distinct[np.arange(k) % 8]).to(dev)
    tag = f'{h} x {w}, {k} masks'
    lines = rows(tag, 'encode', RECORDED['encode'] if first else None,
                 *two_paths(lambda: mask_runs.encode(planes), lambda: mask_runs.encode(planes, text='device'), rounds))
    masks = mask_runs.encode(planes)
    lines += rows(tag, 'decode', RECORDED['decode'] if first else None,
                  *two_paths(lambda: rle.decode(masks, device=dev), lambda: rle.decode(masks, device=dev, parse='device'), rounds))
    # the kernels alone
    counted = mask_runs.count(planes)
    total = int(counted.total.cpu())
    bounds = mask_runs.write(counted, torch.empty(total, dtype=torch.int32, device=dev))
    room = rle_text.max_chars(h * w) * (total + k)
    text_len, text_base = torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.int64, device=dev)
    text_total, chars = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(room, dtype=torch.uint8, device=dev)
    t_count = [queued(lambda: rle_text._launch_encode_count(counted.n, counted.base, bounds, total, h, w, text_len, text_base, text_total, None),
                      sleep_cycles) for _ in range(rounds)]
    t_write = [queued(lambda: rle_text._launch_encode_write(counted.n, counted.base, bounds, total, h, w, text_base, chars, room), sleep_cycles)
               for _ in range(rounds)]
    texts = [m['counts'].encode() for m in masks]
    body = b''.join(texts)
    first_d = torch.from_numpy(np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)).to(dev)
    chars_d = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
    words_cap = 2 * k + 1 + len(body)
    runs, info = torch.empty(words_cap, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    scratch = torch.empty(2 * k, dtype=torch.int32, device=dev)
    t_parse = [queued(lambda: rle_text._launch_parse(chars_d, len(body), first_d, k, h, w, scratch, runs, words_cap, info), sleep_cycles)
               for _ in range(rounds)]
    lines += [f'| {tag}: `deva_text_encode_count` alone, {total + k} counts | {spread(t_count)} |',
              f'| {tag}: `deva_text_encode_write` alone, {int(text_total.cpu())} characters | {spread(t_write)} |',
              f'| {tag}: `deva_text_parse` alone, {len(body)} characters, {int(info.cpu()[1])} words, flags {int(info.cpu()[0])} | {spread(t_parse)} |']
    return lines


def overlap_rows(h, w, n_d, n_g, radius, rounds, dev):
    dt = as_strings(OC.small_blobs(h, w, n_d, seed=1, radius=radius), h, w)
    gt = as_strings(OC.small_blobs(h, w, n_g, seed=2, radius=radius), h, w)
    return rows(f'{h} x {w}, {n_d} x {n_g}', 'intersections', RECORDED['intersections'] if (h, w) == OVERLAPS[0][:2] else None,
                *two_paths(lambda: rle.intersections(dt, gt, device=dev), lambda: rle.intersections(dt, gt, device=dev, parse='device'), rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('rle_text_bench: needs the GPU (a CPU timing says nothing about it)')
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
    lines = [f'{torch.cuda.get_device_name(0)}; blob masks; {args.rounds} alternating rounds (host path, device path)', '',
             '| | ms, median (min, max) |', '|---|---|']
    for h, w, k in SIZES:
        lines += size_rows(h, w, k, args.rounds, dev, sleep_cycles)
    for h, w, n_d, n_g, radius in OVERLAPS:
        lines += overlap_rows(h, w, n_d, n_g, radius, args.rounds, dev)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
