"""The savers' PNG files coded on the device (csrc/png/png_encode.hip) against the host codec, in one process.

    python tools/png_encode_bench.py [--rounds 7] [--frames 100] [--out FILE.md]

Planes: blob id maps of 14 objects (tests/png_case.py `blobs`) at 480 x 854 and 1080 x 1920, as [H,W] with a palette and
as [H,W,3] long-id colours.  Every timing of a whole call is a host clock around the call and a device synchronise, after
a warm-up, in alternating rounds (host path, device path, host path, ...): median, minimum and maximum.  No ratio is asserted.

  whole call     `png.encode(plane, palette=)` -- three launches, the wait for `info`, the copy of the stream, the chunks
                 and CRCs on the host -- against `plane.cpu()` plus PIL `save` into memory
  kernels alone  ten calls of `deva_png_deflate` queued behind a delay kernel between two device events, per call; beside
                 it a device-to-device copy of the plane timed the same way: it moves the bytes of the coder's least
                 traffic (one read of the plane and of the row above = two plane sizes; the copy reads one and writes one)
  file size      the device's file against PIL's
  saver          `FrameResultSaver` over `--frames` frames of synthetic probabilities at 1080 x 1920 (15 channels), `png='host'`
                 against `png='device'`, in frames a second from the first `save_mask` to the return of `end()`"""
import argparse
import io
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import png_case as PC  # noqa: E402
from deva.hip import png  # noqa: E402

QUEUED = 10
SIZES = ((480, 854), (1080, 1920))
PALETTE = bytes(np.random.default_rng(5).integers(0, 256, 768, dtype=np.uint8))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ts):
    return f'{statistics.median(ts):.3f} (min {min(ts):.3f}, max {max(ts):.3f})'


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


def pil_file(plane, rgb):
    host = plane.cpu().numpy()
    image = Image.fromarray(host)
    if not rgb:
        image.putpalette(PALETTE)
    buf = io.BytesIO()
    image.save(buf, format='PNG')
    return buf.getvalue()


def plane_rows(h, w, rgb, rounds, dev, sleep_cycles):
    host = PC.blobs(h, w, objects=14, seed=h, rgb=rgb)
    plane = torch.from_numpy(host).to(dev)
    tag = f'{h} x {w} {"[H,W,3]" if rgb else "[H,W] + palette"}'
    device_call = lambda: png.encode(plane, palette=None if rgb else PALETTE)
    host_call = lambda: pil_file(plane, rgb)
    ours, theirs = device_call(), host_call()                         # warm-up, and the comparison
    same = np.array_equal(np.array(Image.open(io.BytesIO(ours))), host) and np.array_equal(np.array(Image.open(io.BytesIO(theirs))), host)
    t_host, t_device = [], []
    for _ in range(rounds):
        t_host.append(wall(host_call)[0])
        t_device.append(wall(device_call)[0])
    bpp = 3 if rgb else 1
    p = png.plan(h, w, bpp)
    scratch = torch.empty(p.scratch_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(p.worst_case, dtype=torch.uint8, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    t_kernels = [queued(lambda: png._launch_deflate(plane, h, w, bpp, scratch, out, p.worst_case, info), sleep_cycles) for _ in range(rounds)]
    other = torch.empty_like(plane)
    t_copy = [queued(lambda: other.copy_(plane), sleep_cycles) for _ in range(rounds)]
    ratio = statistics.median(t_host) / statistics.median(t_device)
    gb = 2 * plane.numel() / 1e9
    return [f'| {tag}: `plane.cpu()` + PIL `save` | {spread(t_host)} |',
            f'| {tag}: `png.encode` | {spread(t_device)}: host / device = {ratio:.2f} |',
            f'| {tag}: both files decode to the plane | {"yes" if same else "NO"} |',
            f'| {tag}: `deva_png_deflate` alone, {p.segments} segments | {spread(t_kernels)}: {gb / statistics.median(t_kernels) * 1e3:.0f} GB/s of its least traffic |',
            f'| {tag}: device-to-device copy of the plane (the same bytes moved) | {spread(t_copy)}: {gb / statistics.median(t_copy) * 1e3:.0f} GB/s |',
            f'| {tag}: file bytes, device / PIL | {len(ours)} / {len(theirs)} = {len(ours) / len(theirs):.2f} |']


def saver_rows(frames, rounds, dev):
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    h, w, objects = 1080, 1920, 14
    probs = []
    for seed in range(4):
        ids = torch.from_numpy(PC.blobs(h, w, objects=objects, seed=100 + seed).astype(np.int64)).to(dev)
        probs.append(torch.nn.functional.one_hot(ids, objects + 1).permute(2, 0, 1).float().mul(0.9).add(0.1 / (objects + 1)).contiguous())
    lines = []
    for dataset, long_id in (('unsup_davis17', False), ('vipseg', True)):
        times = {'host': [], 'device': []}
        for _ in range(rounds + 1):                                   # (the first round warms up)
            for mode in ('host', 'device'):
                om = ObjectManager()
                om.use_long_id = long_id
                om.add_new_objects([ObjectInfo(id=(1000 * k + 7) if long_id else k, category_id=1, score=0.5) for k in range(1, objects + 1)])
                root = tempfile.mkdtemp(prefix='png_bench_')
                try:
                    saver = FrameResultSaver(root, 'clip', dataset=dataset, object_manager=om, palette=None if long_id else PALETTE, png=mode)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for t in range(frames):
                        saver.save_mask(probs[t % len(probs)], f'{t:05d}.jpg')
                    saver.end()
                    torch.cuda.synchronize()
                    times[mode].append(frames / (time.perf_counter() - t0))
                finally:
                    shutil.rmtree(root, ignore_errors=True)
        for mode in ('host', 'device'):
            fps = times[mode][1:]
            lines.append(f"| saver, {dataset} ({'[H,W,3]' if long_id else '[H,W] + palette'}), {frames} frames at {h} x {w}, png='{mode}' | "
                         f'{statistics.median(fps):.1f} frames/s (min {min(fps):.1f}, max {max(fps):.1f}) |')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--saver-rounds', type=int, default=2)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('png_encode_bench: needs the GPU (a CPU timing says nothing about it)')
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
    lines = [f'{torch.cuda.get_device_name(0)}; blob id maps of 14 objects; {args.rounds} alternating rounds (host path, device path)', '',
             '| | ms, median (min, max) |', '|---|---|']
    for h, w in SIZES:
        for rgb in (False, True):
            lines += plane_rows(h, w, rgb, args.rounds, dev, sleep_cycles)
    lines += saver_rows(args.frames, args.saver_rounds, dev)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
