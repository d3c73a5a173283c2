"""The demo saver's overlay JPEG coded on the device (csrc/jpeg/jpeg_encode.hip) against the host codec, in one process.

    python tools/jpeg_encode_bench.py [--rounds 7] [--frames 100] [--out FILE.md]

Planes: overlays (tests/jpeg_case.py `overlay`: a smooth frame with sensor noise and translucent blobs) at 480 x 854 and
1080 x 1920, quality 75, 4:2:0, one restart interval per MCU row -- what `FrameResultSaver(jpeg='device')` asks for.
Every timing of a whole call is a host clock around the call and a device synchronise, after a warm-up, in alternating
rounds (host path, device path, host path, ...): median, minimum and maximum.  No ratio is asserted.

  whole call     `jpeg.encode(plane)` -- four launches, the wait for `info`, the copy of the data, the markers on the host --
                 against `plane.cpu()` plus PIL `save(quality=75)` into memory; the host path's two halves also on their own
  kernels alone  ten calls of `deva_jpeg_scan` queued behind a delay kernel between two device events, per call; beside
                 it a device-to-device copy of the plane timed the same way
  file           the device's file against PIL's: bytes, and PSNR of the decoded file against the plane
  saver          `FrameResultSaver` (dataset `demo`, `png='device'`) over `--frames` frames of synthetic probabilities at
                 1080 x 1920 (15 channels) with an overlay each, `jpeg='host'` against `jpeg='device'`, in frames a second
                 from the first `save_mask` to the return of `end()`"""
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

import jpeg_case as JC  # noqa: E402
import png_case as PC  # noqa: E402
from deva.hip import jpeg  # noqa: E402

QUEUED = 10
SIZES = ((480, 854), (1080, 1920))


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


def pil_save(host):
    buf = io.BytesIO()
    Image.fromarray(host).save(buf, format='JPEG', quality=75)
    return buf.getvalue()


def plane_rows(h, w, rounds, dev, sleep_cycles):
    host = JC.overlay(h, w, seed=h)
    plane = torch.from_numpy(host).to(dev)
    tag = f'{h} x {w}'
    device_call = lambda: jpeg.encode(plane)
    host_call = lambda: pil_save(plane.cpu().numpy())
    ours, theirs = device_call(), host_call()                         # warm-up, and the comparison
    psnr_ours, psnr_theirs = (JC.psnr(np.array(Image.open(io.BytesIO(f))), host) for f in (ours, theirs))
    t_host, t_device, t_copy_host, t_pil = [], [], [], []
    for _ in range(rounds):
        t_host.append(wall(host_call)[0])
        t_device.append(wall(device_call)[0])
        t_copy_host.append(wall(lambda: plane.cpu())[0])
        t_pil.append(wall(lambda: pil_save(host))[0])
    p = jpeg.plan(h, w)
    scratch = torch.empty(p.scratch_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(p.worst_case, dtype=torch.uint8, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    t_kernels = [queued(lambda: jpeg._launch_scan(plane, h, w, 75, 420, 0, scratch, out, p.worst_case, info), sleep_cycles) for _ in range(rounds)]
    other = torch.empty_like(plane)
    t_copy = [queued(lambda: other.copy_(plane), sleep_cycles) for _ in range(rounds)]
    ratio = statistics.median(t_host) / statistics.median(t_device)
    gb = plane.numel() / 1e9
    return [f'| {tag}: `plane.cpu()` + PIL `save(quality=75)` | {spread(t_host)} |',
            f'| {tag}: of that, `plane.cpu()` alone (pageable) | {spread(t_copy_host)} |',
            f'| {tag}: of that, PIL `save` alone | {spread(t_pil)} |',
            f'| {tag}: `jpeg.encode` | {spread(t_device)}: host / device = {ratio:.2f} |',
            f'| {tag}: `deva_jpeg_scan` alone, {p.intervals} intervals, {p.blocks} blocks | {spread(t_kernels)}: {gb / statistics.median(t_kernels) * 1e3:.0f} GB/s of the plane |',
            f'| {tag}: device-to-device copy of the plane | {spread(t_copy)} |',
            f'| {tag}: file bytes, device / PIL | {len(ours)} / {len(theirs)} = {len(ours) / len(theirs):.3f} |',
            f'| {tag}: PSNR against the plane, device / PIL | {psnr_ours:.3f} / {psnr_theirs:.3f} dB |',
            f'| {tag}: scratch / worst-case capacity of the plan | {p.scratch_bytes / 2 ** 20:.1f} / {p.worst_case / 2 ** 20:.1f} MiB |']


def saver_rows(frames, rounds, dev):
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    h, w, objects = 1080, 1920, 14
    probs, images = [], []
    for seed in range(4):
        ids = torch.from_numpy(PC.blobs(h, w, objects=objects, seed=100 + seed).astype(np.int64)).to(dev)
        probs.append(torch.nn.functional.one_hot(ids, objects + 1).permute(2, 0, 1).float().mul(0.9).add(0.1 / (objects + 1)).contiguous())
        images.append(JC.overlay(h, w, seed=200 + seed))
    lines = []
    times = {'host': [], 'device': []}
    for _ in range(rounds + 1):                                   # (the first round warms up)
        for mode in ('host', 'device'):
            om = ObjectManager()
            om.use_long_id = True
            om.add_new_objects([ObjectInfo(id=1000 * k + 7, category_id=1, score=0.5) for k in range(1, objects + 1)])
            root = tempfile.mkdtemp(prefix='jpeg_bench_')
            try:
                saver = FrameResultSaver(root, 'clip', dataset='demo', object_manager=om, png='device', jpeg=mode)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(frames):
                    saver.save_mask(probs[t % len(probs)], f'{t:05d}.jpg', image_np=images[t % len(images)])
                saver.end()
                torch.cuda.synchronize()
                times[mode].append(frames / (time.perf_counter() - t0))
            finally:
                shutil.rmtree(root, ignore_errors=True)
    for mode in ('host', 'device'):
        fps = times[mode][1:]
        lines.append(f"| saver, demo, {frames} frames at {h} x {w}, png='device', jpeg='{mode}' | "
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
        sys.exit('jpeg_encode_bench: needs the GPU (a CPU timing says nothing about it)')
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
    lines = [f'{torch.cuda.get_device_name(0)}; overlays, quality 75, 4:2:0, an interval per MCU row; {args.rounds} alternating rounds (host path, device path)',
             '', '| | ms, median (min, max) |', '|---|---|']
    for h, w in SIZES:
        lines += plane_rows(h, w, args.rounds, dev, sleep_cycles)
    lines += saver_rows(args.frames, args.saver_rounds, dev)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
