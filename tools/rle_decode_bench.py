"""COCO run-length masks onto the device: `deva.hip.rle.decode` (csrc/rle/rle_decode.hip) against what a user does
without it -- every mask decoded on the host with numpy, the planes stacked, copied to the device and resized there with
`F.interpolate(mode='nearest')`.

    python tools/rle_decode_bench.py [--rounds 7] [--masks 64] [--out FILE.md]

Workload: `--masks` masks of seeded blobs with holes and specks (tests/rle_case.py: eight distinct ones, cycled; one pixel
in 2000 is a speck, which leaves some ten thousand runs a mask at 1080 x 1920), as the compressed strings of a "COCO results" file, at 1080 x 1920 -> 1080 x 1920 and at 720 x 1280 -> 480 x 854, to uint8 planes
(and to float32 ones for the kernel's rate).  Every timing of a whole call is a host clock around the call and a device
synchronise, after a warm-up, in alternating rounds: median, minimum and maximum.

  decode        the whole call: the text parsed, D2 checked, the run starts summed, one pinned copy up, one launch.
  host route    the statement's vectorised decode (np.repeat of the run values over the counts) per mask, np.stack,
                torch.from_numpy(...).to(device), F.interpolate(nearest) on the device.  It starts from counts that are
                parsed already (the only parser at hand without the code under test is a Python loop over characters),
                so it is favoured by the cost of the parse.
  kernel alone  ten launches queued behind a delay kernel between two device events, so that no host time lies between
                them: per launch, and the bytes it writes per second against the HBM rate a float4 copy reaches on this
                part (6.29 TB/s measured, 8.0 TB/s by the data sheet).
  host share    of a decode call: parse (text to counts, D2) and cumsum (counts to the int32 run array)."""
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

import rle_case as LC  # noqa: E402
from deva.hip import rle  # noqa: E402
from deva.hip.ops import _stream  # noqa: E402
from deva.inference.frame_results import coco_strings  # noqa: E402

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


def host_route(all_counts, h, w, size, dev):
    planes = torch.from_numpy(np.stack([LC.plane(c, h, w) for c in all_counts])).to(dev)
    if size != (h, w):
        planes = F.interpolate(planes[None], size=size, mode='nearest')[0]
    return planes


def kernel_alone(parsed, size, dtype, dev, sleep_cycles):
    """-> ms per launch: QUEUED launches of the library's entry point behind a delay kernel, between two events"""
    n = int(parsed.per_mask.size)
    words = rle.run_array(parsed, 0, n)
    host = torch.from_numpy(words).pin_memory()
    runs = host.to(dev)
    out = torch.empty((n,) + size, dtype=dtype, device=dev)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda._sleep(sleep_cycles)
    start.record()
    for _ in range(QUEUED):   # (each with its D2 pass over the run array on the host: well inside the delay)
        rle.check(rle.lib().deva_rle_decode(host.data_ptr(), runs.data_ptr(), words.size, n, parsed.height, parsed.width, size[0], size[1],
                                            rle.DTYPES[dtype], out.data_ptr(), _stream(dev)), 'deva_rle_decode')
    stop.record()
    if start.query():
        raise RuntimeError('kernel_alone: the delay was over before the launches were queued; the timing would hold host time')
    stop.synchronize()
    return start.elapsed_time(stop) / QUEUED


def size_rows(h, w, size, k, rounds, dev, sleep_cycles):
    distinct = [LC.counts_of(LC.blobs(h, w, seed, specks=0.0005)) for seed in range(8)]
    all_counts = [np.asarray(distinct[i % 8], dtype=np.int64) for i in range(k)]
    texts = coco_strings(np.concatenate(all_counts), [c.size for c in all_counts])
    rles = [{'size': [h, w], 'counts': t} for t in texts]
    runs = sum(c.size for c in all_counts)
    out = torch.empty((k,) + size, dtype=torch.uint8, device=dev)
    got = rle.decode(rles, size, out=out)                      # warm-up, and the comparison of the two routes
    want = host_route(all_counts, h, w, size, dev)
    equal = 'yes' if bool(torch.equal(got, want)) else 'NO'
    parsed = rle.parse_checked(rles)
    t_decode, t_host, t_parse, t_cumsum, t_u8, t_f32 = [], [], [], [], [], []
    for _ in range(rounds):
        t_decode.append(wall(lambda: rle.decode(rles, size, out=out))[0])
        t_host.append(wall(lambda: host_route(all_counts, h, w, size, dev))[0])
        t0 = time.perf_counter()
        parsed = rle.parse_checked(rles)
        t1 = time.perf_counter()
        rle.run_array(parsed, 0, k)
        t2 = time.perf_counter()
        t_parse.append((t1 - t0) * 1e3)
        t_cumsum.append((t2 - t1) * 1e3)
        t_u8.append(kernel_alone(parsed, size, torch.uint8, dev, sleep_cycles))
        t_f32.append(kernel_alone(parsed, size, torch.float32, dev, sleep_cycles))
    tag = f'{h} x {w} -> {size[0]} x {size[1]}'
    pixels = k * size[0] * size[1]
    lines = [f'| {tag}: `decode`, {k} masks, {runs} runs, {sum(len(t) for t in texts)} characters | {spread(t_decode)} |',
             f'| {tag}: host route (numpy decode, copy up, interpolate on the device) | {spread(t_host)} |',
             f'| {tag}: ratio of the medians | {statistics.median(t_host) / statistics.median(t_decode):.1f}x |',
             f'| {tag}: same planes on both routes | {equal} |',
             f'| {tag}: host share of `decode`: parse and D2 | {spread(t_parse)} |',
             f'| {tag}: host share of `decode`: cumsum into the run array ({2 * k + 1 + runs} words) | {spread(t_cumsum)} |']
    for name, ts, size_of in (('uint8', t_u8, 1), ('float32', t_f32, 4)):
        rate = pixels * size_of / (statistics.median(ts) * 1e-3)
        lines.append(f'| {tag}: kernel alone, {name}, {pixels * size_of / 1e6:.1f} MB written | {spread(ts)}: {rate / 1e12:.2f} TB/s, '
                     f'{100 * rate / HBM_MEASURED:.0f}% of the measured copy rate, {100 * rate / HBM_SPEC:.0f}% of the data sheet |')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--masks', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('rle_decode_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    # ~40 ms of delay: the host enqueues ten launches (with their D2 pass over the run array) well inside it
    torch.cuda._sleep(1000000)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(20000000)
    b.record()
    b.synchronize()
    sleep_cycles = int(20000000 / a.elapsed_time(b) * 40)
    lines = [f'{torch.cuda.get_device_name(0)}; {args.masks} masks of blobs with holes and specks; {args.rounds} alternating rounds',
             '', '| | ms, median (min, max) |', '|---|---|']
    for (h, w), size in (((1080, 1920), (1080, 1920)), ((720, 1280), (480, 854))):
        lines += size_rows(h, w, size, args.masks, args.rounds, dev, sleep_cycles)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
