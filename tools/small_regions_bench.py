"""Small holes and islands of segmenter masks: `deva.hip.regions.remove_small_regions` (csrc/regions/regions.hip) against
what a user does without it -- the planes copied to the host, `scipy.ndimage.label` + `bincount` + `isin` per plane and
pass, the result copied back -- and what the option costs a frame of the proposal filter.

    python tools/small_regions_bench.py [--rounds 5] [--planes 64] [--min-area 100] [--out FILE.md]

Workload: `--planes` byte planes of blobs with holes and specks (tests/region_case.py: eight distinct ones, cycled) at
1080 x 1920 and at 480 x 854.  Timed with device events around each call on fresh copies of the same inputs, after a
warm-up, in alternating rounds: median, minimum and maximum.  The two labellings alone (`label_components` of the mask and
of its complement: the local, border and flatten stages) are timed beside the whole call (which adds the area counts, the
decide and rewrite stages and the records).  The host baseline is skipped, and reported as skipped, where scipy is not
installed.  Then a frame of tools/proposal_filter_bench.py (16 batches of 192 planes at 1080 x 1920) through
`ProposalFilter` with `min_mask_region_area` off and on."""
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

import proposal_case as PC  # noqa: E402
import region_case as RC  # noqa: E402
from deva.hip import regions  # noqa: E402
from deva.inference.proposals import ProposalFilter  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


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


def host_pass(mask, min_area, holes):
    """one pass of the reference's helper on a boolean plane, scipy's labelling in OpenCV's place"""
    work = ~mask if holes else mask
    lab, n = ndimage.label(work, structure=np.ones((3, 3)))
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    small = np.flatnonzero(sizes < min_area) + 1
    if len(small) == 0:
        return mask
    if holes:
        return mask | np.isin(lab, small)
    if len(small) == n:
        return lab == int(np.argmax(sizes)) + 1
    return mask & ~np.isin(lab, small)


def host_clean(planes_dev, min_area):
    planes = planes_dev.cpu().numpy() != 0
    out = np.stack([host_pass(host_pass(p, min_area, True), min_area, False) for p in planes])
    return torch.from_numpy(out.astype(np.uint8)).to(planes_dev.device)


def size_rows(h, w, k, min_area, rounds, dev):
    distinct = [RC.blobs(h, w, seed) for seed in range(8)]
    planes = torch.from_numpy(np.stack([distinct[i % 8] for i in range(k)])).to(dev)
    scratch = torch.empty(regions.region_scratch_bytes(h, w, k), dtype=torch.uint8, device=dev)
    labels = torch.empty((k, h, w), dtype=torch.int32, device=dev)
    records = torch.empty((k, regions.FIELDS), dtype=torch.int32, device=dev)
    work = planes.clone()

    def clean():
        work.copy_(planes)                      # (outside the events below: the call works in place)
        return timed(lambda: regions.remove_small_regions(work, min_area, scratch=scratch, records=records))[0]
    clean()                                     # warm-up
    timed(lambda: regions.label_components(planes, out=labels))
    same = 'skipped (no scipy here)'
    if ndimage is not None:
        same = 'yes' if bool(torch.equal(host_clean(planes[:8], min_area), work[:8])) else 'NO'
    t_clean, t_mask, t_zero, t_host = [], [], [], []
    for _ in range(rounds):
        t_clean.append(clean())
        t_mask.append(timed(lambda: regions.label_components(planes, out=labels))[0])
        t_zero.append(timed(lambda: regions.label_components(planes, of_zeros=True, out=labels))[0])
        if ndimage is not None:
            t_host.append(timed(lambda: host_clean(planes, min_area))[0])
    rec = records.cpu().numpy()
    lines = [f'| {h} x {w}: `remove_small_regions`, {k} planes | {spread(t_clean)} |',
             f'| {h} x {w}: labelling of the mask alone (local, border, flatten) | {spread(t_mask)} |',
             f'| {h} x {w}: labelling of the complement alone | {spread(t_zero)} |',
             f'| {h} x {w}: host copy, scipy label + bincount + isin per plane and pass, copy back | '
             + (spread(t_host) if t_host else 'skipped: scipy is not installed here') + ' |']
    if t_host:
        lines.append(f'| {h} x {w}: ratio | {statistics.median(t_host) / statistics.median(t_clean):.0f}x |')
    lines.append(f'| {h} x {w}: same planes as the host form (first 8) | {same} |')
    lines.append(f'| {h} x {w}: planes changed, pixels filled, pixels removed | {int(rec[:, 0].sum())} of {k}, {int(rec[:, 1].sum())}, {int(rec[:, 2].sum())} |')
    return lines


def filter_rows(min_area, rounds, dev, n_batches=16, batch=192):
    h, w = 1080, 1920
    p = PC.params()
    distinct = []
    for seed in range(4):
        centres, radii, slopes, grid = PC.draw(h, w, batch, seed)
        distinct.append((PC.ramps(h, w, centres, radii, slopes, device=dev), torch.tensor(grid, dtype=torch.float32).to(dev)))
    batches = [distinct[i % 4] for i in range(n_batches)]
    filters = {area: ProposalFilter(h, w, capacity=4096, min_mask_region_area=area, **p) for area in (0, min_area)}

    def frame(flt):
        flt.reset()
        for logits, iou in batches:
            flt.add(logits, iou)
        return flt.finish()
    times = {area: [] for area in filters}
    kept = {area: int(timed(lambda: frame(flt))[1].masks.shape[0]) for area, flt in filters.items()}      # warm-up
    for _ in range(rounds):
        for area, flt in filters.items():
            times[area].append(timed(lambda: frame(flt))[0])
    off, on = statistics.median(times[0]), statistics.median(times[min_area])
    return [f'| filter frame ({n_batches} batches of {batch} at {h} x {w}), option off: {kept[0]} masks kept | {spread(times[0])} |',
            f'| the same with min_mask_region_area = {min_area}: {kept[min_area]} masks kept | {spread(times[min_area])} |',
            f'| extra cost of `finish` | {on - off:.2f} |']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--planes', type=int, default=64)
    ap.add_argument('--min-area', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('small_regions_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    lines = [f'{torch.cuda.get_device_name(0)}; blobs with holes and specks, min_area {args.min_area}; {args.rounds} alternating rounds',
             '', '| | ms, median (min, max) |', '|---|---|']
    for h, w in ((1080, 1920), (480, 854)):
        lines += size_rows(h, w, args.planes, args.min_area, args.rounds, dev)
    lines += filter_rows(args.min_area, args.rounds, dev)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
