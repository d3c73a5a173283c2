"""Detector output -> (index mask, segments_info): the fused call (`deva.inference.detections`, csrc/detections.hip)
against the same arithmetic in ATen on the same device, host synchronisations included on both sides.

    python tools/detection_assembly_bench.py [--rounds 5] [--iters 3] [--out FILE.md]

The ATen form restates what the reference's detector wrappers do after the detector has run: an fp32 copy of the N
masks, a bilinear resize, the areas, a scaled copy, a background plane concatenated in front, an argmax, and then a
Python loop over the masks with full-frame compares whose `.sum()` results the host branches on.  Both forms are timed
with device events around the whole call (the call returns with its list of segments on the host, so the window ends
synchronised), in alternating rounds on the same inputs; the table gives the median over rounds of the per-round mean.
Sizes: 1080 x 1920 masks to 1080 x 1920 and to 480 x 853; N = 16 / 64 / 256; the three policies.  The bytes column is
what the fused form must read and write at least (twice the N mask planes, the uint16 plane twice, the int64 mask)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from deva.inference import detections as D  # noqa: E402


def make_masks(n, h, w, seed, device):
    """n random boxes of very different sizes (some nested, some overlapping), one empty mask"""
    rng = np.random.default_rng(seed)
    masks = torch.zeros(n, h, w, dtype=torch.bool)
    for k in range(n):
        if k == n // 2:
            continue
        bh, bw = int(h * rng.uniform(0.03, 0.5)), int(w * rng.uniform(0.03, 0.5))
        y0, x0 = int(rng.integers(0, h - bh)), int(rng.integers(0, w - bw))
        masks[k, y0:y0 + bh, x0:x0 + bw] = True
    return masks.to(device)


def aten_automatic(masks, scores, size, suppress, threshold):
    planes = masks.float()
    if tuple(planes.shape[-2:]) != tuple(size):
        planes = F.interpolate(planes.unsqueeze(0), size, mode='bilinear')[0]
    areas = planes.flatten(1).sum(1)
    weight = areas if suppress else areas.max() * 2 - areas
    scored = torch.cat([torch.full((1, *size), 0.1, device=planes.device), planes * weight.view(-1, 1, 1)])
    hard = scored.argmax(0)
    out = torch.zeros(size, dtype=torch.int64, device=planes.device) if suppress else hard
    found = []
    for k in range(planes.shape[0]):
        mine = hard == k + 1
        if suppress:
            owned, original = mine.sum(), (planes[k] > 0.5).sum()
            solid = mine & (planes[k] >= 0.5)
            if owned > 0 and original > 0 and solid.sum() > 0 and not owned / original < threshold:
                out[solid] = len(found) + 1
                found.append((len(found) + 1, scores[k].item()))
        elif mine.sum() > 0:
            found.append((len(found) + 1, scores[k].item()))
    return out, found


def aten_text(masks, confidences, classes, size):
    """(the reference resizes each mask on the host; here that runs on the device too, which is kinder to it)"""
    out = torch.zeros(size, dtype=torch.int64, device=masks.device)
    found = []
    order = np.flip(np.argsort(masks.flatten(1).sum(1).cpu().numpy(), kind='stable'))
    for k in order:
        plane = F.interpolate(masks[k].float()[None, None], size, mode='bilinear')[0, 0] > 0.5
        if plane.sum() > 0:
            out[plane] = len(found) + 1
            found.append((len(found) + 1, classes[k], confidences[k]))
    return out, found


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--counts', type=int, nargs='+', default=[16, 64, 256])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('detection_assembly_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    h, w = 1080, 1920
    lines = ['| output | N | policy | fused ms | ATen ms | ratio | fused GB/s of its least traffic | same result |',
             '|---|---|---|---|---|---|---|---|']
    for size in ((1080, 1920), D.detection_size(h, w, 480)):
        for n in args.counts:
            masks = make_masks(n, h, w, n, dev)
            scores = torch.from_numpy(np.random.default_rng(n).random(n).astype(np.float32))
            dev_scores = scores.to(dev)
            conf, classes = np.linspace(0.9, 0.3, n).astype(np.float32), np.arange(n) % 5
            least = 2 * n * h * w + size[0] * size[1] * (2 + 2 + 8)
            forms = {
                'suppress small': (lambda: D.assemble_automatic(masks, dev_scores, size, suppress_small_objects=True),
                                   lambda: aten_automatic(masks, dev_scores, size, True, 0.8)),
                'prefer small': (lambda: D.assemble_automatic(masks, dev_scores, size, suppress_small_objects=False),
                                 lambda: aten_automatic(masks, dev_scores, size, False, 0.8)),
                'text': (lambda: D.assemble_with_text(masks, conf, classes, size),
                         lambda: aten_text(masks, conf, classes, size)),
            }
            for name, (fused, aten) in forms.items():
                a, b = fused(), aten()           # warm-up of both, and the results side by side
                same = bool(torch.equal(a[0], b[0])) and [o.id for o in a[1]] == [f[0] for f in b[1]]
                t_fused, t_aten = [], []
                for _ in range(args.rounds):     # alternating rounds on the same inputs
                    t_fused.append(timed(fused, args.iters))
                    t_aten.append(timed(aten, max(1, args.iters // 3)))
                f, r = statistics.median(t_fused), statistics.median(t_aten)
                lines.append(f'| {size[0]} x {size[1]} | {n} | {name} | {f:.3f} (min {min(t_fused):.3f}, max {max(t_fused):.3f}) | '
                             f'{r:.2f} | {r / f:.1f}x | {least / f / 1e6:.0f} | {"yes" if same else "NO"} |')
                print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
