"""Proposal filter of a promptable segmenter: the fused path (`deva.inference.proposals.ProposalFilter`,
csrc/proposals.hip) against the reference's arithmetic restated in ATen on the same device, host synchronisations
included on both sides.

    python tools/proposal_filter_bench.py [--rounds 5] [--batches 16] [--batch 192] [--out FILE.md]

A frame is `--batches` batches of `--batch` logit planes at 1080 x 1920 (the planes of tests/proposal_case.py at full
size; four distinct batches, cycled) followed by box NMS.  The ATen form does per batch what the reference's generator
does (automatic_mask_generator.py:332-352): a boolean-index copy of the fp32 planes after the IoU drop, two threshold
counts, a second copy after the stability drop, the binarisation and the four reductions of the boxes; then per frame
(:272-278) the IoU matrix on the device and the greedy walk on the host.  Both forms are timed with device events
around the whole frame (both end synchronised, with their result on the device), in alternating rounds on the same
inputs: median, minimum and maximum over the rounds.  The fused batch passes alone (no finish) are timed the same way
and set against their least traffic, 4 HW bytes per live mask plus (4 + 1) HW per stored mask, and the 8 TB/s roof."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import proposal_case as PC  # noqa: E402
from deva.inference.proposals import ProposalFilter  # noqa: E402

ROOF = 8e12


def mask_boxes(masks):
    """bool [N,H,W] -> int64 [N,4] x0, y0, x1, y1 by four reductions over the planes; 0,0,0,0 for an empty mask"""
    n, h, w = masks.shape
    rows, cols = masks.any(-1), masks.any(-2)
    ys, xs = torch.arange(h, device=masks.device), torch.arange(w, device=masks.device)
    y1, x1 = (rows * ys).amax(-1), (cols * xs).amax(-1)
    y0, x0 = (rows * ys + h * ~rows).amin(-1), (cols * xs + w * ~cols).amin(-1)
    boxes = torch.stack([x0, y0, x1, y1], 1)
    return boxes * rows.any(-1, keepdim=True)


def aten_batch(logits, iou, p):
    if p['pred_iou_thresh'] > 0.0:
        keep = iou > p['pred_iou_thresh']
        logits, iou = logits[keep], iou[keep]                       # (a copy of the fp32 planes, and a synchronisation)
    t, off = p['mask_threshold'], p['stability_score_offset']
    hi = (logits > (t + off)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    lo = (logits > (t - off)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    stability = hi / lo
    if p['stability_score_thresh'] > 0.0:
        keep = stability >= p['stability_score_thresh']
        logits, iou, stability = logits[keep], iou[keep], stability[keep]
    masks = logits > t
    return masks, iou, stability, mask_boxes(masks)


def aten_nms(boxes, scores, thresh):
    """torchvision's CPU arithmetic: the pair matrix on the device, the greedy walk on the host"""
    order = torch.sort(scores, descending=True, stable=True).indices
    b = boxes[order].float()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0])).clamp(min=0)
    ih = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = iw * ih
    over = (inter / (area[:, None] + area[None, :] - inter)).double() > thresh
    over = over.cpu().numpy()                                        # (synchronises)
    removed, keep = [False] * len(order), []
    for r in range(len(order)):
        if not removed[r]:
            keep.append(r)
            for c in over[r, r + 1:].nonzero()[0]:
                removed[r + 1 + c] = True
    return order[torch.tensor(keep, dtype=torch.int64, device=order.device)]


def aten_frame(batches, p):
    parts = [aten_batch(logits, iou, p) for logits, iou in batches]
    masks, iou, stability, boxes = (torch.cat([part[i] for part in parts]) for i in range(4))
    keep = aten_nms(boxes, iou, p['box_nms_thresh'])
    return masks[keep], iou[keep], stability[keep], boxes[keep]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', type=int, default=16)
    ap.add_argument('--batch', type=int, default=192)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('proposal_filter_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    h, w = 1080, 1920
    p = PC.params()
    distinct = []
    for seed in range(4):                                            # the recipe's ramps, built on the device
        centres, radii, slopes, grid = PC.draw(h, w, args.batch, seed)
        logits = PC.ramps(h, w, centres, radii, slopes, device=dev)
        iou = torch.tensor(grid, dtype=torch.float32)
        distinct.append((logits, iou.to(dev)))
    batches = [distinct[i % 4] for i in range(args.batches)]
    flt = ProposalFilter(h, w, capacity=4096, **{k: v for k, v in p.items()})

    def fused_batches():
        flt.reset()
        for logits, iou in batches:
            flt.add(logits, iou)

    def fused_frame():
        fused_batches()
        return flt.finish()

    _, found = timed(fused_frame)                                    # warm-up of both, and the results side by side
    _, ref = timed(lambda: aten_frame(batches, p))
    same = (tuple(found.masks.shape) == tuple(ref[0].shape) and bool(torch.equal(found.masks, ref[0].to(torch.uint8)))
            and bool(torch.equal(found.iou_preds, ref[1])) and bool(torch.equal(found.stability, ref[2]))
            and found.boxes.tolist() == ref[3].tolist())
    live = sum(int((iou > p['pred_iou_thresh']).sum()) for _, iou in batches)
    stored = int(flt._state.host[1])
    least = (4 * live + 5 * stored) * h * w
    t_pass, t_fused, t_aten = [], [], []
    for _ in range(args.rounds):                                     # alternating rounds on the same inputs
        t_pass.append(timed(fused_batches)[0])
        flt.finish()
        t_fused.append(timed(fused_frame)[0])
        t_aten.append(timed(lambda: aten_frame(batches, p))[0])
    med = statistics.median(t_pass)
    f, r = statistics.median(t_fused), statistics.median(t_aten)
    name = torch.cuda.get_device_name(0)
    lines = [f'{name}; {args.batches} batches of {args.batch} planes at {h} x {w}: {live} live, {stored} stored, '
             f'{found.masks.shape[0]} kept after NMS; {args.rounds} alternating rounds',
             '',
             '| | ms, median (min, max) |', '|---|---|',
             f'| fused frame (batches, finish, host copy, gather) | {spread(t_fused)} |',
             f'| ATen frame | {spread(t_aten)} |',
             f'| ratio | {r / f:.1f}x |',
             f'| fused batch passes alone | {spread(t_pass)} |',
             f'| their least traffic | {least / 1e9:.1f} GB: {least / med / 1e6:.0f} GB/s, {least / med / 1e-3 / ROOF:.2f} of the 8 TB/s roof |',
             f'| same result | {"yes" if same else "NO"} |']
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
