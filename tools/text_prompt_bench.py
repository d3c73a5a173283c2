"""Box prompts of a text-prompted detection frame: (a) `ops.box_mask_select` (csrc/box_prompts.hip: one launch, only the
chosen planes are read) against the ATen statement `logits[arange(B), scores.argmax(1)] > t` on the same device, and
(b) the whole `detections.text_detections` call with its two host copies against the reference's lines
(grounding_dino.py:101-142) in ATen on the device, its per-box host round trips included.

    python tools/text_prompt_bench.py [--rounds 7] [--calls 50] [--out FILE.md]

(a) 1080 x 1920, M = 3 candidates, B = 16 boxes.  Kernel time by device events around `--calls` consecutive calls; the
two forms run in alternating rounds on the same tensors: median, minimum and maximum over the rounds.  The least traffic
of the selection is 5 bytes per pixel and box (4 read, 1 written); it is set against the 8 TB/s roof.  The ATen form
gathers the chosen planes (4 + 4 bytes) and compares them (4 + 1): 13 bytes at least.
(b) 900 raw boxes of which about 8 / 32 / 128 survive NMS, 1080p frames assembled at 480 x 853; both forms end with their
segments on the host, so a host clock around whole calls is the measure.  The segmenter is the same stand-in for both:
it hands out views of one preallocated block of logits (no work of its own), so the difference is the plumbing.  The
ATen baseline runs NMS on the host boxes with the CPU statement of tests/emu_text.py (torchvision, which the reference
calls there, is not installed here: the baseline's NMS time is therefore reported separately and NOT counted)."""
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

import emu_text as ET  # noqa: E402
from deva.hip import ops  # noqa: E402
from deva.inference import detections as D  # noqa: E402
from deva.inference.object_info import ObjectInfo  # noqa: E402

ROOF = 8e12
H, W, SIZE = 1080, 1920, (480, 853)


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


def host_us(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()                                                        # (ends with its segments on the host: synchronised)
    return (time.perf_counter() - t0) / calls * 1e6


# ------------------------------------------------------------------------------------------ (a)
def select_table(args, dev):
    b, m = 16, 3
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(b, m, H, W, generator=g).to(dev)
    scores = torch.rand(b, m, generator=g).to(dev)
    out = torch.empty((b, H, W), dtype=torch.uint8, device=dev)
    rows = torch.arange(b, device=dev)
    fused = lambda: ops.box_mask_select(logits, scores, 0.0, out=out)            # noqa: E731
    aten = lambda: logits[rows, scores.argmax(1)] > 0.0                          # noqa: E731
    same = bool(torch.equal(fused()[0], aten().to(torch.uint8)))
    t_fused, t_aten = [], []
    for _ in range(args.rounds):
        t_fused.append(event_us(fused, args.calls))
        t_aten.append(event_us(aten, args.calls))
    f, r = statistics.median(t_fused), statistics.median(t_aten)
    least = 5 * b * H * W
    slower = f - r > max(t_fused) - min(t_fused)
    return [f'(a) box_mask_select, {H} x {W}, M = {m}, B = {b}; {args.rounds} alternating rounds of {args.calls} calls, '
            'microseconds per call by device events, median (min, max)', '',
            '| form | per call | least traffic | rate | of the 8 TB/s roof | same planes |', '|---|---|---|---|---|---|',
            f'| box_mask_select | {spread(t_fused)} | {least / 1e6:.0f} MB (5 B / pixel and box) | {least / f / 1e3:.0f} GB/s | '
            f'{least / f * 1e6 / ROOF:.2f} | {"yes" if same else "NO"} |',
            f'| ATen gather + compare | {spread(t_aten)} | {13 * b * H * W / 1e6:.0f} MB (13 B) | {13 * b * H * W / r / 1e3:.0f} GB/s | '
            f'{13 * b * H * W / r * 1e6 / ROOF:.2f} | |',
            f'| ratio | {r / f:.2f}x{" -- SLOWER THAN ATen BEYOND THE SPREAD: a defect" if slower else ""} | | | | |', '']


# ------------------------------------------------------------------------------------------ (b)
def raw_boxes(kept, total=900, seed=0):
    """`kept` well-separated boxes on a grid over the frame, each with total / kept - 1 jittered copies of lower
    confidence that NMS at 0.8 removes"""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(kept * W / H)))
    rows = -(-kept // cols)
    cw, ch = W / cols, H / rows
    base = np.array([[(k % cols) * cw + 0.1 * cw, (k // cols) * ch + 0.1 * ch, (k % cols) * cw + 0.9 * cw, (k // cols) * ch + 0.9 * ch]
                     for k in range(kept)], dtype=np.float32)
    copies = np.repeat(base, -(-total // kept), axis=0)[:total - kept]
    copies = copies + rng.uniform(-0.01, 0.01, copies.shape).astype(np.float32) * np.float32(min(cw, ch))
    boxes = np.concatenate([base, copies]).astype(np.float32)
    conf = np.concatenate([rng.uniform(0.8, 0.9, kept), rng.uniform(0.35, 0.7, total - kept)]).astype(np.float32)
    order = rng.permutation(total)
    return boxes[order], conf[order], np.array([int(k) % 3 for k in order], dtype=object)


class BlockSegmenter:
    """hands out views of one preallocated block: logits fp32 [16,3,H,W] with a rectangle per plane, scores fp32 [16,3]"""
    mask_threshold = 0.0

    def __init__(self, dev):
        g = torch.Generator().manual_seed(2)
        self.logits = torch.full((16, 3, H, W), -4.0)
        for k in range(16):
            for m in range(3):
                y, x = int(torch.randint(0, H - 300, (1,), generator=g)), int(torch.randint(0, W - 400, (1,), generator=g))
                self.logits[k, m, y:y + 60 + 15 * k, x:x + 80 + 20 * k + 7 * m] = 4.0
        self.logits, self.scores = self.logits.to(dev), torch.rand(16, 3, generator=g).to(dev)

    def predict_boxes(self, boxes_px):
        n = boxes_px.shape[0]
        return self.logits[:n], self.scores[:n]

    def predict_box(self, j):
        """what kept box j gets inside a batch of 16, asked for alone (the reference asks box by box)"""
        return self.logits[j % 16:j % 16 + 1], self.scores[j % 16:j % 16 + 1]


def reference_lines(boxes, conf, classes, segmenter, keep, dev):
    """grounding_dino.py:105-142 in ATen on the device after the NMS: per box a predict, the thresholded planes and the
    scores to the host, np.argmax, a numpy mask; then per mask an upload, F.interpolate, a sum and a masked write"""
    boxes, conf, classes = boxes[keep], conf[keep], classes[keep]
    result_masks = []
    for j, box in enumerate(boxes):
        box_px = torch.from_numpy(box)[None].to(dev)        # (the upload of the box: SamPredictor.predict does one)
        logits, scores = segmenter.predict_box(j)
        masks, scores = (logits[0] > segmenter.mask_threshold).cpu().numpy(), scores[0].cpu().numpy()
        result_masks.append(masks[np.argmax(scores)])
    masks = np.array(result_masks)
    area = masks.reshape(len(masks), -1).sum(1)
    output_mask = torch.zeros(SIZE, dtype=torch.int64, device=dev)
    curr_id, segments_info = 1, []
    for i in np.flip(np.argsort(area, kind='stable')):
        mask = torch.from_numpy(masks[i].astype(np.float32)).to(dev)
        mask = F.interpolate(mask.unsqueeze(0).unsqueeze(0), SIZE, mode='bilinear')[0, 0]
        mask = (mask > 0.5).float()
        if mask.sum() > 0:
            output_mask[mask > 0] = curr_id
            segments_info.append(ObjectInfo(id=curr_id, category_id=classes[i], score=conf[i]))
            curr_id += 1
    return output_mask, segments_info


def frame_table(args, dev):
    segmenter = BlockSegmenter(dev)
    lines = [f'(b) text_detections, 900 raw boxes, {H} x {W} -> {SIZE[0]} x {SIZE[1]}; {args.rounds} alternating rounds, '
             'milliseconds per call by the host clock, median (min, max); the host NMS of the baseline is not counted', '',
             '| kept | text_detections | reference lines in ATen | ratio | host NMS (not counted) | same mask and segments |',
             '|---|---|---|---|---|---|']
    for kept in (8, 32, 128):
        boxes, conf, classes = raw_boxes(kept)
        t0 = time.perf_counter()
        keep = ET.nms_xyxy(boxes, conf, 0.8)
        t_nms = (time.perf_counter() - t0) * 1e3
        fused = lambda: D.text_detections(boxes, conf, classes, segmenter, (H, W), SIZE, nms_threshold=0.8, device=dev)   # noqa: E731
        aten = lambda: reference_lines(boxes, conf, classes, segmenter, keep, dev)                                        # noqa: E731
        (ma, ia), (mb, ib) = fused(), aten()
        same = bool(torch.equal(ma, mb)) and [(o.id, o.category_ids, o.scores) for o in ia] == [(o.id, o.category_ids, o.scores) for o in ib]
        calls = max(1, args.calls // max(kept // 4, 1))
        t_fused, t_aten = [], []
        for _ in range(args.rounds):
            t_fused.append(host_us(fused, calls) / 1e3)
            t_aten.append(host_us(aten, calls) / 1e3)
        f, r = statistics.median(t_fused), statistics.median(t_aten)
        lines.append(f'| {len(keep)} | {spread(t_fused, 2)} | {spread(t_aten, 2)} | {r / f:.1f}x | {t_nms:.0f} ms | '
                     f'{"yes" if same else "NO"} |')
    return lines + ['']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('text_prompt_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    lines = [torch.cuda.get_device_name(0), ''] + select_table(args, dev) + frame_table(args, dev)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
