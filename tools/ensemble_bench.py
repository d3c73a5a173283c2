#!/usr/bin/env python
"""Test-time ensemble timings on one GPU: 1080p frames, network input 480p, 5 objects, K = 2, 4 and 6 variants.
    python tools/ensemble_bench.py [--rounds 7] [--frames 10] [--out FILE.json]

(a) the output tail alone -- `ops.ensemble_index_mask` (one launch) against the same merge written with ATen
    (F.interpolate, flip, * 255, .to(uint8), sum, argmax, lut[...]) on the same K probability tensors;
(b) a whole frame -- `EnsembleInferenceCore.step` against K sequential `DEVAInferenceCore.step` calls (device input
    head per variant, torch.flip for the mirrored ones) followed by that ATen merge.

Each pair is timed with device events after a warm-up of every shape, in alternating windows (new, old, new, old, ...)
of --frames frames; the figure is the median window, per frame.  Both sides of (b) see the same frames in the same
order from the same annotated start, and the two masks of (a) are compared before timing."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
from workload import synth  # noqa: E402

H, W, OBJECTS = 1080, 1920, 5
SIZES = {2: (480,), 4: (480, 540), 6: (480, 540, 600)}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def aten_merge(probs, flips, size, lut):
    """the reference protocol with ATen: eval_vos.py:170-177,188-189 per run, merge_multi_scale.py:44-66 over the runs"""
    total = None
    for p, flip in zip(probs, flips):
        if tuple(p.shape[-2:]) != tuple(size):
            p = F.interpolate(p.unsqueeze(1), size, mode='bilinear', align_corners=False)[:, 0]
        if flip:
            p = torch.flip(p, dims=[-1])
        q = (p * 255).to(torch.uint8)
        total = q.float() if total is None else total + q
    return lut[torch.argmax(total, dim=0)]


def timed(fn, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(n):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n


def alternate(new, old, rounds, n):
    """-> (median ms per call of new, of old) over alternating windows"""
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(new, n))
        b.append(timed(old, n))
    return statistics.median(a), statistics.median(b)


def u8_frames(n, device):
    mean, std = (torch.tensor(v, device=device).view(3, 1, 1) for v in (MEAN, STD))
    return [((f * std + mean).clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
            for f in bench.make_clip(H, W, n, seed=7, device=device)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ensemble_bench: needs a HIP device (timings on a CPU say nothing about the GPU)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    from deva.hip import ops
    from deva.inference.ensemble import EnsembleInferenceCore
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.utils.tensor_utils import frame_to_network_input, network_input_size, unpad

    net, _ = bench.build_network(dev)
    cfg = synth.base_config(enable_long_term=False, enable_long_term_count_usage=False)
    frames = u8_frames(args.frames, dev)
    mask0 = synth.box_mask(H, W, OBJECTS).to(dev)
    objects = list(range(1, OBJECTS + 1))
    results = []
    for k, sizes in SIZES.items():
        variants = [(s, f) for s in sizes for f in (False, True)]
        flips = [f for _, f in variants]

        # ---- (a) the tail alone, on soft-max probabilities of the variants' shapes
        g = torch.Generator().manual_seed(k)
        probs = [torch.softmax(torch.randn(OBJECTS + 1, *network_input_size(H, W, s), generator=g) * 2, dim=0).to(dev)
                 for s, _ in variants]
        lut = torch.arange(OBJECTS + 1, device=dev)
        new, old = ops.ensemble_index_mask(probs, (H, W), flips, lut), aten_merge(probs, flips, (H, W), lut)
        differ = int((new != old).sum())  # (bytes at a rounding boundary of the resize may move a label)
        for _ in range(3):
            ops.ensemble_index_mask(probs, (H, W), flips, lut)
            aten_merge(probs, flips, (H, W), lut)
        tail_new, tail_old = alternate(lambda i: ops.ensemble_index_mask(probs, (H, W), flips, lut),
                                       lambda i: aten_merge(probs, flips, (H, W), lut), args.rounds, 20)

        # ---- (b) whole frames from the same annotated start
        ens = EnsembleInferenceCore(net, cfg, sizes=sizes, flips=(False, True))
        ens.step(frames[0], mask0, objects)
        cores = [DEVAInferenceCore(net, cfg) for _ in variants]

        def sequential(i, mask=None, objs=None):
            frame = frames[i % len(frames)]
            outs = []
            for core, (size, flip) in zip(cores, variants):
                image, pad = frame_to_network_input(torch.flip(frame, dims=[1]) if flip else frame, size, pad_to=16)
                m = mask
                if m is not None:
                    oh, ow = network_input_size(H, W, size)
                    m = F.interpolate(m[None, None].double(), (oh, ow), mode='nearest')[0, 0].long()
                    m = torch.flip(m, dims=[-1]) if flip else m
                outs.append(unpad(core.step(image, m, objs), pad))
            return aten_merge(outs, flips, (H, W), cores[0].object_manager._tmp_to_obj_table(dev))

        sequential(0, mask0, objects)
        for i in range(1, 4):  # warm-up: every shape of both paths, one memory frame included
            ens.step(frames[i % len(frames)])
            sequential(i)
        step_new, step_old = alternate(lambda i: ens.step(frames[i % len(frames)]), sequential, args.rounds, args.frames)
        row = dict(k=k, sizes=list(sizes), tail_fused_ms=tail_new, tail_aten_ms=tail_old, tail_labels_differing=differ,
                   step_ensemble_ms=step_new, step_sequential_ms=step_old)
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(frame=[H, W], objects=OBJECTS, rounds=args.rounds, frames=args.frames, results=results), f, indent=1)


if __name__ == '__main__':
    main()
