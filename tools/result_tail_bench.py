#!/usr/bin/env python
"""Per-frame result tail timings on one GPU: 1080p output from 480p-input probabilities, 5 and 14 objects.
    python tools/result_tail_bench.py [--rounds 7] [--frames 10] [--out FILE.json]

(a) the device part alone -- `ops.frame_result` (index, stats, colour image, overlay) + `ops.mask_rle` against
    `ops.index_mask` followed by the same products written with ATen on the device (table gathers, bincount,
    scatter_reduce for the boxes, integer overlay, one sort of the label changes for the run boundaries);
(b) a whole saver frame, `save_mask` until the queue is drained -- `FrameResultSaver` against a restatement of the
    reference tail (result_utils.py:98-242: argmax -> .cpu() of the int64 mask -> per-object remap / area / paint /
    float blend in torch / numpy on a worker thread behind the same Queue(maxsize=10)), for `demo` (RGB id image +
    overlay + areas) and `burst` (gray plane + run-length codes).  pycocotools is not installed here, so the
    restatement codes its runs with the same loop-free numpy encoder the package uses; the reference's C encoder
    would be faster than numpy on that one step.  Image files are not written by default on either side (the PNG /
    JPEG codecs are the same PIL calls on both and dwarf everything else); --files adds a row with them.
(c) the device-to-host bytes per frame of both, counted from the shapes.

Host clock around windows that end in a synchronise (both sides of (a) read a count back; (b) is host work), after a
warm-up of every shape, in alternating windows (new, old, new, old, ...); the figures are the median window per frame
and the spread (min .. max).  The two sides' outputs are compared before timing."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from queue import Queue
from threading import Thread

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H, W, IN_H, IN_W = 1080, 1920, 480, 864
OBJECT_COUNTS = (5, 14)


def blob_probabilities(n_obj, frames, device):
    """soft-max of smooth seeded logits: blob-shaped objects, as a tracker's output has (noise would make millions of runs)"""
    g = torch.Generator().manual_seed(n_obj)
    out = []
    for _ in range(frames):
        coarse = torch.randn(1, n_obj + 1, 9, 16, generator=g) * 4
        out.append(torch.softmax(F.interpolate(coarse, (IN_H, IN_W), mode='bicubic', align_corners=False)[0], dim=0)
                   .contiguous().to(device))
    return out


def aten_products(ops, prob, lut, colors, image):
    """the products of `frame_result` + `mask_rle` with ATen, downstream of ops.index_mask"""
    c = prob.shape[0]
    idx = ops.index_mask(prob, (H, W))
    flat = idx.view(-1)
    labels = lut[idx]
    area = torch.bincount(flat, minlength=c)
    ys = torch.arange(H, device=idx.device).view(H, 1).expand(H, W).reshape(-1)
    xs = torch.arange(W, device=idx.device).view(1, W).expand(H, W).reshape(-1)
    big = torch.full((c,), 2**31 - 1, device=idx.device)
    small = torch.full((c,), -1, device=idx.device)
    stats = torch.stack([area, big.scatter_reduce(0, flat, xs, 'amin'), big.scatter_reduce(0, flat, ys, 'amin'),
                         small.scatter_reduce(0, flat, xs, 'amax'), small.scatter_reduce(0, flat, ys, 'amax')], dim=1).int()
    color = colors[idx]
    half = ((image.to(torch.int16) + color.to(torch.int16)) >> 1).to(torch.uint8)
    blend = torch.where((labels == 0).unsqueeze(-1), image, half)
    col = idx.t().reshape(-1)                                   # p = x*H + y
    prev = torch.cat([col.new_zeros(1), col[:-1]])
    p = torch.nonzero(col != prev).view(-1)
    key = torch.cat([prev[p], col[p]])
    pos = torch.cat([p, p])
    keep = key >= 1
    key, pos = key[keep], pos[keep]
    order = torch.argsort(key * (H * W) + pos)
    n = torch.bincount(key, minlength=c).int().cpu()
    return dict(index=idx.to(torch.int16), labels=labels, stats=stats, color=color, blend=blend, n=n,
                bounds=pos[order].int())


def fused_products(ops, prob, lut, colors, image):
    res = ops.frame_result(prob, (H, W), lut, color_lut=colors, image=image,
                           want=('index', 'labels', 'stats', 'color', 'blend'))
    n, bounds = ops.mask_rle(res.index, prob.shape[0])
    return dict(index=res.index, labels=res.labels, stats=res.stats, color=res.color, blend=res.blend, n=n, bounds=bounds)


class ReferenceTail:
    """result_utils.py:88-285 restated on the public pieces (no prompts, no file codecs unless `files`)"""

    def __init__(self, root, dataset, object_manager, files, decide='aten'):
        from deva.inference.frame_results import coco_strings, long_id_colors
        self.root, self.dataset, self.om, self.files, self.decide = root, dataset, object_manager, files, decide
        self.coco_strings, self.colors = coco_strings, long_id_colors
        self.annotations, self.last = [], None
        self.queue = Queue(maxsize=10)
        self.thread = Thread(target=self._work, daemon=True)
        self.thread.start()

    def save_mask(self, prob, frame_name, shape, image_np):
        import copy
        if self.decide == 'aten':
            prob = F.interpolate(prob.unsqueeze(1), shape, mode='bilinear', align_corners=False)[:, 0]
            mask = torch.argmax(prob, dim=0)
        else:   # the comparison run: the package's decision, so that a near-tie label cannot make the outputs differ
            from deva.hip import ops
            mask = ops.index_mask(prob, shape)
        self.queue.put((mask.cpu(), frame_name, image_np, copy.deepcopy(self.om.tmp_id_to_obj),
                        copy.deepcopy(self.om.get_current_segments_info()), list(self.om.all_obj_ids)))

    def end(self):
        self.queue.put(None)
        self.queue.join()
        self.thread.join()

    def _rle(self, m):
        flat = np.asfortranarray(m.numpy()).reshape(-1, order='F')
        change = np.nonzero(np.diff(np.concatenate([[False], flat, [not flat[-1]]]).astype(np.int8)))[0]
        counts = np.diff(np.concatenate([[0], change]))      # (the last change is the end of the frame)
        return {'size': list(m.shape), 'counts': self.coco_strings(counts, np.array([len(counts)]))[0]}

    def _work(self):
        from PIL import Image
        while True:
            item = self.queue.get()
            if item is None:
                self.queue.task_done()
                return
            mask, frame_name, image_np, tmp_id_to_obj, segments, all_ids = item
            new_mask = torch.zeros_like(mask)
            for tmp_id, obj in tmp_id_to_obj.items():
                new_mask[mask == tmp_id] = obj.id
            mask = new_mask
            if self.dataset == 'burst':
                for seg in segments:
                    seg['mask'] = mask == seg['id']
                    seg['area'] = int(seg['mask'].sum())
                    seg['rle_mask'] = self._rle(seg['mask'])
                segments = [s for s in segments if s['area'] > 0]
                self.annotations.append({'file_name': frame_name[:-4] + '.jpg', 'segmentations': [
                    {'id': s['id'], 'score': s['score'], 'rle': s['rle_mask']} for s in segments]})
                out = mask.numpy().astype(np.uint8)
                planes = {'gray': out}
            else:
                for seg in segments:
                    seg['area'] = int((mask == seg['id']).sum())
                segments = [s for s in segments if s['area'] > 0]
                self.annotations.append({'file_name': frame_name[:-4] + '.jpg', 'segments_info': segments})
                out_mask = mask.numpy().astype(np.uint32)
                rgb = np.zeros((*out_mask.shape, 3), dtype=np.uint8)
                for i in all_ids:
                    rgb[out_mask == i] = self.colors([i])[0]
                alpha = ((out_mask == 0).astype(np.float32) * 0.5 + 0.5)[:, :, None]
                planes = {'color': rgb, 'blend': (image_np * alpha + rgb * (1 - alpha)).astype(np.uint8)}
            if self.files:
                for k, a in planes.items():
                    Image.fromarray(a).save(os.path.join(self.root, frame_name[:-4] + ('.jpg' if k == 'blend' else '.png')))
            self.last = planes
            self.queue.task_done()


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def alternate(new, old, rounds, n):
    a, b = [], []
    for _ in range(rounds):
        a.append(window(new, n))
        b.append(window(old, n))
    return dict(new_ms=statistics.median(a), new_min=min(a), new_max=max(a),
                old_ms=statistics.median(b), old_min=min(b), old_max=max(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--files', action='store_true', help='also time (b) with the PNG / JPEG files written on both sides')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('result_tail_bench: needs a HIP device (timings on a CPU say nothing about the GPU)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    from deva.hip import ops
    from deva.inference import frame_results as FR
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager

    g = torch.Generator().manual_seed(3)
    images_np = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).numpy() for _ in range(args.frames)]
    results = []
    for n_obj in OBJECT_COUNTS:
        probs = blob_probabilities(n_obj, args.frames, dev)
        om = ObjectManager()
        om.use_long_id = True
        om.add_new_objects([ObjectInfo(id=1000 + 70001 * i, category_id=i % 3, score=0.5) for i in range(n_obj)])
        lut = om._tmp_to_obj_table(dev)
        colors = torch.from_numpy(FR.long_id_colors(lut.cpu().numpy())).to(dev)
        images = [torch.from_numpy(a).to(dev) for a in images_np]

        # ---- (a) device part
        new, old = fused_products(ops, probs[0], lut, colors, images[0]), aten_products(ops, probs[0], lut, colors, images[0])
        for k in new:
            assert torch.equal(new[k].cpu(), old[k].cpu()), f'(a) {k} differs between the fused tail and ATen'
        runs = int(new['n'].sum())
        for i in range(min(3, args.frames)):
            fused_products(ops, probs[i], lut, colors, images[i])
            aten_products(ops, probs[i], lut, colors, images[i])
        row = dict(objects=n_obj, runs_frame0=runs)
        row['device'] = alternate(lambda i: fused_products(ops, probs[i % args.frames], lut, colors, images[i % args.frames]),
                                  lambda i: aten_products(ops, probs[i % args.frames], lut, colors, images[i % args.frames]),
                                  args.rounds, args.frames)
        only = alternate(lambda i: ops.frame_result(probs[i % args.frames], (H, W), lut, want=('labels',)),
                         lambda i: ops.index_mask(probs[i % args.frames], (H, W), lut), args.rounds, args.frames)
        row['labels_only'] = only                                # (frame_result asked for labels alone vs index_mask)
        full = alternate(lambda i: ops.frame_result(probs[i % args.frames], (H, W), lut, color_lut=colors,
                                                    image=images[i % args.frames],
                                                    want=('index', 'labels', 'stats', 'color', 'blend')),
                         lambda i: ops.mask_rle(new['index'], n_obj + 1), args.rounds, args.frames)
        row['frame_result_ms'], row['mask_rle_ms'] = full['new_ms'], full['old_ms']
        # what the column-major read costs: a transposition of the int16 plane (ATen's, of the same 4 MB in and out as
        # the LDS-tile kernel inside mask_rle) -- the most a column-major copy written by frame_result could save
        row['transpose_ms'] = alternate(lambda i: new['index'].t().contiguous(), lambda i: None, args.rounds, 50)['new_ms']

        # ---- (b) whole saver frames, (c) bytes
        for dataset in ('demo', 'burst'):
            om.use_long_id = dataset == 'demo'
            for files in ([False, True] if args.files else [False]):
                with tempfile.TemporaryDirectory() as root:
                    class Saver(FR.FrameResultSaver):
                        def _save_image(self, img, where):
                            self.last = getattr(self, 'last', {})
                            self.last[where[-4:]] = np.array(img)
                            if files:
                                img.save(where)

                    def run_new(count):
                        s = Saver(root, 'new', dataset=dataset, object_manager=om)
                        for i in range(count):
                            s.save_mask(probs[i % args.frames], f'{i:05d}.jpg', True, (H, W), image_np=images_np[i % args.frames])
                        s.end()
                        return s

                    def run_old(count, decide='aten'):
                        s = ReferenceTail(root, dataset, om, files, decide)
                        for i in range(count):
                            s.save_mask(probs[i % args.frames], f'{i:05d}.jpg', (H, W), images_np[i % args.frames])
                        s.end()
                        return s

                    a, b = run_new(2), run_old(2, 'kernel')
                    run_old(2)                                   # (warm-up of the ATen resize)
                    assert json.dumps(a.video_json[('annotations', 'segmentations')[dataset == 'burst']]) == \
                        json.dumps(b.annotations), f'(b) {dataset}: annotations differ'
                    if dataset == 'demo':
                        assert np.array_equal(a.last['.png'], b.last['color']) and np.array_equal(a.last['.jpg'], b.last['blend'])
                    else:
                        assert np.array_equal(a.last['.png'], b.last['gray'])
                    ws_new, ws_old = [], []
                    for _ in range(args.rounds):
                        torch.cuda.synchronize(); t0 = time.perf_counter(); run_new(args.frames)
                        ws_new.append((time.perf_counter() - t0) * 1e3 / args.frames)
                        torch.cuda.synchronize(); t0 = time.perf_counter(); run_old(args.frames)
                        ws_old.append((time.perf_counter() - t0) * 1e3 / args.frames)
                    t = dict(new_ms=statistics.median(ws_new), new_min=min(ws_new), new_max=max(ws_new),
                             old_ms=statistics.median(ws_old), old_min=min(ws_old), old_max=max(ws_old))
                    row[f'saver_{dataset}' + ('_files' if files else '')] = t
            c = n_obj + 1
            new_bytes = (6 * H * W if dataset == 'demo' else H * W + 4 * runs + 4 * c) + 20 * c
            row[f'd2h_{dataset}'] = dict(new_bytes=new_bytes, old_bytes=8 * H * W)
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(frame=[H, W], input=[IN_H, IN_W], rounds=args.rounds, frames=args.frames, results=results), f, indent=1)


if __name__ == '__main__':
    main()
