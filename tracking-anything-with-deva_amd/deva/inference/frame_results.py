"""Per-frame results from the device (not part of the reference's interface; the reference's own saver,
deva/inference/result_utils.py, stays what `deva.inference.result_utils` resolves to).

The reference's `ResultSaver` copies an int64 H*W mask to the host and then makes, per frame and per object, full-frame
passes for the id remap, the area, the run-length code, the RGB id image and the overlay (result_utils.py:98-242).  Here
`ops.frame_result` produces all of that in one pass over the probabilities and `ops.mask_rle` the COCO run boundaries of
every object; the host receives the byte planes it has to write, a [C,5] table and the boundaries, and only turns the
boundaries into COCO strings (vectorised, no loop over runs) and writes the files.

`ObjectManager.frame_result` is the one-call form; `FrameResultSaver` has the reference saver's interface (minus the
`prompts` of its box drawing, which needs `supervision`; the boxes are in the `FrameResult`) and writes the same PNG /
JPG paths and the same `video_json` structures."""
import os
from dataclasses import dataclass, field
from os import path
from queue import Queue
from threading import Thread
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from deva.hip import jpeg as jpeg_coder, ops, png as png_coder, rle

# ------------------------------------------------------------------------------------------ colours
def long_id_colors(ids: Sequence[int]) -> np.ndarray:
    """ID2RGBConverter._id_to_rgb (pano_utils.py:23-28) for a list of ids -> uint8 [n,3]"""
    ids = np.asarray(ids, dtype=np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536 % 256], axis=1).astype(np.uint8)


# ------------------------------------------------------------------------------------------ COCO strings
def coco_strings(counts: np.ndarray, lengths: np.ndarray) -> List[str]:
    """several objects' COCO run lengths, back to back in `counts` with `lengths[k]` of them for object k -> their
    compressed strings (the COCO API's rleToString): from an object's fourth count on the difference to the count two
    places back is coded; 5 bits per character, low bits first, 0x20 marks a continuation, the code of a value ends
    when the rest is 0 with bit 0x10 clear or -1 with bit 0x10 set; 48 is added to every character.  Vectorised over
    all counts: one numpy step per character position (13 cover 64 bits), no loop over runs."""
    counts = np.asarray(counts, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert int(lengths.sum()) == counts.size
    if counts.size == 0:
        return ['' for _ in lengths]
    starts = np.cumsum(lengths) - lengths
    local = np.arange(counts.size) - np.repeat(starts, lengths)
    x = counts.copy()
    late = local > 2
    x[late] -= counts[np.nonzero(late)[0] - 2]
    chars = np.zeros((counts.size, 13), dtype=np.uint8)
    used = np.zeros((counts.size, 13), dtype=bool)
    active = np.ones(counts.size, dtype=bool)
    for k in range(13):
        c = x & 0x1f
        x = x >> 5
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        chars[:, k] = (c | (more.astype(np.int64) << 5)) + 48
        used[:, k] = active
        active = active & more
        if not active.any():
            break
    text = chars[used].tobytes().decode('ascii')
    per_object = np.add.reduceat(used.sum(axis=1), np.minimum(starts, counts.size - 1))
    per_object[lengths == 0] = 0
    ends = np.cumsum(per_object)
    return [text[e - n:e] for e, n in zip(ends.tolist(), per_object.tolist())]


def rle_counts(n: np.ndarray, bounds: np.ndarray, total: int) -> Tuple[np.ndarray, np.ndarray]:
    """`ops.mask_rle`'s (n, bounds) -> (counts of the channels 1.. back to back, their lengths n[c] + 1):
    counts_c = diff([0, *bounds_c, total])"""
    m = np.asarray(n, dtype=np.int64)[1:]
    bounds = np.asarray(bounds, dtype=np.int64)
    if m.size == 0:
        return np.zeros(0, dtype=np.int64), m
    first = np.cumsum(m + 2) - (m + 2)            # where each channel's [0, *bounds_c, total] starts
    last = first + m + 1
    ext = np.empty(int((m + 2).sum()), dtype=np.int64)
    inner = np.ones(ext.size, dtype=bool)
    inner[first], inner[last] = False, False
    ext[first], ext[last], ext[inner] = 0, total, bounds
    keep = np.ones(ext.size - 1, dtype=bool)
    keep[last[:-1]] = False                        # (differences across two channels)
    return np.diff(ext)[keep], m + 1


def rle_strings(n: np.ndarray, bounds: np.ndarray, total: int) -> List[Optional[str]]:
    """-> the COCO `counts` string of every channel (entry 0, the background, is None)"""
    counts, lengths = rle_counts(n, bounds, total)
    return [None] + coco_strings(counts, lengths)


# ------------------------------------------------------------------------------------------ one frame
@dataclass
class FrameResult:
    """what one frame gives: planes still on the device (None when not asked for) and host-side records, one per
    object of `ObjectManager.get_current_segments_info()` in its order: id, category_id, score, area, bbox (xyxy in
    inclusive pixel coordinates as torchvision.ops.masks_to_boxes gives them, None for area 0) and, with rle=True,
    rle = {'size': [H, W], 'counts': str}"""
    size: Tuple[int, int]
    segments: List[Dict]
    labels: Optional[torch.Tensor] = None    # int64 [H,W] object ids
    gray: Optional[torch.Tensor] = None      # uint8 [H,W] object id & 0xff (short ids: the palette-PNG plane)
    color: Optional[torch.Tensor] = None     # uint8 [H,W,3] id image (long ids) or palette colours
    blend: Optional[torch.Tensor] = None     # uint8 [H,W,3] overlay on the frame
    index: Optional[torch.Tensor] = None     # int16 [H,W] channel (tmp id) plane
    host: Dict[str, np.ndarray] = field(default_factory=dict)   # planes the caller asked to be copied to the host
    channel_ids: Optional[np.ndarray] = None  # int64 [C] the id that each channel of `index` was given in this frame


def _to_host(t: torch.Tensor) -> torch.Tensor:
    """start the copy of a device tensor into a pinned buffer on the current stream (a host tensor is returned as is)"""
    if not t.is_cuda:
        return t
    buf = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    buf.copy_(t, non_blocking=True)
    return buf


class PendingFrame:
    """a frame whose kernels and device-to-host copies are in flight; `finish()` waits for them and builds the records"""

    def __init__(self, size, products, segments, tmp_ids, host_stats, n, host_bounds, host_planes, event):
        self.size, self.products, self.segments, self.tmp_ids = size, products, segments, tmp_ids
        self.host_stats, self.n, self.host_bounds, self.host_planes, self.event = host_stats, n, host_bounds, host_planes, event
        self.channel_ids = None
        self.png = None          # a `deva.hip.png.PendingPng` when the saver codes the PNG on the device
        self.jpeg = None         # a `deva.hip.jpeg.PendingJpeg` when the saver codes the overlay JPEG on the device

    def finish(self) -> FrameResult:
        if self.event is not None:
            self.event.synchronize()
        stats = self.host_stats.numpy()
        h, w = self.size
        texts = None if self.n is None else rle_strings(self.n.numpy(), self.host_bounds.numpy(), h * w)
        records = []
        for seg, tmp in zip(self.segments, self.tmp_ids):
            area, x0, y0, x1, y1 = (int(v) for v in stats[tmp]) if tmp < len(stats) else (0, 0, 0, -1, -1)
            rec = dict(seg, area=area, bbox=[float(x0), float(y0), float(x1), float(y1)] if area > 0 else None)
            if texts is not None:   # (an object without a channel in `prob` is absent: one run of zeros)
                rec['rle'] = {'size': [h, w], 'counts': texts[tmp] if tmp < len(texts) else coco_strings([h * w], [1])[0]}
            records.append(rec)
        p = self.products
        return FrameResult(size=self.size, segments=records, labels=p.labels, gray=p.gray, color=p.color, blend=p.blend,
                           index=p.index, host={k: v.numpy() for k, v in self.host_planes.items()},
                           channel_ids=self.channel_ids)


def launch_frame(object_manager, prob: torch.Tensor, size=None, *, image=None, rle: bool = False, color=None,
                 labels: bool = False, remap: bool = True, planes: Optional[Sequence[str]] = None,
                 host: Sequence[str] = (), id_map: Optional[Dict[int, int]] = None, index: bool = False) -> PendingFrame:
    """start one frame's result on the current stream.  `color`: None = the object manager's mode (long ids: the RGB
    id image; short ids: the gray id plane), 'id' = the long-id image, 'gray', or a uint8 [K,3] palette indexed by
    id % K.  `image` (uint8 [H,W,3], numpy or tensor) adds the overlay.  `planes` overrides which of gray / color / blend
    are produced, `host` names the planes whose copy to pinned host memory is started as well.  The object table is
    read now: later changes to it do not reach this frame.  `id_map` (object id -> id to write) replaces the ids of the
    table and of the colours for this frame (the stuff merging of a VIPSeg run); `index` keeps the channel plane."""
    prob = prob.contiguous()
    c = prob.shape[0]
    oh, ow = tuple(prob.shape[-2:]) if size is None else (int(size[0]), int(size[1]))
    device = prob.device
    table = object_manager._tmp_to_obj_table(device) if remap else None
    ids = np.arange(c, dtype=np.int64)
    if remap:
        ids = np.zeros(c, dtype=np.int64)
        for tmp, obj in object_manager.tmp_id_to_obj.items():
            if tmp < c:
                ids[tmp] = int(obj.id) if id_map is None else int(id_map.get(int(obj.id), obj.id))
        if id_map is not None:
            table = torch.from_numpy(ids).to(device)
    if color is None:
        color = 'id' if object_manager.use_long_id else 'gray'
    if isinstance(color, str):
        if color not in ('id', 'gray'):
            raise ValueError(f"color: None, 'id', 'gray' or a [K,3] palette (got {color!r})")
        colors = long_id_colors(ids)
    else:
        palette = np.asarray(color, dtype=np.uint8).reshape(-1, 3)
        colors = palette[ids % len(palette)]
        color = 'id'
    if planes is None:
        planes = (['gray'] if color == 'gray' else ['color']) + (['blend'] if image is not None else [])
    want = list(planes) + ['stats'] + (['index'] if rle or index else []) + (['labels'] if labels else [])
    color_lut = torch.from_numpy(colors).to(device) if ('color' in want or 'blend' in want) else None
    if 'blend' in want:
        if image is None:
            raise ValueError('the overlay needs the frame (image)')
        image = torch.as_tensor(np.ascontiguousarray(image) if isinstance(image, np.ndarray) else image).to(device)
    products = ops.frame_result(prob, None if size is None else (oh, ow), table, color_lut=color_lut,
                                image=image if 'blend' in want else None, want=want)
    n = host_bounds = None
    if rle:
        n, bounds = ops.mask_rle(products.index, c)
        host_bounds = _to_host(bounds)
    host_stats = _to_host(products.stats)
    host_planes = {k: _to_host(getattr(products, k)) for k in host}
    event = None
    if prob.is_cuda:
        event = torch.cuda.Event()
        event.record()
    segments = object_manager.get_current_segments_info()      # fresh dicts of plain values: a snapshot
    tmp_ids = [tmp for _, tmp in object_manager.obj_to_tmp_id.items()]
    pending = PendingFrame((oh, ow), products, segments, tmp_ids, host_stats, n, host_bounds, host_planes, event)
    pending.channel_ids = ids
    return pending


# ------------------------------------------------------------------------------------------ reading a video_json back
def read_video_json(video_json, size: Optional[Tuple[int, int]] = None, *, dtype=torch.uint8, device=None):
    """the `video_json` that `FrameResultSaver(dataset='burst')` builds (the dict, or the path of a JSON file that holds
    it) -> per frame (file_name, ids, scores, planes): the segments' ids and scores as lists in file order and their masks
    as planes [n,H,W] on the device (`deva.hip.rle.decode`: uint8 0 / 1, or float32), `planes[k]` being `labels == ids[k]`
    of the frame as it was saved.  `size` resizes on the way (nearest, fused into the decode).  A frame without segments
    gives planes of [0,H,W] at the size of the last frame that had any (or `size`; [0,0,0] before either is known)."""
    if not isinstance(video_json, dict):
        import json
        with open(video_json) as f:
            video_json = json.load(f)
    known = None if size is None else (int(size[0]), int(size[1]))
    for frame in video_json['segmentations']:
        segments = frame['segmentations']
        if segments:
            planes = rle.decode([s['rle'] for s in segments], size, dtype=dtype, device=device)
            known = tuple(planes.shape[-2:])
        else:
            planes = torch.zeros((0,) + (known or (0, 0)), dtype=dtype, device=torch.device('cuda' if device is None else device))
        yield frame['file_name'], [s['id'] for s in segments], [s['score'] for s in segments], planes


# ------------------------------------------------------------------------------------------ saver
class FrameResultSaver:
    """`ResultSaver` (result_utils.py:22-123) on the fused tail: the same constructor, `save_mask` (without `prompts`)
    and `end`, the same files and the same `video_json` / `all_annotations`.  `save_mask` launches the frame's kernels
    on the caller's stream, starts the copies of what the dataset needs into pinned memory and hands them to a worker
    thread, which waits for the copies, builds the annotation and writes the files with PIL.

    `id_postprocessor` (dataset 'vipseg' only; None: nothing changes) is a `panoptic_quality.StuffMerger`: the id table
    and the colour table of every frame then carry the merged ids and the merged areas are sums of the channel areas, so
    the PNG and the `video_json` are what the reference's merge_stuff would have written from the unmerged output,
    without reading a plane twice or re-writing a file.  `frame_hook(frame_name, result, annotation)` is called by the
    worker after a frame's files are written, with the `FrameResult` (its `index` plane and `channel_ids` included) and
    the annotation just appended: where an online scorer is fed.

    `png='host'` (the default) is the above.  With `png='device'` the PNG's plane (`gray` or `color`) is not copied to
    the host: `deva.hip.png.encode` codes its zlib stream on the caller's stream (include/deva_png.h) with a capacity
    that adapts -- 64 KB at first, then twice the largest stream seen; a longer stream is copied a second time at its
    exact size -- and the worker wraps the copied stream into the file (chunks and CRCs on the host) and writes the bytes
    to the same path.  The file decodes to the same pixels and palette; its bytes are not PIL's and it is two to four
    times as large.  `FrameResult.host` then lacks the PNG's plane.

    `jpeg='host'` (the default): PIL codes the `blend` overlay of the `demo` dataset on the worker.  With `jpeg='device'`
    `blend` is not copied to the host either: `deva.hip.jpeg.encode` codes the entropy-coded data of a baseline JPEG
    (quality 75, 4:2:0, a restart interval per MCU row: include/deva_jpeg.h) on the caller's stream, with a capacity that
    adapts like the PNG's -- 256 KB at first -- and the worker puts the markers around the copied data and writes the bytes
    to the same `Visualizations/.../NAME.jpg`.  The file is not PIL's bytes: it decodes to within a few hundredths of a
    dB of PIL's file at a size within a few percent.  The two options are independent of each other."""

    PNG_FIRST_CAPACITY = 65536
    JPEG_FIRST_CAPACITY = 262144

    def __init__(self, output_root: str, video_name: str, *, dataset: str, object_manager, palette=None,
                 id_postprocessor=None, frame_hook=None, png: str = 'host', jpeg: str = 'host'):
        self.output_root = output_root
        self.video_name = video_name
        self.dataset = dataset.lower()
        self.palette = palette
        self.object_manager = object_manager
        self.id_postprocessor = id_postprocessor
        self.frame_hook = frame_hook
        if id_postprocessor is not None and self.dataset != 'vipseg':
            raise ValueError("id_postprocessor: the stuff merging belongs to dataset 'vipseg'")
        if png not in ('host', 'device'):
            raise ValueError(f"png: 'host' or 'device' (got {png!r})")
        self.png = png
        self.png_capacity = self.PNG_FIRST_CAPACITY
        self.png_largest = 0
        if jpeg not in ('host', 'device'):
            raise ValueError(f"jpeg: 'host' or 'device' (got {jpeg!r})")
        self.jpeg = jpeg
        self.jpeg_capacity = self.JPEG_FIRST_CAPACITY
        self.jpeg_largest = 0
        self.need_remapping = False
        self.json_style = None
        self.output_postfix = None
        self.visualize = False
        self.visualize_postfix = None
        if self.dataset == 'vipseg':
            self.all_annotations = []
            self.video_json = {'video_id': video_name, 'annotations': self.all_annotations}
            self.need_remapping = True
            self.json_style = 'vipseg'
            self.output_postfix = 'pan_pred'
        elif self.dataset == 'burst':
            self.need_remapping = True
            self.all_annotations = []
            self.video_json = {'dataset': path.dirname(video_name), 'seq_name': path.basename(video_name),
                               'segmentations': self.all_annotations}
            self.json_style = 'burst'
        elif self.dataset == 'unsup_davis17':
            self.need_remapping = True
        elif self.dataset == 'ref_davis':
            pass
        elif self.dataset == 'demo':
            self.need_remapping = True
            self.all_annotations = []
            self.video_json = {'annotations': self.all_annotations}
            self.json_style = 'vipseg'
            self.visualize = True
            self.visualize_postfix = 'Visualizations'
            self.output_postfix = 'Annotations'
        else:   # ('gradio' needs a cv2 writer)
            raise NotImplementedError
        self.error = None
        self.queue = Queue(maxsize=10)
        self.thread = Thread(target=self._work)
        self.thread.daemon = True
        self.thread.start()

    def save_mask(self, prob: torch.Tensor, frame_name: str, need_resize: bool = False,
                  shape: Optional[Tuple[int, int]] = None, save_the_mask: bool = True, image_np: np.ndarray = None,
                  path_to_image: str = None) -> None:
        long_id = bool(self.object_manager.use_long_id)
        planes = []
        if save_the_mask:
            planes.append('color' if long_id else 'gray')
            if self.visualize and long_id:
                if image_np is None:
                    if path_to_image is None:
                        raise ValueError('Cannot visualize without image_np or path_to_image')
                    from PIL import Image
                    image_np = np.array(Image.open(path_to_image))
                planes.append('blend')
        merge = None
        if self.id_postprocessor is not None:   # ids are allotted now: they go into this frame's tables
            merge = self.id_postprocessor.assign(self.object_manager.get_current_segments_info())
        pending = launch_frame(self.object_manager, prob, shape if need_resize else None,
                               image=image_np if 'blend' in planes else None, rle=self.json_style == 'burst',
                               color='id' if long_id else 'gray', remap=self.need_remapping, planes=planes,
                               host=planes if self.png == self.jpeg == 'host' else [
                                   p for k, p in enumerate(planes)
                                   if not (self.png == 'device' and k == 0) and not (self.jpeg == 'device' and p == 'blend')],
                               id_map=None if merge is None else merge[0], index=self.frame_hook is not None)
        if self.png == 'device' and save_the_mask:   # the stream is coded now, on the caller's stream; nothing is waited for
            plane = pending.products.color if long_id else pending.products.gray
            pending.png = png_coder.encode(plane, palette=None if long_id else self.palette, capacity=self.png_capacity)
        if self.jpeg == 'device' and 'blend' in planes:   # likewise the overlay's JPEG
            pending.jpeg = jpeg_coder.encode(pending.products.blend, capacity=self.jpeg_capacity)
        self.queue.put((pending, frame_name, long_id) if merge is None else (pending, frame_name, long_id, merge))

    def end(self) -> None:
        self.queue.put(None)
        self.queue.join()
        self.thread.join()
        if self.error is not None:
            raise self.error

    # ---------------------------------------------------------------- worker thread
    def _work(self) -> None:
        while True:
            item = self.queue.get()
            try:
                if item is None:
                    break
                if self.error is None:
                    self._write(*item)
            except Exception as e:   # (kept for `end`: a daemon thread's traceback would be lost)
                self.error = e
            finally:
                self.queue.task_done()

    def _out_dir(self, postfix) -> str:
        out = self.output_root if postfix is None else path.join(self.output_root, postfix)
        if self.video_name is not None:
            out = path.join(out, self.video_name)
        os.makedirs(out, exist_ok=True)
        return out

    def _write(self, pending: PendingFrame, frame_name: str, long_id: bool, merge=None) -> None:
        from PIL import Image
        result = pending.finish()
        live = [s for s in result.segments if s['area'] > 0]     # zero-area segments are filtered out
        if merge is not None:   # merge_stuff's annotation: the areas of a merged id are sums of its channels' areas
            id_map, stuff = merge
            self.all_annotations.append({
                'file_name': frame_name[:-4] + '.jpg',
                'segments_info': self.id_postprocessor.annotation(live, id_map, stuff, {s['id']: s['area'] for s in live})})
        elif self.json_style == 'vipseg':
            self.all_annotations.append({
                'file_name': frame_name[:-4] + '.jpg',
                'segments_info': [{'category_id': s['category_id'], 'id': s['id'], 'score': s['score'], 'area': s['area']}
                                  for s in live]})
        elif self.json_style == 'burst':
            self.all_annotations.append({
                'file_name': frame_name[:-4] + '.jpg',
                'segmentations': [{'id': s['id'], 'score': s['score'], 'rle': s['rle']} for s in live]})
        if 'color' in result.host:
            out_img = Image.fromarray(result.host['color'])
        elif 'gray' in result.host:
            out_img = Image.fromarray(result.host['gray'])
            if self.palette is not None:
                out_img.putpalette(self.palette)
        else:
            out_img = None
        coded = pending.png
        if coded is not None:
            data = coded.finish()
            self.png_largest = max(self.png_largest, coded.total)
            self.png_capacity = 2 * self.png_largest
            self._save_bytes(data, path.join(self._out_dir(self.output_postfix), frame_name[:-4] + '.png'))
        if out_img is not None or coded is not None:
            if out_img is not None:
                self._save_image(out_img, path.join(self._out_dir(self.output_postfix), frame_name[:-4] + '.png'))
            if 'blend' in result.host:
                self._save_image(Image.fromarray(result.host['blend']),
                                 path.join(self._out_dir(self.visualize_postfix), frame_name[:-4] + '.jpg'))
        if pending.jpeg is not None:
            data = pending.jpeg.finish()
            self.jpeg_largest = max(self.jpeg_largest, pending.jpeg.total)
            self.jpeg_capacity = 2 * self.jpeg_largest
            self._save_bytes(data, path.join(self._out_dir(self.visualize_postfix), frame_name[:-4] + '.jpg'))
        if self.frame_hook is not None:
            self.frame_hook(frame_name, result, self.all_annotations[-1] if self.json_style is not None else None)

    def _save_image(self, image, where: str) -> None:
        image.save(where)

    def _save_bytes(self, data: bytes, where: str) -> None:
        with open(where, 'wb') as f:
            f.write(data)
