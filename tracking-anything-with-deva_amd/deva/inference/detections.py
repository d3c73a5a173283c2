"""From a detector's output to what `DEVAInferenceCore.incorporate_detection` takes (not part of the reference's
interface: the reference does this inside its detector wrappers, deva/ext/automatic_sam.py:93-145 and
deva/ext/grounding_dino.py:117-142, which stay what `deva.ext` resolves to).

A detector gives N binary instance masks and a score each.  The reference turns them into an index mask and a list of
`ObjectInfo` with an N*H*W fp32 copy, two scaled copies, an argmax and a Python loop over the masks that synchronises
several times per mask.  Here `ops.detection_assemble` does the arithmetic on the device in five launches; the host
receives one small table (8 int32 per mask) and builds the list from it.

Two quirks of the reference are reproduced on purpose (include/deva_hip.h has the contract):
  * `assemble_automatic(..., suppress_small_objects=False)` returns a mask that holds the UNCOMPACTED index k + 1 of
    mask k while `segments_info` is compacted to 1, 2, ...: with an empty mask in the list the two disagree, and
    `incorporate_detection` then reads some segments from the wrong pixels (or none).  `consistent_ids=True` writes the
    compacted id into the mask instead; it is off by default because the default is parity with the reference.
  * `assemble_with_text` lists a mask that later, smaller masks painted over completely: its id is in
    `segments_info` and absent from the mask.
The text policy paints in descending area, among equal areas the higher index first: `np.flip` of a stable ascending
sort.  numpy's default `argsort` is stable only for short arrays, so for long lists the reference's own order among
equal areas is unspecified; this one is fixed.

Choosing prompt points from a forward mask (automatic_sam.py:67-89) feeds the detector: `forward_prompt_points` does
it on the device (`ops.prompt_points`: three launches and one copy of 8 bytes per point) from the mask that
`estimate_forward_mask` gives.  The masks and scores of `assemble_automatic` come out of
`deva.inference.proposals.ProposalFilter`, which filters a promptable segmenter's raw logits on the device;
`deva.inference.automatic.AutomaticProcessor` ties all of it into the reference's frame loop.

The text-prompted path (grounding_dino.py:101-142) is `text_detections`: the detector's fp32 boxes through
`ops.box_nms_xyxy`, the kept ones to a box-prompted segmenter batch by batch, the best candidate mask per box chosen and
binarised on the device by `ops.box_mask_select`, then `assemble_with_text`: two small host copies per detection frame.
`deva.inference.with_text.TextPromptedProcessor` is its frame loop.

Detections that arrive as COCO run lengths (a detector's "COCO results" file: `CocoResults`) go through `rle_detections`:
`deva.hip.rle.decode` puts the byte planes on the device at the assembly size and the two functions above take them from
there.  The other direction is `DetectionRecorder`: what a processor's `_detect` returned, frame by frame, written as such a
file with the run lengths encoded on the device (`deva.hip.rle.encode_labels`, `encode`), so that
`rle_detections(..., policy='recorded')` gives the recorded pair back and `deva.inference.automatic.RecordedProcessor`
re-runs the tracker over the same detections without the segmenter."""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from deva.hip import lowres as lowres_ops
from deva.hip import ops, rle
from deva.inference.object_info import ObjectInfo
from deva.utils.tensor_utils import pad_divide_by, unpad


def detection_size(h: int, w: int, min_side: int) -> Tuple[int, int]:
    """the size the reference's detectors assemble at (automatic_sam.py:60-65): the shorter side scaled to `min_side`,
    each side truncated (`int(h * scale)`); (h, w) itself for min_side <= 0"""
    if min_side > 0:
        scale = min_side / min(h, w)
        return int(h * scale), int(w * scale)
    return h, w


def _records(masks: torch.Tensor, size, policy: str, scores, **kw):
    """run the assembly and fetch its record table: one pinned, non-blocking copy and one event wait
    -> (mask on the device, records as a list of rows, scores as floats)"""
    device = masks.device
    n = masks.shape[0]
    on_device = torch.is_tensor(scores) and scores.device == device and scores.dtype == torch.float32
    mask, records = ops.detection_assemble(masks, size, policy, scores=scores if on_device else None, **kw)
    if n == 0:
        return mask, [], []
    if records.is_cuda:
        host = torch.empty(records.shape, dtype=records.dtype, pin_memory=True)
        host.copy_(records, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        event.synchronize()
    else:
        host = records
    values = ([float(v) for v in host[:, 6].contiguous().view(torch.float32).tolist()] if on_device
              else [v.item() if torch.is_tensor(v) else v for v in scores])
    return mask, host.tolist(), values


def _stack(masks) -> torch.Tensor:
    if not torch.is_tensor(masks):
        raise TypeError('masks: an [N,H,W] tensor on the device expected')
    return masks


def assemble_automatic(masks: torch.Tensor, scores, size: Optional[Tuple[int, int]] = None, *,
                       suppress_small_objects: bool, overlap_threshold: float = 0.8,
                       consistent_ids: bool = False) -> Tuple[torch.Tensor, List[ObjectInfo]]:
    """the tail of `auto_segment` (automatic_sam.py:93-145): `masks` [N,H,W] binary (bool / uint8 / fp32 {0,1}) and
    `scores` [N] (the predicted IoUs: an fp32 tensor on the masks' device travels with the records, anything else is
    read on the host) -> (int64 [OH,OW] index mask on the device, [ObjectInfo(id, score)]).
    `suppress_small_objects=True`: large masks eat small ones, a mask that keeps less than `overlap_threshold`
    (config['SAM_OVERLAP_THRESHOLD']) of its pixels is dropped.  False: small masks win; see the module docstring for
    `consistent_ids`."""
    masks = _stack(masks)
    policy = 'suppress_small' if suppress_small_objects else 'prefer_small'
    mask, rows, values = _records(masks, size, policy, scores, overlap_threshold=overlap_threshold,
                                  consistent_ids=consistent_ids)
    kept = sorted((r[0], k) for k, r in enumerate(rows) if r[0] > 0)
    return mask, [ObjectInfo(id=i, score=values[k]) for i, k in kept]


def assemble_with_text(masks: torch.Tensor, confidences: Sequence, class_ids: Sequence,
                       size: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, List[ObjectInfo]]:
    """the tail of `segment_with_text` (grounding_dino.py:117-142): painter's order, largest mask first ->
    (int64 [OH,OW] index mask on the device, [ObjectInfo(id, category_id, score)] in paint order)"""
    masks = _stack(masks)
    mask, rows, values = _records(masks, size, 'text', confidences)
    classes = class_ids.tolist() if hasattr(class_ids, 'tolist') else list(class_ids)
    kept = sorted((r[0], k) for k, r in enumerate(rows) if r[0] > 0)
    return mask, [ObjectInfo(id=i, category_id=classes[k], score=values[k]) for i, k in kept]


def estimate_forward_mask(core, image: torch.Tensor) -> torch.Tensor:
    """the reference's `estimate_forward_mask` (deva/ext/automatic_processor.py:131-140): what the memory predicts for
    the NEXT frame (`core.curr_ti + 1`), as an index mask of tmp ids at the frame's size.  The features and the key go
    through the feature store, so the `step` / `incorporate_detection` of that frame finds them there.

    Unlike the reference's, the call leaves no trace in the core: the reference lets this read update the sensory
    memory and the usage counters a second time; here the read runs with `update_sensory=False` on a copy of the
    counters, and the following `step` of the frame is bit-identical to a run without the call."""
    padded, pad = pad_divide_by(image, 16)
    batch = padded.unsqueeze(0)
    ti = core.curr_ti + 1
    store = core.image_feature_store
    ms_features = store.get_ms_features(ti, batch)
    key, _, selection = store.get_key(ti, batch)
    saved_map, saved_usage = core._map16, core.memory.save_usage()
    core._map16 = (padded.shape[-2] // 16, padded.shape[-1] // 16, image.device)
    try:
        prob = core._segment(key, selection, ms_features, update_sensory=False)
    finally:
        core._map16 = saved_map
        core.memory.restore_usage(saved_usage)
    return unpad(ops.index_mask(prob.contiguous()), pad)


_GRIDS = {}
_PINNED = {}


def prompt_grid(n_per_side: int, device) -> torch.Tensor:
    """the prompt grid of automatic_sam.py:74-81 as fp32 [n*n,2] normalised (x, y) on `device`: n values from
    1 / (2 n) to 1 - 1 / (2 n) per axis, x fastest.  `torch.linspace` runs on the CPU, so the values are the ones a
    CPU run of the reference samples at, and the upload happens once per (n, device)."""
    n = int(n_per_side)
    if n < 1:
        raise ValueError(f'prompt_grid: at least one point per side (got {n_per_side})')
    key = (n, str(torch.device(device)))
    if key not in _GRIDS:
        offset = 1 / (2 * n)
        side = torch.linspace(offset, 1 - offset, n)
        grid = torch.stack([side.unsqueeze(0).repeat(n, 1), side.unsqueeze(1).repeat(1, n)], dim=-1).view(-1, 2)
        _GRIDS[key] = grid.contiguous().to(device)
    return _GRIDS[key]


def forward_prompt_points(forward_mask: torch.Tensor, n_per_side: Optional[int] = None, *,
                          point_grid: Optional[torch.Tensor] = None, threshold: float = 0.01) -> np.ndarray:
    """automatic_sam.py:67-82: the points of the grid (`prompt_grid(n_per_side)`, or `point_grid`: fp32 [P,2] normalised
    (x, y)) at which the forward mask, blurred to 1/16 of its size, is below `threshold` -> host fp32 [K,2] in grid
    order, what the reference hands to `generate(image, positive_points, None)`.  K = 0 is a valid result.  The host
    pays one pinned, non-blocking copy of 8 P + 4 bytes and one event wait."""
    if (n_per_side is None) == (point_grid is None):
        raise ValueError('forward_prompt_points: give n_per_side or point_grid (one of them)')
    device = forward_mask.device
    grid = prompt_grid(n_per_side, device) if point_grid is None else point_grid
    n = grid.shape[0]
    if not forward_mask.is_cuda:     # (the wrapper refuses; a test's CPU statement of it answers on the host)
        points, _, count = ops.prompt_points(forward_mask.contiguous(), grid, threshold)
        return points[:int(count[0])].numpy().copy()
    packed = torch.empty(2 * n + 1, dtype=torch.float32, device=device)   # the kept points, the count behind them
    ops.prompt_points(forward_mask.contiguous(), grid, threshold, packed=packed)
    host = _PINNED.get(n)
    if host is None:
        host = _PINNED[n] = torch.empty(2 * n + 1, dtype=torch.float32, pin_memory=True)
    host.copy_(packed, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    event.synchronize()
    kept = int(host[2 * n:].view(torch.int32)[0])
    return host[:2 * kept].view(kept, 2).numpy().copy()


# ------------------------------------------------------------------------------------------ text-prompted detections
def _host_array(values, dtype) -> np.ndarray:
    if torch.is_tensor(values):
        values = values.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(values, dtype=dtype))


def lowres_route(segmenter, method: str, lowres: Optional[bool]) -> bool:
    """does a processor take the route without frame-sized logits (include/deva_lowres.h)?  `lowres` None: when the
    segmenter offers `method` (`predict_points_lowres` / `predict_boxes_lowres`; its `input_size` is read after
    `set_image`); True: it must; False: never"""
    offered = callable(getattr(segmenter, method, None))
    if lowres and not offered:
        raise ops.DevaHipError(f'lowres=True: the segmenter has no `{method}`')
    return offered if lowres is None else bool(lowres)


def text_detections(boxes, confidences, class_ids, segmenter, frame_hw: Tuple[int, int], size: Tuple[int, int], *,
                    nms_threshold: float, boxes_per_batch: int = 16, capacity: int = 256,
                    arena: Optional[torch.Tensor] = None, device=None,
                    lowres: Optional[bool] = None) -> Tuple[torch.Tensor, List[ObjectInfo]]:
    """`segment_with_text` from the detector's answer on (grounding_dino.py:101-142): `boxes` fp32 [N,4] xyxy in pixels
    of the frame, `confidences` fp32 [N], `class_ids` [N] (numpy, as GroundingDINO's wrapper returns them, or tensors; a
    class id may be None, the unmatched phrase, and passes through) -> (int64 [OH,OW] index mask on the device,
    [ObjectInfo(id, category_id, score)] in paint order).

    Box NMS runs on the device (`ops.box_nms_xyxy`); ONE small copy brings the keep list and its count to the host, which
    needs the count to batch the segmenter and reorders `confidences` / `class_ids` from it.  The kept boxes are
    gathered on the device and go to `segmenter.predict_boxes` in batches of `boxes_per_batch`; every batch goes
    straight into `ops.box_mask_select`, which writes the chosen byte planes into the arena (`arena`: the caller's
    contiguous uint8 [capacity,H,W]; default: allocated here for the kept boxes).  Nothing synchronises per batch.
    `assemble_with_text` then makes its one copy of the record table.  The segmenter must have seen the frame
    (`set_image`); it is not asked at all when no box is given or kept.  More kept boxes than `capacity` raise
    DevaHipError before the segmenter is asked.

    A segmenter with `predict_boxes_lowres(boxes_px) -> (low fp32 [B,M,LH,LW], scores fp32 [B,M])` and an `input_size`
    attribute (after `set_image`; `model_size` optional, 1024) is asked for those instead, and `lowres.select_masks` writes
    the same arena slices from them: the planes of `ops.box_mask_select` on the resized logits (include/deva_lowres.h, rule
    L6) without resizing any.  `lowres`: None takes that route when it is offered, True insists, False never takes it."""
    h, w = int(frame_hw[0]), int(frame_hw[1])
    size = (int(size[0]), int(size[1]))
    if device is None:
        device = arena.device if arena is not None else (boxes.device if torch.is_tensor(boxes) else torch.device('cuda'))
    if torch.is_tensor(boxes):
        boxes_dev = boxes.detach().to(device=device, dtype=torch.float32).reshape(-1, 4).contiguous()
    else:
        boxes_dev = torch.from_numpy(_host_array(boxes, np.float32).reshape(-1, 4)).to(device)
    n = boxes_dev.shape[0]
    conf_host = _host_array(confidences, np.float32).reshape(-1)
    classes = class_ids.tolist() if hasattr(class_ids, 'tolist') else list(class_ids)
    if conf_host.shape[0] != n or len(classes) != n:
        raise ValueError(f'text_detections: {n} boxes, {conf_host.shape[0]} confidences and {len(classes)} class ids')
    per_batch = int(boxes_per_batch)
    if per_batch < 1:
        raise ValueError(f'text_detections: at least one box per batch (got {boxes_per_batch})')
    if arena is not None and (arena.dtype != torch.uint8 or arena.numel() != capacity * h * w or not arena.is_contiguous()):
        raise ops.DevaHipError(f'text_detections: the arena must be a contiguous uint8 tensor of {capacity} x {h} x {w}')
    if n == 0:
        return torch.zeros(size, dtype=torch.int64, device=device), []
    conf_dev = torch.from_numpy(conf_host).to(device)
    packed = ops.box_nms_xyxy(boxes_dev, conf_dev, nms_threshold,
                              packed=torch.empty(n + 1, dtype=torch.int32, device=device))
    if packed.is_cuda:
        host = torch.empty(n + 1, dtype=torch.int32, pin_memory=True)
        host.copy_(packed, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        event.synchronize()
    else:
        host = packed
    kept = int(host[n])
    keep = host[:kept].tolist()
    if kept > capacity:
        raise ops.DevaHipError(f'text_detections: {kept} boxes are left after NMS, the arena holds {capacity} '
                               '(raise `capacity`, or the detector\'s thresholds)')
    if kept == 0:
        return torch.zeros(size, dtype=torch.int64, device=device), []
    planes = (torch.empty((kept, h, w), dtype=torch.uint8, device=device) if arena is None
              else arena.view(capacity, h, w)[:kept])
    boxes_px = boxes_dev.index_select(0, packed[:kept].to(torch.int64))
    threshold = getattr(segmenter, 'mask_threshold', 0.0)
    use_lowres = lowres_route(segmenter, 'predict_boxes_lowres', lowres)   # (here: the segmenter is not touched before a box is kept)
    for first in range(0, kept, per_batch):
        if use_lowres:
            low, scores = segmenter.predict_boxes_lowres(boxes_px[first:first + per_batch])
            lowres_ops.select_masks(low, scores, segmenter.input_size, (h, w), threshold=threshold,
                                    model_size=getattr(segmenter, 'model_size', 1024), out=planes[first:first + low.shape[0]])
        else:
            logits, scores = segmenter.predict_boxes(boxes_px[first:first + per_batch])
            ops.box_mask_select(logits, scores, threshold, out=planes[first:first + logits.shape[0]])
    return assemble_with_text(planes, [conf_host[k] for k in keep], [classes[k] for k in keep], size)


# ------------------------------------------------------------------------------------------ detections from run lengths
_RLE_POLICIES = ('text', 'large', 'small', 'recorded')


def _recorded(annotations: Sequence[dict], size, source_size, device) -> Tuple[torch.Tensor, List[ObjectInfo]]:
    """what `DetectionRecorder.add` wrote for one frame -> the pair it was given: the pixels of plane k get `id_k`, in file
    order, and every entry is listed, whether a pixel holds its id or not"""
    for k, a in enumerate(annotations):
        if 'id' not in a:
            raise ValueError(f"rle_detections: entry {k} carries no 'id': policy='recorded' reads what DetectionRecorder wrote")
    planes = rle.decode([a['segmentation'] for a in annotations], size, dtype=torch.uint8, source_size=source_size, device=device)
    mask = torch.zeros(planes.shape[1:], dtype=torch.int64, device=planes.device)
    for plane, a in zip(planes, annotations):
        mask = torch.where(plane != 0, int(a['id']), mask)
    return mask, [ObjectInfo(int(a['id']), a.get('category_id'), score=a['score']) for a in annotations]


def rle_detections(annotations: Sequence[dict], size: Optional[Tuple[int, int]] = None, *, policy: str = 'text',
                   score_threshold: Optional[float] = None, overlap_threshold: float = 0.8, consistent_ids: bool = False,
                   source_size: Optional[Tuple[int, int]] = None, device=None) -> Tuple[torch.Tensor, List[ObjectInfo]]:
    """one frame of a detector's "COCO results" (`[{'segmentation': {'size', 'counts'}, 'score', 'category_id'?}, ...]`,
    the masks as COCO run lengths in any form `deva.hip.rle.parse_counts` takes) -> what `incorporate_detection` takes:
    (int64 [OH,OW] index mask on the device, [ObjectInfo]).

    The masks are decoded on the device (`deva.hip.rle.decode`) straight at `size` (the masks' own when None; otherwise
    the nearest resize of a frame reader's mask transform, fused into the decode), and the byte planes go as they are
    into `assemble_with_text` (`policy='text'`: painter's order, `category_id` carried, None where absent) or
    `assemble_automatic` ('large': `suppress_small_objects=True` with `overlap_threshold`; 'small': False, see
    `consistent_ids` there).  `policy='recorded'`: the annotations are a `DetectionRecorder`'s, every one with its 'id', and
    the result is the recorded pair itself, nothing is assembled again: uncompacted ids and a listed id that no pixel
    holds (its run lengths are [H * W]) come back as they were.  `score_threshold`: annotations whose score is below it
    are left out before anything is decoded.  No annotation (left) gives an empty mask of `size`, which must then be
    given."""
    if policy not in _RLE_POLICIES:
        raise ValueError(f'rle_detections: policy must be one of {_RLE_POLICIES} (got {policy!r})')
    kept = [a for a in annotations if score_threshold is None or float(a['score']) >= score_threshold]
    if not kept:
        if size is None:
            raise ValueError('rle_detections: no annotation is left and no `size` says how large the empty mask is')
        return torch.zeros((int(size[0]), int(size[1])), dtype=torch.int64, device=torch.device('cuda' if device is None else device)), []
    if policy == 'recorded':
        return _recorded(kept, size, source_size, device)
    planes = rle.decode([a['segmentation'] for a in kept], size, dtype=torch.uint8, source_size=source_size, device=device)
    scores = [float(a['score']) for a in kept]
    if policy == 'text':
        return assemble_with_text(planes, scores, [a.get('category_id') for a in kept])
    return assemble_automatic(planes, scores, suppress_small_objects=policy == 'large', overlap_threshold=overlap_threshold,
                              consistent_ids=consistent_ids)


class DetectionRecorder:
    """detections as they are made, kept as the entries of a "COCO results" file that `CocoResults` reads: per object
    {'image_id', 'id', 'score', 'segmentation': {'size', 'counts'}} and 'category_id' when the object has one.  The run
    lengths are encoded on the device; the host receives the run boundaries, never a plane."""

    def __init__(self, path=None):
        self.path = path
        self.annotations: List[dict] = []

    def add(self, image_id, mask: torch.Tensor, segments_info: Sequence[ObjectInfo]) -> None:
        """the (index mask, [ObjectInfo]) pair that `incorporate_detection` takes, under `image_id` (a frame's name); an
        object that no pixel holds is listed with the run lengths [H * W]"""
        segments_info = list(segments_info)
        if not segments_info:
            return
        for obj, seg in zip(segments_info, rle.encode_labels(mask, [obj.id for obj in segments_info])):
            score, category = obj.scores[0], obj.category_ids[0]
            entry = {'image_id': image_id, 'id': int(obj.id), 'score': None if score is None else float(score), 'segmentation': seg}
            if category is not None:
                entry['category_id'] = int(category)
            self.annotations.append(entry)

    def add_planes(self, image_id, planes: torch.Tensor, scores: Sequence, category_ids: Optional[Sequence] = None,
                   threshold: Optional[float] = None) -> None:
        """raw proposals: [N,H,W] planes on the device (uint8 / bool, or float32 logits with `threshold`; they may
        overlap) with a score each, numbered 1.. in the call's order"""
        scores = scores.tolist() if hasattr(scores, 'tolist') else list(scores)
        categories = None if category_ids is None else (category_ids.tolist() if hasattr(category_ids, 'tolist') else list(category_ids))
        if len(scores) != planes.shape[0] or (categories is not None and len(categories) != planes.shape[0]):
            raise ValueError(f'add_planes: {planes.shape[0]} planes, {len(scores)} scores'
                             + ('' if categories is None else f' and {len(categories)} category ids'))
        for k, seg in enumerate(rle.encode(planes, threshold=threshold)):
            entry = {'image_id': image_id, 'id': k + 1, 'score': float(scores[k]), 'segmentation': seg}
            if categories is not None and categories[k] is not None:
                entry['category_id'] = int(categories[k])
            self.annotations.append(entry)

    def write(self, path=None) -> str:
        """the entries as a JSON list -> the path written"""
        import json
        path = self.path if path is None else path
        if path is None:
            raise ValueError('DetectionRecorder.write: no path was given')
        with open(path, 'w') as f:
            json.dump(self.annotations, f)
        return path


class CocoResults:
    """a "COCO results" file (Mask2Former, SAM exporters, any COCO evaluator's input): a list of
    {'image_id', 'category_id', 'score', 'segmentation': {'size', 'counts'}}, grouped by `image_id` in the order of first
    appearance, the annotations of an image in file order.  Host bookkeeping only: nothing is decoded until a frame is
    asked for."""

    def __init__(self, path_or_list):
        if isinstance(path_or_list, (str, bytes)) or hasattr(path_or_list, '__fspath__'):
            import json
            with open(path_or_list) as f:
                path_or_list = json.load(f)
        self.frames = {}
        for k, ann in enumerate(path_or_list):
            if not isinstance(ann, dict) or 'image_id' not in ann or 'segmentation' not in ann or 'score' not in ann:
                raise ValueError(f"CocoResults: entry {k} must hold 'image_id', 'score' and 'segmentation'")
            self.frames.setdefault(ann['image_id'], []).append(ann)

    def __len__(self) -> int:
        return len(self.frames)

    def __contains__(self, image_id) -> bool:
        return image_id in self.frames

    def __iter__(self):
        return iter(self.frames.items())

    def image_ids(self) -> list:
        return list(self.frames)

    def annotations(self, image_id) -> List[dict]:
        """the annotations of one image; an image the file does not mention has none"""
        return self.frames.get(image_id, [])

    def detections(self, image_id, size: Optional[Tuple[int, int]] = None, **kw) -> Tuple[torch.Tensor, List[ObjectInfo]]:
        """`rle_detections` of one image"""
        return rle_detections(self.annotations(image_id), size, **kw)
