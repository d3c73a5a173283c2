"""From a promptable segmenter's raw output to what `detections.assemble_automatic` takes (not part of the reference's
interface: the reference does this inside its mask generator, deva/ext/SAM/automatic_mask_generator.py:332-352 per batch
of prompts and :272-278 per image, which stays what `deva.ext` resolves to).

A point-prompted segmenter gives, per batch of prompts, B mask-logit planes [B,H,W] fp32 at frame size and one
predicted IoU each.  The reference drops by predicted IoU, counts two thresholds per plane for a stability score, drops
by it, binarises, reduces a box per mask -- five to seven passes over the fp32 planes, a boolean-index copy of the
survivors after every drop, each a host synchronisation -- and ends with box NMS.  `ProposalFilter` takes the batches as
they come: a live plane is read once, a surviving one twice, the survivors are kept as byte planes on the device, and the
frame costs one small host copy.  The rules are in include/deva_hip.h (deva_proposal_batch).  They are this library's
statement, not torchvision's or segment_anything's code: the order among equal predictions, which torchvision leaves
open on the device, is fixed here (the earlier arrival first).

Crops (`crop_n_layers > 0`) are out of scope: the reference does not configure them (automatic_sam.py:26-40).  The
generator's `postprocess_small_regions` (automatic_mask_generator.py:361-409, `min_mask_region_area`) is the last step of
`finish` when asked for: holes and islands below an area go (`deva.hip.regions`, rules R1-R7 of include/deva_regions.h),
the boxes are taken again and box NMS runs once more, preferring the masks that needed no fixing.  Choosing the prompt
points stays with the caller, as `detections.py` says."""
from typing import Optional

import torch

from deva.hip import DevaHipError, lowres, ops, regions
from deva.hip.ops import ProposalResult

__all__ = ['ProposalFilter', 'ProposalResult']


class ProposalFilter:
    """Streaming proposal filter of one video: `add` every batch of a detection frame, `finish` once, again for the
    next frame.

        flt = ProposalFilter(h, w, capacity=512)
        for points in batches:                       # the generator's loop (automatic_mask_generator.py:264-268)
            logits, iou_preds = segmenter(points)    # [B,h,w] fp32, [B] fp32, on the device
            flt.add(logits, iou_preds)               # three launches, no synchronisation
            # or, from the mask decoder's own [B,256,256] output, without the frame-sized planes:
            # flt.add_lowres(low_logits, iou_preds, input_size)
        found = flt.finish()                         # box NMS, ONE host copy, the kept planes in keep order
        mask, segments = assemble_automatic(found.masks, found.iou_preds, suppress_small_objects=True)

    Memory, allocated at the first `add` and reused for every later frame: `capacity` * height * width bytes of arena
    (2 MB per mask at 1080p: 1 GB for capacity=512), under 2.3 MB of scratch and 128 KB of result table on the device
    and as much pinned host memory; `finish` allocates the [K,H,W] uint8 result.  `capacity` (1 to 4096, what
    `assemble_automatic` takes) is the number of masks that may pass the two drops in one frame, BEFORE NMS; there is no
    hidden growth: a frame in which more pass makes `finish` raise with their number, and nothing is written outside
    the arena.  `arena` may be the caller's own contiguous uint8 tensor of capacity*height*width elements.

    The thresholds are those of the reference's generator; `mask_threshold` is the segmenter's (0.0 for SAM).  A
    `pred_iou_thresh` or `stability_score_thresh` <= 0 disables that drop, as the reference's `> 0.0` guards do.

    `min_mask_region_area` > 0 (the generator's option; 0, the default, changes nothing, not even the launches) makes
    `finish` end with the generator's `postprocess_small_regions` on the K kept planes, all on the device:
    `regions.remove_small_regions` in place (holes, then islands, below that area), the boxes from its records, scores
    `1 - changed`, `ops.box_nms` at `region_nms_thresh` (None: `box_nms_thresh`; the reference passes
    max(box_nms_thresh, crop_nms_thresh), both 0.7), and planes, `iou_preds`, `stability`, `index` and boxes selected in
    that keep order: the masks that needed no fixing first, in the order they had, then the fixed ones.  That costs ONE
    more small host copy per frame -- the records and the second keep list together, 4 * (9 K + 1) bytes -- so a frame
    has two.  The kept planes' records are on the host afterwards as `last_regions` (int32 [K',8]: changed, filled,
    removed, area, x0, y0, x1, y1; None without the option).  The scratch of the region kernels (8 bytes per pixel of a
    plane in flight, at most `regions.DEFAULT_SCRATCH` bytes) is allocated at the first such `finish` and reused."""

    def __init__(self, height: int, width: int, *, capacity: int, pred_iou_thresh: float = 0.88,
                 stability_score_thresh: float = 0.95, stability_score_offset: float = 1.0, mask_threshold: float = 0.0,
                 box_nms_thresh: float = 0.7, arena: Optional[torch.Tensor] = None, min_mask_region_area: int = 0,
                 region_nms_thresh: Optional[float] = None):
        self.height, self.width, self.capacity = int(height), int(width), int(capacity)
        if self.height <= 0 or self.width <= 0:
            raise DevaHipError(f'ProposalFilter: bad frame size {(height, width)}')
        if not 1 <= self.capacity <= ops.PROPOSAL_MAX_MASKS:
            raise DevaHipError(f'ProposalFilter: a capacity of 1 to {ops.PROPOSAL_MAX_MASKS} masks (got {capacity})')
        self.thresholds = dict(pred_iou_thresh=float(pred_iou_thresh), stability_score_thresh=float(stability_score_thresh),
                               stability_score_offset=float(stability_score_offset), mask_threshold=float(mask_threshold))
        self.box_nms_thresh = float(box_nms_thresh)
        if isinstance(min_mask_region_area, bool) or int(min_mask_region_area) != min_mask_region_area or min_mask_region_area < 0:
            raise DevaHipError(f'ProposalFilter: min_mask_region_area must be 0 (off) or a positive area (got {min_mask_region_area})')
        self.min_mask_region_area = int(min_mask_region_area)
        self.region_nms_thresh = self.box_nms_thresh if region_nms_thresh is None else float(region_nms_thresh)
        self.last_regions = None
        self._regions = None          # `regions.region_buffers`, at the first `finish` that needs them
        self._arena = arena
        self._state = None
        self._begun = False

    def _ready(self, device):
        if self._state is None:
            self._state = ops.proposal_state(self.height, self.width, self.capacity, device, arena=self._arena)
        if not self._begun:
            ops.proposal_begin(self._state)
            self._begun = True
        return self._state

    def add(self, logits: torch.Tensor, iou_preds: torch.Tensor) -> None:
        """one batch: `logits` fp32 [B,H,W] contiguous and `iou_preds` fp32 [B], both on the device; B may be 0"""
        ops.proposal_batch(self._ready(logits.device), logits, iou_preds, **self.thresholds)

    def add_lowres(self, low_logits: torch.Tensor, iou_preds: torch.Tensor, input_size, *, model_size: int = 1024) -> None:
        """one batch straight from the segmenter's mask decoder: `low_logits` fp32 [B,LH,LW] contiguous (SAM: 256 x 256) and
        `iou_preds` fp32 [B], both on the device; `input_size` = (IH, IW), the frame after the segmenter's longest-side
        resize (`lowres.sam_input_size(h, w, model_size)` for SAM).  The same as `add(lowres.upsample_logits(low_logits,
        input_size, (height, width)), iou_preds)`, bit for bit, without the frame-sized fp32 planes (include/deva_lowres.h,
        rules L1-L5); a frame may mix both kinds of batch.  Three launches, no synchronisation; B may be 0."""
        lowres.proposal_batch(self._ready(low_logits.device), low_logits, iou_preds, input_size, model_size=model_size,
                              **self.thresholds)

    def finish(self) -> ProposalResult:
        """-> the frame's `ProposalResult` (masks uint8 [K,H,W], iou_preds and stability fp32 [K] on the device; boxes
        int32 [K,4] and the arrival index int32 [K] on the host), and the filter is ready for the next frame.  Raises
        `DevaHipError` when more masks passed than `capacity`."""
        if self._state is None:
            raise DevaHipError('ProposalFilter.finish: no batch was added yet (the device is taken from the first one)')
        state = self._ready(None)
        self._begun = False
        found = ops.proposal_finish(state, self.box_nms_thresh)
        if self.min_mask_region_area > 0:
            found = self._postprocess_small_regions(found)
        return found

    def _postprocess_small_regions(self, found: ProposalResult) -> ProposalResult:
        k = int(found.masks.shape[0])
        if k == 0:
            self.last_regions = torch.zeros((0, regions.FIELDS), dtype=torch.int32)
            return found
        if self._regions is None:
            self._regions = regions.region_buffers(self.height, self.width, self.capacity, found.masks.device)
        # in place on the kept planes, then the frame's second host copy: the records and the second keep list together
        records, keep, keep_device = regions.clean_and_suppress(found.masks, self.min_mask_region_area, self.region_nms_thresh,
                                                                self._regions)
        rows = records[keep].clone()
        self.last_regions = rows
        if len(keep) == k and bool((keep == torch.arange(k)).all()):       # nothing went and nothing moved
            masks, iou_preds, stability = found.masks, found.iou_preds, found.stability
        else:
            masks = found.masks.index_select(0, keep_device)
            iou_preds, stability = found.iou_preds.index_select(0, keep_device), found.stability.index_select(0, keep_device)
        return ProposalResult(masks, iou_preds, stability, rows[:, regions.X0:regions.Y1 + 1].contiguous(), found.index[keep].contiguous())

    def reset(self) -> None:
        """forget what was added since the last `finish` (the memory stays)"""
        self._begun = False
