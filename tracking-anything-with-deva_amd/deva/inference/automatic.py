"""The reference's automatic frame loop on this package's pieces (not part of the reference's interface: the reference
runs it as deva/ext/automatic_processor.py:28-128 `process_frame_automatic` with deva/ext/automatic_sam.py `auto_segment`
and demo_utils.py `flush_buffer`, modules that import OpenCV and segment_anything when they load).

    processor = AutomaticProcessor(core, segmenter, saver=FrameResultSaver(...))
    for ti, (name, image_np) in enumerate(frames):        # RGB uint8 H*W*3
        processor.process_frame(image_np, ti, name)
    processor.flush()

A detection frame is: `estimate_forward_mask` (once the memory is engaged) -> `forward_prompt_points` (the grid points on
background: one copy of 8 bytes per point) -> the segmenter, batch by batch -> `ProposalFilter` (one copy of the result
table) -> `assemble_automatic` -> `incorporate_detection(..., incremental=True)`; the other frames are `step`.

The segmenter is any object with
    set_image(image_np)                  the frame, RGB uint8 H*W*3 (numpy)
    predict_points(points_px)            fp32 [B,2] pixel (x, y) on the device -> (logits fp32 [B*M,H,W] contiguous at the
                                         frame's own size, iou_preds fp32 [B*M]), both on the device
    reset_image()                        optional
    mask_threshold                       optional attribute (default 0.0, SAM's)
and optionally, for the route without frame-sized logits (`ProposalFilter.add_lowres`, include/deva_lowres.h),
    predict_points_lowres(points_px)     -> (low_logits fp32 [B*M,LH,LW] contiguous: the mask decoder's own output,
                                         iou_preds fp32 [B*M]), both on the device
    input_size                           attribute, valid after `set_image`: (IH, IW), the frame after the segmenter's
                                         longest-side resize
    model_size                           optional attribute (default 1024, SAM's)
INTEGRATION.md wraps a `SamPredictor` both ways.

`FrameLoop` is the loop itself; `deva.inference.with_text.TextPromptedProcessor` runs the same loop with detections
from a text-prompted detector."""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from deva.inference import detections
from deva.inference.object_info import ObjectInfo
from deva.inference.proposals import ProposalFilter
from deva.utils.tensor_utils import frame_to_network_input

__all__ = ['AutomaticProcessor', 'BufferedFrame', 'FrameLoop', 'RecordedProcessor', 'CONFIG_KEYS']

CONFIG_KEYS = ('size', 'suppress_small_objects', 'temporal_setting', 'num_voting_frames', 'detection_every',
               'SAM_NUM_POINTS_PER_SIDE', 'SAM_NUM_POINTS_PER_BATCH', 'SAM_PRED_IOU_THRESHOLD', 'SAM_OVERLAP_THRESHOLD')


class BufferedFrame:
    """what the semi-online buffer holds: the fields of the reference's FrameInfo (frame_utils.py:7-30) that
    `vote_in_temporary_buffer` and `clear_buffer` read, plus the decoded frame for the saver's overlay"""

    def __init__(self, image: torch.Tensor, mask: Optional[torch.Tensor], segments_info: Optional[List[ObjectInfo]], ti: int,
                 info: Dict, image_np: Optional[np.ndarray] = None):
        self.image, self.mask, self.segments_info, self.ti, self.info, self.image_np = image, mask, segments_info, ti, info, image_np

    name = property(lambda self: self.info['frame'][0])
    shape = property(lambda self: self.info['shape'])


class FrameLoop:
    """The frame loop that the reference's two demos share, and `flush_buffer`, around a `DEVAInferenceCore`:
    automatic_processor.py:28-128 and with_text_processor.py:30-122 differ only in how a detection is made and in the
    keywords of `incorporate_detection`.  A processor gives `config_keys`, `incorporate_keywords` and
    `_detect(image, image_np) -> (index mask, [ObjectInfo])`.

    The configuration is `core.config`; every key of `config_keys` must be there (a missing one raises KeyError with its
    name: no default is invented).
    `saver`: anything with `save_mask(prob, frame_name, need_resize=, shape=, image_np=)`, e.g. `FrameResultSaver`.
    `recorder`: a `detections.DetectionRecorder`; every result of `_detect` is recorded under the frame's name before it
    is used (in the semi-online setting that is each buffered frame's detection, not the vote).  Without one the loop is
    call for call the same.
    `next_voting_frame` starts at num_voting_frames - 1, as the demos set it."""
    config_keys: Tuple[str, ...] = ()
    incorporate_keywords: Dict = {}

    def __init__(self, core, saver=None, recorder=None):
        self.core, self.saver, self.recorder = core, saver, recorder
        self.frame_name = None          # of the frame `_detect` is asked about
        for key in self.config_keys:
            if key not in core.config:
                raise KeyError(key)
        if core.config['temporal_setting'] not in ('online', 'semionline'):
            raise ValueError(f"temporal_setting must be 'online' or 'semionline' (got {core.config['temporal_setting']!r})")
        self.next_voting_frame = core.config['num_voting_frames'] - 1

    def _detect(self, image: torch.Tensor, image_np: np.ndarray) -> Tuple[torch.Tensor, List[ObjectInfo]]:
        raise NotImplementedError

    def _detection(self, image: torch.Tensor, image_np: np.ndarray, frame_name: str) -> Tuple[torch.Tensor, List[ObjectInfo]]:
        self.frame_name = frame_name
        mask, segments_info = self._detect(image, image_np)
        if self.recorder is not None:
            self.recorder.add(frame_name, mask, segments_info)
        return mask, segments_info

    def _emit(self, produced: List, prob: torch.Tensor, frame_name: str, image_np: np.ndarray) -> None:
        produced.append((frame_name, prob))
        if self.saver is not None:
            h, w = image_np.shape[:2]
            self.saver.save_mask(prob, frame_name, need_resize=self.core.config['size'] > 0, shape=(h, w), image_np=image_np)

    def process_frame(self, image_np: np.ndarray, ti: int, frame_name: str) -> List[Tuple[str, torch.Tensor]]:
        """one frame of the video (RGB uint8 H*W*3) -> the (frame name, probabilities) pairs this call produced: one in
        the online setting; none, one or a voting window's worth in the semi-online one"""
        core, cfg = self.core, self.core.config
        h, w = image_np.shape[:2]
        image = frame_to_network_input(image_np, cfg['size'], antialias=False)   # the demo's rule (demo_utils.py:10-19)
        produced: List[Tuple[str, torch.Tensor]] = []
        if cfg['temporal_setting'] == 'semionline':
            if ti + cfg['num_voting_frames'] > self.next_voting_frame:
                mask, segments_info = self._detection(image, image_np, frame_name)
                info = {'frame': [frame_name], 'shape': [h, w]}
                core.add_to_temporary_buffer(BufferedFrame(image, mask, segments_info, ti, info, image_np))   # wait for more
                if ti == self.next_voting_frame:
                    first = core.frame_buffer[0]
                    _, mask, new_segments_info = core.vote_in_temporary_buffer(keyframe_selection='first')
                    prob = core.incorporate_detection(first.image, mask, new_segments_info, **self.incorporate_keywords)
                    self.next_voting_frame += cfg['detection_every']
                    self._emit(produced, prob, first.name, first.image_np)
                    for frame in core.frame_buffer[1:]:
                        self._emit(produced, core.step(frame.image, None, None), frame.name, frame.image_np)
                    core.clear_buffer()
            else:
                self._emit(produced, core.step(image, None, None), frame_name, image_np)    # standard propagation
        elif cfg['temporal_setting'] == 'online':
            if ti % cfg['detection_every'] == 0:
                mask, segments_info = self._detection(image, image_np, frame_name)
                prob = core.incorporate_detection(image, mask, segments_info, **self.incorporate_keywords)
            else:
                prob = core.step(image, None, None)
            self._emit(produced, prob, frame_name, image_np)
        else:
            raise ValueError(f"temporal_setting must be 'online' or 'semionline' (got {cfg['temporal_setting']!r})")
        return produced

    def flush(self) -> List[Tuple[str, torch.Tensor]]:
        """`flush_buffer` (demo_utils.py:22-46): step the frames that are still buffered when the video ends"""
        produced: List[Tuple[str, torch.Tensor]] = []
        for frame in self.core.frame_buffer:
            self._emit(produced, self.core.step(frame.image, None, None), frame.name, frame.image_np)
        return produced


class AutomaticProcessor(FrameLoop):
    """`process_frame_automatic` and `flush_buffer` of the reference's demo as one object around a `DEVAInferenceCore`
    (the loop is `FrameLoop`'s; a detection is incorporated with `incremental=True`).

    Every key of `CONFIG_KEYS` must be in `core.config`.  `capacity` is the `ProposalFilter`'s (masks that may pass the
    drops in one frame), and so is `min_mask_region_area` (0: off; above 0 the holes and islands below that area go from
    every kept mask before the masks are assembled).

    `lowres`: None (the default) takes the low-resolution route when the segmenter offers it (`predict_points_lowres` and
    `input_size`) and `predict_points` otherwise; True insists on it (a segmenter without it is refused), False never
    takes it."""
    config_keys = CONFIG_KEYS
    incorporate_keywords = {'incremental': True}

    def __init__(self, core, segmenter, *, capacity: int = 512, saver=None, min_mask_region_area: int = 0, recorder=None,
                 lowres: Optional[bool] = None):
        super().__init__(core, saver, recorder)
        self.segmenter, self.capacity, self.min_mask_region_area = segmenter, int(capacity), int(min_mask_region_area)
        self.lowres = detections.lowres_route(segmenter, 'predict_points_lowres', lowres)
        self._filter = None

    # ------------------------------------------------------------------ auto_segment
    def _proposal_filter(self, h: int, w: int) -> ProposalFilter:
        flt = self._filter
        if flt is None or (flt.height, flt.width) != (h, w):   # once per processor, again when the frame size changes
            flt = self._filter = ProposalFilter(h, w, capacity=self.capacity,
                                                pred_iou_thresh=self.core.config['SAM_PRED_IOU_THRESHOLD'],
                                                mask_threshold=getattr(self.segmenter, 'mask_threshold', 0.0),
                                                min_mask_region_area=self.min_mask_region_area)
        return flt

    def segment(self, image_np: np.ndarray, forward_mask: Optional[torch.Tensor],
                device=None) -> Tuple[torch.Tensor, List[ObjectInfo]]:
        """`auto_segment` (automatic_sam.py:47-145): the frame and the tracker's forward mask (None: the whole grid is
        asked) -> (int64 index mask at `detection_size`, on the device; [ObjectInfo(id, score)])"""
        cfg = self.core.config
        h, w = image_np.shape[:2]
        size = detections.detection_size(h, w, cfg['size'])
        n = cfg['SAM_NUM_POINTS_PER_SIDE']
        if forward_mask is not None:
            device = forward_mask.device
            points = detections.forward_prompt_points(forward_mask, n)
        else:
            device = torch.device('cuda') if device is None else device
            points = detections.prompt_grid(n, 'cpu').numpy()
        if len(points) == 0:          # everything is tracked: the segmenter is not asked (automatic_sam.py:83-86)
            return torch.zeros(size, dtype=torch.int64, device=device), []
        self.segmenter.set_image(image_np)
        # pixel coordinates as the generator forms them (automatic_mask_generator.py:253-257): fp32 points times the
        # integer (w, h), in double; the segmenter takes fp32
        points_px = torch.from_numpy((points * np.array([w, h])[None, :]).astype(np.float32)).to(device)
        flt = self._proposal_filter(h, w)
        flt.reset()
        per_batch = int(cfg['SAM_NUM_POINTS_PER_BATCH'])
        for first in range(0, points_px.shape[0], per_batch):
            if self.lowres:
                low_logits, iou_preds = self.segmenter.predict_points_lowres(points_px[first:first + per_batch])
                flt.add_lowres(low_logits, iou_preds, self.segmenter.input_size,
                               model_size=getattr(self.segmenter, 'model_size', 1024))
            else:
                logits, iou_preds = self.segmenter.predict_points(points_px[first:first + per_batch])
                flt.add(logits, iou_preds)
        if hasattr(self.segmenter, 'reset_image'):
            self.segmenter.reset_image()
        found = flt.finish()
        return detections.assemble_automatic(found.masks, found.iou_preds, size,
                                             suppress_small_objects=cfg['suppress_small_objects'],
                                             overlap_threshold=cfg['SAM_OVERLAP_THRESHOLD'])

    # ------------------------------------------------------------------ make_segmentation (automatic_processor.py)
    def _detect(self, image: torch.Tensor, image_np: np.ndarray) -> Tuple[torch.Tensor, List[ObjectInfo]]:
        forward_mask = detections.estimate_forward_mask(self.core, image) if self.core.memory.engaged else None
        return self.segment(image_np, forward_mask, device=image.device)


class RecordedProcessor(FrameLoop):
    """the frame loop over detections that were computed once and saved (the reference's evaluation/eval_with_detections.py),
    here over a recording of this package's own processors: `results` is a `detections.CocoResults` of a file that a
    `DetectionRecorder` wrote, and a detection is `results.detections(frame name, detection_size, policy='recorded')`:
    exactly the pair the recorded run's `_detect` returned.  A frame the file does not mention is an empty detection.

    No configuration keys of its own (the loop's: size, temporal_setting, num_voting_frames, detection_every).
    `incorporate_keywords`: those of the processor that was recorded ({'incremental': True} for `AutomaticProcessor`, none
    for `TextPromptedProcessor`)."""

    def __init__(self, core, results, *, saver=None, incorporate_keywords: Optional[Dict] = None):
        super().__init__(core, saver)
        self.results = results
        self.incorporate_keywords = dict(incorporate_keywords or {})

    def _detect(self, image: torch.Tensor, image_np: np.ndarray) -> Tuple[torch.Tensor, List[ObjectInfo]]:
        h, w = image_np.shape[:2]
        size = detections.detection_size(h, w, self.core.config['size'])
        return self.results.detections(self.frame_name, size, policy='recorded', device=image.device)
