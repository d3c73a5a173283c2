"""The reference's text-prompted frame loop on this package's pieces (not part of the reference's interface: the reference
runs it as deva/ext/with_text_processor.py:30-122 `process_frame_with_text` with deva/ext/grounding_dino.py:78-142
`segment_with_text` and demo_utils.py `flush_buffer`, modules that import OpenCV, torchvision, groundingdino and
segment_anything when they load).

    processor = TextPromptedProcessor(core, detector, segmenter, saver=FrameResultSaver(...))
    for ti, (name, image_np) in enumerate(frames):        # RGB uint8 H*W*3
        processor.process_frame(image_np, ti, name)
    processor.flush()

A detection frame is: `segmenter.set_image` -> the detector -> `detections.text_detections` (box NMS on the device, one
copy of the keep list, the kept boxes to the segmenter batch by batch, the best mask per box chosen and binarised on the
device, `assemble_with_text` with its one copy of the record table) -> `incorporate_detection(image, mask, segments)`
WITHOUT `incremental` (with_text_processor.py:74, :113); the other frames are `step`.  Unlike the automatic loop no
forward mask is estimated, and `category_id` travels with the segments.

The detector is any object with
    predict_with_classes(image_rgb_np, classes, box_threshold, text_threshold)
                                         the frame, RGB uint8 H*W*3 (numpy), and the list of class names ->
                                         (xyxy fp32 [N,4] in pixels of the frame, confidence fp32 [N], class_id [N]),
                                         numpy or tensors; a class id may be None (a phrase that matched no class)
and the segmenter any object with
    set_image(image_np)                  the frame, RGB uint8 H*W*3 (numpy)
    predict_boxes(boxes_px)              fp32 [B,4] xyxy in pixels of the frame, on the device -> (logits fp32 [B,M,H,W]
                                         contiguous at the frame's own size, scores fp32 [B,M]), both on the device;
                                         M candidate masks per box, 1 <= M <= 16
    reset_image()                        optional
    mask_threshold                       optional attribute (default 0.0, SAM's)
and optionally, for the route without frame-sized logits (`lowres.select_masks`, include/deva_lowres.h),
    predict_boxes_lowres(boxes_px)       -> (low fp32 [B,M,LH,LW] contiguous: the mask decoder's own output, scores fp32
                                         [B,M]), both on the device
    input_size                           attribute, valid after `set_image`: (IH, IW), the frame after the segmenter's
                                         longest-side resize; `model_size` optional (default 1024, SAM's)
INTEGRATION.md wraps `groundingdino.util.inference.Model` and a `SamPredictor` this way."""
from typing import List, Tuple

import numpy as np
import torch

from deva.inference import detections
from deva.inference.automatic import FrameLoop
from deva.inference.object_info import ObjectInfo

__all__ = ['TextPromptedProcessor', 'CONFIG_KEYS']

CONFIG_KEYS = ('size', 'temporal_setting', 'num_voting_frames', 'detection_every', 'prompt', 'DINO_THRESHOLD',
               'DINO_NMS_THRESHOLD')


class TextPromptedProcessor(FrameLoop):
    """`process_frame_with_text` and `flush_buffer` of the reference's demo as one object around a `DEVAInferenceCore`
    (the loop is `FrameLoop`'s; a detection is incorporated without `incremental`).

    Every key of `CONFIG_KEYS` must be in `core.config`.  config['prompt'] is split on '.' as the reference splits it
    (with_text_processor.py:42-43: no stripping, an empty string stays a class).  `boxes_per_batch` boxes go to the
    segmenter at a time; `capacity` is the number of boxes that may be left after NMS in one frame.  `lowres`: None (the
    default) takes the low-resolution route when the segmenter offers `predict_boxes_lowres`, True insists on it, False
    never takes it."""
    config_keys = CONFIG_KEYS
    incorporate_keywords = {}

    def __init__(self, core, detector, segmenter, *, saver=None, boxes_per_batch: int = 16, capacity: int = 256, recorder=None,
                 lowres=None):
        super().__init__(core, saver, recorder)
        self.detector, self.segmenter = detector, segmenter
        self.lowres = detections.lowres_route(segmenter, 'predict_boxes_lowres', lowres)
        self.boxes_per_batch, self.capacity = int(boxes_per_batch), int(capacity)

    @property
    def prompts(self) -> List[str]:
        return self.core.config['prompt'].split('.')

    def segment(self, image_np: np.ndarray, device=None) -> Tuple[torch.Tensor, List[ObjectInfo]]:
        """`segment_with_text` (grounding_dino.py:78-142): the frame -> (int64 index mask at `detection_size`, on the
        device; [ObjectInfo(id, category_id, score)] in paint order)"""
        cfg = self.core.config
        h, w = image_np.shape[:2]
        size = detections.detection_size(h, w, cfg['size'])
        self.segmenter.set_image(image_np)                      # before the detector, as the reference does (:93)
        threshold = cfg['DINO_THRESHOLD']
        boxes, confidences, class_ids = self.detector.predict_with_classes(image_np, self.prompts, box_threshold=threshold,
                                                                           text_threshold=threshold)
        found = detections.text_detections(boxes, confidences, class_ids, self.segmenter, (h, w), size,
                                           nms_threshold=cfg['DINO_NMS_THRESHOLD'], boxes_per_batch=self.boxes_per_batch,
                                           capacity=self.capacity, device=torch.device('cuda') if device is None else device,
                                           lowres=self.lowres)
        if hasattr(self.segmenter, 'reset_image'):
            self.segmenter.reset_image()
        return found

    def _detect(self, image: torch.Tensor, image_np: np.ndarray) -> Tuple[torch.Tensor, List[ObjectInfo]]:
        return self.segment(image_np, device=image.device)
