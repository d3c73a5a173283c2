"""The input recipe of the text-prompted tests (tests/test_text_cpu.py, tests/test_gpu_s_text.py, the reference-loop test)
and of tests/golden/make_text_golden.py, which runs the REFERENCE's segment_with_text on the same fakes: a deterministic
detector, a box-prompted segmenter with three candidate masks per box, the clip of the frame-loop tests and the
straight-line restatement of the reference's loop.  Everything is regenerated from the rectangles of the clip.

What the detector reports for a frame whose objects are the rectangles (y0, y1, x0, x1), in this order:
  per rectangle k   `shifted` (the main box 1 px to the right, confidence 0.6), `main` (the rectangle shrunk by a
                    fraction of a pixel, confidence 0.9 - 0.1 k) and `dup` (the main box again, the same confidence: the
                    lower index wins the tie and suppresses it); class k % len(classes)
  `part`            a 6-pixel-wide box inside rectangle 0 with the confidence of main 0 (equal confidences among KEPT
                    boxes) and class None, GroundingDINO's unmatched phrase
  `right`, `left`   (only with `halves`) the right and the left 60 % of rectangle 0 with equal confidences 0.75
                    (`equal_halves=False`: the left 55 %, a smaller mask.  The REFERENCE paints in np.argsort order,
                    and numpy's default sort is not stable, on some processors not even for five elements: among equal
                    areas the reference's own order depends on the machine, so the runs of the reference itself --
                    the golden file and the reference-loop test -- leave the tie out; this package's order among equal
                    areas is fixed, include/deva_hip.h, and every other test keeps the tie)
With an NMS threshold of 0.8 the kept boxes are main 0, part, main 1, right, left, main 2, in that order.

What the segmenter answers for a box: three logit planes (+8 inside, -8 outside) of the box's pixel region grown by 2, 0
and 1 pixels; the best one is plane floor(2 y0) % 3 (score 0.9 against 0.5), so the best index differs between boxes:
  main 0            plane 1: the rectangle itself
  right, left       plane 0 (grown by 2): two masks of EQUAL areas that together paint main 0's mask over completely
  part              scores 0.7, 0.9, 0.9: a tie, the first maximum (plane 1) wins
  a box with x0 < 10 in the lower half of the frame (rectangle 2 of the clip's frame 0): its best plane is EMPTY"""
import hashlib

import numpy as np
import torch

import driver_loops
import prompt_case

MARGINS = (2, 0, 1)
NMS_THRESHOLD = 0.8
CLIP_FRAMES = prompt_case.CLIP_FRAMES


def detector_output(rects, n_classes, halves, equal_halves=True):
    """-> (xyxy fp32 [N,4], confidence fp32 [N], class_id object [N]) as GroundingDINO's wrapper returns them"""
    boxes, conf, cls = [], [], []
    for k, (y0, y1, x0, x1) in enumerate(rects):
        main = (x0 + 0.25, y0 + 0.5, x1 - 0.25, y1 - 0.5)
        for box, c in (((main[0] + 1.0, main[1], main[2] + 1.0, main[3]), 0.6), (main, 0.9 - 0.1 * k), (main, 0.9 - 0.1 * k)):
            boxes.append(box), conf.append(c), cls.append(k % n_classes)
    if rects:
        y0, y1, x0, x1 = rects[0]
        boxes.append((x0 + 4.5, y0 + 3.25, x0 + 10.5, y0 + 9.75)), conf.append(0.9), cls.append(None)
        if halves:
            part = 0.6 * (x1 - x0)
            boxes.append((x1 - part, y0, x1, y1)), conf.append(0.75), cls.append(1 % n_classes)
            boxes.append((x0, y0, x0 + (part if equal_halves else 0.55 * (x1 - x0)), y1)), conf.append(0.75), cls.append(0)
    return (np.array(boxes, dtype=np.float32).reshape(-1, 4), np.array(conf, dtype=np.float32),
            np.array(cls, dtype=object))


class FakeDetector:
    """knows the clip: `predict_with_classes` answers `detector_output` for the rectangles of the frame it is shown
    (the halves on the frames listed in `halves`).  `calls` records (classes, box_threshold, text_threshold)."""

    def __init__(self, frames, rects, halves=(), equal_halves=True):
        self.equal_halves = equal_halves
        self.by_frame = {hashlib.sha1(f.tobytes()).hexdigest(): (r, t in halves) for t, (f, r) in enumerate(zip(frames, rects))}
        self.calls = []

    def predict_with_classes(self, image, classes, box_threshold, text_threshold):
        rects, halves = self.by_frame[hashlib.sha1(np.ascontiguousarray(image).tobytes()).hexdigest()]
        self.calls.append((list(classes), box_threshold, text_threshold))
        return detector_output(rects, len(classes), halves, self.equal_halves)


def box_answer(box, h, w):
    """one box (x0, y0, x1, y1) -> (logits fp32 [3,h,w], scores fp32 [3])"""
    x0, y0, x1, y1 = (float(v) for v in box)
    key = int(np.floor(2 * y0)) % 3
    scores = np.full(3, 0.5, dtype=np.float32)
    scores[key] = 0.9
    if x1 - x0 < 8:
        scores[:] = (0.7, 0.9, 0.9)
        key = 1
    logits = np.full((3, h, w), -8.0, dtype=np.float32)
    for m, margin in enumerate(MARGINS):
        if m == key and x0 < 10 and y0 > h / 2:
            continue                                          # the best plane of this box is empty
        ya, yb = max(int(np.floor(y0)) - margin, 0), min(int(np.ceil(y1)) + margin, h)
        xa, xb = max(int(np.floor(x0)) - margin, 0), min(int(np.ceil(x1)) + margin, w)
        logits[m, ya:yb, xa:xb] = 8.0
    return logits, scores


class FakeBoxSegmenter:
    """a box-prompted segmenter: `predict_boxes` answers `box_answer` for every box at the size of the frame given to
    `set_image`.  `calls` records every call (the boxes of `predict_boxes` as numpy)."""
    mask_threshold = 0.0

    def __init__(self):
        self.shape, self.calls = None, []

    def set_image(self, image_np):
        self.shape = image_np.shape[:2]
        self.calls.append(('set_image', None))

    def predict_boxes(self, boxes_px):
        assert boxes_px.dtype == torch.float32 and boxes_px.dim() == 2 and boxes_px.shape[1] == 4 and boxes_px.shape[0] > 0
        h, w = self.shape
        boxes = boxes_px.cpu().numpy()
        self.calls.append(('predict_boxes', boxes.copy()))
        answers = [box_answer(b, h, w) for b in boxes]
        logits = torch.from_numpy(np.stack([a[0] for a in answers]))
        scores = torch.from_numpy(np.stack([a[1] for a in answers]))
        return logits.to(boxes_px.device), scores.to(boxes_px.device)

    def reset_image(self):
        self.calls.append(('reset_image', None))

    def asked(self):
        return [c[1] for c in self.calls if c[0] == 'predict_boxes']


# ------------------------------------------------------------------------------------------ the golden case
GOLDEN_HW = (48, 64)
GOLDEN_RECTS = [(6, 26, 5, 29), (28, 46, 33, 61), (30, 45, 2, 15)]
GOLDEN_CLASSES = ['person', 'dog', 'a hat']
GOLDEN_MIN_SIDES = (0, 30)            # 30: the 48 x 64 masks are assembled at 30 x 40


def golden_inputs(equal_halves=False):
    """-> boxes [12,4], confidences [12], class ids (object [12]) of the golden frame (no two masks of equal areas: see
    the module docstring)"""
    return detector_output(GOLDEN_RECTS, len(GOLDEN_CLASSES), True, equal_halves)


# ------------------------------------------------------------------------------------------ the frame-loop clip
HALVES = (5,)                         # a frame with one rectangle, a detection frame of both settings: its halves are reported too


def clip():
    """the 13-frame 96 x 128 clip of prompt_case.clip(): numpy RGB frames and the rectangles of every frame"""
    return prompt_case.clip()


def loop_config(temporal_setting, **over):
    from workload import synth
    cfg = synth.base_config(mem_every=2, max_missed_detection_count=2, max_num_objects=-1, size=-1,
                            temporal_setting=temporal_setting, num_voting_frames=3, detection_every=5,
                            prompt='person.dog.a hat', DINO_THRESHOLD=0.35, DINO_NMS_THRESHOLD=NMS_THRESHOLD)
    cfg.update(over)
    return cfg


class RecordingSaver:
    def __init__(self):
        self.saved = []

    def save_mask(self, prob, frame_name, need_resize=False, shape=None, image_np=None):
        self.saved.append((frame_name, prob, need_resize, tuple(shape), image_np))


def restated_loop(core, detector, segmenter, frames, names, *, boxes_per_batch=16, capacity=256, seen=None):
    """deva/ext/with_text_processor.py:30-122, grounding_dino.py:78-100 and demo_utils.py:22-46, restated in a straight
    line against the public pieces (no TextPromptedProcessor) -> [(frame name, prob)] in the order the reference saves
    them.  `seen` collects (index mask, segments) of every incorporate_detection."""
    from deva.inference import detections as D
    from deva.utils.tensor_utils import frame_to_network_input
    cfg = core.config
    prompts = cfg['prompt'].split('.')
    saved = []
    next_voting_frame = cfg['num_voting_frames'] - 1

    def make_segmentation_with_text(image_np, device):
        h, w = image_np.shape[:2]
        segmenter.set_image(image_np)
        xyxy, confidence, class_id = detector.predict_with_classes(image_np, prompts, box_threshold=cfg['DINO_THRESHOLD'],
                                                                   text_threshold=cfg['DINO_THRESHOLD'])
        return D.text_detections(xyxy, confidence, class_id, segmenter, (h, w), D.detection_size(h, w, cfg['size']),
                                 nms_threshold=cfg['DINO_NMS_THRESHOLD'], boxes_per_batch=boxes_per_batch, capacity=capacity,
                                 device=device)

    def incorporate(image, mask, segments_info):
        if seen is not None:
            seen.append((mask.cpu().clone(), [(o.id, list(o.category_ids), list(o.scores)) for o in segments_info]))
        return core.incorporate_detection(image, mask, segments_info)

    for ti, (image_np, frame_name) in enumerate(zip(frames, names)):
        image = frame_to_network_input(image_np, cfg['size'], antialias=False)
        h, w = image_np.shape[:2]
        if cfg['temporal_setting'] == 'semionline':
            if ti + cfg['num_voting_frames'] > next_voting_frame:
                mask, segments_info = make_segmentation_with_text(image_np, image.device)
                frame_info = driver_loops.FrameInfo(image, mask, segments_info, ti, {'frame': [frame_name], 'shape': [h, w]})
                frame_info.image_np = image_np
                core.add_to_temporary_buffer(frame_info)
                if ti == next_voting_frame:
                    this_image, this_frame_name = core.frame_buffer[0].image, core.frame_buffer[0].name
                    _, mask, new_segments_info = core.vote_in_temporary_buffer(keyframe_selection='first')
                    prob = incorporate(this_image, mask, new_segments_info)
                    next_voting_frame += cfg['detection_every']
                    saved.append((this_frame_name, prob))
                    for frame_info in core.frame_buffer[1:]:
                        saved.append((frame_info.name, core.step(frame_info.image, None, None)))
                    core.clear_buffer()
            else:
                saved.append((frame_name, core.step(image, None, None)))
        elif cfg['temporal_setting'] == 'online':
            if ti % cfg['detection_every'] == 0:
                mask, segments_info = make_segmentation_with_text(image_np, image.device)
                prob = incorporate(image, mask, segments_info)
            else:
                prob = core.step(image, None, None)
            saved.append((frame_name, prob))
    for frame_info in core.frame_buffer:                      # flush_buffer
        saved.append((frame_info.name, core.step(frame_info.image, None, None)))
    return saved


def run_processor(core, detector, segmenter, frames, names, saver=None, **kw):
    """the same clip through TextPromptedProcessor -> ([(frame name, prob)], what `flush` alone produced, the processor)"""
    from deva.inference.with_text import TextPromptedProcessor
    processor = TextPromptedProcessor(core, detector, segmenter, saver=saver, **kw)
    produced = []
    for ti, (image_np, name) in enumerate(zip(frames, names)):
        produced += processor.process_frame(image_np, ti, name)
    flushed = processor.flush()
    return produced + flushed, flushed, processor


def check_clip(setting, make_core, monkeypatch):
    """both runs of one temporal setting; shared by the CPU test (emulated ops) and tests/test_gpu_s_text.py.
    -> (what the processor produced, what `flush` produced, the processor, the keywords of every incorporate_detection)"""
    frames, rects = clip()
    names = [f'{t:05d}.jpg' for t in range(len(frames))]
    np.random.seed(11)
    want_seen = []
    want = restated_loop(make_core(setting), FakeDetector(frames, rects, HALVES), FakeBoxSegmenter(), frames, names, seen=want_seen)
    detector, segmenter, saver = FakeDetector(frames, rects, HALVES), FakeBoxSegmenter(), RecordingSaver()
    core = make_core(setting)
    keywords, got_seen = [], []
    real = core.incorporate_detection

    def recording(image, mask, segments_info, **kw):
        keywords.append(kw)
        got_seen.append((mask.cpu().clone(), [(o.id, list(o.category_ids), list(o.scores)) for o in segments_info]))
        return real(image, mask, segments_info, **kw)

    monkeypatch.setattr(core, 'incorporate_detection', recording)
    np.random.seed(11)
    got, flushed, processor = run_processor(core, detector, segmenter, frames, names, saver)
    assert [n for n, _ in got] == [n for n, _ in want] == names                   # every frame once, in order
    for (name, a), (_, b) in zip(got, want):
        assert a.shape[0] >= 2 and torch.equal(a.cpu(), b.cpu()), name            # bit-identical probabilities
    assert len(got_seen) == len(want_seen) == 3 and max(len(info) for _, info in got_seen) >= 3
    for (mask_a, info_a), (mask_b, info_b) in zip(got_seen, want_seen):
        assert torch.equal(mask_a, mask_b) and info_a == info_b and len(info_a) >= 1
    assert [s[0] for s in saver.saved] == names and all(s[2] is False and s[3] == (96, 128) for s in saver.saved)
    assert all(s[1] is p for s, (_, p) in zip(saver.saved, got)) and all(s[4] is f for s, f in zip(saver.saved, frames))
    # the detector saw the prompt split on '.', both thresholds DINO_THRESHOLD, and every detection frame set the image first
    assert all(c == (['person', 'dog', 'a hat'], 0.35, 0.35) for c in detector.calls)
    kinds = [c[0] for c in segmenter.calls]
    assert kinds.count('set_image') == len(detector.calls) == (3 if setting == 'online' else 9)
    assert all(0 < len(b) <= 16 for b in segmenter.asked())
    return got, flushed, processor, keywords
