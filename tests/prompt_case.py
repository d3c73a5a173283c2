"""The input recipe of the prompt-point tests (tests/test_prompts_cpu.py, tests/test_gpu_r_prompts.py) and of
tests/golden/make_prompt_golden.py, which runs the REFERENCE's auto_segment on the same masks: forward masks with
drifting discs and rectangles (ids up to beyond 2^31, as long ids are), the prompt grid, the clip of the frame-loop tests
and its fake segmenter.  Everything is regenerated from seeds: the golden file holds the kept points only."""
import hashlib

import numpy as np
import torch

import driver_loops

LONG_IDS = (7, 255, 256, (1 << 31) + 5, (1 << 40) + 3, 12)


def forward_mask(h, w, seed, t=0, *, objects=5):
    """int64 [h,w]: `objects` discs and rectangles on background 0, each drifting with t; ids from LONG_IDS"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), dtype=np.int64)
    for k in range(objects):
        cy, cx = rng.uniform(0.1, 0.9) * h + 1.5 * t, rng.uniform(0.1, 0.9) * w + 2.5 * t
        ry, rx = rng.uniform(0.08, 0.3) * h, rng.uniform(0.08, 0.3) * w
        if k % 2 == 0:
            inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        else:
            inside = (np.abs(yy - cy) <= ry * 0.8) & (np.abs(xx - cx) <= rx * 0.8)
        m[inside] = LONG_IDS[k % len(LONG_IDS)]
    return torch.from_numpy(m)


def grid(n):
    """the grid of automatic_sam.py:74-81, fp32 [n*n,2] on the CPU (what `detections.prompt_grid` uploads)"""
    from deva.inference import detections
    return detections.prompt_grid(n, 'cpu')


# name -> (h, w, n_per_side, seed, t); 'covered' is all foreground: no point is left and the generator is never called
GOLDEN_CASES = {
    '1080x1920_n32': (1080, 1920, 32, 3, 0),
    '1080x1920_n32_t9': (1080, 1920, 32, 3, 9),
    '480x854_n32': (480, 854, 32, 4, 2),
    '481x853_n32': (481, 853, 32, 5, 1),
    '96x128_n8': (96, 128, 8, 6, 0),
    'covered_96x128_n8': (96, 128, 8, None, 0),
}


def golden_mask(name):
    h, w, n, seed, t = GOLDEN_CASES[name]
    if seed is None:
        return torch.full((h, w), 9, dtype=torch.int64)
    return forward_mask(h, w, seed, t)


# ------------------------------------------------------------------------------------------ the frame-loop clip
CLIP_FRAMES = 13


def clip():
    """the 96 x 128 clip of driver_loops.semionline_clip as numpy RGB frames, and the rectangles (y0, y1, x0, x1) its
    detections draw on every frame"""
    frames, _ = driver_loops.semionline_clip(frames=CLIP_FRAMES)
    rects = []
    for t in range(CLIP_FRAMES):
        r = [(12, 52, 10 + 2 * t, 58 + 2 * t)]
        if t % 4 != 1:
            r.append((56, 92, 66, 122))
        if t == 0:
            r.append((60, 90, 4, 30))
        rects.append(r)
    return [f.numpy() for f in frames], rects


def loop_config(temporal_setting, **over):
    from workload import synth
    cfg = synth.base_config(mem_every=2, max_missed_detection_count=2, max_num_objects=-1, size=-1,
                            suppress_small_objects=True, temporal_setting=temporal_setting, num_voting_frames=3,
                            detection_every=5, SAM_NUM_POINTS_PER_SIDE=8, SAM_NUM_POINTS_PER_BATCH=24,
                            SAM_PRED_IOU_THRESHOLD=0.88, SAM_OVERLAP_THRESHOLD=0.8)
    cfg.update(over)
    return cfg


class FakeSegmenter:
    """a point-prompted segmenter that knows the clip: a point inside rectangle r of the frame given to `set_image`
    yields three logit planes of that rectangle grown by 0, 1 and 2 pixels (+8 inside, -8 outside: stability 1) with
    predicted IoUs 0.96, 0.95 and 0.94; a point on background yields three empty planes with a predicted IoU of 0.5,
    which the filter drops unread.  `calls` records every call."""
    MARGINS, IOUS = (0, 1, 2), (0.96, 0.95, 0.94)

    def __init__(self, frames, rects):
        self.by_frame = {hashlib.sha1(f.tobytes()).hexdigest(): r for f, r in zip(frames, rects)}
        self.rects, self.shape, self.calls = None, None, []

    def set_image(self, image_np):
        self.rects, self.shape = self.by_frame[hashlib.sha1(image_np.tobytes()).hexdigest()], image_np.shape[:2]
        self.calls.append(('set_image', None))

    def predict_points(self, points_px):
        assert points_px.dtype == torch.float32 and points_px.dim() == 2 and points_px.shape[1] == 2
        h, w = self.shape
        pts = points_px.cpu().numpy()
        self.calls.append(('predict_points', pts.copy()))
        logits = torch.full((len(pts) * 3, h, w), -8.0)
        iou = torch.full((len(pts) * 3,), 0.5)
        for i, (x, y) in enumerate(pts):
            for y0, y1, x0, x1 in self.rects:
                if y0 <= y < y1 and x0 <= x < x1:
                    for m, margin in enumerate(self.MARGINS):
                        logits[3 * i + m, max(y0 - margin, 0):y1 + margin, max(x0 - margin, 0):x1 + margin] = 8.0
                        iou[3 * i + m] = self.IOUS[m]
                    break
        return logits.to(points_px.device), iou.to(points_px.device)

    def reset_image(self):
        self.calls.append(('reset_image', None))

    def asked(self):
        """the pixel points of every `predict_points` since the last `set_image`, and how many frames were set"""
        return [c[1] for c in self.calls if c[0] == 'predict_points']
