"""TEST INFRASTRUCTURE of tests/test_reference_text_loop_cpu.py: run the reference's UNCHANGED text-prompted frame loop
(deva/ext/with_text_processor.py `process_frame_with_text`, deva/ext/grounding_dino.py `segment_with_text`,
demo_utils.py `flush_buffer`) on top of this package, and `TextPromptedProcessor` on the same clip, in this process, with

* sys.path = [overlay package, reference checkout]  -- INTEGRATION.md's PYTHONPATH order: deva.ext, demo_utils,
  frame_utils and result_utils resolve to the reference's modules, the core to this package;
* stand-in modules for what those import and this image lacks: cv2 (`cvtColor` hands the frame on unchanged),
  torchvision (`ops.nms` is this project's statement of torchvision's CPU rule, tests/emu_text.py:nms_xyxy),
  groundingdino, segment_anything, supervision, pycocotools and the SAM variants under deva/ext;
* the fakes of tests/text_case.py behind the interfaces the reference calls (a GroundingDINO `Model` whose
  `predict_with_classes` returns a Detections-like object, a `SamPredictor` whose `predict(box=, multimask_output=True)`
  returns three masks and scores), without the equal-area tie (tests/text_case.py says why);
* without a GPU: the HIP ops replaced by their CPU statements and `.cuda()` turned into a no-op.

It compares, exactly: every index mask and segment list handed to `incorporate_detection`, its keywords, and every
saved probability, bit for bit; a differing pixel is printed with both values.  Exit code 0: everything agrees.

usage: python tests/run_reference_text_loop.py <online|semionline> <state_dict.pth>"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('DEVA_REFERENCE_ROOT', '/root/reference')


class _Lenient(types.ModuleType):
    """a module that has every attribute: a placeholder type per name"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


class _Setter:
    @staticmethod
    def setattr(obj, name, value):
        setattr(obj, name, value)


def install_stand_ins():
    import run_reference_driver as RD
    import emu_text as ET
    RD.install_third_party_stubs()
    for name in ('segment_anything', 'cv2', 'groundingdino', 'groundingdino.util', 'groundingdino.util.inference',
                 'deva.ext.MobileSAM', 'deva.ext.MobileSAM.setup_mobile_sam', 'deva.ext.LightHQSAM',
                 'deva.ext.LightHQSAM.setup_light_hqsam'):
        sys.modules[name] = _Lenient(name)
    sys.modules['supervision'] = _Lenient('supervision')
    sys.modules['torchvision.ops'].nms = lambda boxes, scores, threshold: torch.tensor(
        ET.nms_xyxy(boxes.numpy(), scores.numpy(), threshold), dtype=torch.int64)
    sys.modules['cv2'].cvtColor = lambda image, code: image
    sys.modules['cv2'].COLOR_RGB2BGR = 4
    if not torch.cuda.is_available():
        import emu_detections
        import emu_ops
        import emu_proposals
        RD.install_cpu_shims()
        for emu in (emu_ops, emu_detections, emu_proposals, ET):
            emu.install(_Setter)


class Detections:
    """what supervision's Detections gives the reference: `area` is the per-mask pixel count once masks are present"""

    def __init__(self, xyxy, confidence, class_id):
        self.xyxy, self.confidence, self.class_id, self.mask = xyxy, confidence, class_id, None

    @property
    def area(self):
        return np.array([m.sum() for m in self.mask]) if len(self.mask) else np.zeros(0)


class DinoModel:
    def __init__(self, detector, device):
        self.detector, self.device = detector, device

    def predict_with_classes(self, image, classes, box_threshold, text_threshold):
        return Detections(*self.detector.predict_with_classes(image, classes, box_threshold, text_threshold))


class SamPredictor:
    def __init__(self, segmenter, device):
        self.segmenter, self.device = segmenter, device

    def set_image(self, image, image_format='RGB'):
        assert image_format == 'RGB'
        self.segmenter.set_image(image)

    def predict(self, box, multimask_output):
        assert multimask_output
        boxes = torch.from_numpy(np.asarray(box, dtype=np.float32))[None].to(self.device)
        logits, scores = self.segmenter.predict_boxes(boxes)
        return (logits[0] > self.segmenter.mask_threshold).cpu().numpy(), scores[0].cpu().numpy(), None


class Saver:
    def __init__(self):
        self.saved = []

    def save_mask(self, prob, frame_name, need_resize=False, shape=None, image_np=None, prompts=None):
        self.saved.append((frame_name, prob.cpu().clone(), prompts))


def recorded(core, seen):
    real = core.incorporate_detection

    def recording(image, mask, segments_info, **kw):
        seen.append((mask.cpu().clone(), [(o.id, list(o.category_ids), [float(s) for s in o.scores]) for o in segments_info], kw))
        return real(image, mask, segments_info, **kw)

    core.incorporate_detection = recording


def main():
    setting, checkpoint = sys.argv[1], sys.argv[2]
    sys.path[:0] = [os.path.join(ROOT, 'tracking-anything-with-deva_amd'), REF, HERE, ROOT]
    install_stand_ins()
    torch.set_grad_enabled(False)
    import text_case as TC
    from deva.ext.with_text_processor import process_frame_with_text
    from deva.inference.demo_utils import flush_buffer
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.with_text import TextPromptedProcessor
    from deva.model.network import DEVA
    for name in ('deva.ext.with_text_processor', 'deva.ext.grounding_dino', 'deva.inference.demo_utils'):
        assert os.path.realpath(sys.modules[name].__file__).startswith(os.path.realpath(REF)), name
    assert not os.path.realpath(sys.modules['deva.inference.inference_core'].__file__).startswith(os.path.realpath(REF))
    device = torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
    net = DEVA(TC.loop_config(setting))
    net.load_weights(torch.load(checkpoint))
    net = net.to(device).eval()
    frames, rects = TC.clip()
    names = [f'{t:05d}.jpg' for t in range(len(frames))]

    # the reference's loop, as the demo drives it (demo/demo_with_text.py: next_voting_frame, then frame by frame, then flush)
    np.random.seed(11)
    core = DEVAInferenceCore(net, TC.loop_config(setting))
    core.next_voting_frame = core.config['num_voting_frames'] - 1
    theirs_seen, saver = [], Saver()
    recorded(core, theirs_seen)
    detector, segmenter = TC.FakeDetector(frames, rects, TC.HALVES, equal_halves=False), TC.FakeBoxSegmenter()
    for ti, (image_np, name) in enumerate(zip(frames, names)):
        process_frame_with_text(core, DinoModel(detector, device), SamPredictor(segmenter, device), '/clip/' + name, saver, ti,
                                image_np=image_np)
    flush_buffer(core, saver)
    theirs = saver.saved

    np.random.seed(11)
    core = DEVAInferenceCore(net, TC.loop_config(setting))
    ours_seen, saver = [], Saver()
    recorded(core, ours_seen)
    processor = TextPromptedProcessor(core, TC.FakeDetector(frames, rects, TC.HALVES, equal_halves=False), TC.FakeBoxSegmenter(),
                                      saver=types.SimpleNamespace(save_mask=lambda prob, name, **kw: saver.save_mask(prob, name)))
    for ti, (image_np, name) in enumerate(zip(frames, names)):
        processor.process_frame(image_np, ti, name)
    processor.flush()
    ours = saver.saved

    failures = 0
    print(f'{setting}: {len(theirs_seen)} detections incorporated by the reference loop, {len(ours_seen)} by TextPromptedProcessor')
    if len(theirs_seen) != len(ours_seen) or len(theirs_seen) != 3:
        failures += 1
    for k, ((mask_a, info_a, kw_a), (mask_b, info_b, kw_b)) in enumerate(zip(theirs_seen, ours_seen)):
        print(f'  detection {k}: segments {info_a}')
        if kw_a != {} or kw_b != {}:
            failures += 1
            print(f'  detection {k}: keywords {kw_a} (reference) / {kw_b} (ours)')
        if info_a != info_b:
            failures += 1
            print(f'  detection {k}: segments differ, ours {info_b}')
        if mask_a.shape != mask_b.shape or not torch.equal(mask_a, mask_b):
            failures += 1
            for y, x in (mask_a != mask_b).nonzero()[:20].tolist() if mask_a.shape == mask_b.shape else []:
                print(f'  detection {k}: pixel (y={y}, x={x}) is {int(mask_a[y, x])} in the reference, {int(mask_b[y, x])} in ours')
    if [n for n, _, _ in theirs] != names or [n for n, _, _ in ours] != names:
        failures += 1
        print('  saved frames:', [n for n, _, _ in theirs], [n for n, _, _ in ours])
    if any(p != ['person', 'dog', 'a hat'] for _, _, p in theirs):
        failures += 1
    for (name, a, _), (_, b, _) in zip(theirs, ours):
        same = a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
        if not same:
            failures += 1
            print(f'  {name}: probabilities differ, shapes {tuple(a.shape)} / {tuple(b.shape)}')
    print(f'{len(theirs)} frames compared, {max(p.shape[0] for _, p, _ in theirs)} channels at most, {failures} failures')
    sys.exit(1 if failures else 0)


if __name__ == '__main__':
    main()
