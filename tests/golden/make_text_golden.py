"""Generate tests/golden/text_segmentation.npz by running the REFERENCE's own segment_with_text
(deva/ext/grounding_dino.py:78-142) on the golden frame of tests/text_case.py: 12 detector boxes on a 48 x 64 frame, three
candidate masks per box, once with min_side 0 and once with a min_side that resizes (30: assembled at 30 x 40).

Run where a checkout of the reference exists:
    DEVA_REFERENCE_ROOT=<reference checkout> python tests/golden/make_text_golden.py
The module imports detectors that are not installed here (segment_anything, groundingdino, the SAM variants under
deva/ext) and torchvision / cv2; lenient stand-in modules are registered before the import, as
make_detection_golden.py does, and the detectors are the fakes of tests/text_case.py behind the interfaces the
reference calls:
  * a GroundingDINO model whose `predict_with_classes` gives xyxy / confidence / class_id (and `area`, the per-mask
    pixel count: supervision's definition once masks are present);
  * a SAM predictor whose `predict(box=, multimask_output=True)` returns the THREE masks of the fake segmenter
    (logits > 0) and their scores, so the reference's own np.argmax picks.
THE NMS INSIDE THIS FIXTURE IS NOT A TORCHVISION RUN.  torchvision is not installed where this was generated; the
stand-in `torchvision.ops.nms` is this project's statement of torchvision's CPU rule (tests/emu_text.py:nms_xyxy, rules
N1-N4 of include/deva_hip.h).  Everything after the NMS -- argmax, masks, areas, paint order, ids -- is the reference's
own code.  Nothing here is imported by the product or the tests."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('DEVA_REFERENCE_ROOT')
if not REF or not os.path.isdir(os.path.join(REF, 'deva')):
    sys.exit('make_text_golden: set DEVA_REFERENCE_ROOT to a checkout of the reference')


class _Lenient(types.ModuleType):
    """a module that has every attribute: a placeholder type per name"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


for name in ('segment_anything', 'torchvision', 'torchvision.ops', 'cv2', 'groundingdino', 'groundingdino.util',
             'groundingdino.util.inference', 'deva.ext.MobileSAM', 'deva.ext.MobileSAM.setup_mobile_sam',
             'deva.ext.LightHQSAM', 'deva.ext.LightHQSAM.setup_light_hqsam'):
    sys.modules.setdefault(name, _Lenient(name))
# the overlay in front of the reference (INTEGRATION.md's order): deva.ext resolves to the reference's modules,
# deva.hip (which tests/emu_text.py names for its error type) to this package
sys.path[:0] = [os.path.join(ROOT, 'tracking-anything-with-deva_amd'), REF, os.path.join(ROOT, 'tests'), ROOT]
import emu_text as ET  # noqa: E402
import text_case as TC  # noqa: E402

sys.modules['torchvision'].ops = sys.modules['torchvision.ops']
sys.modules['torchvision.ops'].nms = lambda boxes, scores, threshold: torch.tensor(
    ET.nms_xyxy(boxes.numpy(), scores.numpy(), threshold), dtype=torch.int64)
sys.modules['cv2'].cvtColor = lambda image, code: image
sys.modules['cv2'].COLOR_RGB2BGR = 4
from deva.ext.grounding_dino import segment_with_text  # noqa: E402

assert os.path.realpath(sys.modules['deva.ext.grounding_dino'].__file__).startswith(os.path.realpath(REF))
torch.set_grad_enabled(False)


class FakeDetections:
    def __init__(self, xyxy, confidence, class_id):
        self.xyxy, self.confidence, self.class_id, self.mask = xyxy, confidence, class_id, None

    @property
    def area(self):
        return np.array([m.sum() for m in self.mask]) if len(self.mask) else np.zeros(0)


class FakeDino:
    device = 'cpu'

    def predict_with_classes(self, image, classes, box_threshold, text_threshold):
        assert list(classes) == TC.GOLDEN_CLASSES
        return FakeDetections(*TC.golden_inputs())


class FakeSam:
    def __init__(self):
        self.segmenter = TC.FakeBoxSegmenter()

    def set_image(self, image, image_format):
        self.segmenter.set_image(image)

    def predict(self, box, multimask_output):
        assert multimask_output
        logits, scores = self.segmenter.predict_boxes(torch.from_numpy(np.asarray(box, dtype=np.float32))[None])
        return (logits[0] > self.segmenter.mask_threshold).numpy(), scores[0].numpy(), None


def run(min_side):
    image = np.zeros((*TC.GOLDEN_HW, 3), dtype=np.uint8)
    config = {'DINO_THRESHOLD': 0.35, 'DINO_NMS_THRESHOLD': TC.NMS_THRESHOLD}
    out, info = segment_with_text(config, FakeDino(), FakeSam(), image, TC.GOLDEN_CLASSES, min_side)
    assert out.dtype == torch.int64
    ids = np.array([o.id for o in info], dtype=np.int64)
    cats = np.array([-1 if o.category_ids[0] is None else int(o.category_ids[0]) for o in info], dtype=np.int64)
    vals = np.array([float(o.scores[0]) for o in info], dtype=np.float64)
    return out.numpy().astype(np.int16), ids, cats, vals


if __name__ == '__main__':
    boxes, conf, cls = TC.golden_inputs()
    h, w = TC.GOLDEN_HW
    answers = [TC.box_answer(b, h, w) for b in boxes]
    arrays = {'boxes': boxes, 'confidences': conf,
              'class_ids': np.array([-1 if c is None else int(c) for c in cls], dtype=np.int64),
              'logits': np.stack([a[0] for a in answers]), 'scores': np.stack([a[1] for a in answers])}
    assert len(boxes) <= 12 and arrays['logits'].shape == (len(boxes), 3, h, w)
    for min_side in TC.GOLDEN_MIN_SIDES:
        key = f'min_side_{min_side}'
        mask, ids, cats, vals = run(min_side)
        arrays[key + '/mask'], arrays[key + '/ids'], arrays[key + '/categories'], arrays[key + '/scores'] = mask, ids, cats, vals
        print(key, mask.shape, 'mask ids', np.unique(mask).tolist(), 'info ids', ids.tolist(), 'categories', cats.tolist())
    where = os.path.join(HERE, 'text_segmentation.npz')
    np.savez_compressed(where, **arrays)
    print('text_segmentation.npz', os.path.getsize(where))
