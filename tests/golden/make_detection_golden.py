"""Generate tests/golden/detection_assembly.npz by running the REFERENCE's own auto_segment (deva/ext/automatic_sam.py)
and segment_with_text (deva/ext/grounding_dino.py) on the case of tests/detection_case.py.

Run where a checkout of the reference exists:
    DEVA_REFERENCE_ROOT=<reference checkout> python tests/golden/make_detection_golden.py
The two modules import detectors that are not installed here (segment_anything, groundingdino, the SAM variants under
deva/ext) and torchvision / cv2; lenient stand-in modules are registered before the import, as make_result_golden.py
does, and the detectors themselves are replaced by fakes that hand out the case's masks:
  * a mask generator with `.predictor.device` and `.generate()` -> {'masks', 'iou_preds'}
  * a GroundingDINO model whose `predict_with_classes` gives xyxy / confidence / class_id (and `area`, the per-mask
    pixel count: supervision's definition once masks are present), an identity `nms`, and a SAM predictor whose
    `predict` returns the case's mask as the best of three.
Nothing here is imported by the product or the tests."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('DEVA_REFERENCE_ROOT')
if not REF or not os.path.isdir(os.path.join(REF, 'deva')):
    sys.exit('make_detection_golden: set DEVA_REFERENCE_ROOT to a checkout of the reference')


class _Lenient(types.ModuleType):
    """a module that has every attribute: a placeholder type per name"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


for name in ('segment_anything', 'torchvision', 'torchvision.ops', 'cv2', 'groundingdino', 'groundingdino.util',
             'groundingdino.util.inference', 'deva.ext.MobileSAM', 'deva.ext.MobileSAM.setup_mobile_sam',
             'deva.ext.LightHQSAM', 'deva.ext.LightHQSAM.setup_light_hqsam', 'deva.ext.SAM',
             'deva.ext.SAM.automatic_mask_generator', 'pulp'):
    sys.modules.setdefault(name, _Lenient(name))
sys.modules['torchvision'].ops = sys.modules['torchvision.ops']
sys.modules['torchvision.ops'].nms = lambda boxes, scores, threshold: torch.arange(len(boxes))     # identity
sys.modules['cv2'].cvtColor = lambda image, code: image
sys.modules['cv2'].COLOR_RGB2BGR = 4
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)
from deva.ext.automatic_sam import auto_segment  # noqa: E402
from deva.ext.grounding_dino import segment_with_text  # noqa: E402

import detection_case as DC  # noqa: E402

torch.set_grad_enabled(False)


class FakeGenerator:
    def __init__(self, masks, scores):
        self.predictor = types.SimpleNamespace(device='cpu')
        self.masks, self.scores = masks, scores

    def generate(self, image):
        return {'masks': self.masks, 'iou_preds': self.scores}


class FakeDetections:
    """xyxy: box i is (i, 0, i + 1, 1), which is how the fake SAM below knows the mask asked for"""

    def __init__(self, masks):
        n = len(masks)
        self.xyxy = np.stack([np.arange(n), np.zeros(n), np.arange(n) + 1, np.ones(n)], axis=1).astype(np.float32).reshape(n, 4)
        self.confidence = DC.confidences(n)
        self.class_id = DC.class_ids(n)
        self.mask = None

    @property
    def area(self):
        return np.array([m.sum() for m in self.mask]) if len(self.mask) else np.zeros(0)


class FakeDino:
    device = 'cpu'

    def __init__(self, masks):
        self.masks = masks

    def predict_with_classes(self, image, classes, box_threshold, text_threshold):
        return FakeDetections(self.masks)


class FakeSam:
    def __init__(self, masks):
        self.masks = masks

    def set_image(self, image, image_format):
        pass

    def predict(self, box, multimask_output):
        mask = self.masks[int(box[0])]
        return np.stack([np.zeros_like(mask), mask, np.ones_like(mask)]), np.array([0.1, 0.9, 0.2]), None


def run(policy, threshold, size_in, size_out, n):
    masks = DC.case_masks(size_in, n)
    image = np.zeros((*size_out, 3), dtype=np.uint8)     # min_side = 0: the output has the image's size
    if policy == 'text':
        planes = masks.numpy()
        areas = planes.reshape(n, size_in[0] * size_in[1]).sum(1)
        if n and not np.array_equal(np.flip(np.argsort(areas)), np.flip(np.argsort(areas, kind='stable'))):
            print('NOTE', size_in, n, ': numpy\'s default argsort is not the stable one on these areas')
        config = {'DINO_THRESHOLD': 0.35, 'DINO_NMS_THRESHOLD': 0.8}
        out, info = segment_with_text(config, FakeDino(planes), FakeSam(planes), image, ['a'], 0)
    else:
        config = {'SAM_OVERLAP_THRESHOLD': threshold}
        out, info = auto_segment(config, FakeGenerator(masks, DC.scores(n)), image, None, 0, policy == 'suppress')
    assert tuple(out.shape) == tuple(size_out) and out.dtype == torch.int64
    ids = np.array([o.id for o in info], dtype=np.int64)
    cats = np.array([-1 if o.category_ids[0] is None else int(o.category_ids[0]) for o in info], dtype=np.int64)
    vals = np.array([float(o.scores[0]) for o in info], dtype=np.float64)
    return out.numpy().astype(np.int16), ids, cats, vals


if __name__ == '__main__':
    arrays = {}
    for case in DC.golden_cases():
        key = DC.golden_key(*case)
        mask, ids, cats, vals = run(*case)
        arrays[key + '/mask'], arrays[key + '/ids'], arrays[key + '/categories'], arrays[key + '/scores'] = mask, ids, cats, vals
        print(key, mask.shape, 'mask ids', np.unique(mask).tolist(), 'info ids', ids.tolist())
    where = os.path.join(HERE, 'detection_assembly.npz')
    np.savez_compressed(where, **arrays)
    print('detection_assembly.npz', os.path.getsize(where))
