"""Generate tests/golden/prompt_points.npz by running the REFERENCE's own auto_segment (deva/ext/automatic_sam.py) on
the forward masks of tests/prompt_case.py and recording the `positive_points` it hands to the mask generator.

Run where a checkout of the reference exists:
    DEVA_REFERENCE_ROOT=<reference checkout> python tests/golden/make_prompt_golden.py
automatic_sam.py imports detectors that are not installed here (segment_anything, the SAM variants under deva/ext);
lenient stand-in modules are registered before the import, as make_detection_golden.py does, and the generator is a fake
with `.predictor.device` ('cpu': the whole statement runs on the CPU) whose `generate(image, positive, negative)` records
its arguments and returns no mask.  Only the kept points are stored (the recipe regenerates the masks); a case whose
mask leaves no point must never reach the generator.  Nothing here is imported by the product or the tests."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('DEVA_REFERENCE_ROOT')
if not REF or not os.path.isdir(os.path.join(REF, 'deva')):
    sys.exit('make_prompt_golden: set DEVA_REFERENCE_ROOT to a checkout of the reference')


class _Lenient(types.ModuleType):
    """a module that has every attribute: a placeholder type per name"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


for name in ('segment_anything', 'torchvision', 'torchvision.ops', 'cv2', 'deva.ext.MobileSAM',
             'deva.ext.MobileSAM.setup_mobile_sam', 'deva.ext.SAM', 'deva.ext.SAM.automatic_mask_generator', 'pulp'):
    sys.modules.setdefault(name, _Lenient(name))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)
from deva.ext.automatic_sam import auto_segment  # noqa: E402

torch.set_grad_enabled(False)


class RecordingGenerator:
    def __init__(self):
        self.predictor = types.SimpleNamespace(device='cpu')
        self.calls = []

    def generate(self, image, positive_points=None, negative_points=None):
        assert negative_points is None
        self.calls.append(np.array(positive_points, dtype=np.float32, copy=True))
        h, w = image.shape[:2]
        return {'masks': torch.zeros(0, h, w, dtype=torch.bool), 'iou_preds': torch.zeros(0)}


if __name__ == '__main__':
    import prompt_case as PC   # (its masks need no `deva`: sys.modules holds the reference's)
    arrays = {}
    for name in PC.GOLDEN_CASES:
        mask, (h, w, n, seed, t) = PC.golden_mask(name), PC.GOLDEN_CASES[name]
        gen = RecordingGenerator()
        image = np.zeros((h, w, 3), dtype=np.uint8)
        out, info = auto_segment({'SAM_NUM_POINTS_PER_SIDE': n, 'SAM_OVERLAP_THRESHOLD': 0.8}, gen, image, mask, 0, True)
        assert tuple(out.shape) == (h, w) and info == [] and len(gen.calls) <= 1
        points = gen.calls[0] if gen.calls else np.zeros((0, 2), dtype=np.float32)
        arrays[name + '/points'] = points.astype(np.float32)
        arrays[name + '/called'] = np.array(len(gen.calls), dtype=np.int64)
        print(name, 'kept', len(points), 'of', n * n, 'generator calls', len(gen.calls))
    where = os.path.join(HERE, 'prompt_points.npz')
    np.savez_compressed(where, **arrays)
    print('prompt_points.npz', os.path.getsize(where))
