"""Generate tests/golden/result_saver.npz / .json by running the REFERENCE's own ResultSaver + save_result
(deva/inference/result_utils.py) on the case of tests/result_case.py.

Run where a checkout of the reference exists:
    DEVA_REFERENCE_ROOT=<reference checkout> python tests/golden/make_result_golden.py
The reference module imports torchvision, pycocotools and supervision at module level; none of them is installed here
and none is reached by the datasets generated (vipseg, demo without prompts, unsup_davis17), so empty stand-in modules
are registered before the import, as make_golden.py does for `pulp`.  Nothing here is imported by the product or the
tests."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('DEVA_REFERENCE_ROOT')
if not REF or not os.path.isdir(os.path.join(REF, 'deva')):
    sys.exit('make_result_golden: set DEVA_REFERENCE_ROOT to a checkout of the reference')
for name in ('pulp', 'torchvision', 'pycocotools', 'pycocotools.mask', 'supervision'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules['pycocotools'].mask = sys.modules['pycocotools.mask']
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)
from deva.inference.object_info import ObjectInfo  # noqa: E402
from deva.inference.object_manager import ObjectManager  # noqa: E402
from deva.inference.result_utils import ResultSaver  # noqa: E402

import result_case as RC  # noqa: E402

torch.set_grad_enabled(False)


def decoded(root):
    """every PNG under root -> {relative path: array}, palettes under '<path>#palette'"""
    out = {}
    for base, _, files in os.walk(root):
        for f in sorted(files):
            rel = os.path.relpath(os.path.join(base, f), root)
            if f.endswith('.png'):
                img = Image.open(os.path.join(base, f))
                out[rel] = np.array(img)
                if img.mode == 'P':
                    out[rel + '#palette'] = np.array(img.getpalette(), dtype=np.uint8)
            else:
                out[rel] = np.array(Image.open(os.path.join(base, f)).size)   # (lossy: only that it exists, and its size)
    return out


if __name__ == '__main__':
    arrays, jsons = {}, {}
    for dataset in RC.DATASETS:
        with tempfile.TemporaryDirectory() as root:
            saver, _ = RC.run_saver(ResultSaver, ObjectManager, ObjectInfo, dataset, root)
            for rel, a in decoded(root).items():
                arrays[f'{dataset}/{rel}'] = a
            if saver.json_style is not None:
                jsons[dataset] = saver.video_json
    np.savez_compressed(os.path.join(HERE, 'result_saver.npz'), **arrays)
    with open(os.path.join(HERE, 'result_saver.json'), 'w') as f:
        json.dump(jsons, f, indent=1, sort_keys=True)
    for k, a in arrays.items():
        print(k, a.shape, a.dtype)
    print({k: [len(a['segments_info']) for a in v['annotations']] for k, v in jsons.items()})
    for f in ('result_saver.npz', 'result_saver.json'):
        print(f, os.path.getsize(os.path.join(HERE, f)))
