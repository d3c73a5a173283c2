"""Generate tests/golden/unsup_limit.npz by running the REFERENCE's own `limit_max_id`
(deva/inference/postprocess_unsup_davis17.py) on small trees of PNGs written here.

Run where a checkout of the reference exists:
    DEVA_REFERENCE_ROOT=<reference checkout> python tests/golden/make_unsup_golden.py

The reference's file is loaded by path under a stub `deva` package, so that `deva/__init__` (the whole model) is not
imported; its `deva.utils.palette` (data only) is loaded by path as well.  Only data is stored: the label planes fed in
(8 x 12), what the reference wrote for them and the palette of its files."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

REF = os.environ.get('DEVA_REFERENCE_ROOT')
if not REF:
    sys.exit('make_unsup_golden: set DEVA_REFERENCE_ROOT to a checkout of the reference')
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'unsup_limit.npz')
H, W = 8, 12


def load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


for pkg in ('deva', 'deva.utils'):
    sys.modules[pkg] = types.ModuleType(pkg)
    sys.modules[pkg].__path__ = []
load('deva.utils.palette', os.path.join(REF, 'deva', 'utils', 'palette.py'))
reference = load('reference_postprocess_unsup', os.path.join(REF, 'deva', 'inference', 'postprocess_unsup_davis17.py'))


def plane(boxes):
    """[(label, y0, y1, x0, x1)] painted in order -> int32 [H,W]"""
    out = np.zeros((H, W), dtype=np.int32)
    for label, y0, y1, x0, x1 in boxes:
        out[y0:y1, x0:x1] = label
    return out


# name -> (max_num_objects, rgb, {video: [planes]})
CASES = {
    # two labels in every frame and a third from frame 1 on: the list is 7 3 | 7 3 9 -> full at 4 entries as 7 3 7 3;
    # the reference appends without looking, so 7 -> 3, 3 -> 4 and 9 is never kept
    'quirk': (4, False, {'a': [plane([(7, 0, 4, 0, 6), (3, 4, 8, 0, 4)]),
                               plane([(7, 0, 4, 0, 6), (3, 4, 8, 0, 4), (9, 5, 8, 8, 12)]),
                               plane([(7, 0, 4, 1, 7), (3, 4, 8, 0, 4), (9, 4, 8, 7, 12)])]}),
    # areas 12, 12, 12, 6: the tie goes to the larger label first (sorted by (area, label), descending)
    'tie': (20, False, {'a': [plane([(2, 0, 3, 0, 4), (5, 0, 3, 4, 8), (4, 3, 6, 0, 4), (1, 6, 8, 0, 3)]),
                              plane([(2, 0, 3, 0, 4), (5, 0, 3, 4, 8), (4, 3, 6, 0, 4), (1, 6, 8, 0, 3), (8, 6, 8, 6, 12)])]}),
    # five labels in the first frame, three kept: the three largest
    'crowded': (3, False, {'a': [plane([(1, 0, 2, 0, 2), (2, 0, 4, 2, 8), (3, 4, 8, 0, 5), (4, 4, 6, 6, 9), (5, 6, 8, 6, 12)]),
                                 plane([(1, 0, 2, 0, 2), (2, 0, 4, 2, 8), (3, 4, 8, 0, 5), (6, 4, 8, 6, 12)])],
                           'b': [plane([(4, 0, 8, 0, 3)]), plane([]), plane([(4, 0, 8, 0, 3), (2, 0, 2, 4, 6)])]}),
    # the default of 20 with few labels: the list never fills, duplicates and all
    'default': (20, False, {'a': [plane([(11, 0, 4, 0, 6), (12, 4, 8, 0, 4)]), plane([(12, 0, 4, 0, 6), (13, 4, 8, 0, 4)]),
                                  plane([(11, 1, 3, 1, 3)])]}),
    # ids beyond a byte, written as R * 65536 + G * 256 + B
    'rgb': (4, True, {'a': [plane([(70000, 0, 4, 0, 6), (300, 4, 8, 0, 4), (5, 6, 8, 8, 12)]),
                            plane([(70000, 0, 4, 0, 6), (300, 4, 8, 0, 5), (65536, 0, 3, 8, 12)])]}),
}


def main():
    store = {}
    palette = None
    with tempfile.TemporaryDirectory() as root:
        for name, (max_num_objects, rgb, videos) in CASES.items():
            src, dst = os.path.join(root, name, 'in'), os.path.join(root, name, 'out')
            for video, planes in videos.items():
                os.makedirs(os.path.join(src, video))
                for t, p in enumerate(planes):
                    if rgb:
                        img = Image.fromarray(np.stack([p >> 16, (p >> 8) & 255, p & 255], axis=2).astype(np.uint8))
                    else:
                        img = Image.fromarray(p.astype(np.uint8), mode='P')
                        img.putpalette([v for i in range(256) for v in (i, i, i)])
                    img.save(os.path.join(src, video, '%05d.png' % t))
            reference.limit_max_id(src, dst, max_num_objects)
            store[f'{name}/max'] = np.int64(max_num_objects)
            store[f'{name}/rgb'] = np.bool_(rgb)
            for video, planes in videos.items():
                store[f'{name}/{video}/in'] = np.stack(planes).astype(np.int32)
                outs = []
                for t in range(len(planes)):
                    img = Image.open(os.path.join(dst, video, '%05d.png' % t))
                    assert img.mode == 'P'
                    palette = np.array(img.getpalette(), dtype=np.uint8)
                    outs.append(np.array(img))
                store[f'{name}/{video}/out'] = np.stack(outs).astype(np.uint8)
    store['palette'] = palette
    np.savez_compressed(OUT, **store)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(store)} arrays')


if __name__ == '__main__':
    main()
