"""Shared case of the result-saver tests (tests/golden/make_result_golden.py runs the reference's ResultSaver on it,
tests/test_frame_result_cpu.py the package's FrameResultSaver): a seeded 3-object, 4-frame, 48 x 64 probability
sequence in which object 3 vanishes on frame 2, with the object tables of three datasets."""
import numpy as np
import torch

H, W, FRAMES = 48, 64, 4
NAMES = [f'{t:05d}.jpg' for t in range(FRAMES)]
RESIZED = (60, 80)          # the vipseg leg saves at another size (need_resize)
# dataset -> (long ids, [(object id, category, score)], save at RESIZED)
DATASETS = {
    'vipseg': (True, [(1000, 3, 0.9), (70000, 17, 0.5), (66051, 3, None)], True),
    'demo': (True, [(300, 0, 0.75), (65536 * 5 + 7, 1, 0.25), (256, None, None)], False),
    'unsup_davis17': (False, [(5, None, None), (9, None, None), (200, None, None)], False),
}
BURST = (False, [(7, 2, 0.5), (3, 4, 0.125), (250, 2, 1.0)], False)


def probabilities():
    """-> list of [4,48,64] fp32 tensors (softmax of smooth seeded logits; channel 3 is zero on frame 2)"""
    g = torch.Generator().manual_seed(2024)
    out = []
    for t in range(FRAMES):
        coarse = torch.randn(1, 4, 6, 8, generator=g) * 3
        logits = torch.nn.functional.interpolate(coarse, (H, W), mode='bilinear', align_corners=False)[0]
        logits = logits + torch.randn(4, H, W, generator=g) * 0.3
        p = torch.softmax(logits, dim=0)
        if t == 2:
            p[3] = 0
            p = p / p.sum(0, keepdim=True)
        out.append(p.contiguous())
    return out


def images(size):
    g = torch.Generator().manual_seed(77)
    return [torch.randint(0, 256, (*size, 3), generator=g, dtype=torch.uint8).numpy() for _ in range(FRAMES)]


def palette():
    """a 256-colour palette as bytes (seeded; entry 0 black)"""
    rng = np.random.default_rng(5)
    pal = rng.integers(0, 256, size=(256, 3), dtype=np.uint8)
    pal[0] = 0
    return pal.tobytes()


def object_manager(make_manager, make_info, long_id, objects):
    om = make_manager()
    om.use_long_id = long_id
    om.add_new_objects([make_info(id=i, category_id=c, score=s) for i, c, s in objects])
    return om


def run_saver(make_saver, make_manager, make_info, dataset, root, spec=None):
    """drive one saver over the clip -> (saver after end(), object manager)"""
    long_id, objects, resized = spec or DATASETS[dataset]
    om = object_manager(make_manager, make_info, long_id, objects)
    saver = make_saver(root, 'clip', dataset=dataset, object_manager=om,
                       palette=None if long_id else palette())
    size = RESIZED if resized else (H, W)
    for t, (prob, image) in enumerate(zip(probabilities(), images(size))):
        saver.save_mask(prob, NAMES[t], need_resize=resized, shape=size if resized else None, image_np=image)
        if t == 1:
            om.find_object_by_id(objects[0][0]).scores.append(0.0)   # the table changes between frames: snapshots
    saver.end()
    return saver, om
