"""The prompt-point choice and the automatic frame loop without a GPU: the two entry points on the ABI and their argument
errors, the CPU contract (tests/emu_prompts.py) against torch's own F.interpolate + F.grid_sample and against what the
REFERENCE's auto_segment kept (tests/golden/prompt_points.npz), and `AutomaticProcessor` on the emulated ops against a
straight-line restatement of the reference's loop (deva/ext/automatic_processor.py:28-128, demo_utils.py:22-46)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_util
import emu_detections as ED
import emu_ops
import emu_prompts as EM
import emu_proposals as EP
import prompt_case as PC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('deva_prompt_scratch', 'deva_prompt_points')
THRESHOLD = 0.01


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    ED.install(monkeypatch)
    EP.install(monkeypatch)
    EM.install(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)   # (frame_to_network_input uploads the frame)


# ------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_exported_declared_and_bound():
    from deva.hip import ops
    header = abi_util.inference_entry_points(NAMES)
    assert 'prompt_points' in ops.__all__
    for ref in ('automatic_sam.py:67-89', 'automatic_sam.py:69', 'automatic_sam.py:70-73', 'automatic_sam.py:80',
                'automatic_sam.py:82'):
        assert ref in header, ref


A, S = 1 << 30, 1 << 20   # made-up addresses: validation fails before anything is dereferenced or launched


def _call(L, mask=A, elem=8, h=96, w=128, pts=A, n=64, thr=0.01, scratch=S, nbytes=1 << 24, out=A, labels=A, count=A):
    return L.deva_prompt_points(mask, elem, h, w, pts, n, thr, scratch, nbytes, out, labels, count, None)


def test_argument_errors_before_any_launch():
    from deva import hip
    L = hip.lib()
    err = L.deva_hip_last_error
    assert _call(L, mask=None) == 2 and b'mask' in err()
    assert _call(L, mask=A + 4) == 2 and b'misaligned mask' in err()        # int64 elements
    assert _call(L, mask=A + 3, elem=1, scratch=None) == 2 and b'scratch' in err()   # bytes may start anywhere
    assert _call(L, pts=None) == 2 and b'points' in err()
    assert _call(L, pts=A + 2) == 2 and b'misaligned points' in err()
    assert _call(L, out=None) == 2 and b'kept points' in err()
    assert _call(L, out=A + 1) == 2 and b'kept points' in err()
    assert _call(L, labels=None) == 2 and b'labels' in err()
    assert _call(L, count=None) == 2 and b'count' in err()
    assert _call(L, count=A + 2) == 2 and b'count' in err()
    assert _call(L, h=15) == 2 and b'at least 16 x 16' in err()
    assert _call(L, w=15) == 2 and b'at least 16 x 16' in err()
    assert _call(L, h=0) == 2 and _call(L, h=-5) == 2
    assert _call(L, h=65537) == 2 and b'mask size' in err()
    assert _call(L, h=40000, w=40000) == 2 and b'mask size' in err()
    assert _call(L, n=0) == 2 and b'at least one point' in err()
    assert _call(L, n=16385) == 2 and b'16384' in err()
    for elem in (0, 2, 4, 16, -1):
        assert _call(L, elem=elem) == 2 and b'1-byte or 8-byte' in err()
    assert _call(L, thr=float('nan')) == 2 and b'not a number' in err()
    assert _call(L, scratch=None) == 2 and b'scratch' in err()
    assert _call(L, scratch=S + 8) == 2 and b'scratch' in err()             # not 16-byte aligned
    need = L.deva_prompt_scratch(96, 128, 64)
    assert _call(L, nbytes=need - 1) == 2 and b'scratch' in err() and str(need).encode() in err()
    assert all(b'deva_prompt_points' in (_call(L, **kw), err())[1] for kw in (dict(h=3), dict(n=0), dict(elem=3)))
    # the scratch holds the row pass [H][W/16] and the map [H/16][W/16] in fp32, each rounded up to 256 bytes
    assert need == 96 * 8 * 4 + 6 * 8 * 4 + 64 == L.deva_prompt_scratch(96, 128, 16384)
    assert 1080 * 120 * 4 + 67 * 120 * 4 <= L.deva_prompt_scratch(1080, 1920, 1024) < 1080 * 120 * 4 + 67 * 120 * 4 + 512
    for h, w, n in ((15, 128, 64), (96, 15, 64), (96, 128, 0), (96, 128, 16385), (65537, 16, 1), (40000, 40000, 1), (-1, -1, -1)):
        assert L.deva_prompt_scratch(h, w, n) == -1


def test_wrapper_errors_before_any_launch():
    """the wrapper checks shapes and sizes first, then refuses host tensors: no CPU path"""
    from deva.hip import DevaHipError, ops
    from deva.inference import detections as D
    grid = PC.grid(4)
    mask = torch.zeros(32, 48, dtype=torch.int64)
    with pytest.raises(DevaHipError, match=r'H,W'):
        ops.prompt_points(mask[None], grid)
    with pytest.raises(DevaHipError, match='int64, uint8 or bool'):
        ops.prompt_points(mask.int(), grid)
    with pytest.raises(DevaHipError, match='at least 16 x 16'):
        ops.prompt_points(mask[:15], grid)
    with pytest.raises(DevaHipError, match=r'P,2'):
        ops.prompt_points(mask, grid.view(-1))
    with pytest.raises(DevaHipError, match='16384 points'):
        ops.prompt_points(mask, torch.zeros(16385, 2))
    with pytest.raises(DevaHipError, match='16384 points'):
        ops.prompt_points(mask, torch.zeros(0, 2))
    with pytest.raises(DevaHipError, match='not a number'):
        ops.prompt_points(mask, grid, float('nan'))
    with pytest.raises(DevaHipError, match='HIP device'):
        ops.prompt_points(mask, grid)
    with pytest.raises(ValueError, match='one of them'):
        D.forward_prompt_points(mask)
    with pytest.raises(ValueError, match='one of them'):
        D.forward_prompt_points(mask, 4, point_grid=grid)
    with pytest.raises(DevaHipError, match='HIP device'):
        D.forward_prompt_points(mask, 4)


def test_prompt_grid_is_the_reference_linspace():
    from deva.inference import detections as D
    for n in (1, 2, 8, 32, 64):
        grid = D.prompt_grid(n, 'cpu')
        offset = 1 / (2 * n)
        side = torch.linspace(offset, 1 - offset, n)
        assert grid.dtype == torch.float32 and tuple(grid.shape) == (n * n, 2) and grid.is_contiguous()
        assert torch.equal(grid[:, 0].view(n, n), side.view(1, n).expand(n, n))       # x fastest
        assert torch.equal(grid[:, 1].view(n, n), side.view(n, 1).expand(n, n))
        assert D.prompt_grid(n, 'cpu') is grid                                         # cached per (n, device)


# ------------------------------------------------------------------------------------------ the contract against torch
def torch_labels(mask, grid, n, *, wrong_way=False):
    """automatic_sam.py:69-80 in torch's own ops on the CPU.  wrong_way: `size=` in place of `scale_factor=`, which
    filters with H / out_H instead of 16"""
    fg = (mask > 0).float()[None, None]
    h, w = mask.shape
    kw = dict(size=(h // 16, w // 16)) if wrong_way else dict(scale_factor=1 / 16)
    low = F.interpolate(fg, mode='bilinear', antialias=True, **kw)
    assert tuple(low.shape[-2:]) == (h // 16, w // 16)
    return F.grid_sample(low, grid.view(1, n, n, 2) * 2 - 1, align_corners=False).view(-1)


@pytest.fixture(scope='module')
def cases():
    """every golden case once: mask, grid, the contract's answer and torch's labels (shared, never modified)"""
    out = {}
    for name, (h, w, n, seed, t) in PC.GOLDEN_CASES.items():
        mask, grid = PC.golden_mask(name), PC.grid(n)
        points, labels, count = EM.prompt_points(mask, grid, THRESHOLD)
        out[name] = dict(mask=mask, grid=grid, n=n, points=points, labels=labels, count=int(count), torch=torch_labels(mask, grid, n))
    return out


def test_contract_labels_are_torchs_to_1e5(cases):
    """each label is fewer than 80 rounded fp32 operations on values in [0, 1]: 80 * 2^-24 = 4.8e-6 < 1e-5"""
    for name, c in cases.items():
        err = float((c['labels'] - c['torch']).abs().max())
        print(name, f'max |label - torch| = {err:.3e}')
        assert err <= 1e-5, (name, err)
    # small and odd shapes, a dense grid whose outermost points reach outside the map
    for (h, w, n, seed) in ((16, 16, 2, 1), (17, 33, 3, 2), (31, 47, 3, 3), (100, 100, 64, 4), (481, 853, 33, 5)):
        mask, grid = PC.forward_mask(h, w, seed), PC.grid(n)
        labels = EM.prompt_points(mask, grid)[1]
        err = float((labels - torch_labels(mask, grid, n)).abs().max())
        print((h, w, n), f'max |label - torch| = {err:.3e}')
        assert err <= 1e-5, ((h, w, n), err)


def test_contract_keeps_exactly_what_the_reference_kept(cases, golden_dir):
    golden = np.load(os.path.join(golden_dir, 'prompt_points.npz'))
    assert sorted({k.split('/')[0] for k in golden.files}) == sorted(PC.GOLDEN_CASES)       # no case is left out
    for name, c in cases.items():
        margin = float((c['torch'] - np.float32(THRESHOLD)).abs().min())
        print(name, f'min |label - 0.01| = {margin:.3e}, kept {c["count"]} of {c["n"] ** 2}')
        assert margin >= 1e-4, (name, margin)                                               # the condition of exactness
        want = golden[name + '/points']
        assert want.dtype == np.float32 and c['count'] == len(want)
        assert np.array_equal(c['points'][:c['count']].numpy().view(np.int32), want.view(np.int32)), name   # set AND order
        assert int(golden[name + '/called']) == (1 if len(want) else 0)
        assert bool(torch.isnan(c['points'][c['count']:]).all())                            # beyond the count: not written
    assert cases['covered_96x128_n8']['count'] == 0 and min(c['count'] for n, c in cases.items() if 'covered' not in n) >= 8


def test_the_filter_scale_is_16_not_the_ratio_of_the_sizes(cases):
    """rule 2: 1080 / 67 = 16.12 is not the scale the reference filters with; a caller who resizes with `size=` prompts
    other points"""
    c = cases['1080x1920_n32']
    wrong = torch_labels(c['mask'], c['grid'], c['n'], wrong_way=True)
    assert float((wrong - c['torch']).abs().max()) > 0.05
    kept_wrong, kept = (wrong < THRESHOLD), (c['labels'] < THRESHOLD)
    assert int((kept_wrong != kept).sum()) >= 1
    # where both sides are multiples of 16 the two are the same map
    c = cases['96x128_n8']
    assert float((torch_labels(c['mask'], c['grid'], c['n'], wrong_way=True) - c['torch']).abs().max()) <= 1e-6


def test_contract_rules_by_hand():
    grid = PC.grid(4)
    zero = torch.zeros(32, 48, dtype=torch.int64)
    points, labels, count = EM.prompt_points(zero, grid)
    assert int(count) == 16 and torch.equal(points, grid) and bool((labels == 0).all())     # every point, in order
    full = torch.full((32, 48), 3, dtype=torch.uint8)
    points, labels, count = EM.prompt_points(full, grid)
    assert int(count) == 0 and bool(torch.isnan(points).all())
    # the outermost points of a dense grid sample outside the map: an all-foreground map is 1 inside, less at the rim
    dense = EM.prompt_points(full, PC.grid(16))[1].view(16, 16)
    assert float(dense[4:12, 4:12].min()) == 1.0 and 0.2 < float(dense[0, 0]) < 0.6 and float(dense[0, 8]) < 1.0
    # 64-bit ids: 2^31 + 5 and 2^40 are foreground, -3 and -2^40 are not
    ids = torch.zeros(32, 48, dtype=torch.int64)
    ids[:, :24] = (1 << 31) + 5
    ids[:16, 24:] = -3
    ids[16:, 24:] = -(1 << 40)
    same = EM.prompt_points((ids > 0).to(torch.uint8), grid)
    got = EM.prompt_points(ids, grid)
    assert torch.equal(got[1], same[1]) and int(got[2]) == int(same[2]) and 0 < int(got[2]) < 16
    assert bool((got[1].view(4, 4)[:, 0] > 0.5).all()) and bool((got[1].view(4, 4)[:, 3] == 0).all())
    # strict comparison in fp32: a label equal to the threshold is not kept
    label = float(got[1].view(4, 4)[0, 1])
    assert 0 < label < 1
    assert int(EM.prompt_points(ids, grid[1:2], label)[2]) == 0
    assert int(EM.prompt_points(ids, grid[1:2], float(np.nextafter(np.float32(label), np.float32(2))))[2]) == 1


# ------------------------------------------------------------------------------------------ the frame loop
class RecordingSaver:
    def __init__(self):
        self.saved = []

    def save_mask(self, prob, frame_name, need_resize=False, shape=None, image_np=None):
        self.saved.append((frame_name, prob, need_resize, tuple(shape), image_np))


def restated_loop(core, segmenter, frames, names, *, capacity=512):
    """deva/ext/automatic_processor.py:28-128 and demo_utils.py:22-46, restated in a straight line against the public
    pieces (no AutomaticProcessor): -> [(frame name, prob)] in the order the reference saves them"""
    from deva.inference import detections as D
    from deva.inference.proposals import ProposalFilter
    from deva.utils.tensor_utils import frame_to_network_input
    cfg = core.config
    saved = []
    next_voting_frame = cfg['num_voting_frames'] - 1
    filters = {}

    def auto_segment(image_np, forward_mask, device):
        h, w = image_np.shape[:2]
        new_h, new_w = D.detection_size(h, w, cfg['size'])
        if forward_mask is not None:
            positive_points = D.forward_prompt_points(forward_mask, cfg['SAM_NUM_POINTS_PER_SIDE'])
            if len(positive_points) == 0:
                return torch.zeros((new_h, new_w), dtype=torch.int64, device=device), []
        else:
            positive_points = D.prompt_grid(cfg['SAM_NUM_POINTS_PER_SIDE'], 'cpu').numpy()
        segmenter.set_image(image_np)
        points_for_image = positive_points * np.array((h, w))[None, ::-1]
        if (h, w) not in filters:
            filters[(h, w)] = ProposalFilter(h, w, capacity=capacity, pred_iou_thresh=cfg['SAM_PRED_IOU_THRESHOLD'])
        flt = filters[(h, w)]
        for first in range(0, len(points_for_image), cfg['SAM_NUM_POINTS_PER_BATCH']):
            batch = points_for_image[first:first + cfg['SAM_NUM_POINTS_PER_BATCH']]
            flt.add(*segmenter.predict_points(torch.as_tensor(batch.astype(np.float32), device=device)))
        segmenter.reset_image()
        found = flt.finish()
        return D.assemble_automatic(found.masks, found.iou_preds, (new_h, new_w), suppress_small_objects=cfg['suppress_small_objects'],
                                    overlap_threshold=cfg['SAM_OVERLAP_THRESHOLD'])

    def make_segmentation(image, image_np):
        forward_mask = D.estimate_forward_mask(core, image) if core.memory.engaged else None
        return auto_segment(image_np, forward_mask, image.device)

    for ti, (image_np, frame_name) in enumerate(zip(frames, names)):
        image = frame_to_network_input(image_np, cfg['size'], antialias=False)
        h, w = image_np.shape[:2]
        if cfg['temporal_setting'] == 'semionline':
            if ti + cfg['num_voting_frames'] > next_voting_frame:
                mask, segments_info = make_segmentation(image, image_np)
                frame_info = PC.driver_loops.FrameInfo(image, mask, segments_info, ti, {'frame': [frame_name], 'shape': [h, w]})
                frame_info.image_np = image_np
                core.add_to_temporary_buffer(frame_info)
                if ti == next_voting_frame:
                    this_image, this_frame_name = core.frame_buffer[0].image, core.frame_buffer[0].name
                    _, mask, new_segments_info = core.vote_in_temporary_buffer(keyframe_selection='first')
                    prob = core.incorporate_detection(this_image, mask, new_segments_info, incremental=True)
                    next_voting_frame += cfg['detection_every']
                    saved.append((this_frame_name, prob))
                    for frame_info in core.frame_buffer[1:]:
                        saved.append((frame_info.name, core.step(frame_info.image, None, None)))
                    core.clear_buffer()
            else:
                saved.append((frame_name, core.step(image, None, None)))
        elif cfg['temporal_setting'] == 'online':
            if ti % cfg['detection_every'] == 0:
                mask, segments_info = make_segmentation(image, image_np)
                prob = core.incorporate_detection(image, mask, segments_info, incremental=True)
            else:
                prob = core.step(image, None, None)
            saved.append((frame_name, prob))
    for frame_info in core.frame_buffer:                      # flush_buffer
        saved.append((frame_info.name, core.step(frame_info.image, None, None)))
    return saved


def run_processor(core, segmenter, frames, names, saver=None):
    """the same clip through AutomaticProcessor -> ([(frame name, prob)], what `flush` alone produced)"""
    from deva.inference.automatic import AutomaticProcessor
    processor = AutomaticProcessor(core, segmenter, capacity=512, saver=saver)
    produced = []
    for ti, (image_np, name) in enumerate(zip(frames, names)):
        produced += processor.process_frame(image_np, ti, name)
    flushed = processor.flush()
    return produced + flushed, flushed, processor


def interior(forward_mask, reach=8):
    """pixels whose whole (2 reach + 1)^2 neighbourhood is foreground: at least a quarter of the weight of the nearest
    cell of the map lies on foreground there, so the label is far above 0.01"""
    fg = (forward_mask > 0).float()[None, None]
    return (-F.max_pool2d(-fg, 2 * reach + 1, stride=1, padding=reach))[0, 0] > 0.5


def check_clip(setting, make_core, frames, rects, names, monkeypatch):
    """both runs of one temporal setting; shared by the CPU test (emulated ops) and tests/test_gpu_r_prompts.py"""
    from deva.inference import detections as D
    forward_masks = []
    real = D.estimate_forward_mask

    def recording(core, image):
        forward_masks.append(real(core, image))
        segmenter.calls.append(('forward_mask', forward_masks[-1]))
        return forward_masks[-1]

    segmenter, saver = PC.FakeSegmenter(frames, rects), RecordingSaver()
    np.random.seed(11)
    want = restated_loop(make_core(setting), PC.FakeSegmenter(frames, rects), frames, names)
    monkeypatch.setattr(D, 'estimate_forward_mask', recording)
    np.random.seed(11)
    got, flushed, processor = run_processor(make_core(setting), segmenter, frames, names, saver)
    monkeypatch.setattr(D, 'estimate_forward_mask', real)
    assert [n for n, _ in got] == [n for n, _ in want] == names                   # every frame once, in order
    for (name, a), (_, b) in zip(got, want):
        assert a.shape[0] >= 2 and torch.equal(a.cpu(), b.cpu()), name            # bit-identical probabilities
    assert [s[0] for s in saver.saved] == names and all(s[2] is False and s[3] == (96, 128) for s in saver.saved)
    assert all(s[1] is p for s, (_, p) in zip(saver.saved, got)) and all(s[4] is f for s, f in zip(saver.saved, frames))
    # what the segmenter was asked: the whole grid while nothing is tracked; once the memory is engaged fewer points
    # (none at all where the forward mask leaves no background), and never one where the forward mask is solid
    grid_px = (PC.grid(8).numpy() * np.array([128, 96])).astype(np.float32)
    asked, current = [], None                                                     # (forward mask or None, [batches])
    for kind, what in segmenter.calls:
        if kind == 'forward_mask':
            current = what
        elif kind == 'set_image':
            asked.append((current, []))
            current = None
        elif kind == 'predict_points':
            assert 0 < len(what) <= 24
            asked[-1][1].append(what)
    blind = [np.concatenate(b) for m, b in asked if m is None]
    assert len(blind) >= 1 and all(np.array_equal(pts, grid_px) for pts in blind) and len(forward_masks) >= 2
    assert sum(int(interior(m.cpu()).sum()) for m in forward_masks) > 0
    for m, batches in asked:
        if m is not None:
            pts, inner = np.concatenate(batches), interior(m.cpu())
            assert 0 < len(pts) < 64 and not any(bool(inner[int(y), int(x)]) for x, y in pts)
    return got, flushed, processor


def emulated_core_factory(recipe_state_dict):
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    net = DEVA(PC.loop_config('online'))
    net.load_weights(recipe_state_dict[0])
    return lambda setting: DEVAInferenceCore(net, PC.loop_config(setting))


@pytest.mark.parametrize('setting', ['online', 'semionline'])
def test_processor_is_the_restated_reference_loop(setting, emu, recipe_state_dict, monkeypatch):
    frames, rects = PC.clip()
    names = [f'{t:05d}.jpg' for t in range(len(frames))]
    got, flushed, processor = check_clip(setting, emulated_core_factory(recipe_state_dict), frames, rects, names, monkeypatch)
    if setting == 'semionline':
        # 13 frames, windows voted at 2, 7 and 12: nothing is left; a clip that ends inside a window is flushed
        assert flushed == [] and processor.next_voting_frame == 17
        _, flushed, processor = run_processor(emulated_core_factory(recipe_state_dict)(setting),
                                              PC.FakeSegmenter(frames, rects), frames[:7], names[:7])
        assert [n for n, _ in flushed] == names[5:7] and processor.next_voting_frame == 7
    else:
        assert flushed == []


def test_a_covered_forward_mask_asks_nothing(emu, recipe_state_dict, monkeypatch):
    from deva.inference import detections as D
    from deva.inference.automatic import AutomaticProcessor
    frames, rects = PC.clip()
    core = emulated_core_factory(recipe_state_dict)('online')
    segmenter = PC.FakeSegmenter(frames, rects)
    processor = AutomaticProcessor(core, segmenter)
    seen = []
    real = core.incorporate_detection
    monkeypatch.setattr(core, 'incorporate_detection', lambda image, mask, info, **kw: (seen.append((mask, info, kw)), real(image, mask, info, **kw))[1])
    monkeypatch.setattr(D, 'estimate_forward_mask', lambda core, image: torch.ones(image.shape[-2:], dtype=torch.int64))
    for ti in range(6):
        out = processor.process_frame(frames[ti], ti, f'{ti}.jpg')
        assert len(out) == 1 and out[0][0] == f'{ti}.jpg'
    assert [c[0] for c in segmenter.calls].count('set_image') == 1                # frame 0 only: nothing was tracked yet
    assert len(seen) == 2 and len(seen[0][1]) >= 2
    mask, info, kw = seen[1]
    assert info == [] and mask.dtype == torch.int64 and tuple(mask.shape) == (96, 128) and int(mask.abs().sum()) == 0
    assert kw == dict(incremental=True)


def test_a_missing_key_is_named(emu, recipe_state_dict):
    from deva.inference.automatic import CONFIG_KEYS, AutomaticProcessor
    core = emulated_core_factory(recipe_state_dict)('online')
    full = dict(core.config)
    for key in CONFIG_KEYS:
        core.config = {k: v for k, v in full.items() if k != key}
        with pytest.raises(KeyError, match=key):
            AutomaticProcessor(core, object())
    core.config = dict(full, temporal_setting='offline')
    with pytest.raises(ValueError, match='temporal_setting'):
        AutomaticProcessor(core, object())
    import deva.inference.automatic as M
    src = open(M.__file__).read()
    banned = r'^\s*(?:import|from)\s+(?:cv2|segment_anything|torchvision|deva\.ext|deva\.inference\.(?:frame_utils|result_utils|demo_utils))\b'
    assert not re.search(banned, src, flags=re.M)
