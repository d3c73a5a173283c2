"""Per-frame results without a GPU: the new entry points on the ABI and their argument errors, the COCO run-length
coding (loop encoder / decoder of tests/emu_frame_result.py against each other, against hand-derived strings and
against the product's vectorised encoder), and `FrameResultSaver` on the emulated ops against what the reference's own
`ResultSaver` wrote for the same clip (tests/golden/result_saver.*, made by tests/golden/make_result_golden.py)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import abi_util
import emu_frame_result as E
import emu_ops
import full_frame_shapes as FS
import result_case as RC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('deva_frame_result', 'deva_mask_rle_scratch', 'deva_mask_rle_count', 'deva_mask_rle_write')


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    E.install(monkeypatch)


# ------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_exported_declared_and_bound():
    from deva.hip import ops
    abi_util.inference_entry_points(NAMES)
    assert 'frame_result' in ops.__all__ and 'mask_rle' in ops.__all__


def test_argument_errors_before_any_launch():
    """the launchers refuse bad arguments on the host (pointers are never dereferenced: validation fails first)"""
    from deva import hip
    L = hip.lib()
    P, O = 4096, 1 << 20
    none = (None,) * 6
    assert L.deva_frame_result(None, 3, 8, 8, 8, 8, None, 0, None, None, O, None, None, None, None, None, None) != 0
    assert b'deva_frame_result' in L.deva_hip_last_error()
    assert L.deva_frame_result(P, 3, 8, 8, 8, 8, None, 0, None, None, *none, None) != 0
    assert b'no output' in L.deva_hip_last_error()
    assert L.deva_frame_result(P, 32768, 8, 8, 8, 8, None, 0, None, None, O, None, None, None, None, None, None) != 0
    assert b'32767' in L.deva_hip_last_error()
    assert L.deva_frame_result(P, 3, 8, 8, 8, 8, None, 0, None, None, None, None, None, O, None, None, None) != 0
    assert b'color table' in L.deva_hip_last_error()
    assert L.deva_frame_result(P, 3, 8, 8, 8, 8, None, 0, P, None, None, None, None, None, None, O, None) != 0
    assert b'image' in L.deva_hip_last_error()
    assert L.deva_frame_result(P, 3, 8, 8, 8, 8, P, 0, None, None, O, None, None, None, None, None, None) != 0
    assert b'empty table' in L.deva_hip_last_error()
    # run lengths: channel limit, scratch size, capacity
    assert L.deva_mask_rle_scratch(8, 8, 4097) == -1 and L.deva_mask_rle_scratch(0, 8, 2) == -1
    need = L.deva_mask_rle_scratch(1080, 1920, 15)
    assert need >= 1080 * 1920 * 2 + 15 * 4
    assert L.deva_mask_rle_count(None, 8, 8, 3, P, 1 << 20, P, None) != 0
    assert L.deva_mask_rle_count(P, 8, 8, 4097, P, 1 << 20, P, None) != 0 and b'4096' in L.deva_hip_last_error()
    assert L.deva_mask_rle_count(P, 1080, 1920, 15, P, need - 1, P, None) != 0 and b'scratch' in L.deva_hip_last_error()
    n_host = (ctypes.c_int32 * 3)(0, 4, 2)
    assert L.deva_mask_rle_write(8, 8, 3, P, 1 << 20, n_host, O, 5, None) != 0
    assert b'do not fit' in L.deva_hip_last_error()
    assert L.deva_mask_rle_write(8, 8, 3, P, 1 << 20, None, O, 5, None) != 0


def test_wrapper_errors_before_any_launch():
    """`ops.frame_result` / `ops.mask_rle` check shapes and sizes first, then refuse host tensors: no CPU path"""
    from deva.hip import DevaHipError, ops
    prob = torch.rand(3, 8, 8)
    with pytest.raises(DevaHipError, match='want'):
        ops.frame_result(prob, want=('index', 'outline'))
    with pytest.raises(DevaHipError, match='C,H,W'):
        ops.frame_result(prob[0])
    with pytest.raises(DevaHipError, match='32767'):
        ops.frame_result(torch.empty(32768, 1, 1), want=('index',))
    with pytest.raises(DevaHipError, match='color table'):
        ops.frame_result(prob, want=('color',), color_lut=torch.zeros(2, 3, dtype=torch.uint8))
    with pytest.raises(DevaHipError, match='output size'):   # the image must have the OUTPUT size
        ops.frame_result(prob, (16, 16), want=('blend',), color_lut=torch.zeros(3, 3, dtype=torch.uint8),
                         image=torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(DevaHipError, match='HIP device'):
        ops.frame_result(prob)
    with pytest.raises(DevaHipError, match='int16'):
        ops.mask_rle(torch.zeros(8, 8, dtype=torch.int64), 2)
    with pytest.raises(DevaHipError, match='HIP device'):
        ops.mask_rle(torch.zeros(8, 8, dtype=torch.int16), 2)


# ------------------------------------------------------------------------------------------ COCO coding
def test_hand_derived_strings():
    """4 x 4 with the centre 2 x 2 set: column-major runs 5, 2, 2, 2, 5; the fourth and fifth are coded as differences
    to the count two places back (2 - 2 = 0, 5 - 2 = 3) -> '5', '2', '2', '0', '3'.  2 x 2 all ones: an empty run of
    zeros first -> [0, 4] -> '04'"""
    m = np.zeros((4, 4), dtype=bool)
    m[1:3, 1:3] = True
    assert E.coco_counts(m) == [5, 2, 2, 2, 5] and E.coco_string([5, 2, 2, 2, 5]) == '52203'
    assert E.coco_counts(np.ones((2, 2), dtype=bool)) == [0, 4] and E.coco_string([0, 4]) == '04'
    assert E.coco_counts(np.zeros((3, 5), dtype=bool)) == [15] and E.coco_parse('52203') == [5, 2, 2, 2, 5]
    from deva.inference.frame_results import coco_strings
    assert coco_strings(np.array([5, 2, 2, 2, 5, 0, 4, 15]), np.array([5, 2, 1])) == ['52203', '04', E.coco_string([15])]


def test_loop_encoder_and_decoder_round_trip():
    rng = np.random.default_rng(1)
    for t in range(30):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        m = rng.random((h, w)) < (0.05, 0.5, 0.95)[t % 3]
        if t % 5 == 0:
            m[:, : w // 2] = True      # long runs
        rle = E.coco_encode(m)
        assert rle['size'] == [h, w] and np.array_equal(E.coco_decode(rle), m)
        assert sum(E.coco_counts(m)) == h * w


def test_vectorised_encoder_equals_the_loop_encoder():
    """random count lists of several objects at once: small counts, counts above 2^20 (5 and more characters), the
    int32 range, alternating large and small counts (negative differences from the fourth count on)"""
    from deva.inference.frame_results import coco_strings
    rng = np.random.default_rng(2)
    for t in range(60):
        lengths = rng.integers(1, 40, size=int(rng.integers(1, 7)))
        top = (4, 40, 2**21, 2**31 - 1)[t % 4]
        lists = []
        for n in lengths:
            c = rng.integers(0, top, size=n)
            if t % 2:
                c[::2] = c[::2] // 1000   # large, small, large, ...: differences of both signs
            lists.append(c)
        got = coco_strings(np.concatenate(lists), lengths)
        assert got == [E.coco_string(c.tolist()) for c in lists], t
        assert all(E.coco_parse(s) == c.tolist() for s, c in zip(got, lists))
    assert len(coco_strings(np.array([2**21]), np.array([1]))[0]) == 5 and coco_strings(np.array([15]), np.array([1])) == ['?']
    assert coco_strings(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)) == []


def test_boundaries_to_strings():
    """`rle_strings` on the boundary contract equals the loop encoder on every object's mask: an object that owns p = 0,
    one that owns the last position, an absent one"""
    from deva.inference.frame_results import rle_strings
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 5, size=(9, 7))
    idx[idx == 3] = 0
    idx[0, 0], idx[-1, -1] = 1, 2
    n, bounds = E.rle_bounds(idx, 6)
    assert n[0] == 0 and n[3] == 0 and n[5] == 0
    texts = rle_strings(n, np.concatenate(bounds), idx.size)
    assert texts[0] is None
    for c in range(1, 6):
        assert texts[c] == E.coco_encode(idx == c)['counts'], c
    assert texts[3] == E.coco_string([63])


def test_contract_of_the_products():
    """the emulated `frame_result` against plain statements: labels are `index_mask`'s, the stats are area and
    inclusive box, the overlay is the float formula of the reference"""
    g = torch.Generator().manual_seed(4)
    prob = torch.softmax(torch.randn(4, 20, 30, generator=g) * 2, dim=0)
    lut = torch.tensor([0, 300, 0, 70000], dtype=torch.int64)
    from deva.inference.frame_results import long_id_colors
    colors = torch.from_numpy(long_id_colors(lut.numpy()))
    image = torch.randint(0, 256, (33, 41, 3), generator=g, dtype=torch.uint8)
    res = E.frame_result(prob, (33, 41), lut, color_lut=colors, image=image,
                         want=('index', 'labels', 'stats', 'color', 'gray', 'blend'))
    assert torch.equal(res.labels, emu_ops.index_mask(prob, (33, 41), lut))
    ids = res.labels.numpy()
    for c in range(4):
        m = res.index.numpy() == c
        ys, xs = np.nonzero(m)
        assert res.stats[c].tolist() == [int(m.sum()), xs.min(), ys.min(), xs.max(), ys.max()]
    rgb = res.color.numpy()
    assert np.array_equal(rgb[ids == 70000][0], [70000 % 256, 70000 // 256 % 256, 1])
    alpha = ((ids == 0).astype(np.float32) * 0.5 + 0.5)[:, :, None]
    assert np.array_equal(res.blend.numpy(), (image.numpy() * alpha + rgb * (1 - alpha)).astype(np.uint8))
    assert np.array_equal(res.gray.numpy(), ids.astype(np.uint8))


def test_vectorised_boundary_reference_equals_the_loop():
    """`E.rle_bounds_fast` (what the 4096-channel device test is judged by) against `E.rle_bounds` on every hand-built
    plane of the device tests and on random planes with values outside the table, of both signs and at both ends"""
    from test_gpu_o_frame_result import _planes
    cases = [(plane, channels) for _, plane, channels in _planes(33, 47)]
    rng = np.random.default_rng(5)
    for t in range(12):
        h, w, channels = int(rng.integers(1, 30)), int(rng.integers(1, 30)), int(rng.integers(1, 9))
        plane = rng.integers(-2, channels + 2, size=(h, w)).astype(np.int16)
        plane[rng.random((h, w)) < 0.1] = (-32768, 32767, channels, -1)[t % 4]
        if t % 3 == 0:
            plane[:, : w // 2] = channels - 1     # long runs (of the background when channels == 1)
        cases.append((plane, channels))
    for plane, channels in cases:
        n, bounds = E.rle_bounds(plane, channels)
        fast_n, fast_b = E.rle_bounds_fast(plane, channels)
        assert fast_n.dtype == np.int32 and fast_b.dtype == np.int32
        assert np.array_equal(fast_n, n) and np.array_equal(fast_b, np.concatenate(bounds))


# ------------------------------------------------------------------------------------------ shapes and the paths they reach
# the caps of the grids, each written once, with the line of the launcher it mirrors
FRAME_RESULT_BLOCKS = 4096     # csrc/frame_result.hip, deva_frame_result: `if (blocks > 4096) blocks = 4096;`
LUT_REMAP_BLOCKS = 8192        # csrc/merge.hip, deva_lut_remap: `if (blocks > 8192) blocks = 8192;`
MERGE_PAINT_BLOCKS = 8192      # csrc/merge.hip, deva_merge_paint: `if (blocks > 8192) blocks = 8192;`
LABEL_HISTOGRAM_BLOCKS = 2048  # csrc/merge.hip, deva_label_histogram: `if (blocks > 2048) blocks = 2048;`
THREADS = 256                  # `dim3(256)` in all four launches; frame_result: one 4-pixel group per thread and step
SCAN_THREADS = 256             # csrc/frame_result.hip, rle_scan_kernel: `const int chunk = (groups + 255) / 256;`


def _ceil256(v):
    return -(-v // 256) * 256


def _rle_groups(h, w, channels):
    """the number of ranges `rle_plan` makes, from the scratch size it asks for: ceil256(2 * total) for the transposed
    plane, ceil256(4 * channels * groups) for the count table, ceil256(4 * channels) for the bases.  With 64 | channels
    the middle term is exactly 4 * channels * groups"""
    from deva import hip
    assert channels % 64 == 0
    nbytes = hip.lib().deva_mask_rle_scratch(h, w, channels)
    middle = nbytes - _ceil256(2 * h * w) - _ceil256(4 * channels)
    assert middle > 0 and middle % (4 * channels) == 0
    return middle // (4 * channels)


def test_rle_shapes_reach_the_paths_they_are_named_for():
    """254 ranges for the plane the suite already had (one table entry per scan thread), 282 and 771 for the two new
    ones (chunks of 2 and 4, the last busy thread of the larger with 3), 945 ranges of more than 512 positions at 4096
    channels"""
    for (h, w, groups, chunk) in (FS.RLE_ONE_ENTRY, FS.RLE_TWO_ENTRIES, FS.RLE_PARTIAL_CHUNK):
        assert _rle_groups(h, w, 64) == groups == -(-h * w // 512)
        assert -(-groups // SCAN_THREADS) == chunk
    assert [s[2] for s in (FS.RLE_ONE_ENTRY, FS.RLE_TWO_ENTRIES, FS.RLE_PARTIAL_CHUNK, FS.RLE_GROWN_RANGE)] == \
        [254, 282, 771, 945]
    groups = FS.RLE_TWO_ENTRIES[2]
    assert groups % 2 == 0 and groups // 2 == 141                       # threads 0..140 busy, no partial chunk
    groups = FS.RLE_PARTIAL_CHUNK[2]
    assert groups // 4 == 192 and groups % 4 == 3 and SCAN_THREADS - 193 == 63
    h, w, groups, chunk = FS.RLE_GROWN_RANGE
    assert _rle_groups(h, w, FS.RLE_GROWN_CHANNELS) == groups and -(-groups // SCAN_THREADS) == chunk
    assert groups < -(-h * w // 512)                                      # the range really grew ...
    assert -(-h * w // groups) > 512 and -(-h * w // 576) == groups       # ... to 576 positions
    assert 4 * FS.RLE_GROWN_CHANNELS * groups > 15 * 10**6                # the count table: 15.5 MB


def test_full_frame_shapes_exceed_the_grid_caps():
    (oh, ow), (eh, ew) = FS.FRAME_PACKED, FS.FRAME_ELEMENTWISE
    assert ow % 4 == 0 and oh * (ow // 4) == 1050624 > FRAME_RESULT_BLOCKS * THREADS
    assert ew % 4 == 2 and eh * ((ew + 3) // 4) == 1052676 > FRAME_RESULT_BLOCKS * THREADS
    pixels = FS.MERGE_LARGE[0] * FS.MERGE_LARGE[1]
    assert pixels > LUT_REMAP_BLOCKS * THREADS and pixels > MERGE_PAINT_BLOCKS * THREADS
    assert pixels > LABEL_HISTOGRAM_BLOCKS * THREADS
    assert 1080 * 1920 <= LUT_REMAP_BLOCKS * THREADS                      # (what 1080p does not reach)
    # the mirrored lines are still what the launchers say
    csrc = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
    bodies = {}
    for file in ('frame_result.hip', 'merge.hip'):
        for part in open(os.path.join(csrc, file)).read().split('extern "C" ')[1:]:
            bodies[re.match(r'\w+ (\w+)', part).group(1)] = part
    for name, cap in (('deva_frame_result', FRAME_RESULT_BLOCKS), ('deva_lut_remap', LUT_REMAP_BLOCKS),
                      ('deva_merge_paint', MERGE_PAINT_BLOCKS), ('deva_label_histogram', LABEL_HISTOGRAM_BLOCKS)):
        assert f'if (blocks > {cap}) blocks = {cap};' in bodies[name], name
        assert f'dim3({THREADS})' in bodies[name] or f't({THREADS})' in bodies[name], name


# ------------------------------------------------------------------------------------------ saver against the reference's
@pytest.fixture(scope='module')
def golden(golden_dir):
    arrays = dict(np.load(os.path.join(golden_dir, 'result_saver.npz')))
    with open(os.path.join(golden_dir, 'result_saver.json')) as f:
        return arrays, json.load(f)


def _package_saver(dataset, root, spec=None):
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    return RC.run_saver(FrameResultSaver, ObjectManager, ObjectInfo, dataset, root, spec)


@pytest.mark.parametrize('dataset', sorted(RC.DATASETS))
def test_saver_writes_what_the_reference_saver_wrote(dataset, emu, golden, tmp_path):
    arrays, jsons = golden
    saver, om = _package_saver(dataset, str(tmp_path))
    assert saver.queue.empty() and not saver.thread.is_alive()
    want = {k[len(dataset) + 1:]: v for k, v in arrays.items() if k.startswith(dataset + '/')}
    assert len(want) >= RC.FRAMES
    for rel, ref in want.items():
        if rel.endswith('#palette'):
            continue
        file = tmp_path / rel
        assert file.exists(), rel
        img = Image.open(file)
        if rel.endswith('.png'):
            got = np.array(img)
            assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), rel
            if rel + '#palette' in want:
                assert img.mode == 'P' and np.array_equal(np.array(img.getpalette(), dtype=np.uint8), want[rel + '#palette'])
        else:
            assert list(img.size) == ref.tolist(), rel          # the JPEG itself is lossy: the overlay is checked below
    written = sorted(os.path.relpath(os.path.join(b, f), tmp_path) for b, _, fs in os.walk(tmp_path) for f in fs)
    assert written == sorted(k for k in want if not k.endswith('#palette'))
    if dataset in jsons:
        assert json.loads(json.dumps(saver.video_json)) == jsons[dataset]
        assert [len(a['segments_info']) for a in saver.video_json['annotations']] == [3, 3, 2, 3]   # frame 2: zero area filtered
    else:
        assert not hasattr(saver, 'video_json')


def test_overlay_is_the_reference_formula(emu):
    """the pre-encode overlay of the demo leg against result_utils.py:240-242 in numpy"""
    from deva.inference.frame_results import long_id_colors
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    long_id, objects, _ = RC.DATASETS['demo']
    om = RC.object_manager(ObjectManager, ObjectInfo, long_id, objects)
    for prob, image in zip(RC.probabilities(), RC.images((RC.H, RC.W))):
        res = om.frame_result(prob, image=image, labels=True)
        out_mask = res.labels.numpy().astype(np.uint32)
        rgb_mask = np.zeros((*out_mask.shape, 3), dtype=np.uint8)
        for i in om.all_obj_ids:
            rgb_mask[out_mask == i] = long_id_colors([i])[0]
        alpha = ((out_mask == 0).astype(np.float32) * 0.5 + 0.5)[:, :, None]
        assert np.array_equal(res.blend.numpy(), (image * alpha + rgb_mask * (1 - alpha)).astype(np.uint8))
        assert np.array_equal(res.color.numpy(), rgb_mask) and res.gray is None


def test_burst_saver_against_the_masks(emu, tmp_path):
    """pycocotools is not available to make a golden: every emitted RLE is decoded by the loop decoder and must be the
    object's exact mask; ids, scores and areas against the table (scores as they were when the frame was saved)"""
    saver, om = _package_saver('burst', str(tmp_path), RC.BURST)
    assert saver.video_json['dataset'] == '' and saver.video_json['seq_name'] == 'clip'
    objects = RC.BURST[1]
    table = [0] + [o[0] for o in objects]
    frames = saver.video_json['segmentations']
    assert [a['file_name'] for a in frames] == RC.NAMES and [len(a['segmentations']) for a in frames] == [3, 3, 2, 3]
    for t, (prob, ann) in enumerate(zip(RC.probabilities(), frames)):
        ids = np.asarray(table)[prob.argmax(0).numpy()]
        live = [o for o in objects if (ids == o[0]).any()]
        assert [s['id'] for s in ann['segmentations']] == [o[0] for o in live]
        for seg, (oid, _, score) in zip(ann['segmentations'], live):
            assert set(seg) == {'id', 'score', 'rle'} and seg['rle']['size'] == [RC.H, RC.W]
            assert np.array_equal(E.coco_decode(seg['rle']), ids == oid), (t, oid)
            want = score if not (oid == objects[0][0] and t > 1) else (score + 0.0) / 2
            assert seg['score'] == pytest.approx(want)
    json.dumps(saver.video_json)
    pngs = sorted(os.listdir(tmp_path / 'clip'))
    assert pngs == [n[:-4] + '.png' for n in RC.NAMES]
    assert np.array_equal(np.array(Image.open(tmp_path / 'clip' / pngs[0])),
                          (np.asarray(table)[RC.probabilities()[0].argmax(0).numpy()] & 0xff).astype(np.uint8))


def test_frame_result_records(emu):
    """`ObjectManager.frame_result`: one record per object in table order with area, xyxy box (None for area 0) and the
    COCO dict; labels only when asked"""
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    om = RC.object_manager(ObjectManager, ObjectInfo, *RC.BURST[:2])
    prob = RC.probabilities()[2]
    res = om.frame_result(prob, rle=True)
    assert res.labels is None and res.color is None and res.blend is None and res.gray is not None
    assert res.size == (RC.H, RC.W) and [s['id'] for s in res.segments] == [7, 3, 250]
    idx = prob.argmax(0).numpy()
    for tmp, seg in enumerate(res.segments, start=1):
        m = idx == tmp
        assert seg['area'] == int(m.sum()) and seg['category_id'] == RC.BURST[1][tmp - 1][1]
        if seg['area']:
            ys, xs = np.nonzero(m)
            assert seg['bbox'] == [xs.min(), ys.min(), xs.max(), ys.max()] and all(isinstance(v, float) for v in seg['bbox'])
        else:
            assert seg['bbox'] is None
        assert np.array_equal(E.coco_decode(seg['rle']), m)
    assert res.segments[2]['area'] == 0 and res.segments[2]['rle']['counts'] == E.coco_string([RC.H * RC.W])
    assert torch.equal(om.frame_result(prob, (30, 50), labels=True).labels, om.prob_to_obj_cls(prob, (30, 50)))


def test_unknown_and_unsupported_datasets(emu, tmp_path):
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_manager import ObjectManager
    for name in ('gradio', 'nothing'):
        with pytest.raises(NotImplementedError):
            FrameResultSaver(str(tmp_path), 'clip', dataset=name, object_manager=ObjectManager())
    om = ObjectManager()
    om.use_long_id = True
    saver = FrameResultSaver(str(tmp_path), 'clip', dataset='demo', object_manager=om)
    with pytest.raises(ValueError, match='visualize'):
        saver.save_mask(RC.probabilities()[0][:1], '00000.jpg')
    saver.end()
