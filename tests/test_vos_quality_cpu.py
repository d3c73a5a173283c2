"""Scoring a DAVIS-style run without a GPU: libdeva_vos_metrics.so on its ABI, its argument errors, its radius rule and its
launch plan; the host arithmetic of J, F and the sequence statistics (rule R6 of include/deva_vos_metrics.h) on records
written by hand; `deva.inference.vos_quality` on the CPU contract of the counts (tests/emu_vos.py, the numpy statement of
tests/vos_case.py); the kernels' static resources.  (The HIP-free checks under the host sanitizers: tests/test_plan_sanitize_cpu.py.)"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import abi_util
import emu_vos as EV
import vos_case as VC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_vos_metrics.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc', 'vos_metrics')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
WANT = ['deva_vos_boundary_counts', 'deva_vos_boundary_plan', 'deva_vos_boundary_radius', 'deva_vos_boundary_scratch_bytes',
        'deva_vos_last_error', 'deva_vos_version']


@pytest.fixture()
def emu(monkeypatch):
    EV.install(monkeypatch)


def _built():
    from deva.hip import vos_metrics
    return abi_util.built(vos_metrics)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    vm = _built()
    exported, _ = abi_util.exported(vm.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(vm.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_VOS_ABI_VERSION 1\b', header)
    assert vm.ABI_VERSION == 1 and vm.lib().deva_vos_version() == 1
    for name, value in (('U8', vm.U8), ('I32', vm.I32), ('I64', vm.I64), ('INDEX16', vm.INDEX16), ('BINARY', vm.BINARY),
                        ('MAX_OBJECTS', vm.MAX_OBJECTS), ('MAX_RADIUS', vm.MAX_RADIUS), ('FIELDS', vm.FIELDS), ('STRIP', vm.STRIP),
                        ('INNER_RADIUS', vm.INNER_RADIUS), ('MIDDLE_RADIUS', vm.MIDDLE_RADIUS)):
        assert re.search(rf'#define DEVA_VOS_{name} {value}\b', header), name
    for rule in ('R1', 'R2', 'R3', 'R4', 'R5', 'R6'):
        assert re.search(rf'^ \*   {rule}  ', header, flags=re.M), rule


def test_no_symbol_is_shared_with_the_other_two_libraries():
    from deva import hip
    from deva.hip import metrics
    vm = _built()
    exported, mine = abi_util.exported(vm.LIB_PATH)
    assert all(name.startswith('deva_vos_') for name in exported)
    for other in (hip.LIB_PATH, metrics.LIB_PATH):
        theirs_exported, theirs = abi_util.exported(other)
        assert not any(n.startswith('deva_vos') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other, shared)


def test_plan_mirror_has_the_c_layout(tmp_path):
    vm = _built()
    fields = [f[0] for f in vm.Plan._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_vos_metrics.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(deva_vos_plan));\n' +
                   ''.join(f'printf("%zu\\n", offsetof(deva_vos_plan, {f}));\n' for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(vm.Plan) and vals[1:] == [getattr(vm.Plan, f).offset for f in fields]


# ------------------------------------------------------------------------------------------ refusals
A = 1 << 30   # made-up addresses: validation fails before anything is dereferenced or launched
GT, PRED, IDS, LUT, SCRATCH, COUNTS = A, A + (1 << 28), A + (2 << 28), A + (3 << 28), A + (4 << 28), A + (6 << 28)


def _counts(L, gt=GT, gt_enc=0, pred=PRED, pred_enc=0, ids=IDS, n=3, lut=None, channels=0, h=8, w=12, radius=2, scratch=SCRATCH,
            scratch_bytes=16 * 8 * 12, counts=COUNTS):
    return L.deva_vos_boundary_counts(gt, gt_enc, pred, pred_enc, ids, n, lut, channels, h, w, radius, scratch, scratch_bytes,
                                      counts, None)


def test_argument_errors_before_any_launch():
    vm = _built()
    L = vm.lib()
    err = L.deva_vos_last_error
    for enc in (2, 3, -1, 4, 512, 256 + 2):
        assert _counts(L, gt_enc=enc) == 2 and b'ground truth is U8 (0) or I32 (1)' in err(), enc
    for enc in (-1, 4, 512, 256 + 4):
        assert _counts(L, pred_enc=enc) == 2 and b'unknown encoding' in err(), enc
    for n in (0, -1, 65):
        assert _counts(L, n=n) == 2 and b'1 to 64 objects' in err()
    for radius in (-1, 129):
        assert _counts(L, radius=radius) == 2 and b'radius 0 to 128' in err()
    assert _counts(L, h=0) == 2 and b'bad plane size' in err()
    assert _counts(L, w=-3) == 2 and b'bad plane size' in err()
    assert _counts(L, h=32769, w=32768, scratch_bytes=1 << 40) == 2 and b'bad plane size' in err()     # above 2^30 pixels
    assert _counts(L, gt=None) == 2 and b'ground-truth plane' in err()
    assert _counts(L, gt=GT + 8) == 2 and b'misaligned ground-truth plane' in err()
    assert _counts(L, pred=None) == 2 and b'predicted plane' in err()
    assert _counts(L, pred=PRED + 4) == 2 and b'misaligned predicted plane' in err()
    assert _counts(L, ids=None) == 2 and b'id table' in err()
    assert _counts(L, ids=IDS + 2) == 2 and b'misaligned id table' in err()
    fast = dict(pred_enc=3, lut=LUT, channels=7)
    assert _counts(L, **dict(fast, lut=None)) == 2 and b'channel table' in err()
    assert _counts(L, **dict(fast, lut=LUT + 1)) == 2 and b'channel table' in err()
    for channels in (0, -1, 32768):
        assert _counts(L, **dict(fast, channels=channels)) == 2 and b'1 to 32767 channels' in err()
    assert _counts(L, scratch=None) == 2 and b'scratch' in err()
    assert _counts(L, scratch=SCRATCH + 8) == 2 and b'misaligned scratch' in err()
    assert _counts(L, scratch_bytes=16 * 8 * 12 - 1) == 2 and b'1536 are needed' in err()
    assert _counts(L, counts=None) == 2 and b'counts' in err()
    assert _counts(L, counts=COUNTS + 2) == 2 and b'misaligned counts' in err()
    # BINARY holds one object, on either side
    for kw in (dict(gt_enc=256), dict(pred_enc=256 + 1), dict(gt_enc=257, pred_enc=256)):
        assert _counts(L, **kw) == 2 and b'BINARY planes hold one object' in err()
    # the output over an input: a plane's last byte, the id table's last entry, the channel table, the scratch
    assert _counts(L, counts=GT + 8 * 12 - 4) == 2 and b'counts overlaps an input' in err()
    assert _counts(L, pred_enc=2, counts=PRED + 8 * 12 * 8 - 4) == 2 and b'counts overlaps an input' in err()
    assert _counts(L, counts=IDS + 8) == 2 and b'counts overlaps an input' in err()
    assert _counts(L, **dict(fast, counts=LUT + 12)) == 2 and b'counts overlaps an input' in err()
    assert _counts(L, counts=SCRATCH + 16 * 8 * 12 - 4) == 2 and b'counts overlaps an input' in err()
    assert _counts(L, gt=COUNTS + 16) == 2 and b'counts overlaps an input' in err()
    assert _counts(L, scratch=GT + 16 * 5) == 2 and b'scratch overlaps an input' in err()
    assert all(b'deva_vos_boundary_counts' in (_counts(L, **kw), err())[1] for kw in (dict(h=0), dict(gt=None), dict(n=0)))
    plan, r, nbytes = vm.Plan(), ctypes.c_int(), ctypes.c_int64()
    assert L.deva_vos_boundary_plan(8, 12, 3, 2, None) == 2 and b'deva_vos_boundary_plan: null plan' in err()
    assert L.deva_vos_boundary_plan(8, 12, 65, 2, ctypes.byref(plan)) == 2 and b'1 to 64 objects' in err()
    assert L.deva_vos_boundary_plan(8, 12, 3, 129, ctypes.byref(plan)) == 2 and b'radius 0 to 128' in err()
    assert L.deva_vos_boundary_plan(0, 12, 3, 2, ctypes.byref(plan)) == 2 and b'bad plane size' in err()
    assert L.deva_vos_boundary_radius(8, 12, 0.008, None) == 2 and b'null radius' in err()
    assert L.deva_vos_boundary_radius(0, 12, 0.008, ctypes.byref(r)) == 2 and b'bad plane size' in err()
    assert L.deva_vos_boundary_scratch_bytes(8, 12, None) == 2 and b'null bytes' in err()
    assert L.deva_vos_boundary_scratch_bytes(8, -1, ctypes.byref(nbytes)) == 2 and b'bad plane size' in err()


def test_wrapper_errors_before_any_launch():
    from deva.hip import DevaHipError
    vm = _built()
    gt, pred = torch.zeros(4, 6, dtype=torch.int32), torch.zeros(4, 6, dtype=torch.int64)
    with pytest.raises(DevaHipError, match='gt must be an .H,W. plane of torch.uint8, torch.int32'):
        vm.boundary_counts(pred, pred, [1])
    with pytest.raises(DevaHipError, match='pred must be an .H,W. plane'):
        vm.boundary_counts(gt, pred.float(), [1])
    with pytest.raises(DevaHipError, match=r'gt is \(4, 6\) and pred \(4, 5\)'):
        vm.boundary_counts(gt, pred[:, :5], [1])
    with pytest.raises(DevaHipError, match='go together'):
        vm.boundary_counts(gt, pred.to(torch.int16), [1])
    with pytest.raises(DevaHipError, match='go together'):
        vm.boundary_counts(gt, pred, [1], pred_lut=torch.zeros(3, dtype=torch.uint16))
    for bad in ([3, 2], [2, 2], [0, 1], [-4], [2**31]):
        with pytest.raises(DevaHipError, match='distinct, ascending'):
            vm.boundary_counts(gt, pred, bad)
    with pytest.raises(DevaHipError, match='at least one object id'):
        vm.boundary_counts(gt, pred, [])
    with pytest.raises(DevaHipError, match='binary planes hold one object'):
        vm.boundary_counts(gt, pred, [1, 2], binary=True)
    with pytest.raises(DevaHipError, match="binary is False, True"):
        vm.boundary_counts(gt, pred, [1], binary='both')
    with pytest.raises(DevaHipError, match='radius 0 to 128'):
        vm.boundary_counts(gt, pred, [1], radius=129)
    with pytest.raises(DevaHipError, match='an integer'):
        vm.boundary_counts(gt, pred, [1], bound_th=2.5)
    with pytest.raises(DevaHipError, match=r'`out` must be uint32 \[2,8\]'):
        vm.boundary_counts(gt, pred, [1, 2], out=torch.zeros(2, 8, dtype=torch.int32))
    with pytest.raises(DevaHipError, match=r'`scratch` must be uint8 \[384\]'):
        vm.boundary_counts(gt, pred, [1, 2], scratch=torch.zeros(383, dtype=torch.uint8))
    with pytest.raises(DevaHipError, match='HIP device'):
        vm.boundary_counts(gt, pred, [1])


# ------------------------------------------------------------------------------------------ R3 and the plan
def test_radius_rule():
    vm = _built()
    for h, w in ((480, 854), (480, 910), (720, 1280), (1080, 1920), (2160, 3840), (375, 500), (3, 4)):   # the last two: integer diagonals
        assert vm.boundary_radius(h, w, 0.008) == int(np.ceil(0.008 * np.linalg.norm((h, w)))), (h, w)
        assert vm.boundary_radius(h, w) == VC.radius_of(h, w)
    assert [vm.boundary_radius(*s) for s in ((480, 854), (1080, 1920), (2160, 3840), (375, 500), (3, 4))] == [8, 18, 36, 5, 1]
    for r in (1, 5, 128):
        assert vm.boundary_radius(480, 854, r) == r == vm.boundary_radius(3, 4, float(r))
    assert vm.boundary_radius(480, 854, 0) == 0
    for bad, text in ((129, 'radius 0 to 128'), (2.5, 'an integer'), (-0.1, 'not negative'), (float('nan'), 'finite'),
                      (float('inf'), 'finite')):
        with pytest.raises(vm.DevaHipError, match=text):
            vm.boundary_radius(480, 854, bad)
    with pytest.raises(vm.DevaHipError, match='radius 0 to 128'):
        vm.boundary_radius(20000, 20000, 0.008)     # 227 pixels


def test_plan_is_host_side():
    vm = _built()
    # 480 x 854: 107 strips of 8 a row, 51 360 strips; 409 920 pixels, 6 405 chunks of 64 for at most 1024 x 4 waves
    assert vm.boundary_plan(240, 427, 5, 4).match_grid == 401          # 102 480 pixels: 1 602 chunks, a wave each
    assert vm.boundary_plan(480, 854, 5, 8) == vm.PlanInfo(201, 1024, 256, 80, 3, 8, 16 * 480 * 854)
    assert vm.boundary_scratch_bytes(480, 854) == 16 * 480 * 854
    assert vm.boundary_plan(480, 854, 64, 8) == vm.PlanInfo(201, 1024, 256, 1024, 3, 8, 16 * 480 * 854)
    assert vm.boundary_plan(1, 1, 1, 0) == vm.PlanInfo(1, 1, 256, 16, 0, 0, 16)
    assert vm.boundary_plan(9, 1, 2, 2).inner_radius == 2 and vm.boundary_plan(9, 1, 2, 128).inner_radius == 3
    big = vm.boundary_plan(32768, 32768, 1, 36)             # capped: the rest is a grid-stride loop
    assert (big.label_grid, big.match_grid, big.scratch_bytes) == (2048, 1024, 1 << 34)
    for n in (0, 65):
        with pytest.raises(vm.DevaHipError, match='1 to 64 objects'):
            vm.boundary_plan(480, 854, n, 8)
    with pytest.raises(vm.DevaHipError, match='bad plane size'):
        vm.boundary_plan(0, 5, 1, 1)


# ------------------------------------------------------------------------------------------ R6 by hand
def test_j_and_f_from_records_by_hand():
    from deva.inference.vos_quality import jf_from_counts
    records = np.array([[30, 40, 50, 10, 20, 5, 8, 0],      # J = 30 / 60; P = 8 / 20, R = 5 / 10: F = 2 * .4 * .5 / .9
                        [0, 40, 0, 12, 0, 0, 0, 0],         # nothing predicted: (P, R) = (1, 0), F = 0, J = 0
                        [0, 0, 17, 0, 9, 0, 0, 0],          # nothing to find: (0, 1), F = 0, J = 0
                        [0, 0, 0, 0, 0, 0, 0, 0],           # neither: union 0 -> J = 1; (1, 1) -> F = 1
                        [0, 9, 9, 6, 6, 0, 0, 0],           # boundaries on both sides, none matched: P + R = 0 -> F = 0
                        [12, 12, 12, 7, 7, 7, 7, 0]],       # the prediction is the ground truth
                       dtype=np.uint32)
    j, f = jf_from_counts(records)
    assert j.dtype == np.float64 and j.tolist() == [0.5, 0.0, 0.0, 1.0, 0.0, 1.0]
    assert f.tolist() == [2 * 0.4 * 0.5 / (0.4 + 0.5), 0.0, 0.0, 1.0, 0.0, 1.0]
    assert [VC.jf(r) for r in records] == list(zip(j.tolist(), f.tolist()))
    j2, f2 = jf_from_counts(records.reshape(2, 3, 8))           # any leading shape
    assert j2.shape == (2, 3) and np.array_equal(j2.reshape(-1), j) and np.array_equal(f2.reshape(-1), f)
    # a full plane at 2^30 pixels does not overflow
    j, _ = jf_from_counts(np.array([[2**30, 2**30, 2**30, 0, 0, 0, 0, 0]], dtype=np.uint32))
    assert j.tolist() == [1.0]


def _edges(n):
    return ((np.round(np.linspace(1, n, 5) + 1e-10) - 1).astype(np.int64) % 256).tolist()


def test_sequence_statistics_by_hand():
    from deva.inference.vos_quality import sequence_statistics
    m, o, d = sequence_statistics([0.2, 0.6, np.nan, 1.0])
    # length 4: edges 0, 1, 2, 2, 3 -> bins v[0:2], v[1:3], v[2:3], v[2:4]; the NaN is skipped (and is not "> 0.5")
    assert _edges(4) == [0, 1, 2, 2, 3]
    assert m == pytest.approx(0.6, abs=1e-15) and o == 0.5 and d == pytest.approx(0.4 - 1.0, abs=1e-15)
    assert _edges(5) == [0, 1, 2, 3, 4] and _edges(50) == [0, 12, 25, 37, 49]
    v = np.linspace(1.0, 0.0, 50)
    m, o, d = sequence_statistics(v)
    assert m == np.mean(v) and o == np.mean(v > 0.5) == 0.5 and d == np.mean(v[0:13]) - np.mean(v[37:50])
    v = np.array([0.9, 0.8, 0.7, 0.2, 0.1])
    assert sequence_statistics(v) == (np.mean(v), 0.6, np.mean(v[0:2]) - np.mean(v[3:5]))
    # 300 frames: the edges 0, 75, 150, 224, 299 become 0, 75, 150, 224, 43 as uint8; the last bin v[224:44] is empty
    assert _edges(300) == [0, 75, 150, 224, 43]
    v = np.linspace(1.0, 0.0, 300)
    m, o, d = sequence_statistics(v)
    assert m == np.mean(v) and o == 0.5 and np.isnan(d)
    assert all(a == b or (np.isnan(a) and np.isnan(b)) for a, b in zip(sequence_statistics(v), VC.statistics(v)))
    # all NaN and empty: NaN, no warning escapes
    assert all(np.isnan(x) for x in sequence_statistics([np.nan, np.nan])[::2])
    assert np.isnan(sequence_statistics([])[0])


# ------------------------------------------------------------------------------------------ the scorer on the contract
def _clip(h, w, n, frames, seed):
    """`frames` frames of one video: the case generator with one seed per frame"""
    out = [VC.case(h, w, n, seed + t) for t in range(frames)]
    return [c[0] for c in out], [c[1] for c in out], out[0][2]


def _reference(videos, skip_ends, radius=None):
    """the numpy statement applied video by video -> (per_object list for VC.table, {name: counts [T,n,8]})"""
    per_object, counts = [], {}
    for name, gts, preds, ids in videos:
        h, w = gts[0].shape
        r = VC.radius_of(h, w) if radius is None else radius
        c = np.stack([VC.counts(g, p, ids, r) for g, p in zip(gts, preds)])
        counts[name] = c
        scored = c[1:-1] if skip_ends else c
        for k in range(len(ids)):
            jf = [VC.jf(rec) for rec in scored[:, k]]
            per_object.append((name, k + 1, [a for a, _ in jf], [b for _, b in jf]))
    return per_object, counts


def _feed(scorer, videos, form=lambda pred, ids: pred.astype(np.int64)):
    for name, gts, preds, ids in videos:
        scorer.start_video(name, ids.tolist())
        for g, p in zip(gts, preds):
            scorer.add_frame(form(p, ids), g.astype(np.uint8))
        scorer.end_video()
    return scorer.result()


@pytest.fixture(scope='module')
def two_videos():
    a = ('bear',) + _clip(24, 40, 2, 6, 10)
    b = ('koala',) + _clip(30, 22, 3, 5, 40)
    return [a, b]


@pytest.mark.parametrize('skip_ends', [True, False])
def test_scorer_on_two_videos(two_videos, skip_ends, emu):
    from deva.inference.vos_quality import GLOBAL_HEADER, VideoObjectScorer
    res = _feed(VideoObjectScorer(skip_ends=skip_ends), two_videos)
    per_object, counts = _reference(two_videos, skip_ends)
    want = VC.table(per_object)
    assert list(res['global']) == GLOBAL_HEADER
    assert np.allclose([res['global'][k] for k in GLOBAL_HEADER], want, rtol=0, atol=1e-12)
    assert list(res['sequences']) == ['bear_1', 'bear_2', 'koala_1', 'koala_2', 'koala_3']
    for name, k, j, f in per_object:
        fr = res['frames'][name]
        assert np.array_equal(fr['counts'], counts[name]) and fr['ids'] == list(range(1, fr['J'].shape[0] + 1))
        assert fr['J'].shape == (len(fr['ids']), len(counts[name]) - (2 if skip_ends else 0))
        assert fr['J'][k - 1].tolist() == j and fr['F'][k - 1].tolist() == f
        seq = res['sequences'][f'{name}_{k}']
        assert seq['J-Mean'] == pytest.approx(np.mean(j), abs=1e-12) and seq['F-Mean'] == pytest.approx(np.mean(f), abs=1e-12)
    assert 0.3 < res['global']['J&F-Mean'] < 1.0     # the clip scores something


class _Result:
    """shaped like `FrameResult`: the channel plane and the id of every channel"""

    def __init__(self, index, channel_ids):
        self.index, self.channel_ids = torch.from_numpy(index), channel_ids


def test_frame_result_form_equals_the_planes(two_videos, emu):
    from deva.inference.vos_quality import VideoObjectScorer
    listed = lambda pred, ids: np.where(np.isin(pred, ids), pred, 0)   # noqa: E731  (the channel form drops unlisted ids)
    planes = _feed(VideoObjectScorer(), two_videos, lambda pred, ids: listed(pred, ids).astype(np.int32))
    seeds = iter(range(100))

    def as_result(pred, ids):
        index, lut, channel_ids = VC.channel_form(pred, ids, next(seeds))
        assert np.array_equal(channel_ids[index][np.isin(pred, ids)], pred[np.isin(pred, ids)])
        return _Result(index, channel_ids)
    fast = _feed(VideoObjectScorer(), two_videos, as_result)
    assert fast['global'] == planes['global'] and fast['sequences'] == planes['sequences']
    for name in ('bear', 'koala'):
        assert np.array_equal(fast['frames'][name]['counts'], planes['frames'][name]['counts'])
    # uint8, int32 and int64 planes, tensors or arrays: the same records
    for form in (lambda p, i: p.astype(np.uint8), lambda p, i: torch.from_numpy(p.astype(np.int32)), lambda p, i: torch.from_numpy(p)):
        other = _feed(VideoObjectScorer(), two_videos, form)
        assert np.array_equal(other['frames']['koala']['counts'], _feed(VideoObjectScorer(), two_videos)['frames']['koala']['counts'])


def test_scorer_misuse(emu):
    from deva.inference.vos_quality import VideoObjectScorer
    scorer = VideoObjectScorer()
    with pytest.raises(RuntimeError, match='start_video'):
        scorer.add_frame(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8))
    with pytest.raises(RuntimeError, match='start_video'):
        scorer.end_video()
    scorer.start_video('a', [2, 1, 2])
    assert scorer._ids.tolist() == [1, 2]
    with pytest.raises(RuntimeError, match='end_video'):
        scorer.start_video('b', [1])
    with pytest.raises(Exception, match=r'gt is \(4, 4\) and pred \(4, 5\)'):
        scorer.add_frame(np.zeros((4, 5), np.uint8), np.zeros((4, 4), np.uint8))     # another size is refused
    with pytest.raises(ValueError, match='no channel plane'):
        scorer.add_frame(_ResultNone(), np.zeros((4, 4), np.uint8))


class _ResultNone:
    index, channel_ids = None, None


GLOBAL_CSV = ('J&F-Mean,J-Mean,J-Recall,J-Decay,F-Mean,F-Recall,F-Decay\n'
              '0.581,0.608,0.583,0.148,0.554,0.583,0.085\n')
SEQUENCE_CSV = ('Sequence,J-Mean,F-Mean\n'
                'bear_1,0.558,0.519\n'
                'bear_2,0.674,0.513\n'
                'koala_1,0.644,0.652\n'
                'koala_2,0.598,0.449\n'
                'koala_3,0.566,0.638\n')


def test_write_gives_the_two_files_byte_for_byte(two_videos, emu, tmp_path):
    from deva.inference.vos_quality import VideoObjectScorer
    scorer = VideoObjectScorer()
    _feed(scorer, two_videos)
    scorer.write(str(tmp_path / 'out'))
    assert sorted(os.listdir(tmp_path / 'out')) == ['global_results.csv', 'per-sequence_results.csv']
    with open(tmp_path / 'out' / 'global_results.csv', newline='') as f:
        assert f.read() == GLOBAL_CSV
    with open(tmp_path / 'out' / 'per-sequence_results.csv', newline='') as f:
        assert f.read() == SEQUENCE_CSV
    # the strings above are the numpy statement's numbers
    per_object, _ = _reference(two_videos, True)
    assert GLOBAL_CSV.splitlines()[1] == ','.join('%.3f' % v for v in VC.table(per_object))
    assert SEQUENCE_CSV.splitlines()[1:] == ['%s_%d,%.3f,%.3f' % (name, k, np.mean(j), np.mean(f)) for name, k, j, f in per_object]


# ------------------------------------------------------------------------------------------ the offline form
def _write_tree(root, videos, binary):
    for name, gts, preds, ids in videos:
        for kind, planes in (('truth', gts), ('run', preds)):
            os.makedirs(os.path.join(root, kind, name), exist_ok=True)
            for t, plane in enumerate(planes):
                plane = np.where(np.isin(plane, ids), 255, 0) if binary else plane
                img = Image.fromarray(plane.astype(np.uint8), mode='L' if binary else 'P')
                if not binary:
                    img.putpalette([v for i in range(256) for v in (i, 255 - i, (7 * i) % 256)])
                img.save(os.path.join(root, kind, name, '%05d.png' % t))
    return os.path.join(root, 'run'), os.path.join(root, 'truth')


def test_score_directory(two_videos, emu, tmp_path):
    from deva.inference.vos_quality import VideoObjectScorer, score_directory
    run, truth = _write_tree(str(tmp_path), two_videos, False)
    # frame 0 of either video holds every object: the objects are 1 .. max id of that plane, 255 included (a sprinkle)
    clean = [(name, [np.where(g == 255, 0, g) for g in gts], [np.where(p == 255, 0, p) for p in preds], ids)
             for name, gts, preds, ids in two_videos]
    run, truth = _write_tree(str(tmp_path / 'clean'), clean, False)
    offline = score_directory(run, truth)
    online = _feed(VideoObjectScorer(), clean)
    assert offline['global'] == online['global'] and offline['sequences'] == online['sequences']
    assert list(offline['frames']) == ['bear', 'koala']
    only = score_directory(run, truth, ['koala'], skip_ends=False)
    assert list(only['frames']) == ['koala'] and only['frames']['koala']['J'].shape == (3, 5)
    os.remove(os.path.join(run, 'koala', '00002.png'))
    with pytest.raises(FileNotFoundError):
        score_directory(run, truth, ['koala'])


def test_score_directory_binary(two_videos, emu, tmp_path):
    from deva.inference.vos_quality import score_directory
    run, truth = _write_tree(str(tmp_path), two_videos, True)
    res = score_directory(run, truth, binary=True)
    assert list(res['sequences']) == ['bear_1', 'koala_1']
    for name, gts, preds, ids in two_videos:
        want = np.stack([VC.counts(np.isin(g, ids), np.isin(p, ids), [1], VC.radius_of(*g.shape)) for g, p in zip(gts, preds)])
        assert np.array_equal(res['frames'][name]['counts'], want)
        assert res['frames'][name]['ids'] == [1]


# ------------------------------------------------------------------------------------------ static resources
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith('.hip')) if os.path.isdir(CSRC) else []


def test_the_listing_is_not_empty():
    assert 'boundary_counts.hip' in SOURCES


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    kernels = abi_util.kernel_resources(os.path.join(CSRC, src))
    if src == 'boundary_counts.hip':   # 2 ground-truth encodings x 4 predicted, and the disk search
        assert sum('label_kernel' in name for name in kernels) == 8 and sum('match_kernel' in name for name in kernels) == 1
    for name, r in kernels.items():
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0, (name, r)  # (SGPR spills go to VGPR lanes, not to memory)
        assert r.get('LDS Size', 0) <= 160 * 1024, (name, r)
        assert r['Occupancy'] >= 4, (name, r)            # the launches are sized for 8 workgroups of 4 waves per CU
