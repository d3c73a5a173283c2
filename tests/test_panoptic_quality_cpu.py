"""Scoring a VIPSeg run without a GPU: libdeva_metrics.so on its ABI and its argument errors, the CPU contract of the joint
count (tests/emu_panoptic.py) by hand, and `deva.inference.panoptic_quality` on that contract against what the
REFERENCE's merge_stuff, eval_stq and eval_vpq produced (tests/golden/panoptic_quality.{npz,json}, made by
tests/golden/make_panoptic_golden.py): integers equal, text files byte-identical, floats within 1e-9 relative (a float64
sum of up to 10^6 terms re-ordered moves by at most about 10^6 x 1.1e-16; eight digits tighter than anything printed)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import abi_util
import emu_frame_result as EF
import emu_ops
import emu_panoptic as EP
import result_case as RC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_metrics.h')
REL = 1e-9


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    EF.install(monkeypatch)
    EP.install(monkeypatch)


def _built():
    from deva.hip import metrics
    return abi_util.built(metrics)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    metrics = _built()
    exported, _ = abi_util.exported(metrics.LIB_PATH)
    want = ['deva_metrics_last_error', 'deva_metrics_panoptic_counts', 'deva_metrics_panoptic_plan', 'deva_metrics_version']
    assert exported == abi_util.declared(HEADER) == sorted(metrics.SIGNATURES) == want
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_METRICS_ABI_VERSION 1\b', header)
    assert metrics.ABI_VERSION == 1 and metrics.lib().deva_metrics_version() == 1
    for ref in ('stuff_merging.py:52-57', 'eval_stq_vipseg.py:132-147', 'eval_vpq_vipseg.py:147,190',
                'segmentation_and_tracking_quality.py:32,142'):
        assert ref in header, ref
    for name, value in (('MAX_IDS', metrics.MAX_IDS), ('STRIP', metrics.STRIP), ('LDS_LIMIT', metrics.LDS_LIMIT),
                        ('RGB8', metrics.RGB8), ('I32', metrics.I32), ('I64', metrics.I64), ('INDEX16', metrics.INDEX16)):
        assert re.search(rf'#define DEVA_METRICS_{name} {value}\b', header), name


def test_plan_mirror_has_the_c_layout(tmp_path):
    metrics = _built()
    fields = [f[0] for f in metrics.Plan._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_metrics.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(deva_metrics_plan));\n' +
                   ''.join(f'printf("%zu\\n", offsetof(deva_metrics_plan, {f}));\n' for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(metrics.Plan) and vals[1:] == [getattr(metrics.Plan, f).offset for f in fields]


def test_the_inference_library_is_untouched_and_shares_no_symbol():
    from deva import hip
    metrics = _built()
    hip_exported, hip_all = abi_util.exported(hip.LIB_PATH)
    assert len(hip_exported) == 80 and hip_exported == sorted(hip.SIGNATURES)
    assert not any(n.startswith('deva_metrics') for n in hip_exported)
    _, metrics_all = abi_util.exported(metrics.LIB_PATH)
    shared = {s for s in hip_all & metrics_all if 'deva' in s}
    assert not shared, shared


A = 1 << 30   # made-up addresses: validation fails before anything is dereferenced or launched


def _counts(L, gt=A, gt_enc=0, gt_ids=A + (1 << 28), n_gt=3, pred=A + (2 << 28), pred_enc=0, pred_ids=A + (3 << 28), n_pred=4,
            lut=None, channels=0, h=8, w=12, counts=A + (4 << 28)):
    return L.deva_metrics_panoptic_counts(gt, gt_enc, gt_ids, n_gt, pred, pred_enc, pred_ids, n_pred, lut, channels, h, w,
                                          counts, None)


def test_argument_errors_before_any_launch():
    metrics = _built()
    L = metrics.lib()
    err = L.deva_metrics_last_error
    assert _counts(L, gt_enc=2) == 2 and b'ground truth is RGB8 (0) or I32 (1)' in err()
    assert _counts(L, gt_enc=3) == 2 and b'ground truth is' in err()
    for enc in (-1, 4):
        assert _counts(L, pred_enc=enc) == 2 and b'unknown encoding' in err()
    assert _counts(L, n_gt=-1) == 2 and b'0 to 1022 ground-truth ids' in err()
    assert _counts(L, n_gt=1023) == 2 and b'0 to 1022 ground-truth ids' in err()
    assert _counts(L, n_pred=-1) == 2 and b'0 to 1022 predicted ids' in err()
    assert _counts(L, n_pred=1023) == 2 and b'0 to 1022 predicted ids' in err()
    assert _counts(L, h=0) == 2 and b'bad plane size' in err()
    assert _counts(L, w=-3) == 2 and b'bad plane size' in err()
    assert _counts(L, h=32769, w=32768) == 2 and b'bad plane size' in err()      # above 2^30 pixels
    assert _counts(L, gt=None) == 2 and b'ground-truth plane' in err()
    assert _counts(L, gt=A + 8) == 2 and b'misaligned ground-truth plane' in err()
    assert _counts(L, pred=None) == 2 and b'predicted plane' in err()
    assert _counts(L, pred=A + (2 << 28) + 4) == 2 and b'misaligned predicted plane' in err()
    assert _counts(L, gt_ids=None) == 2 and b'ground-truth id table' in err()
    assert _counts(L, gt_ids=A + 2) == 2 and b'ground-truth id table' in err()
    assert _counts(L, pred_ids=None) == 2 and b'predicted id table' in err()
    assert _counts(L, pred_ids=A + 1) == 2 and b'predicted id table' in err()
    assert _counts(L, counts=None) == 2 and b'counts' in err()
    assert _counts(L, counts=A + 2) == 2 and b'misaligned counts' in err()
    fast = dict(pred_enc=3, pred_ids=None, lut=A + (5 << 28), channels=7)
    assert _counts(L, **dict(fast, lut=None)) == 2 and b'channel table' in err()
    assert _counts(L, **dict(fast, lut=A + 1)) == 2 and b'channel table' in err()
    for channels in (0, -1, 32768):
        assert _counts(L, **dict(fast, channels=channels)) == 2 and b'1 to 32767 channels' in err()
    # the output over an input: the plane's last byte, a table's last entry, the channel table
    assert _counts(L, counts=A + 8 * 12 * 3 - 4) == 2 and b'overlaps an input' in err()
    assert _counts(L, counts=A + (1 << 28) + 8) == 2 and b'overlaps an input' in err()
    assert _counts(L, pred_enc=2, counts=A + (2 << 28) + 8 * 12 * 8 - 4) == 2 and b'overlaps an input' in err()
    assert _counts(L, **dict(fast, counts=A + (5 << 28) + 12)) == 2 and b'overlaps an input' in err()
    assert _counts(L, gt=A + (4 << 28) + 16) == 2 and b'overlaps an input' in err()
    assert all(b'deva_metrics_panoptic_counts' in (_counts(L, **kw), err())[1] for kw in (dict(h=0), dict(gt=None), dict(n_gt=-1)))
    plan = metrics.Plan()
    assert L.deva_metrics_panoptic_plan(8, 12, 3, 4, None) == 2 and b'deva_metrics_panoptic_plan: null plan' in err()
    assert L.deva_metrics_panoptic_plan(8, 12, 1023, 4, ctypes.byref(plan)) == 2 and b'ground-truth ids' in err()
    assert L.deva_metrics_panoptic_plan(0, 12, 3, 4, ctypes.byref(plan)) == 2 and b'bad plane size' in err()


def test_plan_is_host_side():
    metrics = _built()
    p = metrics.panoptic_plan(720, 1280, 40, 40)
    assert p == metrics.PlanInfo('lds', 225, 256, 4 * (42 * 42 + 80))           # 921600 / 16 / 256 workgroups
    assert metrics.panoptic_plan(1, 1, 0, 0) == metrics.PlanInfo('lds', 1, 256, 16)
    assert metrics.panoptic_plan(32768, 32768, 0, 0).grid == 2048                # capped: the rest is a grid-stride loop
    # the LDS path while 4 (G P + n_gt + n_pred) <= 64 KB
    edge = [n for n in range(1, 1023) if metrics.panoptic_plan(8, 8, 100, n).path == 'lds']
    assert edge == list(range(1, edge[-1] + 1)) and edge[-1] < 1022
    n = edge[-1]
    assert 4 * (102 * (n + 2) + 100 + n) <= metrics.LDS_LIMIT < 4 * (102 * (n + 3) + 101 + n)
    over = metrics.panoptic_plan(8, 8, 100, n + 1)
    assert over.path == 'global' and over.lds_bytes == 4 * (100 + n + 1)
    assert metrics.panoptic_plan(8, 8, 1022, 1022).path == 'global'
    with pytest.raises(metrics.DevaHipError, match='bad plane size'):
        metrics.panoptic_plan(0, 5, 1, 1)


def test_wrapper_errors_before_any_launch():
    from deva.hip import DevaHipError, metrics
    gt, pred = torch.zeros(4, 6, dtype=torch.int32), torch.zeros(4, 6, dtype=torch.int64)
    with pytest.raises(DevaHipError, match='uint8 .H,W,3. or an integer'):
        metrics.panoptic_counts(gt.float(), [1], pred, [1])
    with pytest.raises(DevaHipError, match='gt cannot be torch.int64'):
        metrics.panoptic_counts(pred, [1], pred, [1])
    with pytest.raises(DevaHipError, match=r'gt is \(4, 6\) and pred \(4, 5\)'):
        metrics.panoptic_counts(gt, [1], pred[:, :5], [1])
    with pytest.raises(DevaHipError, match='go together'):
        metrics.panoptic_counts(gt, [1], pred.to(torch.int16), [1])
    with pytest.raises(DevaHipError, match='go together'):
        metrics.panoptic_counts(gt, [1], pred, [1], torch.zeros(3, dtype=torch.uint16))
    for bad in ([3, 2], [2, 2], [0, 1], [-4], [2**31]):
        with pytest.raises(DevaHipError, match='distinct, ascending'):
            metrics.panoptic_counts(gt, bad, pred, [1])
    with pytest.raises(DevaHipError, match='at most 1022 pred_ids'):
        metrics.panoptic_counts(gt, [1], pred, list(range(1, 1024)))
    with pytest.raises(DevaHipError, match='uint16 .channels.'):
        metrics.panoptic_counts(gt, [1], pred.to(torch.int16), 1, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(DevaHipError, match=r'`out` must be uint32 \[3,3\]'):
        metrics.panoptic_counts(gt, [1], pred, [1], out=torch.zeros(3, 3, dtype=torch.int32))
    with pytest.raises(DevaHipError, match='HIP device'):
        metrics.panoptic_counts(gt, [1], pred, [1])
    assert metrics.id_table([5, 0, 3, 5, 70000]).tolist() == [3, 5, 70000]
    with pytest.raises(DevaHipError, match='1 .. 2.31 - 1'):
        metrics.id_table([-1, 4])


# ------------------------------------------------------------------------------------------ the contract by hand
def test_contract_by_hand():
    gt = np.array([[0, 0, 7, 7, 7, 9],
                   [0, 5, 5, 7, 7, 9],
                   [5, 5, 5, 5, 9, 9],
                   [66051, 66051, 5, 5, 0, 9]], dtype=np.int32)
    pred = np.array([[3, 3, 3, 4, 4, 4],
                     [3, 3, 8, 8, 4, 4],
                     [0, 0, 8, 8, 4, 11],
                     [0, 6, 6, 8, 4, -2]], dtype=np.int64)
    # gt table [5, 7]: 9 and 66051 are unlisted (slot 1); predicted table [3, 4, 8]: 6, 11 and -2 are unlisted
    want = np.array([[0, 0, 3, 1, 0],      # gt 0: under 3, 3, 3 / 4
                     [1, 3, 0, 3, 0],      # unlisted gt (9, 66051): 0 / 6, 11, -2 / 4 x 3
                     [2, 1, 1, 0, 4],      # gt 5
                     [0, 0, 1, 3, 1]],     # gt 7
                    dtype=np.uint32)
    got = EP.counts(gt, [5, 7], pred, [3, 4, 8])
    assert got.dtype == np.uint32 and np.array_equal(got, want) and got.sum() == 24
    rgb = np.stack([gt % 256, gt // 256 % 256, gt // 65536], axis=-1).astype(np.uint8)
    assert np.array_equal(EP.counts(rgb, [5, 7], pred.astype(np.int32), [3, 4, 8]), want)
    # the fast form: channels 0..5 carry the ids 0, 3, 4, 8, 8 (a shared slot), 6 (unlisted -> 1); an entry >= P -> 1
    channel = {3: 1, 4: 2, 8: 3, 0: 0, 6: 5, 11: 6, -2: -1}
    index = np.vectorize(channel.get)(pred).astype(np.int16)
    index[1, 2] = 4                                         # the second channel of id 8
    lut = np.array([0, 2, 3, 4, 4, 1, 9], dtype=np.uint16)  # channel 6: entry 9 >= P = 5; channel -1: outside
    assert np.array_equal(EP.counts(gt, [5, 7], index, pred_lut=lut, n_pred=3), want)
    # listing 66051 moves its two pixels to a row of their own
    more = EP.counts(rgb, [5, 7, 66051], pred, [3, 4, 8])
    assert more.shape == (5, 5) and more[4].tolist() == [1, 1, 0, 0, 0] and more[1].tolist() == [0, 2, 0, 3, 0]
    # the installed wrapper: the same table as a uint32 tensor
    t = EP.panoptic_counts(torch.from_numpy(gt), [5, 7], torch.from_numpy(index), 3, torch.from_numpy(lut))
    assert t.dtype == torch.uint32 and np.array_equal(t.numpy(), want)


# ------------------------------------------------------------------------------------------ against the reference
@pytest.fixture(scope='module')
def golden(golden_dir):
    arrays = dict(np.load(os.path.join(golden_dir, 'panoptic_quality.npz')))
    with open(os.path.join(golden_dir, 'panoptic_quality.json')) as f:
        return arrays, json.load(f)


def _rgb(plane):
    return np.stack([plane % 256, plane // 256 % 256, plane // 65536 % 256], axis=-1).astype(np.uint8)


def write_tree(root, arrays, jsons, which):
    """the PNG tree and pred.json of the golden's unmerged ('pred') or merged prediction, and the truth tree + JSON"""
    for name in jsons['videos']:
        for kind, base in ((which, os.path.join(root, which, 'pan_pred')), ('gt', os.path.join(root, 'truth'))):
            os.makedirs(os.path.join(base, name), exist_ok=True)
            for t, plane in enumerate(arrays[f'{name}/{kind}']):
                Image.fromarray(_rgb(plane)).save(os.path.join(base, name, '%05d.png' % t))
    with open(os.path.join(root, which, 'pred.json'), 'w') as f:
        json.dump(jsons['raw_pred_json' if which == 'pred' else 'merged_pred_json'], f)
    with open(os.path.join(root, 'gt.json'), 'w') as f:
        json.dump(jsons['gt_json'], f)
    return os.path.join(root, which), os.path.join(root, 'truth'), os.path.join(root, 'gt.json')


def _isthing(jsons):
    return {c['id']: c['isthing'] == 1 for c in jsons['gt_json']['categories']}


def test_stuff_merger_gives_the_reference_ids(golden):
    from deva.inference.panoptic_quality import StuffMerger, remap_ids
    arrays, jsons = golden
    redrawn = 0
    for raw, merged in zip(jsons['raw_pred_json']['annotations'], jsons['merged_pred_json']['annotations']):
        np.random.seed(42)
        merger = StuffMerger(_isthing(jsons))
        name = raw['video_id']
        for t, (ann, want) in enumerate(zip(raw['annotations'], merged['annotations'])):
            id_map, segments = merger.frame(ann['segments_info'])
            assert segments == want['segments_info'] and want['file_name'] == ann['file_name']
            assert np.array_equal(remap_ids(arrays[f'{name}/pred'][t].astype(np.int64), id_map), arrays[f'{name}/merged'][t])
            redrawn += sum(new not in id_map for new in id_map.values())
    assert redrawn > 0   # (a category change took an id that was already given away)


def test_merge_directory_writes_what_merge_stuff_wrote(golden, tmp_path):
    from deva.inference.panoptic_quality import merge_directory
    arrays, jsons = golden
    raw, _, _ = write_tree(str(tmp_path), arrays, jsons, 'pred')
    # merge_stuff seeds nothing; the golden was made one video at a time under seed 42, so is this
    from deva.inference import panoptic_quality as PQ
    original = PQ.StuffMerger.__init__

    def seeded(self, *a, **k):
        np.random.seed(42)
        original(self, *a, **k)
    PQ.StuffMerger.__init__ = seeded
    try:
        out_json = merge_directory(raw, str(tmp_path / 'out'), _isthing(jsons))
    finally:
        PQ.StuffMerger.__init__ = original
    assert out_json == jsons['merged_pred_json']
    with open(tmp_path / 'out' / 'pred.json') as f:
        assert json.load(f) == jsons['merged_pred_json']
    for name in jsons['videos']:
        for t, want in enumerate(arrays[f'{name}/merged']):
            got = np.array(Image.open(tmp_path / 'out' / 'pan_pred' / name / ('%05d.png' % t)))
            assert got.dtype == np.uint8 and np.array_equal(got, _rgb(want)), (name, t)


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= REL * np.abs(b)))


def check_against_golden(result, texts, jsons):
    for k in jsons['windows']:
        per_class = result['vpq'][k]['per_class']
        want = jsons['vpq'][str(k)]
        touched = {str(c) for c, r in per_class.items() if r['tp'] + r['fp'] + r['fn'] > 0}
        assert touched == set(want), k
        for c, w in want.items():
            r = per_class[int(c)]
            assert (r['tp'], r['fp'], r['fn']) == (w['tp'], w['fp'], w['fn']), (k, c)
            assert _close(r['iou'], w['iou']), (k, c, r['iou'], w['iou'])
    stq, want = result['stq'], jsons['stq']
    assert stq['Length_per_seq'] == want['Length_per_seq'] and stq['ID_per_seq'] == want['ID_per_seq']
    assert np.array_equal(stq['confusion'], np.array(want['confusion']))
    for key in ('STQ', 'AQ', 'IoU', 'STQ_per_seq', 'AQ_per_seq', 'IoU_per_seq'):
        assert _close(stq[key], want[key]), key
    assert texts == jsons['texts']


def test_score_directory_against_the_reference(golden, emu, tmp_path):
    from deva.inference.panoptic_quality import score_directory
    arrays, jsons = golden
    submit, truth, gt_json = write_tree(str(tmp_path), arrays, jsons, 'merged')
    result = score_directory(submit, truth, gt_json)
    texts = {}
    for name in jsons['texts']:
        with open(os.path.join(submit, name)) as f:
            texts[name] = f.read()
    assert sorted(os.listdir(submit)) == sorted(list(jsons['texts']) + ['pan_pred', 'pred.json'])
    check_against_golden(result, texts, jsons)
    assert result['videos'] == jsons['videos']


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and not isinstance(a, np.ndarray):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def test_online_scorer_equals_score_directory(golden, emu, tmp_path):
    """frame by frame, every encoding of the planes, no hint of the video's ids: the same result to the last bit"""
    from deva.inference.panoptic_quality import VideoPanopticScorer, score_directory
    arrays, jsons = golden
    submit, truth, gt_json = write_tree(str(tmp_path), arrays, jsons, 'merged')
    offline = score_directory(submit, truth, gt_json, write=False)
    gt_j = {v['video_id']: v['annotations'] for v in jsons['gt_json']['annotations']}
    pred_j = {v['video_id']: v['annotations'] for v in jsons['merged_pred_json']['annotations']}
    scorers = {form: VideoPanopticScorer(jsons['gt_json']['categories']) for form in ('int', 'rgb', 'index')}
    for name in jsons['videos']:
        for form, scorer in scorers.items():
            scorer.start_video(name)
            for t, (gt, pred) in enumerate(zip(arrays[f'{name}/gt'], arrays[f'{name}/merged'])):
                if form == 'int':
                    planes = torch.from_numpy(pred.astype(np.int64)), torch.from_numpy(gt)
                elif form == 'rgb':
                    planes = _rgb(pred), torch.from_numpy(_rgb(gt))
                else:      # the tracker's form: a channel plane and the id of each channel, two channels sharing an id
                    ids = np.unique(pred)
                    channel_ids = np.concatenate([[0], ids[ids != 0], ids[ids != 0][:1], [123456]])
                    index = (np.searchsorted(ids[ids != 0], pred) + 1) * (pred != 0)
                    first = index == 1
                    first[::2] = False
                    index[first] = len(channel_ids) - 2
                    assert np.array_equal(channel_ids[index], pred)
                    planes = (torch.from_numpy(index.astype(np.int16)), channel_ids), torch.from_numpy(gt)
                scorer.add_frame(planes[0], pred_j[name][t]['segments_info'], planes[1], gt_j[name][t]['segments_info'])
            scorer.end_video()
    for form, scorer in scorers.items():
        assert _same(scorer.result(), offline), form
    check_against_golden(scorers['index'].result(), scorers['index'].texts(), jsons)


def test_scorer_keeps_the_reference_key_errors(golden, emu):
    from deva.inference.panoptic_quality import VideoPanopticScorer
    arrays, jsons = golden
    name = jsons['videos'][1]
    gt, pred = arrays[f'{name}/gt'][0], arrays[f'{name}/merged'][0]
    gt_info = jsons['gt_json']['annotations'][1]['annotations'][0]['segments_info']
    pred_info = jsons['merged_pred_json']['annotations'][1]['annotations'][0]['segments_info']
    cats = jsons['gt_json']['categories']
    for planes in ((torch.from_numpy(pred.astype(np.int64)),), (_rgb(pred),)):
        scorer = VideoPanopticScorer(cats)
        scorer.start_video(name)
        scorer.add_frame(planes[0], pred_info[1:], torch.from_numpy(gt), gt_info)
        with pytest.raises(KeyError, match=f'Segment with ID {pred_info[0]["id"]} is presented in PNG and not presented in JSON'):
            scorer.end_video()
    scorer = VideoPanopticScorer(cats)
    scorer.start_video(name)
    scorer.add_frame(torch.from_numpy(pred.astype(np.int64)), pred_info + [{'id': 31337, 'category_id': 2, 'isthing': 1}],
                     torch.from_numpy(gt), gt_info)
    with pytest.raises(KeyError, match=r'segment IDs \[31337\] are presented in JSON and not presented in PNG'):
        scorer.end_video()
    scorer = VideoPanopticScorer(cats)
    scorer.start_video(name)
    bad = [dict(pred_info[0], category_id=777)] + pred_info[1:]
    scorer.add_frame(torch.from_numpy(pred.astype(np.int64)), bad, torch.from_numpy(gt), gt_info)
    with pytest.raises(KeyError, match=f'Segment with ID {pred_info[0]["id"]} has unknown category_id 777'):
        scorer.end_video()


# ------------------------------------------------------------------------------------------ the saver's hook
def _run_saver(root, jsons, merge):
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    from deva.inference.panoptic_quality import StuffMerger
    seen = []

    def make(out, video, **kw):
        if merge:
            kw.update(id_postprocessor=StuffMerger(_isthing(jsons)), frame_hook=lambda name, res, ann: seen.append((name, res, ann)))
        return FrameResultSaver(out, video, **kw)
    # objects 1000 and 66051 are one stuff category; 70000 is a thing; a fourth object takes a second category of 70000's
    spec = (True, [(1000, 3, 0.9), (70000, 2, 0.5), (66051, 3, None)], True)
    np.random.seed(42)
    saver, om = RC.run_saver(make, ObjectManager, ObjectInfo, 'vipseg', root, spec)
    return saver, seen


def test_saver_with_the_merger_writes_what_merge_directory_writes(golden, emu, tmp_path):
    from deva.inference.panoptic_quality import merge_directory
    _, jsons = golden
    plain, _ = _run_saver(str(tmp_path / 'plain'), jsons, False)
    with open(tmp_path / 'plain' / 'pred.json', 'w') as f:
        json.dump({'annotations': [plain.video_json]}, f)
    np.random.seed(42)
    want = merge_directory(str(tmp_path / 'plain'), str(tmp_path / 'offline'), _isthing(jsons))
    hooked, seen = _run_saver(str(tmp_path / 'hooked'), jsons, True)
    assert json.loads(json.dumps(hooked.video_json)) == want['annotations'][0]
    merged_ids = [[s['id'] for s in a['segments_info']] for a in hooked.video_json['annotations']]
    assert merged_ids == [[70000, 1000]] * 4        # the two stuff objects became one segment, listed after the thing
    for t in range(RC.FRAMES):
        rel = os.path.join('pan_pred', 'clip', '%05d.png' % t)
        with open(tmp_path / 'hooked' / rel, 'rb') as a, open(tmp_path / 'offline' / rel, 'rb') as b:
            assert a.read() == b.read(), rel
    # the hook saw every frame with its channel plane and the ids the channels were given
    assert [s[0] for s in seen] == RC.NAMES and all(s[2] is a for s, a in zip(seen, hooked.video_json['annotations']))
    for (_, res, _), t in zip(seen, range(RC.FRAMES)):
        assert res.channel_ids.tolist() == [0, 1000, 70000, 1000] and res.index.dtype == torch.int16
        got = np.array(Image.open(tmp_path / 'hooked' / 'pan_pred' / 'clip' / ('%05d.png' % t)))
        assert np.array_equal(_rgb(res.channel_ids[res.index.numpy().astype(np.int64)]), got)


def test_saver_without_the_keyword_writes_the_same_bytes_as_before(golden_dir, emu, tmp_path):
    """(against the reference saver's golden of tests/test_frame_result_cpu.py: planes and JSON)"""
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    arrays = dict(np.load(os.path.join(golden_dir, 'result_saver.npz')))
    with open(os.path.join(golden_dir, 'result_saver.json')) as f:
        jsons = json.load(f)
    saver, _ = RC.run_saver(FrameResultSaver, ObjectManager, ObjectInfo, 'vipseg', str(tmp_path))
    assert saver.id_postprocessor is None and saver.frame_hook is None
    assert json.loads(json.dumps(saver.video_json)) == jsons['vipseg']
    planes = {k[len('vipseg/'):]: v for k, v in arrays.items() if k.startswith('vipseg/')}
    assert len(planes) >= RC.FRAMES
    for rel, ref in planes.items():
        assert np.array_equal(np.array(Image.open(tmp_path / rel)), ref), rel
    with pytest.raises(ValueError, match="belongs to dataset 'vipseg'"):
        FrameResultSaver(str(tmp_path), 'clip', dataset='demo', object_manager=ObjectManager(), id_postprocessor=object())
