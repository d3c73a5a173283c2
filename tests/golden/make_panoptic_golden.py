"""Regenerates tests/golden/panoptic_quality.{npz,json} from the REFERENCE's scoring scripts (CPU, well under a second):
    DEVA_REFERENCE_ROOT=<reference checkout> python tests/golden/make_panoptic_golden.py
Synthetic 48 x 64 videos are written as the two PNG trees the scripts read (ground truth, and the unmerged prediction
with its pred.json) into a temporary directory; then the reference's
    stuff_merging.process_single_video   per video, under np.random.seed(42)
    eval_stq_vipseg.eval_stq             (its STQuality.result() is captured on the way)
    eval_vpq_vipseg.vpq_compute_single_core per video and window, and eval_vpq for the text files
run on them.  Only data is stored: the id planes (int32), the segment lists, the merged annotations, the per-class
iou / tp / fp / fn per window, the STQ dict and the text of the output files.  `pulp` is stubbed as make_golden.py does.
Nothing here is imported by the product or the tests.

Between them the videos hold: a stuff category split over two predicted ids; a thing whose predicted category changes
mid-video (a re-drawn id); a crowd ground-truth segment; VOID strips on both sides; an unlisted non-zero ground-truth
id; a prediction mostly on VOID and one mostly on a same-category crowd; a duplicate id in a ground-truth JSON; a video
whose first-listed ground-truth id is a thing; a video shorter than every window but 1 and 2; ids using all three
colour bytes."""
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('DEVA_REFERENCE_ROOT')
if not REF or not os.path.isdir(os.path.join(REF, 'deva')):
    sys.exit('make_panoptic_golden: set DEVA_REFERENCE_ROOT to a checkout of the reference')
sys.modules.setdefault('pulp', types.ModuleType('pulp'))
sys.path.insert(0, REF)
from deva.utils.vipseg_categories import VIPSEG_CATEGORIES  # noqa: E402
from deva.vps_metrics import eval_stq_vipseg, eval_vpq_vipseg, stuff_merging  # noqa: E402
import deva.vps_metrics.segmentation_and_tracking_quality as numpy_stq  # noqa: E402

H, W = 48, 64
WINDOWS = [1, 2, 4, 6, 8, 10, 999]
DOOR, TABLE, PERSON_LIKE = 2, 4, 8       # thing categories
WALL, CEILING, FLOOR = 0, 1, 3           # stuff categories
assert {c['id']: bool(c['isthing']) for c in VIPSEG_CATEGORIES if c['id'] in (0, 1, 2, 3, 4, 8)} == \
    {DOOR: True, TABLE: True, PERSON_LIKE: True, WALL: False, CEILING: False, FLOOR: False}


def paint(rects):
    plane = np.zeros((H, W), dtype=np.int32)
    for seg_id, y0, y1, x0, x1 in rects:
        plane[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)] = seg_id
    return plane


def rgb(plane):
    return np.stack([plane % 256, plane // 256 % 256, plane // 65536 % 256], axis=-1).astype(np.uint8)


def listed(plane, entries):
    """segments_info of a plane: (id, fields) in order, with the true area; an id given twice has its area split"""
    out, seen = [], {}
    for seg_id, fields in entries:
        seen[seg_id] = seen.get(seg_id, 0) + 1
    used = {}
    for seg_id, fields in entries:
        area = int((plane == seg_id).sum())
        if seen[seg_id] > 1:
            k = used.get(seg_id, 0)
            used[seg_id] = k + 1
            area = area // 2 if k == 0 else area - area // 2
        if area > 0 or 'iscrowd' in fields:
            out.append(dict(id=seg_id, area=area, **fields))
    return out


def video_a(t):
    """first-listed ground-truth id is a thing; crowd; VOID strips; unlisted id; duplicate JSON id; category change"""
    gt = paint([(131844, 0, H, 0, 60), (77, 0, 8, 0, 60), (66051, 12 + t, 30 + t, 4 + 2 * t, 20 + 2 * t), (500, 30, 44, 30, 44),
                (900, 10, 26, 44, 58), (999, 44, 47, 2, 6)])             # columns 60..63 stay VOID; 999 is not listed
    gt_info = listed(gt, [(66051, dict(category_id=DOOR, iscrowd=0)), (500, dict(category_id=TABLE, iscrowd=0)),
                          (131844, dict(category_id=WALL, iscrowd=0))] +
                     [(77, dict(category_id=CEILING, iscrowd=0))] * (2 if t == 2 else 1) +
                     [(900, dict(category_id=TABLE, iscrowd=1))])
    pred = paint([(1193046, 0, 46, 0, 30), (400, 0, 46, 30, 58), (410, 0, 7, 0, 58), (300, 13 + t, 30 + t, 4 + 2 * t, 21 + 2 * t),
                  (301, 31, 44, 29, 44), (420, 30, 40, 58, 64), (430, 12, 24, 46, 57)])   # rows 46, 47 stay VOID
    cat_301 = TABLE if t < 3 else PERSON_LIKE
    pred_info = listed(pred, [(1193046, dict(category_id=WALL, score=0.9)), (300, dict(category_id=DOOR, score=0.8)),
                              (301, dict(category_id=cat_301, score=0.7)), (400, dict(category_id=WALL, score=0.6)),
                              (410, dict(category_id=CEILING, score=0.5)), (420, dict(category_id=DOOR, score=0.4)),
                              (430, dict(category_id=TABLE, score=0.3))])
    return gt, gt_info, pred, pred_info


def video_b(t):
    """first-listed id is stuff; a thing that is missed for two frames; a prediction with a poor overlap"""
    gt = paint([(70000, 0, H, 0, W), (70001, 30, H, 0, W), (256, 8, 24, 8 + 3 * t, 24 + 3 * t), (65536, 26, 40, 40, 56)])
    gt_info = listed(gt, [(70000, dict(category_id=WALL, iscrowd=0)), (70001, dict(category_id=FLOOR, iscrowd=0)),
                          (256, dict(category_id=PERSON_LIKE, iscrowd=0)), (65536, dict(category_id=DOOR, iscrowd=0))])
    rects = [(513, 0, 31, 0, W), (514, 31, H, 0, 40), (70002, 31, H, 40, W), (9000, 8, 24, 9 + 3 * t, 26 + 3 * t)]
    if t not in (1, 2):
        rects.append((9001, 20, 40, 30, 62))
    pred = paint(rects)
    pred_info = listed(pred, [(513, dict(category_id=WALL, score=0.9)), (514, dict(category_id=FLOOR, score=0.9)),
                              (70002, dict(category_id=FLOOR, score=0.8)), (9000, dict(category_id=PERSON_LIKE, score=0.7)),
                              (9001, dict(category_id=DOOR, score=0.6))])
    return gt, gt_info, pred, pred_info


def video_c(t):
    """three frames: shorter than the windows 4 .. 999; an object whose id is taken by a stuff category's first id"""
    gt = paint([(16777215, 0, H, 0, W), (1000, 10, 30, 10 + t, 34 + t)])
    gt_info = listed(gt, [(1000, dict(category_id=TABLE, iscrowd=0)), (16777215, dict(category_id=CEILING, iscrowd=0))])
    pred = paint([(2000, 0, H, 0, W), (2001, 10, 31, 11 + t, 34 + t), (2002, 40, 46, 50, 60)])
    pred_info = listed(pred, [(2000, dict(category_id=CEILING if t < 2 else TABLE, score=0.9)),
                              (2001, dict(category_id=TABLE, score=0.8)), (2002, dict(category_id=CEILING, score=0.7))])
    return gt, gt_info, pred, pred_info


VIDEOS = (('a_first_thing', video_a, 7), ('b_first_stuff', video_b, 5), ('c_short', video_c, 3))


def tolist(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (list, tuple)):
        return [tolist(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


def check_rounding(values):
    for v in values:
        frac = (float(v) * 10) % 1.0
        assert abs(frac - 0.5) > 1e-5, f'{v} is at a %.1f rounding boundary: change the scene'


def main():
    planes, gt_videos, gt_annos, raw_annos = {}, [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        truth, raw, merged = (os.path.join(tmp, d) for d in ('truth', 'raw', 'merged'))
        for name, make, frames in VIDEOS:
            os.makedirs(os.path.join(truth, name))
            os.makedirs(os.path.join(raw, 'pan_pred', name))
            gts, preds, gt_frames, pred_frames, images = [], [], [], [], []
            for t in range(frames):
                gt, gt_info, pred, pred_info = make(t)
                file_name = '%05d.png' % t
                Image.fromarray(rgb(gt)).save(os.path.join(truth, name, file_name))
                Image.fromarray(rgb(pred)).save(os.path.join(raw, 'pan_pred', name, file_name))
                gts.append(gt)
                preds.append(pred)
                images.append({'file_name': file_name})
                gt_frames.append({'file_name': file_name, 'segments_info': gt_info})
                pred_frames.append({'file_name': file_name[:-4] + '.jpg', 'segments_info': pred_info})
            planes[name + '/gt'], planes[name + '/pred'] = np.stack(gts), np.stack(preds)
            gt_videos.append({'video_id': name, 'images': images})
            gt_annos.append({'video_id': name, 'annotations': gt_frames})
            raw_annos.append({'video_id': name, 'annotations': pred_frames})
        gt_json = {'categories': VIPSEG_CATEGORIES, 'videos': gt_videos, 'annotations': gt_annos}
        gt_json_file = os.path.join(tmp, 'gt.json')
        with open(gt_json_file, 'w') as f:
            json.dump(gt_json, f)
        with open(os.path.join(raw, 'pred.json'), 'w') as f:
            json.dump({'annotations': raw_annos}, f)

        # ---- merge_stuff, one video at a time (merge_stuff itself only adds a process pool and a progress bar)
        merged_annos = []
        for vid in raw_annos:
            np.random.seed(42)
            merged_annos.append(stuff_merging.process_single_video(vid, raw, merged))
        with open(os.path.join(merged, 'pred.json'), 'w') as f:
            json.dump({'annotations': merged_annos}, f)
        for name, _, frames in VIDEOS:
            out = []
            for t in range(frames):
                a = np.array(Image.open(os.path.join(merged, 'pan_pred', name, '%05d.png' % t))).astype(np.int32)
                out.append(a[:, :, 0] + 256 * a[:, :, 1] + 65536 * a[:, :, 2])
            planes[name + '/merged'] = np.stack(out)
        redrawn = [s['id'] for v in merged_annos for a in v['annotations'] for s in a['segments_info']]
        raw_ids = set(s['id'] for v in raw_annos for a in v['annotations'] for s in a['segments_info'])
        assert any(i not in raw_ids for i in redrawn), 'no id was re-drawn'

        # ---- STQ
        captured = {}
        original = numpy_stq.STQuality.result

        def result(self):
            captured['result'] = original(self)
            captured['confusion'] = sum(self._iou_confusion_matrix_per_sequence.values())
            return captured['result']
        numpy_stq.STQuality.result = result
        eval_stq_vipseg.eval_stq(merged, truth, gt_json_file)
        numpy_stq.STQuality.result = original
        stq = {k: tolist(v) for k, v in captured['result'].items()}
        stq['confusion'] = tolist(captured['confusion'])

        # ---- VPQ: the per-class sums from vpq_compute_single_core, the text files from eval_vpq
        categories = {el['id']: el for el in VIPSEG_CATEGORIES}
        merged_by_video = {v['video_id']: v['annotations'] for v in merged_annos}
        vpq = {}
        for k in WINDOWS:
            total = eval_vpq_vipseg.PQStat()
            for video, annos in zip(gt_videos, gt_annos):
                name = video['video_id']
                gt_names = [os.path.join(truth, name, im['file_name']) for im in video['images']]
                pred_names = [os.path.join(merged, 'pan_pred', name, im['file_name']) for im in video['images']]
                total += eval_vpq_vipseg.vpq_compute_single_core(
                    categories, k, list(zip(json.loads(json.dumps(annos['annotations'])),
                                            json.loads(json.dumps(merged_by_video[name])), gt_names, pred_names, video['images'])))
            _, per_class = total.pq_average(categories, None)
            vpq[str(k)] = {str(c): {key: tolist(r[key]) for key in ('iou', 'tp', 'fp', 'fn')} for c, r in per_class.items()
                           if r['tp'] + r['fp'] + r['fn'] > 0}
        eval_vpq_vipseg.eval_vpq(merged, truth, gt_json_file, num_processes=1)
        texts = {}
        for fn in ['vpq-%d.txt' % k for k in WINDOWS] + ['vpq-simple.txt', 'stq.txt']:
            with open(os.path.join(merged, fn)) as f:
                texts[fn] = f.read()

    printed = [stq['STQ'] * 100, stq['AQ'] * 100, stq['IoU'] * 100]
    for k in WINDOWS:
        for r in vpq[str(k)].values():
            q = r['tp'] + 0.5 * r['fp'] + 0.5 * r['fn']
            printed += [r['iou'], 100 * r['iou'] / q, 100 * r['tp'] / q] + ([100 * r['iou'] / r['tp']] if r['tp'] else [])
    for line in texts['vpq-simple.txt'].split(','):
        assert line == '' or len(line.split('/')) == 3
    check_rounding(printed)
    for k in WINDOWS:     # the All / Things / Stuff averages, re-read from the text at full precision is not possible: recompute
        for isthing in (None, True, False):
            rows = [r for c, r in vpq[str(k)].items() if isthing is None or bool(categories[int(c)]['isthing']) == isthing]
            qs = [(r['iou'] / (r['tp'] + 0.5 * r['fp'] + 0.5 * r['fn']), r['iou'] / r['tp'] if r['tp'] else 0,
                   r['tp'] / (r['tp'] + 0.5 * r['fp'] + 0.5 * r['fn'])) for r in rows]
            check_rounding([100 * sum(q[i] for q in qs) / len(qs) for i in range(3)])

    np.savez_compressed(os.path.join(HERE, 'panoptic_quality.npz'), **planes)
    with open(os.path.join(HERE, 'panoptic_quality.json'), 'w') as f:
        json.dump({'size': [H, W], 'windows': WINDOWS, 'videos': [v[0] for v in VIDEOS], 'gt_json': gt_json,
                   'raw_pred_json': {'annotations': raw_annos}, 'merged_pred_json': {'annotations': merged_annos},
                   'vpq': vpq, 'stq': stq, 'texts': texts}, f, separators=(',', ':'))
    print({k: v for k, v in texts.items() if k in ('vpq-simple.txt', 'stq.txt')})
    print(texts['vpq-1.txt'][:400])


if __name__ == '__main__':
    main()
