"""Scoring a VIPSeg run from one joint count per frame (not part of the reference's interface, as frame_results.py is
not): stuff merging without a second pass, VPQ and STQ.

After the last frame the reference runs `merge_stuff` (deva/vps_metrics/stuff_merging.py), which re-reads and re-writes
every PNG, then `eval_stq` and `eval_vpq`, which read both PNG trees again and call np.unique over stacked frames for
each window size.  Everything those compute per pixel depends only on the pair (ground-truth segment, predicted
segment) at that pixel, so here one G x P table per frame (`deva.hip.metrics.panoptic_counts`, one pass over planes
that are already on the device) replaces all of it, and what remains is host arithmetic over a few hundred integers
per frame.  The arithmetic below restates the reference from those tables, keyed back to ids:

  StuffMerger         the policy of IDPostprocessor (pano_utils.py:44-82) as a table; the `id_postprocessor` of
                      `FrameResultSaver`, which then writes what merge_stuff would have written
  merge_directory     the offline form of merge_stuff on an existing output tree (numpy)
  VideoPanopticScorer VPQ (eval_vpq_vipseg.py:106-303) and STQ (eval_stq_vipseg.py:103-168,
                      segmentation_and_tracking_quality.py:111-291), fed frame by frame
  score_directory     the same scorer fed from PNG trees and pred.json: eval_vpq + eval_stq of a finished run
"""
import json
import os
from os import path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from deva.hip import metrics

VOID = 0
OTHER = -1     # the key of "an id that the table does not list" in a frame's pair table


# ------------------------------------------------------------------------------------------ stuff merging
class StuffMerger:
    """IDPostprocessor (pano_utils.py:44-82) for one video: a thing keeps one id per (object, category), a stuff
    category keeps one id per video; the default id is the object's own, a taken one is re-drawn with
    np.random.randint(256, 256**3) -- under the same numpy seed the ids are the reference's.

    `frame(segments_info)` is one frame of stuff_merging.py:38-78.  The saver cannot call it as a whole, because the
    ids must be in the tables before the frame is launched and the areas arrive after it: it calls `assign` for every
    object of the table at launch and `annotation` with the areas in its worker.  merge_stuff only ever sees the objects
    with area; the two agree unless an object's first frame under a new (object, category) or stuff category has no
    pixel at all (then that id is allotted one frame early here)."""

    def __init__(self, cat_to_isthing: Dict[int, bool]):
        self.cat_to_isthing = {int(k): bool(v) for k, v in cat_to_isthing.items()}
        self.all_id = set()
        self.thing_obj_to_id = {}
        self.stuff_to_id = {}     # category -> id, in first-seen order

    def _find_new_id(self, default_id: int) -> int:
        new_id = default_id
        while new_id in self.all_id:
            new_id = int(np.random.randint(256, 256**3))
        return new_id

    def convert(self, obj: int, category_id: int) -> int:
        table, key = ((self.thing_obj_to_id, (obj, category_id)) if self.cat_to_isthing[category_id] else
                      (self.stuff_to_id, category_id))
        if key not in table:
            table[key] = self._find_new_id(obj)
            self.all_id.add(table[key])
        return table[key]

    def assign(self, segments_info: Iterable[Dict]) -> Tuple[Dict[int, int], List[Tuple[int, int]]]:
        """-> (old id -> new id for the segments in order, the video's (stuff category, id) list so far)"""
        id_map = {}
        for seg in segments_info:
            id_map[int(seg['id'])] = self.convert(int(seg['id']), int(seg['category_id']))   # (a repeated id: the last wins)
        return id_map, list(self.stuff_to_id.items())

    def annotation(self, segments_info: Iterable[Dict], id_map: Dict[int, int], stuff: Sequence[Tuple[int, int]],
                   areas: Dict[int, int]) -> List[Dict]:
        """merge_stuff's segments_info of a frame: the things in order, then every stuff id of the video with area in
        this frame in first-seen order (stuff_merging.py:52-78); `areas`: pixels per OLD id"""
        out = [{'id': id_map[int(s['id'])], 'category_id': s['category_id'], 'isthing': 1} for s in segments_info
               if self.cat_to_isthing[int(s['category_id'])]]
        merged = {}
        for old, new in id_map.items():
            merged[new] = merged.get(new, 0) + int(areas.get(old, 0))
        out += [{'id': new, 'category_id': cat, 'isthing': 0} for cat, new in stuff if merged.get(new, 0) > 0]
        return out

    def frame(self, segments_info: Sequence[Dict], areas: Optional[Dict[int, int]] = None):
        """-> (old id -> new id, merge_stuff's annotation); `areas` (pixels per old id) default to the segments' own"""
        if areas is None:
            areas = {}
            for s in segments_info:
                areas[int(s['id'])] = int(s['area'])
        id_map, stuff = self.assign(segments_info)
        return id_map, self.annotation(segments_info, id_map, stuff, areas)


def rgb_to_id(rgb: np.ndarray) -> np.ndarray:
    rgb = np.asarray(rgb).astype(np.int64)
    return rgb[:, :, 0] + 256 * rgb[:, :, 1] + 65536 * rgb[:, :, 2]


def id_to_rgb(ids: np.ndarray) -> np.ndarray:
    ids = np.asarray(ids, dtype=np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536 % 256], axis=-1).astype(np.uint8)


def remap_ids(plane: np.ndarray, id_map: Dict[int, int]) -> np.ndarray:
    """output_mask of stuff_merging.py:50-57: new id where the old one is mapped, 0 elsewhere"""
    old = np.array(sorted(id_map), dtype=np.int64)
    if old.size == 0:
        return np.zeros_like(plane)
    new = np.array([id_map[int(o)] for o in old], dtype=np.int64)
    at = np.clip(np.searchsorted(old, plane), 0, old.size - 1)
    return np.where(old[at] == plane, new[at], 0)


def merge_directory(input_path: str, output_path: str, cat_to_isthing: Dict[int, bool]) -> Dict:
    """merge_stuff (stuff_merging.py:91-105) on an existing output tree: reads `input_path`/pred.json and pan_pred/,
    writes the merged PNGs and pred.json under `output_path`, returns the JSON.  numpy on the host, one remap per frame
    (the reference makes one masked assignment per segment)."""
    from PIL import Image
    with open(path.join(input_path, 'pred.json')) as f:
        videos = json.load(f)['annotations']
    out_videos = []
    for vid in videos:
        video_id = vid['video_id']
        out_dir = path.join(output_path, 'pan_pred', video_id)
        os.makedirs(out_dir, exist_ok=True)
        merger = StuffMerger(cat_to_isthing)
        out_frames = []
        for ann in vid['annotations']:
            name = ann['file_name'].replace('.jpg', '.png')
            plane = rgb_to_id(np.array(Image.open(path.join(input_path, 'pan_pred', video_id, name))))
            ids, n = np.unique(plane, return_counts=True)
            id_map, segments = merger.frame(ann['segments_info'], dict(zip(ids.tolist(), n.tolist())))
            out_frames.append({'file_name': ann['file_name'], 'segments_info': segments})
            Image.fromarray(id_to_rgb(remap_ids(plane, id_map))).save(path.join(out_dir, name))
        out_videos.append({'video_id': video_id, 'annotations': out_frames})
    out_json = {'annotations': out_videos}
    with open(path.join(output_path, 'pred.json'), 'w') as f:
        json.dump(out_json, f)
    return out_json


# ------------------------------------------------------------------------------------------ VPQ
class _Stat:
    __slots__ = ('iou', 'tp', 'fp', 'fn')

    def __init__(self):
        self.iou, self.tp, self.fp, self.fn = 0.0, 0, 0, 0


def _merge_segments(segments_info, with_area=True):
    """gt_segms / pred_segms of eval_vpq_vipseg.py:133-144: first entry per id, the areas of duplicates added"""
    out = {}
    for el in segments_info:
        if el['id'] in out:
            out[el['id']]['area'] += el['area']
        else:
            out[el['id']] = dict(el)
    return out


def _vpq_tube(frames, stat: Dict[int, _Stat]) -> None:
    """steps 2-4 of vpq_compute_single_core (eval_vpq_vipseg.py:170-255) for one tube of frames"""
    gt_segms, pred_segms, pairs = {}, {}, {}
    for fr in frames:
        for table, segms in ((gt_segms, fr.gt_segms), (pred_segms, fr.pred_segms)):
            for k, seg in segms.items():
                if k not in table:
                    table[k] = dict(seg)
                else:
                    table[k]['area'] += seg['area']
        for key, n in fr.pairs.items():
            pairs[key] = pairs.get(key, 0) + n
    gt_matched, pred_matched = set(), set()
    for (gt_label, pred_label) in sorted(k for k in pairs if k[0] != OTHER and k[1] != OTHER):   # (np.unique's order)
        if gt_label not in gt_segms or pred_label not in pred_segms:
            continue
        gt, pred = gt_segms[gt_label], pred_segms[pred_label]
        if gt['iscrowd'] == 1 or gt['category_id'] != pred['category_id']:
            continue
        inter = pairs[(gt_label, pred_label)]
        union = pred['area'] + gt['area'] - inter - pairs.get((VOID, pred_label), 0)
        iou = inter / union
        assert iou <= 1.0, 'INVALID IOU VALUE : %d' % gt_label
        if iou > 0.5:
            stat[gt['category_id']].tp += 1
            stat[gt['category_id']].iou += iou
            gt_matched.add(gt_label)
            pred_matched.add(pred_label)
    crowd = {}
    for gt_label, gt in gt_segms.items():
        if gt_label in gt_matched:
            continue
        if gt['iscrowd'] == 1:          # neither matched nor FN; the category's last one is its crowd region
            crowd[gt['category_id']] = gt_label
            continue
        stat[gt['category_id']].fn += 1
    for pred_label, pred in pred_segms.items():
        if pred_label in pred_matched:
            continue
        inter = pairs.get((VOID, pred_label), 0)
        if pred['category_id'] in crowd:
            inter += pairs.get((crowd[pred['category_id']], pred_label), 0)
        if inter / pred['area'] > 0.5:   # mostly on VOID and the category's crowd: ignored
            continue
        stat[pred['category_id']].fp += 1


class _StatTable(dict):
    def __missing__(self, key):
        self[key] = _Stat()
        return self[key]


def pq_average(stat: Dict[int, _Stat], categories: Dict[int, Dict], isthing: Optional[bool]):
    """PQStat.pq_average (eval_vpq_vipseg.py:60-99)"""
    pq, sq, rq, n = 0, 0, 0, 0
    per_class = {}
    for label, info in categories.items():
        if isthing is not None and isthing != (info['isthing'] == 1):
            continue
        s = stat[label]
        if s.tp + s.fp + s.fn == 0:
            per_class[label] = {'pq': 0.0, 'sq': 0.0, 'rq': 0.0, 'iou': 0.0, 'tp': 0, 'fp': 0, 'fn': 0}
            continue
        n += 1
        pq_class = s.iou / (s.tp + 0.5 * s.fp + 0.5 * s.fn)
        sq_class = s.iou / s.tp if s.tp != 0 else 0
        rq_class = s.tp / (s.tp + 0.5 * s.fp + 0.5 * s.fn)
        per_class[label] = {'pq': pq_class, 'sq': sq_class, 'rq': rq_class, 'iou': s.iou, 'tp': s.tp, 'fp': s.fp, 'fn': s.fn}
        pq += pq_class
        sq += sq_class
        rq += rq_class
    return {'pq': pq / n, 'sq': sq / n, 'rq': rq / n, 'n': n}, per_class


def vpq_text(results: Dict) -> str:
    """the text of vpq-<k>.txt (eval_vpq_vipseg.py:286-299)"""
    lines = ['================================================\n',
             '{:10s}| {:>5s}  {:>5s}  {:>5s} {:>5s}'.format('', 'PQ', 'SQ', 'RQ', 'N\n'),
             '-' * (10 + 7 * 4) + '\n']
    for name in ('All', 'Things', 'Stuff'):
        r = results[name]
        lines.append('{:10s}| {:5.1f}  {:5.1f}  {:5.1f} {:5d}\n'.format(name, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'], r['n']))
    lines.append('{:4s}| {:>5s} {:>5s} {:>5s} {:>6s} {:>7s} {:>7s} {:>7s}\n'.format('IDX', 'PQ', 'SQ', 'RQ', 'IoU', 'TP', 'FP', 'FN'))
    for idx, r in results['per_class'].items():
        lines.append('{:4d} | {:5.1f} {:5.1f} {:5.1f} {:6.1f} {:7d} {:7d} {:7d}\n'.format(
            idx, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'], r['iou'], r['tp'], r['fp'], r['fn']))
    return ''.join(lines)


# ------------------------------------------------------------------------------------------ one frame of the scorer
def _upload(a: np.ndarray, device: torch.device) -> torch.Tensor:
    """a small host table to the device without waiting for the stream: through pinned memory"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if device.type != 'cuda':
        return t
    if t.numel() == 0:
        return torch.empty(0, dtype=t.dtype, device=device)
    return t.pin_memory().to(device, non_blocking=True)


def _pinned_copy(counts: torch.Tensor):
    """-> (host, event): a device tensor on its way into pinned memory and the event that says it has arrived (a host
    tensor is there already: itself and None)"""
    if not counts.is_cuda:
        return counts, None
    host = torch.empty(counts.shape, dtype=counts.dtype, pin_memory=True)
    host.copy_(counts, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    return host, event


def _as_plane(x, device: torch.device, gt: bool) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        if x.ndim == 2 and x.dtype != np.int32 and (gt or x.dtype != np.int64):
            x = x.astype(np.int32 if gt else np.int64)
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise TypeError(f'a plane must be a tensor or an array (got {type(x).__name__})')
    if gt and x.dim() == 2 and x.dtype == torch.int64:
        x = x.to(torch.int32)
    return x if x.device == device else x.to(device)


class _Frame:
    """one frame in flight: the table's copy to the host, the keys of its rows and columns, and the two segment lists"""

    def __init__(self, host, event, gt_keys, pred_keys, gt_info, pred_info, pred_plane, pred_ids_of_plane):
        self.host, self.event = host, event
        self.gt_keys, self.pred_keys = gt_keys, pred_keys
        self.gt_info, self.pred_info = gt_info, pred_info
        self.pred_plane, self.pred_ids_of_plane = pred_plane, pred_ids_of_plane
        self.pairs = self.cells = self.gt_segms = self.pred_segms = None

    def ready(self) -> bool:
        return self.event is None or self.event.query()

    def finish(self, categories) -> None:
        """wait for the table; key it back to ids; the prediction's sanity checks of eval_vpq_vipseg.py:146-163"""
        if self.pairs is not None:
            return
        if self.event is not None:
            self.event.synchronize()
        counts = self.host.numpy().astype(np.int64)
        g, p = np.nonzero(counts)
        self.cells = [(self.gt_keys[a], self.pred_keys[b], int(counts[a, b])) for a, b in zip(g.tolist(), p.tolist())]
        self.pairs = {(a, b): n for a, b, n in self.cells}
        self.gt_segms = _merge_segments(self.gt_info)
        self.pred_segms = _merge_segments(self.pred_info)
        area = {}
        for (_, b), n in self.pairs.items():
            area[b] = area.get(b, 0) + n
        unlisted = self._unlisted_ids() if area.get(OTHER, 0) > 0 else []
        in_png = sorted([b for b in area if b not in (OTHER, VOID) or (b == VOID and VOID in self.pred_segms)] + unlisted)
        missing = set(el['id'] for el in self.pred_info)
        for label in in_png:
            if label not in self.pred_segms:
                raise KeyError('Segment with ID {} is presented in PNG and not presented in JSON.'.format(label))
            self.pred_segms[label]['area'] = area[label]
            missing.discard(label)
            if self.pred_segms[label]['category_id'] not in categories:
                raise KeyError('Segment with ID {} has unknown category_id {}.'.format(label, self.pred_segms[label]['category_id']))
        if missing:
            raise KeyError('The following segment IDs {} are presented in JSON and not presented in PNG.'.format(list(missing)))
        self.pred_plane = self.pred_ids_of_plane = None

    def _unlisted_ids(self) -> List[int]:
        """the ids of the predicted plane that its JSON does not list: a host pass over the plane, only made to name
        the offender of an error"""
        plane = self.pred_plane
        if plane is None:
            return [OTHER]
        a = plane.cpu().numpy()
        if self.pred_ids_of_plane is not None:
            ids = np.unique(np.asarray(self.pred_ids_of_plane, dtype=np.int64)[np.unique(a.astype(np.int64))])
        else:
            ids = np.unique(rgb_to_id(a) if a.ndim == 3 else a.astype(np.int64))
        return [int(i) for i in ids if i != VOID and int(i) not in self.pred_segms]


# ------------------------------------------------------------------------------------------ STQ
class _Sequence:
    def __init__(self, size: int):
        self.confusion = np.zeros((size, size), dtype=np.int64)
        self.predictions, self.ground_truth, self.intersections = {}, {}, {}
        self.length = 0


def _first_seen(frames_info) -> Dict[int, int]:
    """instance numbers in order of first appearance in the video's JSONs (eval_stq_vipseg.py:103-121)"""
    out = {}
    for info in frames_info:
        for seg in info:
            out.setdefault(seg['id'], len(out))
    return out


def _bump(table: Dict[int, int], fresh: Dict[int, int]) -> None:
    for key in sorted(fresh):      # (_update_dict_stats: np.unique's ascending order decides the insertion order)
        table[key] = table.get(key, 0) + fresh[key]


# ------------------------------------------------------------------------------------------ the scorer
class VideoPanopticScorer:
    """VPQ and STQ of a run, fed frame by frame.

    `add_frame` only launches the joint count on the caller's stream and starts one copy of the table into pinned
    memory; it does not synchronise.  `end_video` waits for the video's tables and does the host arithmetic.
    `categories` is the `categories` list of the ground-truth JSON (dicts with id and isthing)."""

    def __init__(self, categories, windows: Sequence[int] = (1, 2, 4, 6, 8, 10, 999), num_classes: int = 124,
                 ignore_label: int = 255, bit_shift: int = 16):
        cats = categories.values() if isinstance(categories, dict) else categories
        self.categories = {el['id']: el for el in cats}
        self.things = [el['id'] for el in cats if el['isthing']]
        self.windows = tuple(int(k) for k in windows)
        self.num_classes, self.ignore_label, self.bit_shift = int(num_classes), int(ignore_label), int(bit_shift)
        self.offset = 2**24
        if self.offset < self.num_classes << self.bit_shift:
            raise ValueError('num_classes << bit_shift must stay below 2^24')
        self.size = self.num_classes + 1 if self.ignore_label >= self.num_classes else self.num_classes
        self.include = (np.arange(self.num_classes) if self.ignore_label >= self.num_classes else
                        np.array([i for i in range(self.num_classes) if i != self.ignore_label]))
        self.vpq_total = {k: _StatTable() for k in self.windows}
        self.sequences: List[_Sequence] = []
        self.video_ids: List = []
        self._frames: Optional[List[_Frame]] = None
        self._known_gt = set()

    # ---------------------------------------------------------------- feeding
    def start_video(self, video_id, gt_ids: Optional[Iterable[int]] = None) -> None:
        """`gt_ids`: ground-truth ids to list from the first frame on (the ids of the video's JSON).  Without them a
        frame's table lists the ids of the ground-truth JSONs seen so far, and an id that a PNG holds before any JSON
        lists it counts as unlisted in that frame (the reference, which sees the whole tube, would count it)."""
        if self._frames is not None:
            raise RuntimeError('end_video() the previous video first')
        self._frames = []
        self._video_id = video_id
        self._known_gt = set(int(i) for i in (gt_ids or ()) if int(i) != 0)

    def add_frame(self, pred, pred_segments_info: Sequence[Dict], gt, gt_segments_info: Sequence[Dict]) -> None:
        """`gt`: uint8 [H,W,3] or int32 [H,W]; `pred`: those, int64 [H,W], or the fast form: a `FrameResult` (or any
        object with `index` and `channel_ids`, or the pair itself): the int16 channel plane and the id of each channel"""
        if self._frames is None:
            raise RuntimeError('start_video() first')
        for fr in self._frames:                       # release what has arrived (no waiting)
            if fr.pairs is None and fr.ready():
                fr.finish(self.categories)
        channel_ids = None
        if isinstance(pred, tuple):
            pred, channel_ids = pred
        elif hasattr(pred, 'index') and hasattr(pred, 'channel_ids') and not isinstance(pred, (torch.Tensor, np.ndarray)):
            pred, channel_ids = pred.index, pred.channel_ids
        device = next((t.device for t in (pred, gt) if isinstance(t, torch.Tensor)),
                      torch.device('cuda' if torch.cuda.is_available() else 'cpu'))
        gt, pred = _as_plane(gt, device, True), _as_plane(pred, device, False)
        self._known_gt.update(int(s['id']) for s in gt_segments_info if int(s['id']) != 0)
        gt_table = metrics.id_table(self._known_gt, 'ground-truth ids')
        pred_table = metrics.id_table([s['id'] for s in pred_segments_info], 'predicted ids')
        lut = None
        if channel_ids is not None:
            channel_ids = np.asarray(channel_ids, dtype=np.int64).reshape(-1)
            at = np.clip(np.searchsorted(pred_table, channel_ids), 0, max(pred_table.size - 1, 0))
            listed = (pred_table[at] == channel_ids) if pred_table.size else np.zeros(channel_ids.size, dtype=bool)
            lut = np.where(channel_ids == 0, 0, np.where(listed, at + 2, 1)).astype(np.uint16)
            counts = metrics.panoptic_counts(gt, _upload(gt_table, device), pred, int(pred_table.size), _upload(lut, device),
                                             validate=False)
        else:
            counts = metrics.panoptic_counts(gt, _upload(gt_table, device), pred, _upload(pred_table, device), validate=False)
        host, event = _pinned_copy(counts)
        self._frames.append(_Frame(host, event, [VOID, OTHER] + gt_table.tolist(), [VOID, OTHER] + pred_table.tolist(),
                                   [dict(s) for s in gt_segments_info], [dict(s) for s in pred_segments_info], pred, channel_ids))

    # ---------------------------------------------------------------- host arithmetic
    def end_video(self) -> None:
        frames, self._frames = self._frames, None
        if frames is None:
            raise RuntimeError('start_video() first')
        for fr in frames:
            fr.finish(self.categories)
        for k in self.windows:     # eval_vpq_vipseg.py:118: the tubes of k frames, one for a shorter video
            video = _StatTable()
            for idx in range(0, max(len(frames) - k + 1, 1)):
                _vpq_tube(frames[idx:idx + k], video)
            total = self.vpq_total[k]
            for label, s in video.items():     # (PQStat.__iadd__: the video's sums are added to the totals)
                t = total[label]
                t.iou += s.iou
                t.tp += s.tp
                t.fp += s.fp
                t.fn += s.fn
        self._stq_video(frames)
        self.video_ids.append(self._video_id)

    def _stq_video(self, frames: List[_Frame]) -> None:
        seq = _Sequence(self.size)
        gt_number = _first_seen(fr.gt_info for fr in frames)
        pred_number = _first_seen(fr.pred_info for fr in frames)
        things = set(self.things)
        for fr in frames:
            # eval_stq_vipseg.py:130-148: semantic and instance of every listed id (a repeated id: the last entry), 255 else
            gt_label = {el['id']: (el['category_id'], gt_number[el['id']]) for el in fr.gt_info}
            pred_label = {el['id']: (el['category_id'], pred_number[el['id']]) for el in fr.pred_info}
            preds, gts, inters = {}, {}, {}
            for a, b, n in fr.cells:
                sem_g, ins_g = gt_label.get(a, (255, 255))
                sem_p, ins_p = pred_label.get(b, (255, 255))
                y_true = (sem_g << self.bit_shift) + ins_g
                y_pred = (sem_p << self.bit_shift) + ins_p
                sem_g, sem_p = y_true >> self.bit_shift, y_pred >> self.bit_shift
                row = self.num_classes if (self.ignore_label > self.num_classes and sem_g == self.ignore_label) else sem_g
                col = self.num_classes if (self.ignore_label > self.num_classes and sem_p == self.ignore_label) else sem_p
                seq.confusion[row, col] += n
                # segmentation_and_tracking_quality.py:164-195: things only; a thing with instance number 0 (the video's
                # first-listed id) is the reference's "crowd" and is left out on both sides
                g_thing, p_thing = sem_g in things, sem_p in things
                crowd = g_thing and (y_true & ((1 << self.bit_shift) - 1)) == 0
                g_mask, p_mask = g_thing and not crowd, p_thing and not crowd
                if p_mask:
                    preds[y_pred] = preds.get(y_pred, 0) + n
                if g_mask:
                    gts[y_true] = gts.get(y_true, 0) + n
                if g_mask and p_mask:
                    key = y_true * self.offset + y_pred
                    inters[key] = inters.get(key, 0) + n
            _bump(seq.predictions, preds)
            _bump(seq.ground_truth, gts)
            _bump(seq.intersections, inters)
            seq.length += 1
        self.sequences.append(seq)

    def stq(self) -> Dict:
        """STQuality.result (segmentation_and_tracking_quality.py:197-291)"""
        eps = 1e-15
        n = len(self.sequences)
        tubes, aq_per_seq, iou_per_seq = [0] * n, [0] * n, [0] * n
        for index, seq in enumerate(self.sequences):
            outer = 0.0
            tubes[index] = len(seq.ground_truth)
            for gt_id, gt_size in seq.ground_truth.items():
                inner = 0.0
                for pr_id, pr_size in seq.predictions.items():
                    tpa = seq.intersections.get(self.offset * gt_id + pr_id)
                    if tpa is not None:
                        inner += tpa * (tpa / (tpa + (pr_size - tpa) + (gt_size - tpa)))
                outer += 1.0 / gt_size * inner
            aq_per_seq[index] = outer
        aq_mean = np.sum(aq_per_seq) / np.maximum(np.sum(tubes), eps)
        aq_per_seq = aq_per_seq / np.maximum(tubes, eps)
        total = np.zeros((self.size, self.size), dtype=np.int64)
        keep = np.zeros((self.size, 1), dtype=np.int64)
        keep[self.include] = 1      # the ignore row is removed
        with np.errstate(invalid='ignore', divide='ignore'):
            for index, seq in enumerate(self.sequences):
                confusion = seq.confusion * keep
                total += confusion
                inter = confusion.diagonal()
                unions = inter + (confusion.sum(axis=0) - inter) + (confusion.sum(axis=1) - inter)
                iou_per_seq[index] = np.sum(inter.astype(np.double) / np.maximum(unions, 1e-15).astype(np.double)) / \
                    np.count_nonzero(unions)
            inter = total.diagonal()
            unions = inter + (total.sum(axis=0) - inter) + (total.sum(axis=1) - inter)
            iou_mean = np.sum(inter.astype(np.double) / np.maximum(unions, eps).astype(np.double)) / np.count_nonzero(unions)
            return {'STQ': np.sqrt(aq_mean * iou_mean), 'AQ': aq_mean, 'IoU': float(iou_mean),
                    'STQ_per_seq': np.sqrt(aq_per_seq * iou_per_seq), 'AQ_per_seq': aq_per_seq, 'IoU_per_seq': iou_per_seq,
                    'ID_per_seq': list(range(n)), 'Length_per_seq': [seq.length for seq in self.sequences],
                    'confusion': total}

    # ---------------------------------------------------------------- results
    def vpq(self, k: int) -> Dict:
        """vpq_compute's `results` for window k: All / Things / Stuff and per_class"""
        stat = self.vpq_total[k]
        out = {}
        for name, isthing in (('All', None), ('Things', True), ('Stuff', False)):
            out[name], per_class = pq_average(stat, self.categories, isthing)
            if name == 'All':
                out['per_class'] = per_class
        return out

    def result(self) -> Dict:
        """{'vpq': {k: All / Things / Stuff / per_class (iou, tp, fp, fn, pq, sq, rq per class)}, 'vpq_simple': the
        (all, thing, stuff) percentages per window, 'stq': the STQ dict, 'videos': the ids in order}"""
        vpq = {k: self.vpq(k) for k in self.windows}
        simple = [tuple(100 * vpq[k][name]['pq'] for name in ('All', 'Things', 'Stuff')) for k in self.windows]
        return {'vpq': vpq, 'vpq_simple': simple, 'stq': self.stq(), 'videos': list(self.video_ids)}

    def texts(self) -> Dict[str, str]:
        """file name -> text of vpq-<k>.txt, vpq-simple.txt and stq.txt in the reference's formats"""
        res = self.result()
        out = {'vpq-%d.txt' % k: vpq_text(res['vpq'][k]) for k in self.windows}
        out['vpq-simple.txt'] = ''.join(f'{a:.1f}/{t:.1f}/{s:.1f},' for a, t, s in res['vpq_simple'])
        stq = res['stq']
        out['stq.txt'] = f'{stq["STQ"]*100:.1f},{stq["AQ"]*100:.1f},{stq["IoU"]*100:.1f}\n'
        return out

    def write(self, output_dir: str) -> None:
        os.makedirs(output_dir, exist_ok=True)
        for name, text in self.texts().items():
            with open(path.join(output_dir, name), 'w') as f:
                f.write(text)


def score_directory(submit_dir: str, truth_dir: str, pan_gt_json_file: str, *, write: bool = True,
                    scorer: Optional[VideoPanopticScorer] = None) -> Dict:
    """eval_vpq + eval_stq of a finished run (eval_vpq_vipseg.py:331-396, eval_stq_vipseg.py:50-168): the PNGs of
    `submit_dir`/pan_pred and `truth_dir` are read once each, uploaded as they are and counted on the device; the text
    files go to `submit_dir`.  -> `VideoPanopticScorer.result()`"""
    from PIL import Image
    with open(path.join(submit_dir, 'pred.json')) as f:
        pred_j = {v['video_id']: v['annotations'] for v in json.load(f)['annotations']}
    with open(pan_gt_json_file) as f:
        gt_jsons = json.load(f)
    gt_j = {v['video_id']: v['annotations'] for v in gt_jsons['annotations']}
    scorer = scorer or VideoPanopticScorer(gt_jsons['categories'])
    for video in gt_jsons['videos']:
        video_id = video['video_id']
        gt_js, pred_js = gt_j[video_id], pred_j[video_id]
        assert len(gt_js) == len(pred_js)
        scorer.start_video(video_id, gt_ids=[s['id'] for ann in gt_js for s in ann['segments_info']])
        for gt_json, pred_json, image in zip(gt_js, pred_js, video['images']):
            name = image['file_name']
            pred = np.array(Image.open(path.join(submit_dir, 'pan_pred', video_id, name)))
            gt = np.array(Image.open(path.join(truth_dir, video_id, name)))
            scorer.add_frame(pred, pred_json['segments_info'], gt, gt_json['segments_info'])
        scorer.end_video()
    if write:
        scorer.write(submit_dir)
    return scorer.result()
