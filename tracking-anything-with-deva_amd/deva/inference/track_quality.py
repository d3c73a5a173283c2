"""Scoring a BURST-format run on the device (`eval_with_detections.py --dataset burst` of the reference, then its
scripts/merge_burst_json.py, then the benchmark's HOTA / OWTA): the tracker's masks and the ground truth are both COCO
run lengths, and the per-frame table of mask IoUs between them is one call of `deva.hip.rle.intersections` (two launches
over the run lengths, rules O1-O9 of include/deva_rle_overlap.h; no mask is decoded).  The rest is host arithmetic in
fp64 over a G x P table per frame.

Rules of the measures as implemented here, written from the published definition of HOTA (Luiten et al., IJCV 2021) and
of OWTA (Liu et al., CVPR 2022); neither TrackEval nor pycocotools is part of this repository and tests/track_case.py
restates the rules from scratch.  alpha runs over 0.05, 0.10, ..., 0.95; eps is the fp64 machine epsilon.
  T1  frames pair by index: frame t of the prediction belongs to frame t of the ground truth.  A sequence whose two sides
      differ in length is an error that names the sequence.  sim_t[g][p] is the mask IoU inter / (a_g + a_p - inter) of
      ground-truth track g and predicted track p on frame t, 0 where inter is 0.
  T2  gt_id_count[g] and tracker_id_count[p]: the frames on which the track occurs (an entry of the frame's dict; an
      empty mask still occurs).
  T3  potential_matches_count[g][p] is the sum over frames of the normalised similarity
      sim / (row sum + column sum - sim), taken as 0 where that denominator is not above eps.
  T4  the global alignment score is A[g][p] = pmc / (gt_id_count[g] + tracker_id_count[p] - pmc).
  T5  per frame ONE maximum-weight assignment on A * sim_t (`assign_pairs`: every track of the smaller side gets a
      partner).  Among equal optima any one is taken.
  T6  for each alpha the assigned pairs with sim_t >= alpha - eps are the matches of the frame: TP += their number,
      FN += G_t - that, FP += P_t - that, the LocA sum += their sim_t, matches_count[alpha][g][p] += 1.  A frame with no
      ground truth counts FP = P_t only, one with no prediction FN = G_t only, for every alpha.
  T7  per alpha, with mc = matches_count[alpha]:
      AssA = sum(mc * mc / max(1, gt_id_count + tracker_id_count - mc)) / max(1, TP); AssRe and AssPr likewise with
      max(1, gt_id_count) and max(1, tracker_id_count); LocA = max(1e-10, LocA sum) / max(1e-10, TP);
      DetA = TP / max(1, TP + FN + FP); DetRe = TP / max(1, TP + FN); DetPr = TP / max(1, TP + FP);
      HOTA = sqrt(DetA * AssA); OWTA = sqrt(DetRe * AssA).  The reported number of each is its mean over alpha.
  T8  over several sequences TP, FN and FP add up; AssA, AssRe, AssPr and LocA are the sequences' values weighted by
      their TP (divided by max(1, sum of TP); LocA by max(1e-10, .)); the rest follows as in T7.
  T9  `groups={'common': ids, ...}`: a group scores the ground-truth tracks whose `track_category_ids` entry is in its
      ids against EVERY predicted track.  This is this project's rule and not TrackEval's preprocessing (which also
      removes predictions matched to tracks outside the group): a tracker is charged FP for what it finds of the other
      groups' objects.  OWTA, which does not read FP, is unaffected by that.

  assign_pairs               T5 on a rectangular table, on `unsup_quality.assign` (numpy only, no scipy)
  TrackQualityScorer         fed frame by frame without synchronising; the tables of a video are copied at `end_video`
  score_burst_json           the scorer fed from two BURST-format files
  merge_burst_predictions    the reference's scripts/merge_burst_json.py: per-sequence pred.json files into one file
"""
import copy
import json
from os import path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from deva.hip import rle
from deva.hip.rle_overlap import iou_from_counts
from deva.inference.unsup_quality import assign

ALPHAS = np.arange(0.05, 0.99, 0.05)
EPS = float(np.finfo(np.float64).eps)
COUNT_FIELDS = ('HOTA_TP', 'HOTA_FN', 'HOTA_FP')
WEIGHTED_FIELDS = ('AssA', 'AssRe', 'AssPr', 'LocA')
FIELDS = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA', 'OWTA')


# ------------------------------------------------------------------------------------------ T5: the assignment
def assign_pairs(score) -> Tuple[List[int], List[int]]:
    """score: float64 [G, P], finite -> (rows, cols) of min(G, P) pairs, every row and column at most once, with the
    largest total score; the rows ascend.  `unsup_quality.assign` on the table or its transpose, whichever has its
    longer side first (that is the padding a rectangular table needs)."""
    s = np.asarray(score, dtype=np.float64)
    n_g, n_p = s.shape
    if n_g == 0 or n_p == 0:
        return [], []
    if n_p >= n_g:
        cols = assign(s.T)                       # for each g its p
        return list(range(n_g)), [int(c) for c in cols]
    rows = assign(s)                             # for each p its g
    order = np.argsort(rows)
    return [int(rows[k]) for k in order], [int(k) for k in order]


# ------------------------------------------------------------------------------------------ T2-T7: one sequence
Frame = Tuple[Sequence, Sequence, np.ndarray]    # (gt ids, predicted ids, sim float64 [G, P])


def sequence_counts(frames: Iterable[Frame]) -> Dict:
    """T2-T6 and the per-sequence part of T7 -> {'HOTA_TP', 'HOTA_FN', 'HOTA_FP' int64 [19]; 'AssA', 'AssRe', 'AssPr',
    'LocA' float64 [19]; 'gt_tracks', 'pred_tracks', 'gt_dets', 'pred_dets', 'frames'}"""
    frames = [(list(g), list(p), np.asarray(s, dtype=np.float64).reshape(len(g), len(p))) for g, p, s in frames]
    gt_index, pr_index = {}, {}
    for gt_ids, pr_ids, _ in frames:
        for i in gt_ids:
            gt_index.setdefault(i, len(gt_index))
        for i in pr_ids:
            pr_index.setdefault(i, len(pr_index))
    n_g, n_p, n_a = len(gt_index), len(pr_index), len(ALPHAS)
    gt_count, pr_count = np.zeros((n_g, 1)), np.zeros((1, n_p))
    potential = np.zeros((n_g, n_p))
    rows_cols = []
    for gt_ids, pr_ids, sim in frames:                                   # T2, T3
        r = np.array([gt_index[i] for i in gt_ids], dtype=np.int64)
        c = np.array([pr_index[i] for i in pr_ids], dtype=np.int64)
        rows_cols.append((r, c))
        gt_count[r, 0] += 1
        pr_count[0, c] += 1
        if r.size and c.size:
            denom = sim.sum(axis=0, keepdims=True) + sim.sum(axis=1, keepdims=True) - sim
            share = np.zeros_like(sim)
            np.divide(sim, denom, out=share, where=denom > 0 + EPS)
            potential[r[:, None], c[None, :]] += share
    alignment = potential / (gt_count + pr_count - potential) if n_g and n_p else potential   # T4 (a track occurs at least once)
    tp, fn, fp = (np.zeros(n_a, dtype=np.int64) for _ in range(3))
    loc = np.zeros(n_a)
    matches = np.zeros((n_a, n_g, n_p))
    for (gt_ids, pr_ids, sim), (r, c) in zip(frames, rows_cols):         # T5, T6
        if not r.size:
            fp += c.size
            continue
        if not c.size:
            fn += r.size
            continue
        rows, cols = assign_pairs(alignment[r[:, None], c[None, :]] * sim)
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        paired = sim[rows, cols]
        for a, alpha in enumerate(ALPHAS):
            hit = paired >= alpha - EPS
            n = int(hit.sum())
            tp[a] += n
            fn[a] += r.size - n
            fp[a] += c.size - n
            if n:
                loc[a] += paired[hit].sum()
                matches[a, r[rows[hit]], c[cols[hit]]] += 1
    out = {'HOTA_TP': tp, 'HOTA_FN': fn, 'HOTA_FP': fp}
    top = np.maximum(1, tp)
    out['AssA'] = (matches * matches / np.maximum(1, gt_count + pr_count - matches)).sum(axis=(1, 2)) / top          # T7
    out['AssRe'] = (matches * matches / np.maximum(1, gt_count)).sum(axis=(1, 2)) / top
    out['AssPr'] = (matches * matches / np.maximum(1, pr_count)).sum(axis=(1, 2)) / top
    out['LocA'] = np.maximum(1e-10, loc) / np.maximum(1e-10, tp)
    out.update(gt_tracks=n_g, pred_tracks=n_p, gt_dets=int(gt_count.sum()), pred_dets=int(pr_count.sum()), frames=len(frames))
    return out


def combine(records: Sequence[Dict]) -> Dict:
    """T8 -> a record of the same fields"""
    n_a = len(ALPHAS)
    out = {f: np.zeros(n_a, dtype=np.int64) for f in COUNT_FIELDS}
    for f in COUNT_FIELDS:
        for rec in records:
            out[f] = out[f] + rec[f]
    for f in WEIGHTED_FIELDS:
        total = np.zeros(n_a)
        for rec in records:
            total = total + rec[f] * rec['HOTA_TP']
        out[f] = np.maximum(1e-10, total) / np.maximum(1e-10, out['HOTA_TP']) if f == 'LocA' else total / np.maximum(1, out['HOTA_TP'])
    for f in ('gt_tracks', 'pred_tracks', 'gt_dets', 'pred_dets', 'frames'):
        out[f] = int(sum(rec[f] for rec in records))
    return out


def final_fields(record: Dict) -> Dict:
    """the rest of T7 -> the record with 'DetA', 'DetRe', 'DetPr', 'HOTA', 'OWTA' per alpha and, under 'summary', the
    mean over alpha of every field of `FIELDS`"""
    tp, fn, fp = (record[f].astype(np.float64) for f in COUNT_FIELDS)
    out = dict(record)
    out['DetRe'] = tp / np.maximum(1, tp + fn)
    out['DetPr'] = tp / np.maximum(1, tp + fp)
    out['DetA'] = tp / np.maximum(1, tp + fn + fp)
    out['HOTA'] = np.sqrt(out['DetA'] * out['AssA'])
    out['OWTA'] = np.sqrt(out['DetRe'] * out['AssA'])
    out['summary'] = {f: float(np.mean(out[f])) for f in FIELDS}
    return out


# ------------------------------------------------------------------------------------------ the scorer
class _Video:
    def __init__(self, name, categories):
        self.name, self.categories, self.frames = name, categories, []


class TrackQualityScorer:
    """HOTA and OWTA of a run, fed frame by frame:

        scorer.start_video(name, gt_categories)          # gt_categories: track id -> category id (T9), or None
        scorer.add_frame(pred_rles_by_track, gt_rles_by_track)
        scorer.end_video()
        scorer.result()

    `add_frame` takes two dicts, track id -> run-length mask (any form `rle.parse_counts` takes with its size, i.e. a dict
    {'size', 'counts'}), queues one `rle.intersections(pred, gt, pending=True)` on the current stream and returns without
    a wait; `end_video` finishes the video's tables (the first `finish()` waits, the others have landed by then) and does
    T2-T7.  `groups`: T9; without it there is the one group 'all'."""

    def __init__(self, groups: Optional[Dict[str, Iterable[int]]] = None, device=None):
        self.groups = None if groups is None else {str(k): {int(i) for i in v} for k, v in groups.items()}
        self.device = device
        self.videos: Dict[str, Dict[str, Dict]] = {}
        self._video = None

    def start_video(self, name: str, gt_categories: Optional[Dict] = None) -> None:
        if self._video is not None:
            raise ValueError(f'start_video({name!r}): video {self._video.name!r} has not been ended')
        if name in self.videos:
            raise ValueError(f'start_video({name!r}): the video has been scored already')
        if self.groups is not None and gt_categories is None:
            raise ValueError(f'start_video({name!r}): groups need the `track_category_ids` of the ground truth')
        self._video = _Video(name, None if gt_categories is None else {str(k): int(v) for k, v in gt_categories.items()})

    def add_frame(self, pred_rles_by_track: Dict, gt_rles_by_track: Dict) -> None:
        if self._video is None:
            raise ValueError('add_frame: no video has been started')
        pred_ids, gt_ids = [str(k) for k in pred_rles_by_track], [str(k) for k in gt_rles_by_track]
        pending = None
        if pred_ids and gt_ids:
            pending = rle.intersections(list(pred_rles_by_track.values()), list(gt_rles_by_track.values()), pending=True, device=self.device)
        self._video.frames.append((gt_ids, pred_ids, pending))

    def end_video(self) -> Dict[str, Dict]:
        video, self._video = self._video, None
        if video is None:
            raise ValueError('end_video: no video has been started')
        frames = []
        for gt_ids, pred_ids, pending in video.frames:
            if pending is None:
                sim = np.zeros((len(gt_ids), len(pred_ids)))
            else:
                inter, area_p, area_g = pending.finish()                     # [P, G]: the predictions are the detections
                sim = iou_from_counts(inter, area_p, area_g).T
            frames.append((gt_ids, pred_ids, sim))
        records = {}
        for group, ids in ([('all', None)] if self.groups is None else self.groups.items()):
            kept = []
            for gt_ids, pred_ids, sim in frames:                             # T9: rows of the group, every column
                rows = [k for k, i in enumerate(gt_ids) if ids is None or video.categories.get(i) in ids]
                kept.append(([gt_ids[k] for k in rows], pred_ids, sim[rows]))
            records[group] = sequence_counts(kept)
        self.videos[video.name] = records
        return {g: final_fields(r) for g, r in records.items()}

    def result(self) -> Dict[str, Dict]:
        """group -> the combined record (T8) with its 'summary' and, under 'sequences', every video's own"""
        if self._video is not None:
            raise ValueError(f'result: video {self._video.name!r} has not been ended')
        out = {}
        for group in (['all'] if self.groups is None else list(self.groups)):
            per_video = {name: recs[group] for name, recs in self.videos.items()}
            out[group] = final_fields(combine(list(per_video.values())))
            out[group]['sequences'] = {name: final_fields(rec) for name, rec in per_video.items()}
        return out


# ------------------------------------------------------------------------------------------ BURST files
def _load(source):
    if isinstance(source, dict):
        return source
    with open(source) as f:
        return json.load(f)


def _frame_masks(frame: Dict, size: List[int], what: str) -> Dict:
    out = {}
    for track, entry in frame.items():
        if not isinstance(entry, dict) or 'rle' not in entry:
            raise ValueError(f"{what}: track {track}: an entry {{'rle': counts}} expected")
        out[str(track)] = {'size': size, 'counts': entry['rle']}
    return out


def score_burst_json(pred_json, gt_json, groups: Optional[Dict[str, Iterable[int]]] = None, device=None) -> Dict[str, Dict]:
    """two BURST-format files (paths or the loaded dicts): {'sequences': [{'dataset', 'seq_name', 'height', 'width',
    'segmentations': [per frame {track id: {'rle': counts}}], 'track_category_ids': {track id: category}}]}, the
    prediction as `merge_burst_predictions` writes it -> `TrackQualityScorer.result()`.  Sequences pair by
    (dataset, seq_name), frames by index (T1); a sequence the prediction lacks is an error."""
    pred, gt = _load(pred_json), _load(gt_json)
    by_name = {(s['dataset'], s['seq_name']): s for s in pred['sequences']}
    scorer = TrackQualityScorer(groups, device=device)
    for seq in gt['sequences']:
        key = (seq['dataset'], seq['seq_name'])
        name = f'{key[0]}/{key[1]}'
        if key not in by_name:
            raise ValueError(f'score_burst_json: sequence {name}: the prediction does not hold it')
        theirs = by_name[key]['segmentations']
        if len(theirs) != len(seq['segmentations']):
            raise ValueError(f'score_burst_json: sequence {name}: {len(theirs)} predicted frames, {len(seq["segmentations"])} in the ground truth')
        size = [int(seq['height']), int(seq['width'])]
        scorer.start_video(name, seq.get('track_category_ids') if groups is not None else None)
        for t, (mine, truth) in enumerate(zip(theirs, seq['segmentations'])):
            scorer.add_frame(_frame_masks(mine, size, f'{name}: predicted frame {t}'), _frame_masks(truth, size, f'{name}: frame {t}'))
        scorer.end_video()
    return scorer.result()


def merge_burst_predictions(gt_json, pred_root: str, out: str) -> Dict:
    """what the reference's scripts/merge_burst_json.py writes: the ground-truth file with every sequence's
    'segmentations' replaced by the tracker's (per frame {id: {'rle': counts text}}, read from
    <pred_root>/<dataset>/<seq_name>/pred.json, the saver's `video_json`) and its 'track_category_ids' by {id: 0} for
    every predicted id; everything else of the file is kept.  Written with `json.dump`'s defaults, so the integer ids
    become the file's string keys.  -> the merged dict"""
    merged = copy.deepcopy(_load(gt_json))
    for seq in merged['sequences']:
        with open(path.join(pred_root, seq['dataset'], seq['seq_name'], 'pred.json')) as f:
            video = json.load(f)
        frames, categories = [], {}
        for frame in video['segmentations']:
            frames.append({s['id']: {'rle': s['rle']['counts']} for s in frame['segmentations']})
            for s in frame['segmentations']:
                categories[s['id']] = 0
        seq['segmentations'] = frames
        seq['track_category_ids'] = categories
    with open(out, 'w') as f:
        json.dump(merged, f)
    return merged
