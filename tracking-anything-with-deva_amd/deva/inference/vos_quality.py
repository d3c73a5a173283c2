"""Scoring a DAVIS-style run on the device (not part of the reference's interface, as panoptic_quality.py is not): region
similarity J, boundary accuracy F and J&F, the measures of `eval_vos.py` on D16 / D17, `eval_with_detections.py
--dataset unsup_davis17`, `eval_saliency.py` and `eval_ref_davis.py` (the reference's docs/EVALUATION.md).

The public toolkits make one boolean plane per object and frame, take its boundary map and dilate it with a disk, all
on the host.  Everything J and F need from a frame is seven integers per object; `deva.hip.vos_metrics.boundary_counts`
makes them for all objects in two launches over planes that are already on the device, and what remains is host
arithmetic over a few integers per frame (rule R6 of include/deva_vos_metrics.h; the rules were written from the
toolkits' published behaviour, neither toolkit is part of this repository):

  jf_from_counts       J and F of every record
  sequence_statistics  mean, recall and decay of one object's values over its frames
  VideoObjectScorer    fed frame by frame, e.g. from `FrameResultSaver(frame_hook=...)`
  score_directory      the same scorer fed from two PNG trees: a finished run against its annotations

The unsupervised protocol's assignment of the tracker's own ids to objects is `unsup_quality.py`, built on this module.
"""
import os
import warnings
from os import path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from deva.hip import vos_metrics
from deva.inference.panoptic_quality import _pinned_copy, _upload

GLOBAL_HEADER = ['J&F-Mean', 'J-Mean', 'J-Recall', 'J-Decay', 'F-Mean', 'F-Recall', 'F-Decay']
SEQUENCE_HEADER = ['Sequence', 'J-Mean', 'F-Mean']


# ------------------------------------------------------------------------------------------ R6
def jf_from_counts(records) -> Tuple[np.ndarray, np.ndarray]:
    """records: integer [..., 8] (R5) -> (J, F), float64 [...]"""
    r = np.asarray(records).astype(np.int64)
    inter, a_gt, a_pred, n_gt, n_pred, gt_match, pred_match = (r[..., k] for k in range(7))
    union = a_gt + a_pred - inter
    j = np.where(union == 0, 1.0, inter / np.maximum(union, 1))
    precision = np.where(n_pred == 0, 1.0, pred_match / np.maximum(n_pred, 1))
    recall = np.where(n_gt == 0, 1.0, gt_match / np.maximum(n_gt, 1))
    precision = np.where((n_pred > 0) & (n_gt == 0), 0.0, precision)    # a predicted boundary where there is none
    recall = np.where((n_pred == 0) & (n_gt > 0), 0.0, recall)          # no predicted boundary where there is one
    total = precision + recall
    f = np.where(total == 0, 0.0, 2 * precision * recall / np.where(total == 0, 1.0, total))
    return j, f


def sequence_statistics(values) -> Tuple[float, float, float]:
    """(mean M, recall O, decay D) of one object's per-frame values.  The bin edges of the decay are cast to uint8 as the
    toolkits cast them, so they wrap beyond 255 frames: reproduced, not repaired."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)      # (the mean of an empty or all-NaN slice is NaN)
        m = np.nanmean(v)
        o = np.nanmean(v > 0.5)
        ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.uint8)
        bins = [v[int(ids[k]):int(ids[k + 1]) + 1] for k in range(4)]
        d = np.nanmean(bins[0]) - np.nanmean(bins[3])
    return float(m), float(o), float(d)


# ------------------------------------------------------------------------------------------ the scorer
def _as_plane(x, device: torch.device, gt: bool) -> torch.Tensor:
    allowed = (np.uint8, np.int32) if gt else (np.uint8, np.int32, np.int64)
    if isinstance(x, np.ndarray):
        if x.ndim != 2:
            raise ValueError(f'a plane must be [H,W] (got {x.shape})')
        if x.dtype not in allowed:
            x = x.astype(np.int32 if gt else np.int64)
        return _upload(x, device)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f'a plane must be a tensor or an array (got {type(x).__name__})')
    if gt and x.dtype == torch.int64:
        x = x.to(torch.int32)
    return x if x.device == device else x.to(device)


class _Frame:
    """one frame in flight: the records' copy to the host"""

    def __init__(self, host: torch.Tensor, event):
        self.host, self.event = host, event

    def records(self) -> np.ndarray:
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        return self.host.numpy().astype(np.int64)


class VideoObjectScorer:
    """J, F and J&F of a run, fed frame by frame.

    `add_frame` only launches the counts on the caller's stream and starts one copy of the records into pinned memory; it
    does not synchronise.  `end_video` waits for the video's records and does the host arithmetic.  With `skip_ends`
    (the semi-supervised protocol) the first and the last frame of a video are counted but not scored."""

    def __init__(self, bound_th: float = 0.008, skip_ends: bool = True):
        self.bound_th, self.skip_ends = float(bound_th), bool(skip_ends)
        self.videos: List[Dict] = []
        self._frames: Optional[List[_Frame]] = None
        self._scratch: Optional[torch.Tensor] = None

    # ---------------------------------------------------------------- feeding
    def start_video(self, name: str, object_ids: Iterable[int]) -> None:
        if self._frames is not None:
            raise RuntimeError('end_video() the previous video first')
        ids = vos_metrics.id_list(sorted(set(int(i) for i in object_ids)))
        self._name, self._ids, self._ids_dev = str(name), ids, None
        self._frames = []

    def add_frame(self, pred, gt, binary: bool = False) -> None:
        """`gt`: uint8 / int32 [H,W], device tensor or numpy.  `pred`: a `FrameResult` (or any object with `index` and
        `channel_ids`): the int16 channel plane with a table from channel to object built here, no search and 2 bytes a
        pixel; or a plane: uint8 / int32 / int64, device tensor or numpy (uploaded).  `binary`: both planes hold one
        object, every non-zero value (the video has one object id)."""
        if self._frames is None:
            raise RuntimeError('start_video() first')
        channel_ids = None
        if hasattr(pred, 'index') and hasattr(pred, 'channel_ids') and not isinstance(pred, (torch.Tensor, np.ndarray)):
            pred, channel_ids = pred.index, pred.channel_ids
            if pred is None or channel_ids is None:
                raise ValueError('the frame result carries no channel plane (launch_frame(index=True))')
        device = next((t.device for t in (pred, gt) if isinstance(t, torch.Tensor)),
                      torch.device('cuda' if torch.cuda.is_available() else 'cpu'))
        gt, pred = _as_plane(gt, device, True), _as_plane(pred, device, False)
        if self._ids_dev is None or self._ids_dev.device != device:
            self._ids_dev = _upload(self._ids, device)
        lut = None
        if channel_ids is not None:       # channel -> the index of its id among the video's objects, 65535 for none
            channel_ids = np.asarray(channel_ids, dtype=np.int64).reshape(-1)
            at = np.clip(np.searchsorted(self._ids, channel_ids), 0, self._ids.size - 1)
            lut = _upload(np.where(self._ids[at] == channel_ids, at, 65535).astype(np.uint16), device)
        need = 16 * gt.shape[0] * gt.shape[1]
        if device.type == 'cuda' and (self._scratch is None or self._scratch.device != device or self._scratch.numel() < need):
            self._scratch = torch.empty(need, dtype=torch.uint8, device=device)
        counts = vos_metrics.boundary_counts(gt, pred, self._ids_dev, bound_th=self.bound_th, pred_lut=lut, binary=bool(binary),
                                             scratch=self._scratch if device.type == 'cuda' else None, validate=False)
        self._frames.append(_Frame(*_pinned_copy(counts)))

    # ---------------------------------------------------------------- host arithmetic
    def end_video(self) -> None:
        frames, self._frames = self._frames, None
        if frames is None:
            raise RuntimeError('start_video() first')
        n = self._ids.size
        counts = np.stack([fr.records() for fr in frames]) if frames else np.zeros((0, n, vos_metrics.FIELDS), dtype=np.int64)
        scored = counts[1:-1] if self.skip_ends else counts
        j, f = jf_from_counts(scored)                      # [T', n]
        self.videos.append({'name': self._name, 'ids': self._ids.astype(np.int64).tolist(), 'counts': counts,
                            'J': j.T.copy(), 'F': f.T.copy(),
                            'J_stats': [sequence_statistics(j[:, k]) for k in range(n)],
                            'F_stats': [sequence_statistics(f[:, k]) for k in range(n)]})

    # ---------------------------------------------------------------- results
    def result(self) -> Dict:
        """{'global': the seven numbers by name, 'sequences': {'<sequence>_<k>': {'J-Mean', 'F-Mean'}} for the k-th
        object counted from 1, 'frames': {sequence: {'ids', 'counts' int64 [T,n,8] of every frame, 'J' and 'F' float64
        [n,T'] of the scored frames}}}"""
        j_stats = np.array([s for v in self.videos for s in v['J_stats']], dtype=np.float64).reshape(-1, 3)
        f_stats = np.array([s for v in self.videos for s in v['F_stats']], dtype=np.float64).reshape(-1, 3)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            jm, jr, jd = (float(x) for x in j_stats.mean(axis=0)) if len(j_stats) else (float('nan'),) * 3
            fm, fr, fd = (float(x) for x in f_stats.mean(axis=0)) if len(f_stats) else (float('nan'),) * 3
        table = dict(zip(GLOBAL_HEADER, [(jm + fm) / 2, jm, jr, jd, fm, fr, fd]))
        sequences = {}
        for v in self.videos:
            for k, (js, fs) in enumerate(zip(v['J_stats'], v['F_stats']), start=1):
                sequences[f'{v["name"]}_{k}'] = {'J-Mean': js[0], 'F-Mean': fs[0]}
        frames = {v['name']: {'ids': v['ids'], 'counts': v['counts'], 'J': v['J'], 'F': v['F']} for v in self.videos}
        return {'global': table, 'sequences': sequences, 'frames': frames}

    def texts(self) -> Dict[str, str]:
        """file name -> text of global_results.csv and per-sequence_results.csv (our format, after the public toolkit's)"""
        res = self.result()
        glob = ','.join(GLOBAL_HEADER) + '\n' + ','.join('%.3f' % res['global'][k] for k in GLOBAL_HEADER) + '\n'
        seq = ','.join(SEQUENCE_HEADER) + '\n' + ''.join(f'{name},{"%.3f" % s["J-Mean"]},{"%.3f" % s["F-Mean"]}\n'
                                                          for name, s in res['sequences'].items())
        return {'global_results.csv': glob, 'per-sequence_results.csv': seq}

    def write(self, output_dir: str) -> None:
        os.makedirs(output_dir, exist_ok=True)
        for name, text in self.texts().items():
            with open(path.join(output_dir, name), 'w') as f:
                f.write(text)


def score_directory(results_dir: str, annotations_dir: str, sequences: Optional[Sequence[str]] = None, *, binary: bool = False,
                    bound_th: float = 0.008, skip_ends: bool = True, scorer: Optional[VideoObjectScorer] = None) -> Dict:
    """a finished run against its annotations: one sub-folder per sequence in both trees, PNGs matched by name (palette
    or gray, read with PIL and uploaded as they are).  The objects of a sequence are 1 .. the largest id of its first
    annotation; with `binary` the single object is "non-zero".  -> `VideoObjectScorer.result()`"""
    from PIL import Image
    scorer = scorer or VideoObjectScorer(bound_th=bound_th, skip_ends=skip_ends)
    if sequences is None:
        sequences = sorted(d for d in os.listdir(annotations_dir) if path.isdir(path.join(annotations_dir, d)))
    for seq in sequences:
        names = sorted(f for f in os.listdir(path.join(annotations_dir, seq)) if f.endswith('.png'))
        if not names:
            raise FileNotFoundError(f'no annotation in {path.join(annotations_dir, seq)}')
        first = np.array(Image.open(path.join(annotations_dir, seq, names[0])))
        if not binary and int(first.max()) < 1:
            raise ValueError(f'{seq}: the first annotation holds no object')
        scorer.start_video(seq, [1] if binary else range(1, int(first.max()) + 1))
        for name in names:
            gt = first if name == names[0] else np.array(Image.open(path.join(annotations_dir, seq, name)))
            pred = np.array(Image.open(path.join(results_dir, seq, name)))
            if pred.shape != gt.shape:
                raise ValueError(f'{seq}/{name}: the prediction is {pred.shape} and the annotation {gt.shape}')
            scorer.add_frame(pred, gt, binary=binary)
        scorer.end_video()
    return scorer.result()
