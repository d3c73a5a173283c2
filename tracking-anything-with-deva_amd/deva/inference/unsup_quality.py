"""Scoring an unsupervised DAVIS run on the device (`eval_with_detections.py --dataset unsup_davis17` of the reference,
its docs/EVALUATION.md): the tracker invents its own ids, so J and F are taken for EVERY (proposal, ground-truth object)
pair on every frame, averaged over the video, and proposals are assigned to objects one to one so that the total J&F is
largest; only then come the statistics of `vos_quality`.  The pair table of a frame is one call of
`deva.hip.pair_metrics.pair_counts` (two launches, rules P1-P5 of include/deva_pair_metrics.h); the rest is host
arithmetic over a few integers per frame, with `jf_from_counts` and `sequence_statistics` of `vos_quality` unchanged.

Rules of the protocol as implemented here, written from the public toolkit's published behaviour (the toolkit is not
part of this repository; tests/unsup_case.py restates them from scratch):
  U1  at most `max_proposals` (20) distinct proposal ids may occur in a video; more raise ValueError (the toolkit exits).
  U2  with fewer proposals than objects, P < G, the proposals are padded with empty ones up to G.
  U3  every frame is scored unless `skip_ends` (the toolkit scores the unsupervised protocol on all frames).
  U4  score[p][g] = (mean_t J + mean_t F) / 2 with the conventions of R6 (include/deva_vos_metrics.h): an empty
      proposal against an absent object has J = F = 1, against a present one J = 0; then `assign`.
  U5  the statistics and the seven global numbers are those of `VideoObjectScorer`, over each object's assigned series;
      the CSV texts are the same.

  assign                   the assignment: maximum total score, O(n^3), numpy only
  UnsupervisedVideoScorer  fed frame by frame, e.g. from `FrameResultSaver(frame_hook=...)`
  ProposalLimiter          the reference's `postprocess_unsup_davis17.limit_max_id`, online from per-frame areas
  limit_directory          the same, offline, on a tree of PNGs
  score_directory          the scorer fed from two PNG trees
"""
import os
from os import path
from typing import Dict, Iterable, List, Optional, Sequence, Set

import numpy as np
import torch

from deva.hip import pair_metrics
from deva.inference.panoptic_quality import _pinned_copy, _upload
from deva.inference.vos_quality import VideoObjectScorer, _as_plane, _Frame, jf_from_counts, sequence_statistics


# ------------------------------------------------------------------------------------------ U4: the assignment
def assign(score) -> List[int]:
    """score: float64 [P, G] with P >= G -> for each g a distinct row p such that sum_g score[p_g][g] is maximal.

    The Hungarian method in its O(n^3) form with potentials (shortest augmenting paths over the G objects, one at a
    time), on cost = -score.  Among equal optima any one is returned: which of them is not specified."""
    s = np.asarray(score, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] < s.shape[1]:
        raise ValueError(f'assign: score must be [P, G] with P >= G (got {s.shape})')
    if not np.isfinite(s).all():
        raise ValueError('assign: score must be finite')
    n_p, n_g = s.shape
    cost = -s.T                                   # [G, P]: objects are the rows that get assigned
    u, v = np.zeros(n_g + 1), np.zeros(n_p + 1)
    owner = np.zeros(n_p + 1, dtype=np.int64)     # owner[p]: the object (1-based) that column p holds, 0 for none
    way = np.zeros(n_p + 1, dtype=np.int64)
    for g in range(1, n_g + 1):
        owner[0] = g
        j0 = 0
        least = np.full(n_p + 1, np.inf)
        used = np.zeros(n_p + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = owner[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]     # reduced costs of row i0
            free = ~used[1:]
            better = free & (cur < least[1:])
            least[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, least[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[owner[used]] += delta
            v[used] -= delta
            least[1:][free] -= delta
            j0 = j1
            if owner[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            owner[j0] = owner[j1]
            j0 = j1
    out = [-1] * n_g
    for p in range(1, n_p + 1):
        if owner[p]:
            out[owner[p] - 1] = p - 1
    return out


# ------------------------------------------------------------------------------------------ the limiter
class ProposalLimiter:
    """The reference's `deva/inference/postprocess_unsup_davis17.py:limit_max_id`, fed frame by frame with the areas of
    the frame's labels (`{s['id']: s['area'] for s in frame_result.segments}`) instead of re-reading PNGs.

    It follows the reference step for step, its quirk included: the labels of a frame (area > 0, label != 0) are
    appended to a list, sorted by (area, label) descending, WITHOUT checking whether they are listed already, until the
    list has `max_num_objects` entries; a label's new id is the position of its LAST occurrence + 1.  A video with five
    objects in every frame fills the list of 20 after four frames and never keeps a sixth.  `distinct=True` is a
    departure from the reference: only first occurrences are appended, which is what was evidently meant.

    The kept set after frame t is final for frame t (the list only grows), so a scorer can drop unlisted ids online; the
    final numbering (`mapping()`) is known once `full`."""

    def __init__(self, max_num_objects: int = 20, distinct: bool = False):
        self.max_num_objects, self.distinct = int(max_num_objects), bool(distinct)
        self.listed: List[int] = []

    @property
    def full(self) -> bool:
        return len(self.listed) >= self.max_num_objects

    def add_frame(self, areas: Dict[int, int]) -> Set[int]:
        """areas: {label: pixels in this frame} -> the labels kept so far"""
        if not self.full:
            labels = sorted(((int(a), int(k)) for k, a in areas.items() if int(k) != 0 and int(a) > 0), reverse=True)
            ordered = [k for _, k in labels]
            if self.distinct:
                ordered = [k for k in ordered if k not in self.listed]
            self.listed += ordered[:self.max_num_objects - len(self.listed)]
        return set(self.listed)

    def mapping(self) -> Dict[int, int]:
        """old label -> new id (1-based; the last occurrence in the list wins, as the reference's overwriting loop has it)"""
        return {label: at + 1 for at, label in enumerate(self.listed)}


def davis_palette() -> bytes:
    """the DAVIS / PASCAL VOC colour map, 256 x RGB: bit k of the label's index goes to bit 7 - k / 3 of channel k % 3"""
    out = bytearray()
    for i in range(256):
        rgb, c = [0, 0, 0], i
        for shift in range(7, -1, -1):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << shift
            c >>= 3
        out += bytes(rgb)
    return bytes(out)


def _read_labels(file: str) -> np.ndarray:
    """a palette / gray PNG as it is, an RGB-coded one as R * 65536 + G * 256 + B -> int32 [H,W]"""
    from PIL import Image
    mask = np.array(Image.open(file)).astype(np.int32)
    if mask.ndim == 3:
        mask = mask[:, :, 0] * 65536 + mask[:, :, 1] * 256 + mask[:, :, 2]
    return mask


def limit_directory(input_path: str, output_path: str, max_num_objects: int = 20, distinct: bool = False) -> Dict[str, Dict[int, int]]:
    """`limit_max_id` on a tree: one sub-folder per video, palette or RGB-coded PNGs in, palette PNGs with at most
    `max_num_objects` ids 1 .. out (`davis_palette`).  Every file is read once.  -> {video: old label -> new id}"""
    from PIL import Image
    palette = davis_palette()
    maps = {}
    for video in sorted(os.listdir(input_path)):
        frames = sorted(os.listdir(path.join(input_path, video)))
        limiter = ProposalLimiter(max_num_objects, distinct)
        masks = []
        for frame in frames:
            mask = _read_labels(path.join(input_path, video, frame))
            masks.append(mask)
            if not limiter.full:
                labels, areas = np.unique(mask, return_counts=True)
                limiter.add_frame(dict(zip(labels.tolist(), areas.tolist())))
        maps[video] = limiter.mapping()
        os.makedirs(path.join(output_path, video), exist_ok=True)
        for frame, mask in zip(frames, masks):
            new_mask = np.zeros(mask.shape, dtype=np.uint8)
            for label, new in maps[video].items():
                new_mask[mask == label] = new
            img = Image.fromarray(new_mask)
            img.putpalette(palette)
            img.save(path.join(output_path, video, frame))
    return maps


# ------------------------------------------------------------------------------------------ the scorer
class UnsupervisedVideoScorer(VideoObjectScorer):
    """J, F and J&F of an unsupervised run (rules U1-U5 of the module), fed frame by frame.

    `add_frame` launches the pair counts of the ids present in that frame on the caller's stream and starts the copies
    of the two tables into pinned memory.  With a `FrameResult` nothing synchronises: the table from channel to proposal
    is built on the host from `channel_ids`.  With a plane, the frame's proposal ids come from one `torch.unique` on the
    device, which synchronises (`add_frame(..., pred_ids=...)` with ids the caller knows avoids it; `score_directory`
    passes those of the host array it has just read).  `end_video` waits for the records, scatters them into [P, G, T]
    arrays -- a proposal absent from a frame has zero counts there -- assigns and does the host arithmetic."""

    def __init__(self, bound_th: float = 0.008, max_proposals: int = 20, skip_ends: bool = False):
        super().__init__(bound_th=bound_th, skip_ends=skip_ends)
        self.max_proposals = int(max_proposals)

    def start_video(self, name: str, gt_ids: Iterable[int]) -> None:
        if self._frames is not None:
            raise RuntimeError('end_video() the previous video first')
        ids = pair_metrics.id_list(sorted(set(int(i) for i in gt_ids)), 'gt_ids')
        self._name, self._ids, self._ids_dev = str(name), ids, None
        self._frames = []
        self._seen: Set[int] = set()

    def add_frame(self, pred, gt, pred_ids=None, keep: Optional[Set[int]] = None) -> None:
        """`gt`: uint8 / int32 [H,W], device tensor or numpy.  `pred`: a `FrameResult` (or any object with `index` and
        `channel_ids`), or a plane: uint8 / int32 / int64, device tensor or numpy (uploaded).  `pred_ids`: the ids in the
        plane, if the caller knows them.  `keep`: ids outside it are dropped (`ProposalLimiter.add_frame`'s set)."""
        if self._frames is None:
            raise RuntimeError('start_video() first')
        channel_ids = None
        if hasattr(pred, 'index') and hasattr(pred, 'channel_ids') and not isinstance(pred, (torch.Tensor, np.ndarray)):
            pred, channel_ids = pred.index, pred.channel_ids
            if pred is None or channel_ids is None:
                raise ValueError('the frame result carries no channel plane (launch_frame(index=True))')
        elif pred_ids is None and isinstance(pred, np.ndarray):
            pred_ids = np.unique(pred)
        device = next((t.device for t in (pred, gt) if isinstance(t, torch.Tensor)),
                      torch.device('cuda' if torch.cuda.is_available() else 'cpu'))
        gt, pred = _as_plane(gt, device, True), _as_plane(pred, device, False)
        if gt.shape != pred.shape:
            raise ValueError(f'gt is {tuple(gt.shape)} and pred {tuple(pred.shape)}')
        if channel_ids is not None:
            channel_ids = np.asarray(channel_ids, dtype=np.int64).reshape(-1)
            pred_ids = channel_ids
        elif pred_ids is None:
            pred_ids = torch.unique(pred).cpu().numpy()          # (synchronises)
        ids = np.unique(np.asarray(pred_ids, dtype=np.int64).reshape(-1))
        ids = ids[(ids >= 1) & (ids <= 2**31 - 1)]
        if keep is not None:
            ids = ids[np.isin(ids, sorted(keep))]
        self._seen.update(ids.tolist())
        if channel_ids is None and len(self._seen) > self.max_proposals:      # U1, as soon as it is known
            raise ValueError(f'{self._name}: more than {self.max_proposals} proposals ({len(self._seen)} ids so far)')
        if ids.size == 0:                    # nothing proposed in this frame: areas and boundaries of the objects alone
            ids = np.array([2**31 - 1], dtype=np.int64) if channel_ids is not None else self._unused_id(pred_ids)
            listed = np.zeros(0, dtype=np.int64)
        else:
            listed = ids
        if self._ids_dev is None or self._ids_dev.device != device:
            self._ids_dev = _upload(self._ids, device)
        lut = None
        if channel_ids is not None:       # channel -> the index of its id among the frame's proposals, 65535 for none
            at = np.clip(np.searchsorted(listed, channel_ids), 0, max(listed.size - 1, 0))
            hit = listed[at] == channel_ids if listed.size else np.zeros(channel_ids.shape, dtype=bool)
            lut = _upload(np.where(hit, at, 65535).astype(np.uint16), device)
        need = 16 * gt.shape[0] * gt.shape[1]
        if device.type == 'cuda' and (self._scratch is None or self._scratch.device != device or self._scratch.numel() < need):
            self._scratch = torch.empty(need, dtype=torch.uint8, device=device)
        singles, pairs = pair_metrics.pair_counts(gt, pred, self._ids_dev, _upload(ids.astype(np.int32), device), bound_th=self.bound_th,
                                                  pred_lut=lut, scratch=self._scratch if device.type == 'cuda' else None, validate=False)
        self._frames.append((listed, _Frame(*_pinned_copy(singles)), _Frame(*_pinned_copy(pairs))))

    def _unused_id(self, pred_ids) -> np.ndarray:
        """an id that the plane does not hold: the slot of a frame without proposals"""
        present = set(np.asarray(pred_ids, dtype=np.int64).reshape(-1).tolist())
        return np.array([next(i for i in range(2**31 - 1, 0, -1) if i not in present)], dtype=np.int64)

    # ---------------------------------------------------------------- host arithmetic
    def end_video(self) -> None:
        frames, self._frames = self._frames, None
        if frames is None:
            raise RuntimeError('start_video() first')
        n_gt, frames_n = self._ids.size, len(frames)
        host = [(listed, s.records(), p.records()) for listed, s, p in frames]
        # the proposals of the video: the ids that hold a pixel in some frame (a channel without pixels is none)
        alive = sorted({int(i) for listed, s, _ in host for k, i in enumerate(listed.tolist()) if s[n_gt + k, 0] > 0})
        if len(alive) > self.max_proposals:                                               # U1
            raise ValueError(f'{self._name}: more than {self.max_proposals} proposals ({len(alive)} ids)')
        proposals = alive + [None] * max(0, n_gt - len(alive))                            # U2
        row = {i: k for k, i in enumerate(alive)}
        counts = np.zeros((len(proposals), n_gt, frames_n, 8), dtype=np.int64)            # R5 records of every pair
        for t, (listed, s, p) in enumerate(host):
            counts[:, :, t, 1] = s[:n_gt, 0][None, :]
            counts[:, :, t, 3] = s[:n_gt, 1][None, :]
            for k, i in enumerate(listed.tolist()):
                if i in row:
                    r = row[i]
                    counts[r, :, t, 0], counts[r, :, t, 5], counts[r, :, t, 6] = p[:, k, 0], p[:, k, 1], p[:, k, 2]
                    counts[r, :, t, 2], counts[r, :, t, 4] = s[n_gt + k, 0], s[n_gt + k, 1]
        scored = counts[:, :, 1:-1] if self.skip_ends else counts                          # U3
        j, f = jf_from_counts(scored)                                                     # [P, G, T']
        if scored.shape[2]:
            score = (j.mean(axis=2) + f.mean(axis=2)) / 2                                 # U4
        else:
            score = np.zeros(j.shape[:2])
        chosen = assign(score)
        js, fs = [j[chosen[g], g] for g in range(n_gt)], [f[chosen[g], g] for g in range(n_gt)]
        self.videos.append({'name': self._name, 'ids': self._ids.astype(np.int64).tolist(), 'counts': counts,
                            'J': np.stack(js), 'F': np.stack(fs), 'proposals': proposals, 'score': score,
                            'assignment': {int(self._ids[g]): proposals[chosen[g]] for g in range(n_gt)},
                            'J_stats': [sequence_statistics(v) for v in js],              # U5
                            'F_stats': [sequence_statistics(v) for v in fs]})

    def result(self) -> Dict:
        """`VideoObjectScorer.result()`, and per video in 'frames' additionally 'assignment' {gt id: proposal id, or None
        for a padded row}, 'score' float64 [P, G], 'proposals' (the ids of its rows, None for a padded one); 'counts' is
        int64 [P, G, T, 8]: the R5 record of every pair on every frame"""
        res = super().result()
        for v in self.videos:
            res['frames'][v['name']].update(assignment=v['assignment'], score=v['score'], proposals=v['proposals'])
        return res


def score_directory(results_dir: str, annotations_dir: str, sequences: Optional[Sequence[str]] = None, *, bound_th: float = 0.008,
                    max_proposals: int = 20, skip_ends: bool = False, scorer: Optional[UnsupervisedVideoScorer] = None) -> Dict:
    """a finished run against its annotations: one sub-folder per sequence in both trees, PNGs matched by name (palette,
    gray or RGB-coded predictions).  The objects of a sequence are 1 .. the largest id of its first annotation; a frame's
    proposal ids are those of the host array just read.  -> `UnsupervisedVideoScorer.result()`"""
    from PIL import Image
    scorer = scorer or UnsupervisedVideoScorer(bound_th=bound_th, max_proposals=max_proposals, skip_ends=skip_ends)
    if sequences is None:
        sequences = sorted(d for d in os.listdir(annotations_dir) if path.isdir(path.join(annotations_dir, d)))
    for seq in sequences:
        names = sorted(f for f in os.listdir(path.join(annotations_dir, seq)) if f.endswith('.png'))
        if not names:
            raise FileNotFoundError(f'no annotation in {path.join(annotations_dir, seq)}')
        first = np.array(Image.open(path.join(annotations_dir, seq, names[0])))
        if int(first.max()) < 1:
            raise ValueError(f'{seq}: the first annotation holds no object')
        scorer.start_video(seq, range(1, int(first.max()) + 1))
        for name in names:
            gt = first if name == names[0] else np.array(Image.open(path.join(annotations_dir, seq, name)))
            pred = _read_labels(path.join(results_dir, seq, name))
            if pred.shape != gt.shape:
                raise ValueError(f'{seq}/{name}: the prediction is {pred.shape} and the annotation {gt.shape}')
            scorer.add_frame(pred, gt, pred_ids=np.unique(pred))
        scorer.end_video()
    return scorer.result()
