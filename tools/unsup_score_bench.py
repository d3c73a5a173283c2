"""The pair table of a frame scored by the unsupervised DAVIS protocol: `pair_metrics.pair_counts`
(csrc/pair_metrics/pair_counts.hip, two launches) against the two ways a user could get the same integers without it:
(a) G x P calls of `vos_metrics.boundary_counts` on planes relabelled to one pair each (the relabelling is part of the
cost: it is what that way needs), and (b) ATen on the device: one boolean plane per object and proposal, the boundary map
by slicing, ONE `conv2d` with the disk per object and side, then every pair by an AND and a sum.  Neither is the code
under test.

    python tools/unsup_score_bench.py [--rounds 5] [--calls 20] [--out FILE.md]

480 x 854 with 5 objects and 20 proposals (radius 8) and 1080 x 1920 with 10 and 20 (radius 18); uint8 ground truth and
int64 prediction.  Device events around `--calls` consecutive calls (a tenth of them for the slow forms), the forms in
alternating rounds on the same tensors; median, minimum and maximum over the rounds."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import pair_case as PC  # noqa: E402
from deva.hip import pair_metrics, vos_metrics  # noqa: E402

SHAPES = ((480, 854, 5, 20, 8), (1080, 1920, 10, 20, 18))


def spread(ts, digits=1):
    return f'{statistics.median(ts):.{digits}f} (min {min(ts):.{digits}f}, max {max(ts):.{digits}f})'


def event_us(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls * 1e3


def relabelled_calls(gt, pred, gt_ids, pred_ids, radius, scratch, one):
    """(a): every pair by the one-table scorer -> int64 [G, P, 8]"""
    rows = []
    for g in gt_ids.tolist():
        gt_one = (gt == g).to(torch.uint8)
        rows.append(torch.stack([vos_metrics.boundary_counts(gt_one, (pred == p).to(torch.uint8), one, radius=radius, scratch=scratch,
                                                             validate=False)[0] for p in pred_ids.tolist()]))
    return torch.stack(rows)


def aten_pairs(gt, pred, gt_ids, pred_ids, disk):
    """(b): the per-plane statement in ATen, one dilation per object and side -> (singles int64 [G + P, 2], pairs int64 [G, P, 3])"""
    g = gt.unsqueeze(0) == gt_ids.view(-1, 1, 1)
    p = pred.unsqueeze(0) == pred_ids.view(-1, 1, 1)

    def bmap(s):
        b = torch.zeros_like(s)
        b[:, :, :-1] |= s[:, :, :-1] ^ s[:, :, 1:]
        b[:, :-1, :] |= s[:, :-1, :] ^ s[:, 1:, :]
        b[:, :-1, :-1] |= s[:, :-1, :-1] ^ s[:, 1:, 1:]
        return b

    def dilated(b):
        r = disk.shape[-1] // 2
        return (F.conv2d(b.unsqueeze(1).float(), disk, padding=r)[:, 0] > 0).float().flatten(1)
    bg, bp = bmap(g), bmap(p)
    gf, pf, bgf, bpf = (t.float().flatten(1) for t in (g, p, bg, bp))
    pairs = torch.stack([gf @ pf.T, bgf @ dilated(bp).T, dilated(bg) @ bpf.T], dim=2).long()      # (exact: counts below 2^24)
    singles = torch.stack([torch.cat([gf.sum(1), pf.sum(1)]), torch.cat([bgf.sum(1), bpf.sum(1)])], dim=1).long()
    return singles, pairs


def table(args, dev, h, w, n_gt, n_pred, radius):
    gt, pred, gt_ids, pred_ids = PC.case(h, w, n_gt, n_pred, 5)
    pred = np.where(np.isin(pred, pred_ids), pred, 0)
    assert radius == vos_metrics.boundary_radius(h, w)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    gt_d, pred_d, gt64 = up(gt.astype(np.uint8)), up(pred), up(gt)
    ids_g, ids_p, ids_g64, ids_p64 = up(gt_ids.astype(np.int32)), up(pred_ids.astype(np.int32)), up(gt_ids), up(pred_ids)
    one = up(np.array([1], dtype=np.int32))
    scratch = torch.empty(pair_metrics.pair_scratch_bytes(h, w), dtype=torch.uint8, device=dev)
    out = (torch.empty((n_gt + n_pred, 2), dtype=torch.uint32, device=dev), torch.empty((n_gt, n_pred, 4), dtype=torch.uint32, device=dev))
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    disk = up((yy * yy + xx * xx <= radius * radius).astype(np.float32))[None, None]

    fast = lambda: pair_metrics.pair_counts(gt_d, pred_d, ids_g, ids_p, radius=radius, scratch=scratch, out=out, validate=False)   # noqa: E731
    calls = lambda: relabelled_calls(gt_d, pred_d, gt_ids, pred_ids, radius, scratch, one)      # noqa: E731
    aten = lambda: aten_pairs(gt64, pred_d, ids_g64, ids_p64, disk)                             # noqa: E731

    singles, pairs = (t.cpu().numpy().astype(np.int64) for t in fast())
    want = np.transpose(PC.records(singles, pairs), (1, 0, 2))                                   # [G, P, 8]
    a_singles, a_pairs = (t.cpu().numpy() for t in aten())
    same = (np.array_equal(calls().cpu().numpy().astype(np.int64), want) and np.array_equal(a_singles, singles)
            and np.array_equal(a_pairs, pairs[..., :3]))
    t = {k: [] for k in ('fast', 'calls', 'aten')}
    for fn in (fast, calls, aten):
        event_us(fn, 2)
    slow = max(args.calls // 10, 2)
    for _ in range(args.rounds):
        t['fast'].append(event_us(fast, args.calls))
        t['calls'].append(event_us(calls, slow))
        t['aten'].append(event_us(aten, slow))
    plan = pair_metrics.pair_plan(h, w, n_gt, n_pred, radius)
    f = statistics.median(t['fast'])
    boundary = int(singles[:, 1].sum())
    return [f'{h} x {w}, {n_gt} objects, {n_pred} proposals, radius {radius} ({plan.label_grid} + {plan.match_grid} workgroups of '
            f'{plan.block}, {plan.label_lds_bytes} + {plan.match_lds_bytes} B of LDS, {boundary} boundary pixels on the two sides); '
            f'{args.rounds} alternating rounds, microseconds per call, median (min, max); all forms give the same integers: '
            f'{"yes" if same else "NO"}', '',
            '| form | per call | against `pair_counts` |', '|---|---|---|',
            f'| `pair_counts`: two launches | {spread(t["fast"])} | 1 |',
            f'| (a) {n_gt * n_pred} `boundary_counts` calls on relabelled planes | {spread(t["calls"])} | {statistics.median(t["calls"]) / f:.0f}x |',
            f'| (b) ATen: one-hot planes, `conv2d` with the disk per object and side | {spread(t["aten"])} | {statistics.median(t["aten"]) / f:.0f}x |',
            '']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('unsup_score_bench: no HIP device')
    dev = torch.device('cuda')
    lines = [f'# pair_counts: {torch.cuda.get_device_name(0)}', '']
    for shape in SHAPES:
        lines += table(args, dev, *shape)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
