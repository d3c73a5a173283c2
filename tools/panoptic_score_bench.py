"""The joint count of a scored frame: `metrics.panoptic_counts` (csrc/metrics/panoptic_counts.hip, one pass, a G x P table)
and a whole `VideoPanopticScorer.add_frame`, against the two statements a user would otherwise run for the same table:
ATen on the device (`torch.unique(gt * 2**24 + pred, return_counts=True)` after the RGB decode) and numpy on the host
(the np.unique of eval_vpq_vipseg.py:188-190).  Neither baseline is the code under test.

    python tools/panoptic_score_bench.py [--rounds 7] [--calls 50] [--out FILE.md]

720 x 1280 (VIPSeg 720P) and 1080 x 1920, 40 ground-truth and 40 predicted segments laid out as blocks (panoptic maps are
long runs).  Device forms: kernel time by device events around `--calls` consecutive calls, the forms in alternating
rounds on the same tensors; median, minimum and maximum over the rounds.  The host form: a host clock.  The least traffic
of the count is what it must read: 3 + 2 bytes per pixel on the fast path (RGB ground truth, int16 channel plane), 3 + 3
with an RGB prediction; it is set against the 8 TB/s roof.  `add_frame` is timed with a host clock around `--calls` frames
and one `end`-style wait for the last table (it does not synchronise itself), so it includes the tables' uploads."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import panoptic_case as PC  # noqa: E402
from deva.hip import metrics  # noqa: E402
from deva.inference.panoptic_quality import VideoPanopticScorer  # noqa: E402

ROOF = 8e12
SIZES = ((720, 1280), (1080, 1920))
N = 40


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


def host_us(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def frame(h, w):
    """-> gt ids, gt table, predicted ids, predicted table, channel plane, channel -> slot table, channel ids"""
    gt, gt_table, pred, pred_table = PC.planes(h, w, N, N, 5)
    pred = np.where((pred < 0) | (pred >= 2**24), 0, pred)
    pred[~np.isin(pred, pred_table)] = 0              # a tracker's output holds only its own ids
    channel_ids = np.concatenate([[0], pred_table])
    index = (np.searchsorted(pred_table, pred) + 1) * (pred != 0)
    lut = np.arange(N + 1) + 1
    lut[0] = 0
    return gt, gt_table, pred, pred_table, index.astype(np.int16), lut.astype(np.uint16), channel_ids


def table(args, dev, h, w):
    gt, gt_table, pred, pred_table, index, lut, channel_ids = frame(h, w)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    gt_rgb, pred_rgb, index_d, lut_d = up(PC.rgb(gt)), up(PC.rgb(pred)), up(index), up(lut)
    gt_tab, pred_tab = up(gt_table.astype(np.int32)), up(pred_table.astype(np.int32))
    out = torch.empty((N + 2, N + 2), dtype=torch.uint32, device=dev)
    fast = lambda: metrics.panoptic_counts(gt_rgb, gt_tab, index_d, N, lut_d, out=out, validate=False)            # noqa: E731
    both = lambda: metrics.panoptic_counts(gt_rgb, gt_tab, pred_rgb, pred_tab, out=out, validate=False)           # noqa: E731
    weights = torch.tensor([1, 256, 65536], dtype=torch.int64, device=dev)

    def aten():
        g = (gt_rgb.to(torch.int64) * weights).sum(-1)
        p = (pred_rgb.to(torch.int64) * weights).sum(-1)
        return torch.unique(g * 2**24 + p, return_counts=True)

    gt_host, pred_host = PC.rgb(gt), PC.rgb(pred)

    def host():
        g, p = np.uint32(gt_host), np.uint32(pred_host)
        g = g[:, :, 0] + g[:, :, 1] * 256 + g[:, :, 2] * 256 * 256
        p = p[:, :, 0] + p[:, :, 1] * 256 + p[:, :, 2] * 256 * 256
        return np.unique(g.astype(np.uint64) * 2**24 + p.astype(np.uint64), return_counts=True)

    # the same table from all four
    keys, n = host()
    want = {(int(k) >> 24, int(k) & 0xffffff): int(c) for k, c in zip(keys, n)}

    def as_pairs(counts):
        rows, cols = [0, -1] + gt_table.tolist(), [0, -1] + pred_table.tolist()
        c = counts.cpu().numpy()
        return {(rows[a], cols[b]): int(c[a, b]) for a, b in zip(*np.nonzero(c))}
    listed = {k: v for k, v in want.items() if (k[0] == 0 or k[0] in set(gt_table.tolist()))}
    unlisted = sum(v for k, v in want.items() if k not in listed)
    same = True
    for fn in (fast, both):
        got = as_pairs(fn())
        same = same and {k: v for k, v in got.items() if k[0] != -1} == listed and \
            sum(v for k, v in got.items() if k[0] == -1) == unlisted
    ku, nu = aten()
    same = same and {(int(k) >> 24, int(k) & 0xffffff): int(c) for k, c in zip(ku.cpu(), nu.cpu())} == want

    scorer = VideoPanopticScorer(PC.CATEGORIES)
    gt_info = [dict(id=int(i), category_id=2, iscrowd=0, area=1) for i in gt_table]
    pred_info = [dict(id=int(i), category_id=2) for i in pred_table]

    def add_frames(calls):
        scorer.start_video('bench')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            scorer.add_frame((index_d, channel_ids), pred_info, gt_rgb, gt_info)
        enqueue = (time.perf_counter() - t0) / calls * 1e6
        scorer._frames[-1].event.synchronize()
        total = (time.perf_counter() - t0) / calls * 1e6
        scorer._frames = None
        return enqueue, total

    t = {k: [] for k in ('fast', 'both', 'aten', 'host', 'enqueue', 'add')}
    for fn in (fast, both, aten):
        event_us(fn, 3)                                          # warm-up of every form
    add_frames(3)
    for _ in range(args.rounds):
        t['fast'].append(event_us(fast, args.calls))
        t['both'].append(event_us(both, args.calls))
        t['aten'].append(event_us(aten, max(args.calls // 10, 2)))
        e, a = add_frames(args.calls)
        t['enqueue'].append(e)
        t['add'].append(a)
    for _ in range(min(args.rounds, 3)):
        t0 = time.perf_counter()
        host()
        t['host'].append((time.perf_counter() - t0) * 1e6)
    px = h * w
    f, b = statistics.median(t['fast']), statistics.median(t['both'])
    plan = metrics.panoptic_plan(h, w, N, N)
    return [f'{h} x {w}, {N} x {N} segments ({plan.path} path, {plan.grid} workgroups of {plan.block}, {plan.lds_bytes} B of LDS); '
            f'{args.rounds} alternating rounds of {args.calls} calls, microseconds per call, median (min, max); '
            f'all forms give the same table: {"yes" if same else "NO"}', '',
            '| form | per call | least traffic | rate | of the 8 TB/s roof |', '|---|---|---|---|---|',
            f'| panoptic_counts, RGB + channel plane | {spread(t["fast"])} | {5 * px / 1e6:.1f} MB (3 + 2 B / pixel) | '
            f'{5 * px / f / 1e3:.0f} GB/s | {5 * px / f * 1e6 / ROOF:.3f} |',
            f'| panoptic_counts, RGB + RGB | {spread(t["both"])} | {6 * px / 1e6:.1f} MB (3 + 3 B / pixel) | '
            f'{6 * px / b / 1e3:.0f} GB/s | {6 * px / b * 1e6 / ROOF:.3f} |',
            f'| add_frame, whole (host clock, table on the host) | {spread(t["add"])} | | | |',
            f'| add_frame, until it returns (host clock) | {spread(t["enqueue"])} | | | |',
            f'| ATen decode + torch.unique on the device | {spread(t["aten"])} | | | |',
            f'| numpy decode + np.unique on the host | {spread(t["host"], 0)} | | | |',
            f'| ratios to the fast path | ATen {statistics.median(t["aten"]) / f:.0f}x, numpy {statistics.median(t["host"]) / f:.0f}x | | | |',
            '']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('panoptic_score_bench: needs the GPU (a CPU timing says nothing about it)')
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    lines = [torch.cuda.get_device_name(0), '']
    for h, w in SIZES:
        lines += table(args, dev, h, w)
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
