"""Aggregate throughput of `deva.inference.multi_clip.step_clips` against the sequential loop over the same clips.

B in {1, 2, 4, 8} distinct synthetic 480p clips (synth.base_config()), with 1 object and with 5 objects.  Per (objects, B):
two sets of cores over the same frames, one stepped by `step_clips`, one by `for c: c.step(...)`; after the warm-up the
timed steps run in alternating blocks of both, in this process.  Prints one JSON line: clip-frames per second of both,
their ratio, the peak allocation of each, and how far the two runs' outputs are apart.

Check (asserted <= 1e-3): on the first propagated frame, the sequential outputs against `step_clips` over a third set of
cores whose frame features were encoded per clip beforehand, so that the batched decoder is what differs.  Reported beside
it: the first and the last frame of the two timed runs.  Those are free-running and do not stay within 1e-3 of each other:
the batched key encoder rounds differently (another kernel choice, ~1e-6 relative on the query key), that moves top-k
near-ties of the memory read (up to ~3e-2 on single read-out entries at 480p), and each clip feeds its own masks back --
the growth the suite's tie-following harness (tests/memory_audit.py) exists for; DESIGN section 10 has the measurements.

    python tools/multi_clip_bench.py [--steps 30] [--warmup 5] [--batches 1,2,4,8] [--objects 1,5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tracking-anything-with-deva_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402

BLOCK = 5  # timed steps per alternation block


def run(net, clips, n_obj, warmup, steps, device):
    from workload import synth
    from deva.inference.multi_clip import step_clips
    from deva.utils.tensor_utils import pad_divide_by
    cfg = synth.base_config()
    seq = [bench.start_clip(net, cfg, f, n_obj, device) for f in clips]
    bat = [bench.start_clip(net, cfg, f, n_obj, device) for f in clips]
    out_seq, out_bat = [None] * len(clips), [None] * len(clips)

    def seq_steps(t0, t1):
        for t in range(t0, t1):
            for i, c in enumerate(seq):
                out_seq[i] = c.step(clips[i][t])

    def bat_steps(t0, t1):
        for t in range(t0, t1):
            res = step_clips(bat, [f[t] for f in clips])
            for i, p in enumerate(res):
                out_bat[i] = p

    seq_steps(1, 2)
    bat_steps(1, 2)
    first = max((a - b).abs().max().item() for a, b in zip(out_seq, out_bat))
    pre = [bench.start_clip(net, cfg, f, n_obj, device) for f in clips]
    for c, f in zip(pre, clips):  # (the store then holds the frame: step_clips batches the decoder, not the key encoder)
        c.image_feature_store.get_key(c.curr_ti + 1, pad_divide_by(f[1], 16)[0].unsqueeze(0))
    check = max((a - b).abs().max().item() for a, b in zip(out_seq, step_clips(pre, [f[1] for f in clips])))
    assert check <= 1e-3, f'{n_obj} objects, B={len(clips)}: batched decoder outputs differ by {check:.2e}'
    del pre
    seq_steps(2, 1 + warmup)
    bat_steps(2, 1 + warmup)
    t_seq = t_bat = 0.0
    peak_seq = peak_bat = 0
    t = 1 + warmup
    while t < 1 + warmup + steps:
        t1 = min(t + BLOCK, 1 + warmup + steps)
        torch.cuda.reset_peak_memory_stats(device)
        t_seq += bench.timed_region(lambda: seq_steps(t, t1), device=device)
        peak_seq = max(peak_seq, torch.cuda.max_memory_allocated(device))
        torch.cuda.reset_peak_memory_stats(device)
        t_bat += bench.timed_region(lambda: bat_steps(t, t1), device=device)
        peak_bat = max(peak_bat, torch.cuda.max_memory_allocated(device))
        t = t1
    diff = max((a - b).abs().max().item() for a, b in zip(out_seq, out_bat))
    frames = steps * len(clips)
    return dict(objects=n_obj, B=len(clips), seq_fps=round(frames / t_seq, 1), batched_fps=round(frames / t_bat, 1),
                speedup=round(t_seq / t_bat, 3), seq_peak_mib=round(peak_seq / 2**20), batched_peak_mib=round(peak_bat / 2**20),
                check_max_abs_diff=float(f'{check:.3g}'), first_frame_max_abs_diff=float(f'{first:.3g}'), last_frame_max_abs_diff=float(f'{diff:.3g}'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batches', default='1,2,4,8')
    ap.add_argument('--objects', default='1,5')
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=854)
    args = ap.parse_args()
    assert args.warmup >= 5 and args.steps >= 30, 'at least 5 warm-up frames and 30 timed steps'
    torch.set_grad_enabled(False)
    device = torch.device('cuda:0')
    net, _ = bench.build_network(device)
    batches = [int(b) for b in args.batches.split(',')]
    n_frames = 1 + args.warmup + args.steps
    pool = [bench.make_clip(args.height, args.width, n_frames, 100 + i, device) for i in range(max(batches))]
    rows = []
    for n_obj in (int(o) for o in args.objects.split(',')):
        for b in batches:
            rows.append(run(net, pool[:b], n_obj, args.warmup, args.steps, device))
            print(json.dumps(rows[-1]), file=sys.stderr)
    print(json.dumps(dict(tool='multi_clip_bench', height=args.height, width=args.width, steps=args.steps,
                          warmup=args.warmup, rows=rows)))


if __name__ == '__main__':
    main()
