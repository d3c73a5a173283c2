"""Shared pieces of the test-time-ensemble tests (tests/test_ensemble_cpu.py, tests/test_gpu_n_ensemble.py): a literal
restatement of the reference protocol in numpy / ATen on the CPU, the end-to-end clip with its oracle composition, and
the assertions both end-to-end tests make.

Protocol (evaluation/eval_vos.py:162-177,188-211; scripts/merge_multi_scale.py:44-66): per run F.interpolate(bilinear,
align_corners=False) to the frame's size -> torch.flip for a flipped run -> (prob.numpy() * 255).astype(np.uint8);
offline the runs' volumes are summed as float32, np.argmax over channels picks the first maximum and the tmp-id ->
object-id table maps it."""
import numpy as np
import torch
import torch.nn.functional as F

import emu_ops
from workload import synth

# a resized probability r may differ from ATen's by the project's 1e-6 tie margin (tests/test_gpu_c_bank.py:146); a byte
# trunc(255 * r) can therefore differ (by one) only where 255 * r lies within 255e-6 of an integer
BYTE_MARGIN = 255e-6


def resized(prob, size, flip):
    p = prob
    if size is not None and tuple(size) != tuple(p.shape[-2:]):
        p = F.interpolate(p.unsqueeze(1), tuple(size), mode='bilinear', align_corners=False)[:, 0]
    if flip:
        p = torch.flip(p, dims=[-1])
    return p


def restate_scores(prob, size, flip):
    """-> (uint8 numpy [C,OH,OW], the float32 numpy array 255 * resized it was truncated from)"""
    scaled = resized(prob, size, flip).numpy() * 255
    return scaled.astype(np.uint8), scaled


def restate_merge(volumes, table):
    """merge_multi_scale.py:44-66 -> int64 numpy [OH,OW]; table[tmp id] = object id"""
    result_sum = None
    for result in volumes:
        if result_sum is None:
            result_sum = result.astype(np.float32)
        else:
            result_sum += result
    return np.asarray(table, dtype=np.int64)[np.argmax(result_sum, axis=0)]


def near_integer(scaled):
    """bool array: 255 * r within BYTE_MARGIN of an integer (the byte may legitimately come out one off)"""
    return np.abs(scaled - np.rint(scaled)) <= BYTE_MARGIN


def check_bytes(got, prob, size, flip):
    """`scores_u8` output against the restatement: bit-equal without a resize; with one, off by at most 1 and only at
    near-integer 255 * r.  Returns (number of differing bytes, number of bytes)"""
    want, scaled = restate_scores(prob, size, flip)
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = got.astype(np.int16) - want.astype(np.int16)
    if size is None or tuple(size) == tuple(prob.shape[-2:]):
        assert not diff.any(), f'{int((diff != 0).sum())} bytes differ without a resize'
    else:
        bad = diff != 0
        assert np.abs(diff).max(initial=0) <= 1, f'a byte differs by {int(np.abs(diff).max())}'
        assert not (bad & ~near_integer(scaled)).any(), \
            f'{int((bad & ~near_integer(scaled)).sum())} bytes differ away from a rounding boundary'
    return int((diff != 0).sum()), diff.size


def check_labels_attainable(got_idx, probs, size, flips):
    """quantised merge against the CPU restatement: every byte with 255 * r_cpu near an integer may move by one; the
    kernel's channel index must be attainable as a FIRST maximum of the sums under that freedom.  got_idx: channel
    indices [OH,OW] (no table).  Returns the number of labels that differ from the restatement's"""
    total, freedom = None, None
    for p, f in zip(probs, flips):
        vol, scaled = restate_scores(p, size, f)
        total = vol.astype(np.int32) if total is None else total + vol
        free = near_integer(scaled).astype(np.int32)
        freedom = free if freedom is None else freedom + free
    lo, hi = total - freedom, total + freedom
    g = got_idx.cpu().numpy()
    want = np.argmax(total.astype(np.float32), axis=0)
    c = total.shape[0]
    hi_g = np.take_along_axis(hi, g[None], axis=0)[0]
    chan = np.arange(c)[:, None, None]
    ok = np.where(chan < g[None], hi_g[None] > lo, hi_g[None] >= lo) | (chan == g[None])
    assert ok.all(), f'{int((~ok.all(axis=0)).sum())} labels are not attainable as a first maximum'
    return int((g != want).sum())


# ------------------------------------------------------------------------------------------ the end-to-end clip
H, W, FRAMES, OBJECTS = 96, 128, 4, [1, 2, 3]
SIZES, FLIPS = (-1, 120), (False, True)
VARIANTS = [(s, f) for s in SIZES for f in FLIPS]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def clip_config(**over):
    return synth.base_config(mem_every=2, **over)


def clip_frames():
    """the smoke clip (workload.synth.FrameStream(96, 128, seed=1)) as decoded uint8 H*W*3 frames: the stream's frames
    are ImageNet-normalised, so the normalisation is undone and the result rounded to bytes"""
    stream = synth.FrameStream(H, W, seed=1)
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    return [((stream.next() * std + mean).clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
            for _ in range(FRAMES)]


def clip_mask():
    return synth.box_mask(H, W, len(OBJECTS))


def variant_inputs(frame, mask, size, flip):
    """what one reference run of the protocol is fed: the reader's transform of the (mirrored) frame and the
    nearest-neighbour resized (mirrored) mask"""
    from deva.utils.tensor_utils import network_input_size
    oh, ow = network_input_size(H, W, size)
    f = torch.flip(frame, dims=[1]) if flip else frame
    image = emu_ops.input_head(f, None if (oh, ow) == (H, W) else (oh, ow), antialias=True)
    if mask is not None:
        if (oh, ow) != (H, W):
            mask = F.interpolate(mask[None, None].double(), (oh, ow), mode='nearest')[0, 0].long()
        if flip:
            mask = torch.flip(mask, dims=[-1])
    return image, mask


def oracle_composition(state_dict):
    """one oracle.OracleCore per variant, fed that variant's inputs; the runs merged by the restatement ->
    dict(scores[t][k] uint8, masks[t] int64, mapping {object id: tmp id}, table)"""
    from oracle import deva_oracle as O
    cfg = clip_config()
    frames, mask = clip_frames(), clip_mask()
    cores = [O.OracleCore(state_dict, cfg) for _ in VARIANTS]
    table = [0] + OBJECTS
    scores, masks = [], []
    for t, frame in enumerate(frames):
        vols = []
        for core, (size, flip) in zip(cores, VARIANTS):
            image, m = variant_inputs(frame, mask if t == 0 else None, size, flip)
            prob = core.step(image, m, OBJECTS if t == 0 else None)
            vols.append(restate_scores(prob, (H, W), flip)[0])
        scores.append(vols)
        masks.append(restate_merge(vols, table))
    for core in cores:
        assert core.objects == OBJECTS
    return dict(scores=scores, masks=masks, mapping={o: i + 1 for i, o in enumerate(OBJECTS)}, table=table)


def run_ensemble(net, device):
    """the clip through EnsembleInferenceCore -> (masks[t], scores[t][k], core)"""
    from deva.inference.ensemble import EnsembleInferenceCore
    core = EnsembleInferenceCore(net, clip_config(), sizes=SIZES, flips=FLIPS)
    mask = clip_mask()
    masks, scores = [], []
    for t, frame in enumerate(clip_frames()):
        out, vols = core.step(frame.to(device), mask.to(device) if t == 0 else None, OBJECTS if t == 0 else None,
                              return_scores=True)
        masks.append(out.cpu())
        scores.append([v.cpu() for v in vols])
    return masks, scores, core


def check_end_to_end(masks, scores, core, oracle, what):
    """(i) every score byte within 1 of the oracle composition's (0.255 < 1: the project's 1e-3 probability bound);
    (ii) mask == lut[argmax(sum of the returned bytes)] exactly; (iii) mask == the oracle composition's mask wherever
    the oracle's summed top-2 margin exceeds 2K (K bytes off by one on each of two channels), which may leave out at
    most 15 % of a frame; (iv) the tmp -> object mapping is the oracle's"""
    k = len(VARIANTS)
    table = torch.tensor(oracle['table'], dtype=torch.int64)
    for t in range(FRAMES):
        assert len(scores[t]) == k
        worst = 0
        for got, want in zip(scores[t], oracle['scores'][t]):
            assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
            worst = max(worst, int(np.abs(got.numpy().astype(np.int16) - want.astype(np.int16)).max()))
        total = sum(v.to(torch.int32) for v in scores[t])
        own = table[torch.argmax(total, dim=0)]
        osum = sum(v.astype(np.int32) for v in oracle['scores'][t])
        if osum.shape[0] > 1:
            top2 = np.sort(osum, axis=0)[-2:]
            decisive = (top2[1] - top2[0]) > 2 * k
        else:
            decisive = np.ones(osum.shape[1:], dtype=bool)
        left_out = 1.0 - decisive.mean()
        wrong = int(((masks[t].numpy() != oracle['masks'][t]) & decisive).sum())
        print(f'{what} frame {t}: worst byte error {worst}, margin <= {2 * k} at {100 * left_out:.1f} % of the pixels, '
              f'{wrong} decisive labels differ, {int((masks[t].numpy() != oracle["masks"][t]).sum())} labels differ')
        assert worst <= 1, (what, t, worst)                                  # (i)
        assert masks[t].dtype == torch.int64 and torch.equal(masks[t], own), (what, t)   # (ii)
        assert left_out <= 0.15, (what, t, left_out)
        assert wrong == 0, (what, t, wrong)                                  # (iii)
    assert core.tmp_to_obj_mapping() == oracle['mapping']                    # (iv)
