"""The network end to end at the frame geometries a user feeds it, and with many objects in one pass.

The other -m gpu files run full-size frames whose maps are friendly at every scale (480x864 -> 30x54, 1088x1920 ->
68x120, 2160x3840 -> 135x240).  The reference's drivers resize the SHORT side to 480 and keep the aspect ratio, or run at
native size; after pad_divide_by(16) that gives 1/16 maps such as 30x45, 29x53, 54x30, 45x80, on which the dispatcher's
geometry rules (16-byte gathers and output stage: pixel count 4k; Winograd: even width, >= 160 workgroups; the --f16_split
kernels: pixel count 4k; the pointwise kernels' vector forms) flip layer by layer inside one frame.

* `test_lockstep_at_awkward_geometries`: tests/lockstep.py (teacher-forced, every stage of every frame) on the three builds
  at four such sizes, bounds unchanged (2e-4 relative per stage, 1e-3 on logits / probabilities, read-out 1e-4).
* `test_geometry_list_reaches_both_sides_of_the_rules`: a condition on that list of sizes, from the eligibility
  predicates of tests/emu_ops.py alone: at 1/16 the split kernels and the Winograd kernel each take some 3x3 layers and
  refuse others, and so does the Winograd kernel at 1/8.
* `test_unpadded_free_running`: 481x853 (pads on both axes, odd crops on the way out) through DEVAInferenceCore.step
  against the tie-following oracle under the north-star bound.
* `test_many_objects_*`: 20 objects at 1088x1920 and 5 at 2160x3840 in ONE pass.  The decoder's 256-channel 1/4-scale
  maps then span 2^29 floats or more (from 17 objects at 1080p, 5 at 4K): deva_conv2d runs such a batch as consecutive
  sub-batches (include/deva_hip.h), and the pointwise kernels pass the 268 M threads after which their grid-stride loops
  take over.  Held against the chunked pass and, at 1080p, against the CPU oracle run for three of the objects alone.
* `test_24_objects_free_running`: the first end-to-end clip above 14 objects.
"""
import json
import os

import pytest
import torch

import emu_ops
import memory_audit
from gpu_util import dev, max_err
from deva.hip import ops
from oracle import deva_oracle as O
from workload import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRY = os.environ.get('DEVA_TEST_DRYRUN') == '1'  # the builder's CPU run of this file (emulated ops); never set on the GPU box

# (H, W, objects): padded sizes; 1/16 maps 30x45, 29x53, 54x30, 45x80
GEOMETRIES = [(480, 720, 2), (464, 848, 1), (864, 480, 3), (720, 1280, 2)]


def _net(sd, **extra):
    from deva.model.network import DEVA
    net = DEVA(dict(synth.base_config(), **extra))
    net.load_weights(sd)
    return net.to(dev()).eval()


@pytest.fixture(scope='module')
def network(recipe_state_dict):
    return _net(recipe_state_dict[0])


@pytest.fixture(scope='module')
def split_network(recipe_state_dict):
    return _net(recipe_state_dict[0], f16_split=True)


@pytest.fixture(scope='module')
def split_all_network(recipe_state_dict):
    return _net(recipe_state_dict[0], f16_split=True, f16_split_key_encoder=True)


def _census(net, H, W, no):
    """every convolution of one frame (key encoder, key projection, mask decoder, value encoder) as the shapes it is
    called with, and what the eligibility predicates of tests/emu_ops.py say about each: rows of (scale, kernel size,
    split asked for and packed, split taken, Winograd packed and reachable, Winograd taken)"""
    rows, conv2d = [], ops.conv2d

    def recording(pc, x0, x1=None, *, stride=1, pad=0, amp=False, split=False, **kw):
        h = x0.shape[-2]
        batch = max(x0.shape[0], 1 if x1 is None else x1.shape[0], 1 if kw.get('residual') is None else kw['residual'].shape[0])
        asked = bool(split) and pc.weight_split is not None
        wino = pc.weight_wino is not None and not asked and not (amp and pc.weight_f16 is not None)
        rows.append((H // h if h <= H else 0, pc.kh, stride, asked, asked and emu_ops.split_takes(pc, x0, x1, stride, pad),
                     wino, wino and emu_ops.wino_takes(pc, x0, x1, stride, pad, batch)))
        return conv2d(pc, x0, x1, stride=stride, pad=pad, amp=amp, split=split, **kw)

    d = dev()
    img = synth.FrameStream(H, W, seed=5).next().unsqueeze(0).to(d)
    masks, sensory, readout = (t.to(d) for t in synth.stage_inputs(H, W, no))
    ops.conv2d = recording
    try:
        ms, feat = net.encode_image(img)
        net.transform_key(feat)
        net.segment(ms, readout, sensory, masks)
        net.encode_mask(img, ms, sensory, masks)
        torch.cuda.synchronize()
    finally:
        ops.conv2d = conv2d
    return rows


def _counts(rows, scale, which):
    """(taken, not taken) among the 3x3 stride-1 layers at 1/scale that ask for the split (which = 'split') or carry
    Winograd weights (which = 'wino')"""
    asked, taken = (3, 4) if which == 'split' else (5, 6)
    sel = [r for r in rows if r[0] == scale and r[1] == 3 and r[2] == 1 and r[asked]]
    return sum(bool(r[taken]) for r in sel), sum(not r[taken] for r in sel)


@pytest.mark.parametrize('H,W,no', GEOMETRIES, ids=[f'{h}x{w}x{n}' for h, w, n in GEOMETRIES])
def test_lockstep_at_awkward_geometries(network, split_network, split_all_network, recipe_state_dict, H, W, no):
    """fp32, --f16_split and --f16_split --f16_split_key_encoder teacher-forced on ONE oracle pass, 3 frames with a memory
    frame every 2nd (two memory frames, two reads).  No split convolution may FALL BACK (recipe activations sit inside the
    fp16 range; a layer the split kernels do not take is not a fall-back)."""
    import lockstep
    nets = {'fp32': network, 'f16_split': split_network, 'f16_split+key_encoder': split_all_network}
    for tag, net in (('fp32', network), ('f16_split+key_encoder', split_all_network)):
        rows = _census(net, H, W, no)
        print(f'{H}x{W} x{no} [{tag}]: {len(rows)} convolutions; 3x3 layers (taken, not taken) by the split kernels at 1/16 '
              f'{_counts(rows, 16, "split")} 1/8 {_counts(rows, 8, "split")} 1/4 {_counts(rows, 4, "split")}; by Winograd at '
              f'1/16 {_counts(rows, 16, "wino")} 1/8 {_counts(rows, 8, "wino")} 1/4 {_counts(rows, 4, "wino")}; all layers '
              f'asking for the split: taken {sum(bool(r[4]) for r in rows)}, not taken {sum(r[3] and not r[4] for r in rows)}')
    before = ops.split_fallbacks(dev())
    worst = lockstep.run(nets, recipe_state_dict[0], H, W, no, 3, dev())
    for build, w in worst.items():
        print(f'lockstep {H}x{W} x{no} [{build}] worst relative errors:', json.dumps({k: float(f'{v:.2e}') for k, v in w.items()}))
    assert ops.split_fallbacks(dev()) == before


def test_geometry_list_reaches_both_sides_of_the_rules(network, split_all_network):
    """GEOMETRIES must not degrade into friendly shapes: over the four frames the split predicate both takes and
    refuses 3x3 layers at 1/16 (at 1/8 and 1/4 a padded frame always has a pixel count of 4k and an even width), and the
    Winograd predicate does both at 1/16 (odd width) and at 1/8 (the 160-workgroup rule at one object).  A condition on
    the INPUT list, from the predicates of tests/emu_ops.py: if a count is zero, change a size or an object count."""
    total = {}
    for H, W, no in GEOMETRIES:
        split_rows, wino_rows = _census(split_all_network, H, W, no), _census(network, H, W, no)
        for key, rows, scale, which in (('split 1/16', split_rows, 16, 'split'), ('wino 1/16', wino_rows, 16, 'wino'),
                                        ('wino 1/8', wino_rows, 8, 'wino')):
            t, n = _counts(rows, scale, which)
            total[key] = (total.get(key, (0, 0))[0] + t, total.get(key, (0, 0))[1] + n)
    print('3x3 layers (taken, not taken) over the four geometries:', total)
    for key, (t, n) in total.items():
        assert t > 0 and n > 0, (key, t, n)


@pytest.mark.parametrize('build', ['fp32', 'f16_split+key_encoder'])
def test_unpadded_free_running(network, split_all_network, recipe_state_dict, build):
    """481x853 pads to 496x864 on BOTH axes (1/16 map 31x54), 3 objects, 7 frames, a memory frame every 2nd, through the
    public interface (pad, propagate, unpad on odd crops) against the tie-following oracle: 1e-3 max-abs, argmax-identical
    above a 2e-3 reference margin (tests/memory_audit.py)"""
    from deva.inference.inference_core import DEVAInferenceCore
    net = network if build == 'fp32' else split_all_network
    H, W, no, frames = 481, 853, 3, 7
    cfg = synth.base_config(mem_every=2)
    hip, following = DEVAInferenceCore(net, cfg), O.OracleCore(recipe_state_dict[0], cfg)
    stream = synth.FrameStream(H, W, seed=6)
    imgs = [stream.next() for _ in range(frames)]
    mask0, objs = synth.box_mask(H, W, no), list(range(1, no + 1))
    before = ops.split_fallbacks(dev())
    report = memory_audit.paired_steps(
        f'481x853/3obj [{build}]', frames,
        lambda t: hip.step(imgs[t].to(dev()), None if t else mask0.to(dev()), None if t else objs).cpu(),
        lambda t: following.step(imgs[t], None if t else mask0, None if t else objs))
    assert ops.split_fallbacks(dev()) == before
    print(f'481x853 free-running [{build}]:', json.dumps({k: float(f'{v:.3g}') for k, v in report.items()}))


def _rel(got, ref):
    return max_err(got, ref) / max(1.0, ref.abs().max().item())


def _many_objects(net, H, W, no, chunk, P=None, alone=()):
    """one teacher-forced segment and one encode_mask with `no` objects in ONE pass (chunk_size=-1): must run, and agree
    with the same call at chunk_size=chunk within the lock-step stage bound (2e-4 relative; 1e-3 absolute on logits and
    probabilities) -- both are implementations of the same fp32 arithmetic.  alone: object indices for which the CPU
    oracle, run for those objects ALONE, is compared too: sensory output, per-object logit channels, value.  (The oracle's
    sensory / object-logit channels of a subset call are bit-identical to those of the full call, its value agrees to 1e-6;
    the background channel and the probabilities couple all objects and are not compared this way.)"""
    d = dev()
    img = synth.FrameStream(H, W, seed=5).next().unsqueeze(0)
    masks, sensory, readout = synth.stage_inputs(H, W, no)
    if P is not None:
        ms_o, _ = O.encode_image(P, img)
        ms = tuple(x.to(d) for x in ms_o)
    else:
        ms, _ = net.encode_image(img.to(d))
    img_d, masks_d, sensory_d, readout_d = img.to(d), masks.to(d), sensory.to(d), readout.to(d)
    per_object = 256 * (H // 4) * (W // 4)
    print(f'{H}x{W} x{no}: the 1/4-scale 256-channel maps span {no * per_object / 2**29:.2f} x 2^29 floats -> deva_conv2d runs '
          f'sub-batches of {emu_ops.conv_sub_batches(no, 256, H // 4, W // 4, per_object)} images; '
          f'{no * per_object / (65535 * 16 * 256):.2f} x the threads of the pointwise kernels\' largest grid')
    one = net.segment(ms, readout_d, sensory_d, masks_d, chunk_size=-1)
    one_v = net.encode_mask(img_d, ms, sensory_d, masks_d, chunk_size=-1)
    torch.cuda.synchronize()
    some = net.segment(ms, readout_d, sensory_d, masks_d, chunk_size=chunk)
    some_v = net.encode_mask(img_d, ms, sensory_d, masks_d, chunk_size=chunk)
    torch.cuda.synchronize()
    names = ('sensory_seg', 'logits', 'prob', 'value', 'sensory_deep')
    errs = {n: _rel(a.cpu(), b.cpu()) for n, a, b in zip(names, one + one_v, some + some_v)}
    errs['logits_abs'], errs['prob_abs'] = max_err(one[1], some[1]), max_err(one[2], some[2])
    print(f'{H}x{W} x{no}: chunk_size=-1 against chunk_size={chunk}:', json.dumps({k: float(f'{v:.2e}') for k, v in errs.items()}))
    for a in one + one_v:
        assert bool(torch.isfinite(a).all())
    for n in names:
        assert errs[n] <= 2e-4, (n, errs[n])
    assert errs['logits_abs'] <= 1e-3 and errs['prob_abs'] <= 1e-3, errs
    if alone:
        sel = torch.tensor(list(alone))
        s_o, lg_o, _ = O.segment(P, ms_o, readout[:, sel], sensory[:, sel], masks[:, sel])
        v_o, s2_o = O.encode_mask(P, img, ms_o[0], sensory[:, sel], masks[:, sel])
        s_h, lg_h = one[0].cpu()[:, sel], one[1].cpu()[:, sel + 1]
        v_h, s2_h = one_v[0].cpu()[:, sel], one_v[1].cpu()[:, sel]
        ref = dict(sensory_seg=(s_h, s_o), logits=(lg_h, lg_o[:, 1:]), value=(v_h, v_o), sensory_deep=(s2_h, s2_o))
        errs = {n: _rel(a, b) for n, (a, b) in ref.items()}
        errs['logits_abs'] = max_err(lg_h, lg_o[:, 1:])
        print(f'{H}x{W} x{no}: objects {[i + 1 for i in alone]} of the one-pass call against the CPU oracle run for them '
              'alone:', json.dumps({k: float(f'{v:.2e}') for k, v in errs.items()}))
        for n in ref:
            assert errs[n] <= 2e-4, (n, errs[n])
        assert errs['logits_abs'] <= 1e-3, errs


def test_many_objects_one_pass_1080p(network, recipe_state_dict):
    """1088x1920, 20 objects: 20 x 33.4 M floats at 1/4 scale = 1.25 x 2^29, and 668 M elements per pointwise launch.
    Compared with the oracle: the first object, the 17th (the first one past the 2^29-float boundary: where the second
    sub-batch starts) and the last"""
    (H, W), no = ((144, 256), 20) if DRY else ((1088, 1920), 20)
    _many_objects(network, H, W, no, 4, recipe_state_dict[0], alone=(0, 16, no - 1))


def test_many_objects_one_pass_4k(network):
    """2160x3840, 5 objects (5 x 132.7 M floats at 1/4 scale = 1.24 x 2^29) against chunk_size=2; no CPU oracle at this
    size.  Needs ~13 GiB of device memory at the peak (measured: 12.1 GiB allocated); skipped below 24 GiB free."""
    (H, W) = (144, 256) if DRY else (2160, 3840)
    if not DRY:
        free = torch.cuda.mem_get_info()[0]
        if free < 24 * 2**30:
            print(f'skipped: {free / 2**30:.1f} GiB of device memory free, the pass needs 24 GiB with headroom')
            pytest.skip('less than 24 GiB of device memory free')
    _many_objects(network, H, W, 5, 2)


def test_24_objects_free_running(network, recipe_state_dict):
    """480x864, 24 objects from staggered boxes, 4 frames, a memory frame every 2nd, free-running against the
    tie-following oracle under the north-star bound as written"""
    from deva.inference.inference_core import DEVAInferenceCore
    (H, W), no, frames = ((96, 144) if DRY else (480, 864)), 24, 4
    cfg = synth.base_config(mem_every=2)
    hip, following = DEVAInferenceCore(network, cfg), O.OracleCore(recipe_state_dict[0], cfg)
    stream = synth.FrameStream(H, W, seed=8)
    imgs = [stream.next() for _ in range(frames)]
    mask0, objs = synth.box_mask(H, W, no), list(range(1, no + 1))
    assert sorted(mask0.unique().tolist()) == [0] + objs, 'every object must own pixels of the first mask'
    report = memory_audit.paired_steps(
        f'{H}x{W}/24obj', frames,
        lambda t: hip.step(imgs[t].to(dev()), None if t else mask0.to(dev()), None if t else objs).cpu(),
        lambda t: following.step(imgs[t], None if t else mask0, None if t else objs))
    assert hip.object_manager.num_obj == no
    print(f'{H}x{W} 24-object free-running clip:', json.dumps({k: float(f'{v:.3g}') for k, v in report.items()}))
