"""`step_clips` (deva/inference/multi_clip.py) and its kernels on the MI355X: the mapped up-sampling kernels bit for bit
against the broadcast ones, the four E2E clips stepped together against the reference's goldens under the audit harness
of test_gpu_e_network.py, position independence of the batched pass at 480p, stage parity of the batched stages and the
B = 1 identity with `core.step`."""
import json
import os

import numpy as np
import pytest
import torch

import memory_audit
import scenarios
from gpu_util import dev, net_config, rel_err
from oracle import deva_oracle as O
from workload import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope='module')
def network(recipe_state_dict):
    from deva.model.network import DEVA
    sd, _ = recipe_state_dict
    net = DEVA(net_config())
    net.load_weights(sd)
    return net.to(dev()).eval()


@pytest.mark.parametrize('shape', [(5, 32, 30, 54), (4, 16, 15, 27), (3, 8, 4, 6)])
def test_upsample_map_bit_identical_to_broadcast(shape):
    from deva.hip import ops
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(b, c, h, w, generator=gen).to(dev())
    skip = torch.randn(3, c, 2 * h, 2 * w, generator=gen).to(dev())
    index = [2, 0, 1, 2, 0][:b]
    got = ops.upsample2x_add_map(x, skip, ops.clip_index(index, 3, dev()))
    even = h % 2 == 0 and w % 2 == 0
    if even:
        got2, ds2 = ops.upsample2x_add_ds2_map(x, skip, ops.clip_index(index, 3, dev()))
        assert torch.equal(ds2, ops.area_downsample(x, 2))
    for i, s in enumerate(index):
        ref = ops.upsample2x_add(x[i:i + 1].contiguous(), skip[s:s + 1].contiguous())
        assert torch.equal(got[i:i + 1], ref), (shape, i)
        if even:
            assert torch.equal(got2[i:i + 1], ref), (shape, i)


def _feeds(names):
    return [dict(sc=scenarios.E2E[n], stream=synth.FrameStream(scenarios.E2E[n]['H'], scenarios.E2E[n]['W'], seed=1))
            for n in names]


def _args(sc, stream, t):
    img = stream.next()
    end = t == sc['frames'] - 1
    if t == 0:
        return img, synth.box_mask(sc['H'], sc['W'], sc['nobj']), list(range(1, sc['nobj'] + 1)), end
    if sc['second'] is not None and t == sc['second'][0]:
        oid = sc['second'][1]
        m = torch.zeros(sc['H'], sc['W'], dtype=torch.long)
        m[sc['H'] // 2:, :sc['W'] // 4] = oid
        return img, m, [oid], end
    return img, None, None, end


def test_e2e_clips_together_against_reference_golden(network, golden_dir, recipe_state_dict):
    """the four E2E clips in one step_clips call per frame; each clip's memory reads are tapped while its own
    match_memory runs, and the CPU oracle of that clip follows exactly those reads (TieFollowing)"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.multi_clip import step_clips
    P, _ = recipe_state_dict
    names = list(scenarios.E2E)
    feeds = _feeds(names)
    cores = [DEVAInferenceCore(network, synth.base_config(**f['sc']['cfg'])) for f in feeds]
    reads = {n: [] for n in names}
    outs = {n: [] for n in names}
    with memory_audit.ReadTap() as tap:
        for name, core in zip(names, cores):
            def tagged(key, selection, _orig=core.memory.match_memory, _name=name):
                at = len(tap.reads)
                r = _orig(key, selection)
                reads[_name].extend(tap.reads[at:])
                return r
            core.memory.match_memory = tagged
        for t in range(max(f['sc']['frames'] for f in feeds)):
            live = [i for i, f in enumerate(feeds) if t < f['sc']['frames']]
            a = [_args(feeds[i]['sc'], feeds[i]['stream'], t) for i in live]
            probs = step_clips([cores[i] for i in live], [x[0].to(dev()) for x in a],
                               [None if x[1] is None else x[1].to(dev()) for x in a], [x[2] for x in a],
                               end=[x[3] for x in a])
            for i, p in zip(live, probs):
                outs[names[i]].append(p.float().cpu())
    assert sum(len(r) for r in reads.values()) == len(tap.reads)
    for name, core in zip(names, cores):
        sc = scenarios.E2E[name]
        g = np.load(os.path.join(golden_dir, f'e2e_{name}.npz'))
        adopted_at = []
        with memory_audit.TieFollowing(name, reads[name]) as tf:
            following, _ = scenarios.run_scenario(lambda cfg: O.OracleCore(P, cfg), sc,
                                                  on_frame=lambda t, c: adopted_at.append(tf.adopted))
        tf.check()
        assert not tf.queue
        drift = memory_audit.Drift(f'batched {name}', stride=2)
        for t, p in enumerate(outs[name]):
            drift.add(p[:, ::2, ::2], following[t][:, ::2, ::2], torch.from_numpy(g[f'prob_sub_{t}']), frame=t,
                      adopted_so_far=adopted_at[t])
        print(f'batched {name}:', json.dumps({k: float(f'{v:.3g}') for k, v in drift.finish().items()}))
        assert [p.shape[0] for p in outs[name]] == g['nchan'].tolist()
        sizes = json.loads(str(g['sizes']))
        mem = core.memory
        assert {str(b): mem.work_mem.size(b) for b in mem.work_mem.buckets} == sizes['work']
        if mem.use_long_term:
            assert {str(b): mem.long_mem.size(b) for b in mem.long_mem.buckets} == sizes['long']


H480, W480 = 480, 854


def _clips_480p(n_objs, frames, seeds):
    clips = []
    for n, s in zip(n_objs, seeds):
        stream = synth.FrameStream(H480, W480, seed=s)
        clips.append(dict(frames=[stream.next().to(dev()) for _ in range(frames)], n=n,
                          mask=synth.box_mask(H480, W480, n).to(dev())))
    return clips


def _run_batched(network, clips, order):
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.multi_clip import step_clips
    cfg = synth.base_config(mem_every=3)
    cores = {i: DEVAInferenceCore(network, cfg) for i in order}
    outs = {i: [] for i in order}
    for t in range(len(clips[0]['frames'])):
        probs = step_clips([cores[i] for i in order], [clips[i]['frames'][t] for i in order],
                           [clips[i]['mask'] if t == 0 else None for i in order],
                           [list(range(1, clips[i]['n'] + 1)) if t == 0 else None for i in order])
        for i, p in zip(order, probs):
            outs[i].append(p)
    torch.cuda.synchronize()
    return outs


def test_480p_position_independence(network):
    """4 distinct clips (1, 2, 3, 5 objects) in two orders, and 4 copies of one clip: per-clip outputs bit-identical"""
    clips = _clips_480p([1, 2, 3, 5], 7, [11, 12, 13, 14])
    a = _run_batched(network, clips, [0, 1, 2, 3])
    b = _run_batched(network, clips, [3, 1, 0, 2])
    for i in range(4):
        for t, (x, y) in enumerate(zip(a[i], b[i])):
            assert torch.equal(x, y), (i, t, (x - y).abs().max().item())
    copies = [clips[2]] * 4
    c = _run_batched(network, copies, [0, 1, 2, 3])
    for i in range(1, 4):
        for t, (x, y) in enumerate(zip(c[0], c[i])):
            assert torch.equal(x, y), (i, t, (x - y).abs().max().item())


def test_480p_stage_parity(network):
    """batched key encoder + key projection at B = 4 and the ragged batched decoder against the same stages per clip
    (lock-step stage bound 2e-4 relative: batching changes the kernel choice, not the arithmetic's accuracy)"""
    from deva.utils.tensor_utils import pad_divide_by
    g = network.graph()
    imgs = [pad_divide_by(synth.FrameStream(H480, W480, seed=20 + i).next().to(dev()), 16)[0].unsqueeze(0) for i in range(4)]
    batch = torch.cat(imgs, 0)
    ms_b, feat_b = g.encode_image(batch)
    key_b, shr_b, sel_b = g.transform_key(feat_b, True, True)
    per = []
    for i, img in enumerate(imgs):
        ms, feat = network.encode_image(img)
        key, shr, sel = network.transform_key(feat)
        per.append((ms, key))
        for name, x, y in (('f16', ms_b[0][i], ms[0][0]), ('f8', ms_b[1][i], ms[1][0]), ('f4', ms_b[2][i], ms[2][0]),
                           ('key', key_b[i], key[0]), ('shrinkage', shr_b[i], shr[0]), ('selection', sel_b[i], sel[0])):
            assert rel_err(x, y) <= 2e-4, (name, i, rel_err(x, y))
    # ragged decoder: objects 2, 1, 3, 1 of clips 0..3
    n_objs = [2, 1, 3, 1]
    clip = [p for p, n in enumerate(n_objs) for _ in range(n)]
    no, h, w = len(clip), imgs[0].shape[-2] // 16, imgs[0].shape[-1] // 16
    gen = torch.Generator().manual_seed(3)
    readout = torch.randn(no, network.value_dim, h, w, generator=gen).to(dev())
    sensory = torch.randn(no, network.value_dim, h, w, generator=gen).to(dev()) * 0.5
    last16 = torch.rand(no, 1, h, w, generator=gen).to(dev())
    f16 = ms_b[0]
    d8, d4 = g.decoder_skips(ms_b[1], ms_b[2])
    sens_b, logits_b = g.decode(f16, d8, d4, readout, sensory, last16, True, clip=clip)
    at = 0
    for p, n in enumerate(n_objs):
        ms = per[p][0]
        s, lg = g.decode(ms[0], *g.decoder_skips(ms[1], ms[2]), readout[at:at + n].contiguous(),
                         sensory[at:at + n].contiguous(), last16[at:at + n].contiguous(), True)
        assert rel_err(logits_b[at:at + n], lg) <= 2e-4, ('logits', p, rel_err(logits_b[at:at + n], lg))
        assert rel_err(sens_b[at:at + n], s) <= 2e-4, ('sensory', p, rel_err(sens_b[at:at + n], s))
        at += n


def _one_small_frame(network, no):
    """one 64 x 96 frame (a 4 x 6 map at 1/16) and random per-object decoder / value-encoder inputs for `no` objects"""
    H, W = 64, 96
    img = synth.FrameStream(H, W, seed=40).next().to(dev()).unsqueeze(0)
    ms, _ = network.encode_image(img)
    gen = torch.Generator().manual_seed(4)
    readout = torch.randn(no, network.value_dim, H // 16, W // 16, generator=gen).to(dev())
    sensory = torch.randn(no, network.value_dim, H // 16, W // 16, generator=gen).to(dev()) * 0.5
    masks = torch.rand(no, H, W, generator=gen).to(dev())
    return img, ms, readout, sensory, masks


def test_plain_graph_call_equals_a_batch_of_one_clip(network):
    """`CompiledGraph.decode` / `encode_mask` have one body: called plainly with 3 objects (split convolutions, broadcast
    up-sampling) and as a batch of one clip (`clip=[0, 0, 0]`: the split whatever the count, mapped up-sampling) they
    launch the same arithmetic -- logits, sensory and value bit for bit"""
    from deva.hip import ops
    g = network.graph()
    img, ms, readout, sensory, masks = _one_small_frame(network, 3)
    last16 = ops.area_downsample(masks, 16).unsqueeze(1)
    d8, d4 = g.decoder_skips(ms[1], ms[2])
    for update in (True, False):
        s_a, lg_a = g.decode(ms[0], d8, d4, readout, sensory, last16, update)
        s_b, lg_b = g.decode(ms[0], d8, d4, readout, sensory, last16, update, clip=[0, 0, 0])
        assert torch.equal(lg_a, lg_b) and torch.equal(s_a, s_b), update
    v_a, n_a = g.encode_mask(img, ms[0], sensory, masks.unsqueeze(1), True)
    v_b, n_b = g.encode_mask(img, ms[0], sensory, masks.unsqueeze(1), True, clip=[0, 0, 0])
    assert torch.equal(v_a, v_b) and torch.equal(n_a, n_b)


def test_plain_graph_call_with_one_object_is_segment(network):
    """the single-launch rule: one object runs the fusers' first convolutions as ONE two-source launch, in the plain
    graph call as in `DEVA.segment` / `DEVA.encode_mask` on the same inputs -- bit for bit"""
    from deva.hip import ops
    g = network.graph()
    img, ms, readout, sensory, masks = _one_small_frame(network, 1)
    s, lg = g.decode(ms[0], *g.decoder_skips(ms[1], ms[2]), readout, sensory, ops.area_downsample(masks, 16).unsqueeze(1), True)
    sens, logits, prob = network.segment(ms, readout.unsqueeze(0), sensory.unsqueeze(0), masks.unsqueeze(0))
    want_logits, want_prob = network.soft_aggregate(lg[:, 0])
    assert torch.equal(sens[0], s) and torch.equal(logits[0], want_logits) and torch.equal(prob[0], want_prob)
    v, n = g.encode_mask(img, ms[0], sensory, masks.unsqueeze(1), True)
    value, new_h = network.encode_mask(img, ms, sensory.unsqueeze(0), masks.unsqueeze(0))
    assert torch.equal(value[0], v) and torch.equal(new_h[0], n)


def test_480p_single_clip_bit_identical_to_step(network):
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.multi_clip import step_clips
    clip = _clips_480p([2], 4, [30])[0]
    cfg = synth.base_config(mem_every=2)
    a, b = DEVAInferenceCore(network, cfg), DEVAInferenceCore(network, cfg)
    for t, img in enumerate(clip['frames']):
        m, objs = (clip['mask'], [1, 2]) if t == 0 else (None, None)
        pa = step_clips([a], [img], [m], [objs])[0]
        pb = b.step(img, m, objs)
        assert torch.equal(pa, pb), t
