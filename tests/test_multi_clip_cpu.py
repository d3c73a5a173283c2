"""`deva.inference.multi_clip.step_clips` on the CPU (emulated ops): several clips stepped through one batched network
pass are held to what each clip gives alone -- the reference's golden outputs of the four E2E scenarios stepped
together, the B = 1 identity with `core.step`, the argument errors, and plain `step` calls mixed in between."""
import json
import os

import numpy as np
import pytest
import torch

import emu_ops
import scenarios
from workload import synth

torch.set_grad_enabled(False)


def upsample2x_add_map(x, skip, skip_index):
    """contract of deva_upsample2x_add_map: item b is the broadcast op with skip[skip_index[b]]"""
    return emu_ops.upsample2x_add(x, skip[skip_index.long()])


def upsample2x_add_ds2_map(x, skip, skip_index):
    return upsample2x_add_map(x, skip, skip_index), emu_ops.area_downsample(x, 2)


def conv2d_per_item(pc, x0, x1=None, *, residual=None, out=None, **kw):
    """the convolution contract evaluated one batch item at a time.  A CPU convolution library may round a batch of B
    differently from B batches of one (its blocking follows the batch size, the thread count and the instruction set);
    the HIP kernels do not (tests/test_gpu_j_multi_clip.py: position independence).  With the per-item form a batched
    clip here sees the same arithmetic as the clip stepped alone, so the free-running comparisons below test the host
    orchestration and not the top-k near-ties that one rounding difference moves."""
    batch = max(x0.shape[0], 1 if x1 is None else x1.shape[0], 1 if residual is None else residual.shape[0])
    if batch == 1:
        return emu_ops.conv2d(pc, x0, x1, residual=residual, out=out, **kw)

    def item(t, i):
        return None if t is None else (t if t.shape[0] == 1 else t[i:i + 1])

    y = torch.cat([emu_ops.conv2d(pc, item(x0, i), item(x1, i), residual=item(residual, i), **kw) for i in range(batch)])
    if out is not None:
        out.copy_(y)
        return out
    return y


@pytest.fixture()
def emu(monkeypatch):
    from deva.hip import ops
    emu_ops.install(monkeypatch)
    monkeypatch.setattr(ops, 'conv2d', conv2d_per_item)
    monkeypatch.setattr(ops, 'upsample2x_add_map', upsample2x_add_map)
    monkeypatch.setattr(ops, 'upsample2x_add_ds2_map', upsample2x_add_ds2_map)


def _network(recipe_state_dict):
    from deva.model.network import DEVA
    sd, _ = recipe_state_dict
    net = DEVA(synth.base_config())
    net.load_weights(sd)
    return net


class _Feed:
    """the per-frame `step` arguments of a tests/scenarios.py E2E scenario (as run_scenario issues them)"""

    def __init__(self, sc):
        self.sc = sc
        self.stream = synth.FrameStream(sc['H'], sc['W'], seed=1)
        self.mask0 = synth.box_mask(sc['H'], sc['W'], sc['nobj'])

    def next(self, t):
        sc = self.sc
        img = self.stream.next()
        end = t == sc['frames'] - 1
        if t == 0:
            return img, self.mask0, list(range(1, sc['nobj'] + 1)), end
        if sc['second'] is not None and t == sc['second'][0]:
            oid = sc['second'][1]
            m = torch.zeros(sc['H'], sc['W'], dtype=torch.long)
            m[sc['H'] // 2:, :sc['W'] // 4] = oid
            return img, m, [oid], end
        return img, None, None, end


def _run_together(net, names):
    """every named scenario in one `step_clips` call per frame; a clip leaves the batch after its last frame"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.multi_clip import step_clips
    scs = [scenarios.E2E[n] for n in names]
    cores = [DEVAInferenceCore(net, synth.base_config(**sc['cfg'])) for sc in scs]
    feeds = [_Feed(sc) for sc in scs]
    outs = [[] for _ in names]
    batch_sizes = []
    for t in range(max(sc['frames'] for sc in scs)):
        live = [i for i, sc in enumerate(scs) if t < sc['frames']]
        args = [feeds[i].next(t) for i in live]
        probs = step_clips([cores[i] for i in live], [a[0] for a in args], [a[1] for a in args], [a[2] for a in args],
                           end=[a[3] for a in args])
        batch_sizes.append(len(live))
        for i, p in zip(live, probs):
            outs[i].append(p.float())
    return outs, cores, batch_sizes


def _check_against_golden(golden_dir, name, outs, core):
    """what test_e2e_matches_reference asserts for the clip alone"""
    g = np.load(os.path.join(golden_dir, f'e2e_{name}.npz'))
    assert [p.shape[0] for p in outs] == g['nchan'].tolist(), name
    sizes = json.loads(str(g['sizes']))
    mem = core.memory
    assert {str(b): mem.work_mem.size(b) for b in mem.work_mem.buckets} == sizes['work'], name
    if mem.use_long_term:
        assert {str(b): mem.long_mem.size(b) for b in mem.long_mem.buckets} == sizes['long'], name
    worst = max(np.abs(p[:, ::2, ::2].numpy() - g[f'prob_sub_{t}']).max() for t, p in enumerate(outs))
    assert worst <= 2e-3, (name, worst)


def test_e2e_clips_stepped_together_match_reference(emu, golden_dir, recipe_state_dict):
    """lt_evict / two_buckets (96x128, one batched group), no_lt (100x150) and five_obj (90x130): different sizes,
    configs, lengths (45 / 30 / 12 / 9 frames: the batch shrinks) and a second annotation at frame 7 of two_buckets"""
    names = list(scenarios.E2E)
    net = _network(recipe_state_dict)
    outs, cores, batch_sizes = _run_together(net, names)
    assert batch_sizes[0] == 4 and batch_sizes[-1] == 1
    for name, o, core in zip(names, outs, cores):
        _check_against_golden(golden_dir, name, o, core)


def test_single_clip_is_core_step(emu, recipe_state_dict):
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.multi_clip import step_clips
    net = _network(recipe_state_dict)
    sc = scenarios.E2E['no_lt']
    cfg = synth.base_config(**sc['cfg'])
    a, b = DEVAInferenceCore(net, cfg), DEVAInferenceCore(net, cfg)
    fa, fb = _Feed(sc), _Feed(sc)
    for t in range(4):  # (frame 3 commits a memory frame: mem_every=3)
        img, m, objs, end = fa.next(t)
        pa = step_clips([a], [img], [m], [objs], end=[end])[0]
        pb = b.step(*fb.next(t)[:3], end=end)
        assert torch.equal(pa, pb)
    assert a.last_mem_ti == b.last_mem_ti and a.memory.work_mem.size(0) == b.memory.work_mem.size(0)


def test_argument_errors(emu, recipe_state_dict):
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.multi_clip import step_clips
    cfg = synth.base_config()
    net1, net2 = _network(recipe_state_dict), _network(recipe_state_dict)
    img = torch.zeros(3, 32, 32)
    with pytest.raises(ValueError):
        step_clips([DEVAInferenceCore(net1, cfg), DEVAInferenceCore(net2, cfg)], [img, img])
    sharded = DEVAInferenceCore(net1, cfg)
    sharded.memory._shard_group = object()  # what shard_queries / shard_bank set (they need a process group)
    with pytest.raises(NotImplementedError):
        step_clips([DEVAInferenceCore(net1, cfg), sharded], [img, img])


def test_plain_step_between_batched_calls(emu, recipe_state_dict):
    """two clips of one size (a real batched group; B gets a second annotation at frame 7): frames 0-3 batched, frame 4
    of clip A by plain `step` (clip B batched alone), frames 5-8 batched again -- outputs and state of both clips against
    each clip's own `step` loop"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.multi_clip import step_clips
    net = _network(recipe_state_dict)
    scs = [dict(scenarios.E2E['lt_evict'], frames=9), dict(scenarios.E2E['two_buckets'], frames=9)]
    a, b = (DEVAInferenceCore(net, synth.base_config(**sc['cfg'])) for sc in scs)
    fa, fb = (_Feed(sc) for sc in scs)
    outs = ([], [])
    for t in range(9):
        xa, xb = fa.next(t), fb.next(t)
        if t == 4:
            outs[0].append(a.step(*xa[:3], end=xa[3]))
            outs[1].append(step_clips([b], [xb[0]], [xb[1]], [xb[2]], end=[xb[3]])[0])
        else:
            for o, p in zip(outs, step_clips([a, b], [xa[0], xb[0]], [xa[1], xb[1]], [xa[2], xb[2]], end=[xa[3], xb[3]])):
                o.append(p)
    for sc, got, core in zip(scs, outs, (a, b)):
        ref, ref_core = scenarios.run_scenario(lambda cfg: DEVAInferenceCore(net, cfg), sc)
        assert [p.shape for p in got] == [p.shape for p in ref]
        assert max((p - r).abs().max().item() for p, r in zip(got, ref)) <= 1e-4
        assert core.curr_ti == ref_core.curr_ti and core.last_mem_ti == ref_core.last_mem_ti
        mem, ref_mem = core.memory, ref_core.memory
        assert mem.work_mem.buckets == ref_mem.work_mem.buckets
        assert {k: mem.work_mem.size(k) for k in mem.work_mem.buckets} == \
            {k: ref_mem.work_mem.size(k) for k in ref_mem.work_mem.buckets}
        assert sorted(mem.sensory) == sorted(ref_mem.sensory)
        for obj in ref_mem.sensory:
            assert (mem.sensory[obj] - ref_mem.sensory[obj]).abs().max().item() <= 1e-4
        assert len(core.image_feature_store) == 0
