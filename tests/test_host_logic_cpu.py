"""Host-side logic of the package on the CPU: the HIP ops are replaced by the PyTorch emulation of
tests/emu_ops.py, so these tests check weight packing / BN folding, graph wiring, the arena-based
memory stores and the frame state machine against the oracle and the reference's golden vectors.
The kernels themselves are tested on the GPU (tests/test_gpu_*.py)."""
import json
import os

import numpy as np
import pytest
import torch

import emu_ops
import scenarios
from oracle import deva_oracle as O
from workload import synth

torch.set_grad_enabled(False)


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)


def _network(recipe_state_dict):
    from deva.model.network import DEVA
    sd, _ = recipe_state_dict
    net = DEVA(synth.base_config())
    net.load_weights(sd)
    return net


def test_state_dict_is_checkpoint_compatible(recipe_state_dict):
    from deva.model.network import DEVA
    _, spec = recipe_state_dict
    mine = {k: (list(v.shape), str(v.dtype).replace('torch.', '')) for k, v in DEVA(synth.base_config()).state_dict().items()}
    ref = {k: (s, d) for k, s, d in spec['tensors']}
    assert mine == ref


def test_stages_match_reference(emu, golden_dir, recipe_state_dict):
    net = _network(recipe_state_dict)
    g = torch.load(os.path.join(golden_dir, 'stages_96x128.pt'))
    H, W, no = 96, 128, 2
    img = synth.FrameStream(H, W, seed=5).next().unsqueeze(0)
    ms, feat = net.encode_image(img)
    key, shr, sel = net.transform_key(feat)
    masks, sensory, readout = synth.stage_inputs(H, W, no)
    value, sens_deep = net.encode_mask(img, ms, sensory, masks)
    sens_seg, logits, prob = net.segment(ms, readout, sensory, masks)
    got = dict(f16=ms[0], f8=ms[1], f4=ms[2], feat=feat, key=key, shrinkage=shr, selection=sel,
               value=value, sensory_deep=sens_deep, sensory_seg=sens_seg, logits=logits, prob=prob)
    for k, v in got.items():
        assert v.shape == g[k].shape, k
        err = (v - g[k]).abs().max().item()
        assert err <= 2e-4 * max(1.0, g[k].abs().max().item()), (k, err)


def test_chunked_objects_equal_joint(emu, recipe_state_dict):
    net = _network(recipe_state_dict)
    H, W, no = 64, 96, 3
    img = synth.FrameStream(H, W, seed=6).next().unsqueeze(0)
    ms, feat = net.encode_image(img)
    masks, sensory, readout = synth.stage_inputs(H, W, no)
    a = net.segment(ms, readout, sensory, masks)
    b = net.segment(ms, readout, sensory, masks, chunk_size=2)
    for x, y in zip(a, b):
        assert torch.allclose(x, y, atol=1e-5)
    va, sa = net.encode_mask(img, ms, sensory, masks)
    vb, sb = net.encode_mask(img, ms, sensory, masks, chunk_size=1)
    assert torch.allclose(va, vb, atol=1e-5) and torch.allclose(sa, sb, atol=1e-5)


@pytest.mark.parametrize('name', list(scenarios.E2E))
def test_e2e_matches_reference(emu, golden_dir, recipe_state_dict, name):
    from deva.inference.inference_core import DEVAInferenceCore
    net = _network(recipe_state_dict)
    sc = scenarios.E2E[name]
    outs, core = scenarios.run_scenario(lambda cfg: DEVAInferenceCore(net, cfg), sc)
    g = np.load(os.path.join(golden_dir, f'e2e_{name}.npz'))
    assert [p.shape[0] for p in outs] == g['nchan'].tolist()
    sizes = json.loads(str(g['sizes']))
    mem = core.memory
    assert {str(b): mem.work_mem.size(b) for b in mem.work_mem.buckets} == sizes['work']
    if mem.use_long_term:
        assert {str(b): mem.long_mem.size(b) for b in mem.long_mem.buckets} == sizes['long']
    worst = max(np.abs(p[:, ::2, ::2].numpy() - g[f'prob_sub_{t}']).max() for t, p in enumerate(outs))
    assert worst <= 2e-3, (name, worst)


def test_lockstep_teacher_forced_small(emu, recipe_state_dict):
    import lockstep
    net = _network(recipe_state_dict)
    P, _ = recipe_state_dict
    worst = lockstep.run(net, P, 96, 128, 2, 6, torch.device('cpu'))
    assert max(worst.values()) <= 2e-4, worst


@pytest.mark.parametrize('name', ['lt_evict', 'two_buckets'])
def test_memory_events_teacher_forced(emu, recipe_state_dict, name):
    """host logic of consolidation / eviction / usage on the oracle's inputs (tests/memory_audit.py); the
    same audit runs on the HIP kernels in tests/test_gpu_f_memory_events.py"""
    import memory_audit
    P, _ = recipe_state_dict
    report = memory_audit.teacher_forced_memory(P, scenarios.E2E[name], torch.device('cpu'))
    assert report['consolidations'] == 3 and report['evictions'] == (1 if name == 'lt_evict' else 0)
    assert report['tie_swapped_queries'] == 0


def test_store_views_follow_reference_layout(emu):
    from deva.inference.kv_memory_store import KeyValueMemoryStore
    st = KeyValueMemoryStore(save_selection=True, save_usage=True)
    g = torch.Generator().manual_seed(0)
    k1, s1, e1 = torch.randn(64, 10, generator=g), torch.rand(1, 10, generator=g), torch.rand(64, 10, generator=g)
    v1 = {3: torch.randn(8, 10, generator=g), 7: torch.randn(8, 10, generator=g)}
    st.add(k1, v1, s1, e1)
    k2, s2, e2 = torch.randn(64, 6, generator=g), torch.rand(1, 6, generator=g), torch.rand(64, 6, generator=g)
    v2 = {3: torch.randn(8, 6, generator=g), 7: torch.randn(8, 6, generator=g), 9: torch.randn(8, 6, generator=g)}
    st.add(k2, v2, s2, e2)
    assert st.buckets == {0: [3, 7], 1: [9]}
    assert torch.equal(st.key[0], torch.cat([k1, k2], 1)) and torch.equal(st.key[1], k2)
    assert torch.equal(st.value[7], torch.cat([v1[7], v2[7]], 1)) and torch.equal(st.value[9], v2[9])
    assert torch.equal(st.shrinkage[0], torch.cat([s1, s2], 1))
    assert torch.equal(st.selection[1], e2)
    st.sieve_by_range(0, 2, -4, min_size=3)
    keep = list(range(0, 2)) + list(range(12, 16))
    assert torch.equal(st.key[0], torch.cat([k1, k2], 1)[:, keep])
    assert torch.equal(st.value[3], torch.cat([v1[3], v2[3]], 1)[:, keep])
    st.purge_except([9])
    assert st.buckets == {1: [9]} and st.num_objects == 1 and not st.engaged(0)


def test_no_cpu_fallback_in_product(recipe_state_dict):
    """without the emulation the package must refuse to run on the CPU (no silent fallback)"""
    from deva.hip import DevaHipError
    net = _network(recipe_state_dict)
    with pytest.raises(DevaHipError):
        net.encode_image(torch.zeros(1, 3, 32, 32))


def _manager_state(om):
    return dict(ids=[int(o.id) for o in om.obj_to_tmp_id], tmp=[int(t) for t in om.obj_to_tmp_id.values()],
                poke=[int(o.poke_count) for o in om.obj_to_tmp_id],
                cats=[[None if c is None else int(c) for c in o.category_ids] for o in om.obj_to_tmp_id],
                isthing=[o.isthing for o in om.obj_to_tmp_id])


def test_match_and_merge_matches_reference(emu, golden_dir):
    """segment_merging.match_and_merge: same merged masks and the same object-manager side effects
    as the reference (goldens generated by the reference itself)"""
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    from deva.inference.segment_merging import match_and_merge
    gold = torch.load(os.path.join(golden_dir, 'merge_cases.pt'))
    for seed in (0, 1):
        for incremental in (False, True):
            ours, our_info, news, new_info = scenarios.merge_case(seed)
            om = ObjectManager()
            om.add_new_objects([ObjectInfo(**i) for i in our_info])
            merged = match_and_merge(ours, news, om, [ObjectInfo(**i) for i in new_info],
                                     incremental_mode=incremental)
            g = gold[f'seed{seed}_inc{int(incremental)}']
            assert torch.equal(merged.to(torch.uint8), g['onehot'])
            assert _manager_state(om) == g['state']


def test_detection_clip_matches_reference(emu, golden_dir, recipe_state_dict):
    """incorporate_detection + propagation (online setting) against the reference's outputs"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.object_info import ObjectInfo
    net = _network(recipe_state_dict)
    outs, core = scenarios.run_detection_scenario(lambda cfg: DEVAInferenceCore(net, cfg), ObjectInfo,
                                                  scenarios.DETECTION)
    g = np.load(os.path.join(golden_dir, 'e2e_detections.npz'))
    assert [p.shape[0] for p in outs] == g['nchan'].tolist()
    assert _manager_state(core.object_manager) == json.loads(str(g['state']))
    worst = max(np.abs(p[:, ::2, ::2].numpy() - g[f'prob_sub_{t}']).max() for t, p in enumerate(outs))
    assert worst <= 5e-3, worst


def _check_consistent_clip(outs, core, g, tol):
    assert [p.shape[0] for p in outs] == g['nchan'].tolist()
    assert scenarios.manager_state(core.object_manager) == json.loads(str(g['state']))
    sizes = json.loads(str(g['sizes']))
    mem = core.memory
    assert {str(b): mem.work_mem.size(b) for b in mem.work_mem.buckets} == sizes['work']
    assert {str(b): mem.long_mem.size(b) for b in mem.long_mem.buckets} == sizes['long']
    every = scenarios.CONSISTENT['every']
    # detection frames return the +-16 logits of the merged HARD masks (inference_core.py:192): they are compared as
    # masks; once a merged mask differs at a forward-argmax near-tie the memory frames differ and only the object
    # table / bank sizes above remain comparable
    diverged = None
    for t, p in enumerate(outs):
        ref = g[f'prob_sub_{t}']
        if t % every == 0:
            differ = float((p[:, ::2, ::2].numpy().argmax(0) != ref.argmax(0)).mean())
            assert differ <= 2e-3 or diverged is not None, (t, differ)
            if differ and diverged is None:
                diverged = t
        elif diverged is None:
            assert np.abs(p[:, ::2, ::2].numpy() - ref).max() <= tol, t
    assert diverged is None or diverged >= 3


@pytest.mark.parametrize('mode', ['replay', 'record'])
def test_consistent_detection_clip_matches_reference(emu, golden_dir, recipe_state_dict, mode):
    """BASELINE configs[2]'s merge / purge / multi-bucket path (workload/detections.py) against the
    reference's own run: replaying the reference's detections through the public interface, and generating
    them from this run's forward masks through the recording hook (they must come out identical)"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.object_info import ObjectInfo
    from workload import detections
    net = _network(recipe_state_dict)
    g, golden_dets = scenarios.load_consistent_golden(golden_dir)
    holder = {}

    def make(cfg):
        holder['core'] = DEVAInferenceCore(net, cfg)
        return holder['core']

    if mode == 'replay':
        outs, core, _ = scenarios.run_consistent_detection_scenario(make, ObjectInfo, scenarios.CONSISTENT,
                                                                    replay=golden_dets)
    else:
        outs, core, recorded = scenarios.run_consistent_detection_scenario(
            make, ObjectInfo, scenarios.CONSISTENT,
            record=lambda det, rec, frame_of: detections.record_on_package(holder['core'], det, ObjectInfo, rec, frame_of))
        for t, (m, info) in recorded.items():
            assert [i['id'] for i in info] == [i['id'] for i in golden_dets[t][1]], t
            if t <= 6:
                # the emulated ops differ from the reference in the last bits: a few boundary pixels may move (and
                # once a merged hard mask differs, at frame 6, the forward masks the detector sees drift apart)
                assert (m != golden_dets[t][0]).float().mean().item() <= 2e-3, t
    _check_consistent_clip(outs, core, g, 1e-3)


def test_e2e_peaky_matches_reference(emu, golden_dir, peaky_state_dict):
    """with the peaky recipe the north-star bound holds as written on the emulated ops: 1e-3 max-abs"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    net = DEVA(synth.base_config())
    net.load_weights(peaky_state_dict)
    outs, core = scenarios.run_scenario(lambda cfg: DEVAInferenceCore(net, cfg), scenarios.E2E_PEAKY['peaky'])
    g = np.load(os.path.join(golden_dir, 'e2e_peaky.npz'))
    worst = max(np.abs(p[:, ::2, ::2].numpy() - g[f'prob_sub_{t}']).max() for t, p in enumerate(outs))
    assert worst <= 1e-3, worst


def test_spatial_alignment_matches_reference(emu, golden_dir, recipe_state_dict):
    """semi-online voting: the fused one-frame memory read behind
    `spatial_alignment` against the reference's output"""
    from deva.inference.consensus_associated import spatial_alignment
    from deva.inference.image_feature_store import ImageFeatureStore
    net = _network(recipe_state_dict)
    g = torch.load(os.path.join(golden_dir, 'alignment.pt'))
    frames, masks = scenarios.alignment_inputs(scenarios.ALIGNMENT)
    store = ImageFeatureStore(net, no_warning=True)
    out = spatial_alignment(0, frames[0], masks[0], 1, frames[1], net, store, synth.base_config())
    assert out.shape == g['aligned'].shape
    assert (out - g['aligned']).abs().max().item() <= 1e-3


def test_consensus_auto_association_matches_reference(emu, golden_dir, recipe_state_dict):
    """semi-online voting with inferred association (second half): the pairwise-IoU table
    from one joint label histogram per frame pair, the greedy matching, the exact 0/1 selection and the
    painting against the reference's find_consensus_auto_association (tests/golden/consensus_auto.pt)"""
    from deva.inference.image_feature_store import ImageFeatureStore
    from deva.inference.object_info import ObjectInfo
    net = _network(recipe_state_dict)
    got = scenarios.run_consensus_cases(net, lambda: ImageFeatureStore(net, no_warning=True), lambda **kw: ObjectInfo(**kw))
    scenarios.check_consensus_cases(got, torch.load(os.path.join(golden_dir, 'consensus_auto.pt')))


def test_consensus_exact_solver_is_optimal():
    """solve_exact against brute force over all 2^n selections on random conflict graphs"""
    import itertools
    import numpy as np
    from deva.inference.consensus_automatic import solve_exact
    rs = np.random.RandomState(0)
    for n in (1, 4, 7, 10):
        for _ in range(5):
            iou = np.zeros((n, n), dtype=np.float32)
            for i in range(n):
                for j in range(i + 1, n):
                    if rs.rand() < 0.3:
                        iou[i, j] = iou[j, i] = 0.5 + 0.5 * rs.rand()
            ind = iou > 0.49
            w = iou.sum(0) * 2 - 1
            best = max((sum(w[i] for i in s), s) for r in range(n + 1) for s in itertools.combinations(range(n), r)
                       if not any(ind[a, b] for a in s for b in s if a < b))
            got = solve_exact(iou, ind, n)
            assert not any(ind[a, b] for a in range(n) for b in range(a + 1, n) if got[a] and got[b])
            assert abs(sum(w[i] for i in range(n) if got[i]) - best[0]) <= 1e-5


def test_established_association_consensus_matches_reference(emu, golden_dir, recipe_state_dict):
    """find_consensus_with_established_association (keyframe choice + score-weighted projections) against the
    reference's keyframe and consensus of the same three-frame window (tests/golden/alignment.pt)"""
    from deva.inference.consensus_associated import find_consensus_with_established_association
    from deva.inference.image_feature_store import ImageFeatureStore
    net = _network(recipe_state_dict)
    g = torch.load(os.path.join(golden_dir, 'alignment.pt'))
    frames, masks = scenarios.alignment_inputs(scenarios.ALIGNMENT)
    store = ImageFeatureStore(net, no_warning=True)
    key_ti, consensus = find_consensus_with_established_association(
        [0, 1, 2], [f.clone() for f in frames], [m.clone() for m in masks], net, store, synth.base_config())
    assert int(key_ti) == g['keyframe']
    assert (consensus - g['consensus']).abs().max().item() <= 1e-3
    # explicit scores pick the best-scored frame as the keyframe
    key_ti, _ = find_consensus_with_established_association(
        [0, 1, 2], [f.clone() for f in frames], [m.clone() for m in masks], net, ImageFeatureStore(net, no_warning=True),
        synth.base_config(), scores=[0.1, 0.9, 0.3])
    assert int(key_ti) == 1


def test_api_surface_matches_reference(golden_dir):
    """drop-in boundary: every public method / property of the reference's classes on
    the path exists here with the same parameter names, kinds and defaults (read off the reference with
    inspect by tests/golden/make_golden.py)"""
    import inspect
    from deva.inference.image_feature_store import ImageFeatureStore
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.kv_memory_store import KeyValueMemoryStore
    from deva.inference.memory_manager import MemoryManager
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    from deva.model.network import DEVA
    with open(os.path.join(golden_dir, 'api_surface.json')) as f:
        ref = json.load(f)
    mine = {c.__name__: c for c in (DEVA, DEVAInferenceCore, MemoryManager, KeyValueMemoryStore, ObjectManager,
                                    ObjectInfo, ImageFeatureStore)}
    problems = []
    # command-line flags the unchanged drivers parse (names, defaults, types, switches)
    from argparse import ArgumentParser
    from deva.inference.eval_args import add_common_eval_args
    parser = ArgumentParser()
    add_common_eval_args(parser)
    got_args = {a.dest: dict(flags=a.option_strings, default=a.default, nargs=a.nargs,
                             type=None if a.type is None else a.type.__name__,
                             switch=type(a).__name__ == '_StoreTrueAction')
                for a in parser._actions if a.dest != 'help'}
    # flags this package adds on top of the reference's surface (the drivers never pass them)
    for extension in ('f16_split', 'f16_split_key_encoder', 'no_winograd'):
        ext = got_args.pop(extension)
        assert ext['switch'] and ext['default'] is False
    assert got_args == ref.pop('eval_args')
    for cname, spec in ref.items():
        cls = mine[cname]
        for prop in spec['properties']:
            if not isinstance(inspect.getattr_static(cls, prop, None), property):
                problems.append(f'{cname}.{prop}: property missing')
        for mname, params in spec['methods'].items():
            fn = inspect.getattr_static(cls, mname, None)
            if fn is None:
                problems.append(f'{cname}.{mname}: missing')
                continue
            sig = inspect.signature(getattr(cls, mname))
            got = [[p.name, str(p.kind), None if p.default is inspect._empty else repr(p.default)]
                   for p in sig.parameters.values()]
            # extra keyword-only parameters with defaults are allowed (e.g. token_major=False)
            core = [g for g in got if not (g[1] == 'KEYWORD_ONLY' and g[2] is not None and g[0] not in [p[0] for p in params])]
            if core != params:
                problems.append(f'{cname}.{mname}: {core} != {params}')
    assert not problems, '\\n'.join(problems)


def _check_edge_cases(got, g, tol):
    assert got.keys() == g.keys()
    for k in g:
        assert got[k].shape == g[k].shape, k
        assert (got[k].float() - g[k].float()).abs().max().item() <= tol * max(1.0, g[k].float().abs().max().item()), k


def test_edge_paths_match_reference(emu, golden_dir, recipe_state_dict):
    """warnings instead of exceptions, soft-mask annotation, feature-cache control, a detection round
    without segments: same observable behaviour as the reference (tests/scenarios.py:run_edge_cases)"""
    from deva.inference.inference_core import DEVAInferenceCore
    net = _network(recipe_state_dict)
    from deva.inference.object_info import ObjectInfo
    got = scenarios.run_edge_cases(lambda cfg: DEVAInferenceCore(net, cfg), make_info=ObjectInfo)
    _check_edge_cases(got, torch.load(os.path.join(golden_dir, 'edge_cases.pt')), 1e-3)


def test_soft_annotation_on_engaged_memory_and_top_k_validation(emu, recipe_state_dict):
    """(a) an incomplete SOFT annotation while objects are already tracked -- the path the reference
    crashes on (TypeError in inference_core.py:255) -- blends by values and by annotation position;
    (b) an unsupported top_k is rejected when the memory is configured, not at the first read mid-clip"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.memory_manager import MemoryManager
    net = _network(recipe_state_dict)
    core = DEVAInferenceCore(net, synth.base_config(mem_every=2))
    stream = synth.FrameStream(96, 128, seed=3)
    core.step(stream.next(), synth.box_mask(96, 128, 2), [1, 2])
    core.step(stream.next())
    soft = torch.zeros(1, 96, 128)
    soft[0, 60:90, 10:40] = 0.9
    prob = core.step(stream.next(), soft, [7], hard_mask=False)
    assert tuple(prob.shape) == (4, 96, 128) and core.object_manager.all_obj_ids == [1, 2, 7]
    assert (prob[3, 60:90, 10:40] > 0.5).all() and (prob[1:3, 60:90, 10:40] < 0.5).all()
    assert core.step(stream.next()).shape[0] == 4
    with pytest.raises(ValueError, match='top_k'):
        MemoryManager(synth.base_config(top_k=65))
    assert MemoryManager(synth.base_config(top_k=64)).top_k == 64  # 33..64: the dense read kernel
    with pytest.raises(ValueError, match='shard_bank: top_k=48'):  # ... which has no per-shard hand-over format
        MemoryManager(synth.base_config(top_k=48)).shard_bank()
    with pytest.raises(ValueError, match='top_k'):
        core.memory.update_config(synth.base_config(top_k=0, mem_every=2))


def test_prob_to_obj_cls_equals_the_drivers_tail(emu):
    """ObjectManager.prob_to_obj_cls == argmax -> tmp_to_obj_cls (and the resized variant)"""
    import torch.nn.functional as F
    from deva.inference.object_manager import ObjectManager
    om = ObjectManager()
    om.add_new_objects([7, 3, 12])
    g = torch.Generator().manual_seed(2)
    prob = torch.softmax(torch.randn(4, 30, 44, generator=g), dim=0)
    assert torch.equal(om.prob_to_obj_cls(prob), om.tmp_to_obj_cls(torch.argmax(prob, dim=0)))
    big = F.interpolate(prob.unsqueeze(1), (60, 90), mode='bilinear', align_corners=False)[:, 0]
    assert torch.equal(om.prob_to_obj_cls(prob, (60, 90)), om.tmp_to_obj_cls(torch.argmax(big, dim=0)))


def test_frame_to_network_input_shapes(emu, monkeypatch):
    """host side of the device input head: the readers' size rule (torchvision `Resize(size)`: shorter
    side == size exactly, longer side int(size * long / short); video_reader.py:139-144), the demo's rule
    (demo_utils.py:10-19) and the fused pad_divide_by"""
    import numpy as np
    from deva.utils import tensor_utils as TU
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    # known torchvision answers
    for (h, w), want in {(427, 640): (480, 719), (640, 427): (719, 480), (480, 854): (480, 854),
                         (720, 1280): (480, 853), (1080, 1920): (480, 853), (2160, 3840): (480, 853),
                         (352, 500): (480, 681), (358, 640): (480, 858)}.items():
        assert TU.network_input_size(h, w, 480) == want, (h, w)
    # sweep: the shorter side is always exactly `size` (it came out as size-1 for 214 values in 200..2200 before)
    for short in range(200, 2201):
        for long_ in (short, short + 1, int(short * 1.5), short * 16 // 9):
            oh, ow = TU.network_input_size(short, long_, 480)
            assert oh == 480 and ow == (long_ if short == 480 else int(480 * long_ / short)), (short, long_)
            assert TU.network_input_size(long_, short, 480) == (ow, oh)
    assert TU.network_input_size(427, 640, 480, antialias=False) == (479, 719)  # the demo truncates both sides
    assert TU.network_input_size(427, 640, -1) == (427, 640)
    rs = np.random.RandomState(0)
    frame = rs.randint(0, 256, (72, 128, 3), dtype=np.uint8)
    out = TU.frame_to_network_input(frame, 48)
    assert tuple(out.shape) == (3, 48, 85) and out.dtype == torch.float32
    assert tuple(TU.frame_to_network_input(frame).shape) == (3, 72, 128)
    # fused padding == pad_divide_by of the unpadded result, and step() then has nothing left to pad
    for shape, side in (((72, 128, 3), 48), ((50, 70, 3), -1), ((64, 96, 3), -1), ((427, 640, 3), 100)):
        frame = rs.randint(0, 256, shape, dtype=np.uint8)
        plain = TU.frame_to_network_input(frame, side)
        fused, pad = TU.frame_to_network_input(frame, side, pad_to=16)
        want, want_pad = TU.pad_divide_by(plain, 16)
        assert tuple(pad) == tuple(want_pad) and torch.equal(fused, want)
        again, no_pad = TU.pad_divide_by(fused, 16)
        assert no_pad == (0, 0, 0, 0) and again.data_ptr() == fused.data_ptr()
        assert torch.equal(TU.unpad(fused, pad), plain)


def test_read_memory_matches_reference(emu, golden_dir, recipe_state_dict):
    """DEVA.read_memory, the dense training-time read of the public module interface"""
    net = _network(recipe_state_dict)
    g = torch.load(os.path.join(golden_dir, 'read_memory.pt'))
    out = net.read_memory(**g['args'])
    assert out.shape == g['out'].shape
    assert (out - g['out']).abs().max().item() <= 1e-4 * max(1.0, g['out'].abs().max().item())


def test_conv_tile_order_is_a_permutation():
    """csrc/conv_epilogue.h: conv_tile_coords + csrc/conv_plan.h: conv_group_m, restated line by line: for every grid
    the workgroup -> (cout tile, pixel tile) map must hit every tile exactly once, whatever the group size leaves over"""
    def group_m(taps, stride, bm, bn, tiles):
        ratio = taps * bm / (bn * stride * stride)
        c = 48.0 if tiles >= 8 * 48 else float((tiles + 7) // 8)
        g = 1
        while (g + 1) * (g + 1) * ratio <= c * 1.5:
            g += 1
        return g

    def coords(b, nb, tiles_m, tiles_n, group):
        q, r, xcd = nb >> 3, nb & 7, b & 7
        logical = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (b >> 3)
        g = group if 0 < group < tiles_m else tiles_m
        per_group = g * tiles_n
        grp, in_grp = divmod(logical, per_group)
        m_first = grp * g
        gsz = min(g, tiles_m - m_first)
        tile_n = in_grp // gsz
        return m_first + (in_grp - tile_n * gsz), tile_n

    seen_groups = set()
    for tiles_m in (1, 2, 3, 4, 5, 7, 8, 12):
        for tiles_n in (1, 2, 13, 26, 64, 203, 1013):
            for taps, stride in ((1, 1), (9, 1), (9, 2), (49, 2)):
                for bm, bn in ((128, 128), (64, 64), (32, 128)):
                    nb = tiles_m * tiles_n
                    g = group_m(taps, stride, bm, bn, nb)
                    seen_groups.add(min(g, tiles_m))
                    got = sorted(coords(b, nb, tiles_m, tiles_n, g) for b in range(nb))
                    assert got == [(m, n) for m in range(tiles_m) for n in range(tiles_n)], (tiles_m, tiles_n, g)
    assert {1, 2, 3, 5, 8} <= seen_groups  # partial last groups (3 of 2, 5 of 3, ...) were among the cases
    # the two sizes the comments quote: 3x3 on 128x128 tiles -> 2 cout tiles per group, 1x1 -> 8
    assert group_m(9, 1, 128, 128, 768) == 2 and group_m(1, 1, 128, 128, 2026) == 8


def test_bank_versions_follow_every_change_of_the_rows(emu):
    """the cached pre-filter operands of the memory read (MemoryManager._prep_of) are keyed on
    KeyValueMemoryStore.version(bucket): it must change with EVERY call that adds, drops or moves key / shrinkage rows
    (add, sieve / range removal, least-usage eviction, purge of the bucket) and with nothing else (usage bookkeeping,
    read-only views) -- a missed bump would be a silently stale read"""
    from deva.inference.kv_memory_store import KeyValueMemoryStore
    g = torch.Generator().manual_seed(0)
    store = KeyValueMemoryStore(save_selection=True, save_usage=True)
    assert store.version(0) == 0

    def frame(n):
        return (torch.randn(64, n, generator=g), {1: torch.randn(512, n, generator=g), 2: torch.randn(512, n, generator=g)},
                torch.rand(1, n, generator=g) + 1, torch.rand(64, n, generator=g))

    seen = []

    def changed(what):
        v = store.version(0)
        assert v not in seen and v > 0, f'{what}: the bucket version did not change'
        seen.append(v)

    k, v, s, e = frame(40)
    store.add(k, v, s, e)
    changed('first add')
    k, v, s, e = frame(24)
    store.add(k, v, s, e)
    changed('append')
    before = store.version(0)
    store.update_bucket_usage(0, torch.rand(64))          # counters only: the rows stand still
    store.get_all_sliced(0, 8, 16)
    _ = store.key, store.shrinkage, store.size(0), store.engaged(0)
    assert store.version(0) == before, 'usage bookkeeping / read-only views must not invalidate the prepared operands'
    store.sieve_by_range(0, 8, -8, 10)
    changed('sieve_by_range')
    store.remove_obsolete_features(0, store.size(0) - 5)
    changed('remove_obsolete_features')
    k, v, s, e = frame(12)
    store.add(k, {3: v[1]}, s, e)                          # a second bucket: bucket 0 untouched
    assert store.version(0) == seen[-1] and store.version(1) > seen[-1]
    store.purge_except([3])
    assert store.version(0) == 0 and store.version(1) > 0  # purged bucket: nothing left to be stale about


def test_memory_manager_keys_its_prepared_banks_on_the_versions(emu):
    """MemoryManager._prep_of: one BankPrep per live bucket, a key that changes when either store's bucket version (or an
    arena's address) changes, nothing handed out when bank_prep_enabled is off, entries of purged buckets dropped"""
    from deva.inference.memory_manager import MemoryManager
    cfg = synth.base_config(mem_every=1, max_mid_term_frames=3, min_mid_term_frames=2, num_prototypes=4)
    mem = MemoryManager(cfg)
    g = torch.Generator().manual_seed(1)
    h, w = 4, 6

    def add(objs):
        key = torch.randn(1, 64, h, w, generator=g)
        mem.add_memory(key, torch.rand(1, 1, h, w, generator=g) + 1, torch.randn(1, len(objs), 512, h, w, generator=g), objs,
                       selection=torch.rand(1, 64, h, w, generator=g))

    add([1, 2])
    p0 = mem._prep_of(0, False)
    assert set(p0) == {'prep', 'prep_key'} and mem._prep_of(0, False)['prep'] is p0['prep']
    assert mem._prep_of(0, False)['prep_key'] == p0['prep_key']
    add([1, 2])
    assert mem._prep_of(0, False)['prep_key'] != p0['prep_key'], 'a memory frame must change the key of the bucket'
    add([1, 2, 7])                                                     # object 7 opens bucket 1
    assert mem._prep_of(1, False)['prep'] is not p0['prep']
    mem.bank_prep_enabled = False
    assert mem._prep_of(0, False) == {}
    mem.bank_prep_enabled = True
    mem.purge_except([7])
    mem._prep_of(1, False)
    assert 0 not in mem._bank_prep and 1 in mem._bank_prep


def test_broadcasts_are_the_identity_outside_frame_owner_mode():
    """the one frame of `DEVAInferenceCore` calls the manager's broadcasts on every path: on a manager that is not in
    frame-owner mode they hand back the very objects they were given -- no copy, no process group, no traffic counted"""
    import torch.distributed as dist
    from deva.inference.memory_manager import MemoryManager
    mem = MemoryManager(synth.base_config())
    assert not dist.is_initialized() and mem.is_frame_owner and not mem.frame_owner_mode
    h, w = 4, 6
    key, sel = torch.randn(1, 64, h, w), torch.rand(1, 64, h, w)
    shr, value = torch.rand(1, 1, h, w) + 1, torch.randn(1, 2, 512, h, w)
    before = mem.comm_bytes
    qk, qe = mem.broadcast_query(key, sel, h, w, key.device)
    assert qk is key and qe is sel
    k, s, v, e = mem.broadcast_memory_frame(key, shr, value, sel, [1, 2], h, w, key.device)
    assert k is key and s is shr and v is value and e is sel
    data = b'x'
    assert mem.broadcast_bytes(data, key.device) is data
    assert mem.comm_bytes == before and not dist.is_initialized()
    # a read sharded WITHOUT an owner (every rank steps the clip) is not frame-owner mode either
    mem._shard_group = object()
    assert mem.broadcast_query(key, sel, h, w, key.device)[0] is key and mem.broadcast_bytes(data, key.device) is data


def test_winograd_weights_follow_the_flags(emu, recipe_state_dict):
    """which convolutions carry Winograd-transformed weights (deva/model/_graph.py:WINO_SCOPES): the 3x3 layers of the value
    encoder, the mask decoder and the key encoder by default; none with --no_winograd, --f16_split or --amp (their kernels take
    those layers); never the key projection or a 1x1 / 7x7 layer"""
    from deva.model.network import DEVA
    sd, _ = recipe_state_dict

    def wino_layers(**flags):
        net = DEVA(dict(synth.base_config(), **flags))
        net.load_weights(sd)
        g = net.graph()
        return {name for name, pc in g.convs.items() if pc.weight_wino is not None}, g

    on, g = wino_layers()
    assert on, 'no layer carries Winograd weights by default'
    for name in on:
        w = sd[name + '.weight']
        assert tuple(w.shape[2:]) == (3, 3) and w.shape[1] % 8 == 0, name
        assert name.startswith(('mask_encoder.', 'mask_decoder.', 'pixel_encoder.')), name
    eligible = {n[:-len('.weight')] for n, w in sd.items() if n.endswith('.weight') and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)
                and w.shape[1] % 8 == 0 and n.startswith(('mask_encoder.', 'mask_decoder.', 'pixel_encoder.'))}
    assert on == {n for n in eligible if n in g.convs}
    assert not any(n.startswith('key_proj') for n in on)
    for flags in (dict(no_winograd=True), dict(f16_split=True), dict(f16_split=True, f16_split_key_encoder=True), dict(amp=True)):
        assert wino_layers(**flags)[0] == set(), flags
