"""Every launcher off the default stream (tests/stream_probe.py, tests/stream_cases.py), the per-stream scratch of
deva/hip/ops.py under two streams at once and across its eviction rule, the key-encoder prefetch where its layers take
Winograd, split-K and the split-flag ring, and a whole clip inside `with torch.cuda.stream(s)`.

The outputs of the side-stream run are held to the default-stream run bit for bit (every atomic of csrc/ is an integer
one and split-K is tested deterministic); the default-stream values themselves are held to their references by the
op's own test file.  With DEVA_TEST_DRYRUN=1 the builders, runs and comparisons execute on the CPU contracts; the
negative controls and what needs real streams are skipped there."""
import contextlib
import os

import pytest
import torch

import gpu_util
import stream_cases as SC
import stream_probe as SP
from deva.hip import DevaHipError, ops
from gpu_util import dev
from workload import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
needs_streams = pytest.mark.skipif(DRYRUN, reason='needs real streams: nothing to observe on the emulated ops')


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        SC.install_contracts(monkeypatch)


def seeds_of(position):
    """a seed pair of its own per case (real: even, decoy: the next odd one): no recycled allocator block can already
    hold the expected values of another case"""
    return 1000 + 2 * position, 1001 + 2 * position


# ------------------------------------------------------------------------------------------ a. negative controls
def _maxpool_on(stream_of):
    from deva.hip import check, lib

    def run(i, mark):
        x = i['x']
        b, c, h, w = x.shape
        out = ops._alloc((b, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), x.device)
        check(lib().deva_maxpool3x3s2(x.data_ptr(), out.data_ptr(), b * c, h, w, 0, stream_of()), 'deva_maxpool3x3s2')
        return out
    return run


@needs_streams
def test_control_a_launch_on_the_null_stream_is_reported():
    """deva_maxpool3x3s2 through lib() with a null stream handle inside the side-stream context: it cannot wait for the
    delay, reads the decoys, and the probe must say so (and say nothing when the handle is the caller's stream)"""
    g = SC.G(11)
    real, decoy = dict(x=SC.rand(g, 2, 5, 29, 53)), dict(x=SC.rand(g, 2, 5, 29, 53))
    SP.probe(_maxpool_on(ops._stream), real, decoy, 'control: maxpool on the current stream')
    with pytest.raises(SP.Mismatch) as caught:
        SP.probe(_maxpool_on(lambda: None), real, decoy, 'control: maxpool on the null stream')
    print('caught:', caught.value)


@needs_streams
def test_control_a_hand_over_across_streams_is_reported():
    """deva_affinity_topk on the null stream, deva_affinity_finalize on the side stream: the lists that finalize reads
    were made from the decoys"""
    from deva.hip import check, lib
    hw, k, splits = 129, 30, 3

    def pair(first_stream):
        def run(i, mark):
            L = lib()
            part = ops._affinity_workspace(L.deva_affinity_workspace(hw, k, splits), dev())
            idx = torch.empty((hw, k), dtype=torch.int32, device=dev())
            weight = torch.empty((hw, k), dtype=torch.float32, device=dev())
            check(L.deva_affinity_topk(i['kl'].data_ptr(), i['sl'].data_ptr(), i['kl'].shape[0], i['kw'].data_ptr(),
                                       i['sw'].data_ptr(), i['kw'].shape[0], i['qk'].data_ptr(), i['qe'].data_ptr(), hw, k, splits,
                                       part.data_ptr(), first_stream()), 'deva_affinity_topk')
            check(L.deva_affinity_finalize(part.data_ptr(), hw, k, splits, idx.data_ptr(), weight.data_ptr(), None, ops._stream()),
                  'deva_affinity_finalize')
            return idx, weight
        return run
    real, decoy = SC._bank(999, hw, 21, 333), SC._bank(999, hw, 22, 333)
    SP.probe(pair(ops._stream), real, decoy, 'control: topk and finalize on the current stream')
    with pytest.raises(SP.Mismatch) as caught:
        SP.probe(pair(lambda: None), real, decoy, 'control: topk on the null stream')
    print('caught:', caught.value)


# ------------------------------------------------------------------------------------------ b. the table
@pytest.mark.parametrize('position', range(len(SC.CASES)), ids=[c.name for c in SC.CASES])
def test_every_launch_goes_to_the_callers_stream(position):
    c = SC.CASES[position]
    real_seed, decoy_seed = seeds_of(position)
    real, run = c.build(real_seed)
    decoy, _ = c.build(decoy_seed)
    if c.raw and DRYRUN:
        SP.check_inputs(real, decoy)
        pytest.skip('raw pointers: needs the library')
    SP.probe(run, real, decoy, c.name)


# ------------------------------------------------------------------------------------------ c. two streams at once
def _conv_split_k():
    gw = SC.G(5)
    pc = gpu_util.to_dev(ops.pack_conv(SC.rand(gw, 64, 64, 3, 3, scale=0.05), SC.rand(gw, 64, scale=0.1)))
    return (lambda seed: dict(x=SC.rand(SC.G(seed), 1, 64, 8, 8)), lambda i: ops.conv2d(pc, i['x'], pad=1), '_WORKSPACE')


def _conv_split(hot=()):
    gw = SC.G(6)
    pc = gpu_util.to_dev(ops.pack_conv(SC.rand(gw, 64, 768, 1, 1, scale=0.05), SC.rand(gw, 64, scale=0.1), split=True))

    def inputs(seed):
        x = SC.rand(SC.G(seed), 1, 768, 8, 8)
        if seed in hot:
            x[0, 5, 3, 3] = 70000.0
        return dict(x=x)
    return inputs, lambda i: ops.conv2d(pc, i['x'], split=True), '_SPLIT_FLAGS'


def _affinity_read():
    return (lambda seed: SC._bank(999, 129, seed, 333), lambda i: SC._topk(i, 30), '_AFF_WS')


def _dense_read():
    return (lambda seed: SC.dense_inputs(seed), lambda i: SC._dense_read(i, None), '_DENSE_WS')


def _guarded_inputs(inputs):
    out = {}
    for k, v in inputs.items():
        out[k] = SP._device_buffer(v)
        out[k].copy_(v)
    return out


def _storage(entry):
    t = entry[0] if isinstance(entry, list) else entry
    return t.untyped_storage().data_ptr()


@needs_streams
@pytest.mark.parametrize('make', [_conv_split_k, _conv_split, _affinity_read, _dense_read], ids=lambda f: f.__name__.strip('_'))
def test_two_streams_at_once_keep_their_scratch_apart(make):
    """eight alternating calls with different inputs on two streams, both behind delays, nothing synchronised in between:
    every result equals its default-stream result, and the two streams' cache entries are distinct storages"""
    inputs, run, cache_name = make()
    sets = [_guarded_inputs(inputs(300 + j)) for j in range(8)]
    want = [SP.to_host(run(s)) for s in sets]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert streams[0].cuda_stream != streams[1].cuda_stream
    events, outs, keys = [], [], []
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            events.append(SP.delay())
            keys.append(ops._stream_key(dev()))
    for j, data in enumerate(sets):
        with torch.cuda.stream(streams[j % 2]):
            outs.append(run(data))
    blocked = [not e.query() for e in events]
    cache = getattr(ops, cache_name)
    assert keys[0] in cache and keys[1] in cache and keys[0] != keys[1]
    assert _storage(cache[keys[0]]) != _storage(cache[keys[1]]), f'{cache_name}: one storage for two streams'
    got = []
    for j, out in enumerate(outs):
        with torch.cuda.stream(streams[j % 2]):
            got.append(SP.to_host(out))
    for s in streams:
        s.synchronize()
        SP.release(s)
    assert all(blocked), 'probe invalid: a delay was over before the eight calls were enqueued'
    for j in range(8):
        assert SP.differences(want[j], got[j]) == [], (j, SP.differences(want[j], got[j]))


# ------------------------------------------------------------------------------------------ d. bound and eviction
@needs_streams
def test_per_stream_caches_are_bounded_and_survive_eviction():
    """more streams than _MAX_STREAM_CACHES, a split convolution, a memory read and a dense read on each: the fall-back
    count is exact before and after the evictions, no cache grows past the bound, an evicted stream computes the right
    result again, and `affinity_last_read_flag` refuses a stream without a buffer"""
    bound = ops._MAX_STREAM_CACHES
    caches = {n: getattr(ops, n) for n in ('_WORKSPACE', '_SPLIT_FLAGS', '_AFF_WS', '_DENSE_WS')}
    n_streams = bound + 3
    torch.cuda.synchronize()
    for cache in caches.values():                                  # what earlier tests left: the count below starts afresh
        cache.clear()
    hot = {300 + 1, 300 + 4, 300 + bound + 1}                      # two before the first eviction, one after
    conv_inputs, conv, _ = _conv_split(hot)
    read_inputs, read, _ = _affinity_read()
    dense_inputs, dense, _ = _dense_read()
    data = [(_guarded_inputs(conv_inputs(300 + j)), _guarded_inputs(read_inputs(400 + j)), _guarded_inputs(dense_inputs(500 + j)))
            for j in range(n_streams)]
    want = [tuple(SP.to_host(f(d)) for f, d in zip((conv, read, dense), item)) for item in data]
    base = ops.split_fallbacks(dev())                              # (the reference runs raised their flags too)
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    assert len({s.cuda_stream for s in streams}) == n_streams and 0 not in {s.cuda_stream for s in streams}
    keys, got = [], []
    for j, (s, item) in enumerate(zip(streams, data)):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            keys.append(ops._stream_key(dev()))
            got.append(tuple(SP.to_host(f(d)) for f, d in zip((conv, read, dense), item)))
        for name, cache in caches.items():
            assert len(cache) <= bound, (name, len(cache), j)
            assert keys[-1] in cache, (name, j)
        if j == bound - 2:      # the default stream's entries and bound - 1 streams: nothing has been evicted yet
            assert keys[0] in caches['_SPLIT_FLAGS']
            assert ops.split_fallbacks(dev()) == base + 2
    assert ops.split_fallbacks(dev()) == base + 3, 'the fall-back count moved across the evictions'
    for name, cache in caches.items():
        assert len(cache) == bound and keys[0] not in cache, (name, len(cache))
    for j in range(n_streams):
        for a, b in zip(want[j], got[j]):
            assert SP.differences(a, b) == [], (j, SP.differences(a, b))
    with torch.cuda.stream(streams[0]):                            # evicted: no buffer to read a flag from ...
        with pytest.raises(DevaHipError, match='no read has run'):
            ops.affinity_last_read_flag(dev())
        again = tuple(SP.to_host(f(d)) for f, d in zip((conv, read, dense), data[0]))   # ... and new ones on demand
        ops.affinity_last_read_flag(dev())                         # (a buffer again: no refusal)
    for a, b in zip(want[0], again):
        assert SP.differences(a, b) == []
    assert ops.split_fallbacks(dev()) == base + 3                  # (300 is not a hot seed)
    fresh = torch.cuda.Stream()
    assert fresh.cuda_stream not in {s.cuda_stream for s in streams}
    with torch.cuda.stream(fresh):
        with pytest.raises(DevaHipError, match='no read has run'):
            ops.affinity_last_read_flag(dev())
    for s in streams:
        SP.release(s)
    assert ops.split_fallbacks(dev()) == base + 3                  # released rings keep their counts
    for name, cache in caches.items():
        assert not any(k in cache for k in keys), name


@needs_streams
def test_cuda_and_cuda0_share_their_cache_entries():
    assert torch.cuda.current_device() == 0
    a, b = torch.device('cuda'), torch.device('cuda:0')
    assert ops._stream_key(a) == ops._stream_key(b) == ops._stream_key('cuda:0')
    assert ops._workspace(a) is ops._workspace(b)
    assert ops._affinity_workspace(1, a) is ops._affinity_workspace(1, b)
    before = len(ops._SPLIT_FLAGS)
    ops._split_flag(a), ops._split_flag(b)
    assert len(ops._SPLIT_FLAGS) <= before + 1


# ------------------------------------------------------------------------------------------ e. prefetch where it matters
@pytest.fixture(scope='module')
def state_dict(recipe_state_dict):
    return recipe_state_dict[0]


def _network(state_dict, **over):
    from deva.model.network import DEVA
    net = DEVA(synth.base_config(**over))
    net.load_weights(state_dict)
    return net.to(dev()).eval()


def _key_encoder_plans(net, h, w, monkeypatch):
    """the plan of every convolution that `encode_image` + `transform_key` issue for an h x w frame"""
    import emu_ops
    plans, real = [], ops.conv2d

    def recording(pc, x0, x1=None, *, stride=1, pad=0, amp=False, split=False, **kw):
        plans.append(emu_ops.plan_of(pc, x0, x1, stride, pad, amp=amp and pc.weight_f16 is not None,
                                     split=split and pc.weight_split is not None).first)
        return real(pc, x0, x1, stride=stride, pad=pad, amp=amp, split=split, **kw)
    with monkeypatch.context() as m:
        m.setattr(ops, 'conv2d', recording)
        _, pix = net.encode_image(torch.zeros(1, 3, h, w, device=dev()))
        net.transform_key(pix)
    return plans


def _plain_and_prefetch(net, cfg, h, w, frames, seed):
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.utils.tensor_utils import pad_divide_by
    stream = synth.FrameStream(h, w, seed=seed)
    imgs = [stream.next().to(dev()) for _ in range(frames + 1)]
    mask0 = synth.box_mask(h, w, 2).to(dev())
    outs, fallbacks = {}, {}
    for mode in ('plain', 'prefetch'):
        before = ops.split_fallbacks(dev())
        core = DEVAInferenceCore(net, cfg)
        res = [core.step(imgs[0], mask0, [1, 2])]
        for t in range(1, frames):
            if mode == 'prefetch':
                core.image_feature_store.prefetch(core.curr_ti + 2, pad_divide_by(imgs[t + 1], 16)[0].unsqueeze(0))
            res.append(core.step(imgs[t]))
        torch.cuda.synchronize()
        core.image_feature_store.delete(core.curr_ti + 1)
        outs[mode] = [r.cpu() for r in res]
        fallbacks[mode] = ops.split_fallbacks(dev()) - before
    assert all(torch.equal(a, b) for a, b in zip(outs['plain'], outs['prefetch'])), 'prefetch changed the output'
    return fallbacks


@needs_streams
def test_prefetch_is_bit_identical_where_the_key_encoder_takes_winograd_and_split_k(state_dict, monkeypatch):
    """the smallest 3:4 frame (a multiple of 96 x 128, the smoke clip's size) for which the library's plan puts at least
    one key-encoder layer on Winograd and another on split-K: the side stream's split-K scratch and the main stream's are
    then in use at the same time"""
    net = _network(state_dict)
    size = None
    for k in range(1, 13):
        firsts = _key_encoder_plans(net, 96 * k, 128 * k, monkeypatch)
        wino, split_k = sum(p.family == 'wino' for p in firsts), sum(p.family != 'wino' and p.splits > 1 for p in firsts)
        print(f'{96 * k} x {128 * k}: {len(firsts)} key-encoder convolutions, {wino} Winograd, {split_k} split-K')
        if wino and split_k:
            size = (96 * k, 128 * k)
            break
    assert size is not None, 'no 3:4 frame up to 1152 x 1536 has both a Winograd and a split-K layer in the key encoder'
    print(f'plan-derived prefetch size: {size[0]} x {size[1]}')
    _plain_and_prefetch(net, synth.base_config(mem_every=2), *size, frames=4, seed=4)


@needs_streams
def test_prefetch_is_bit_identical_on_the_split_kernels(state_dict):
    """f16_split + f16_split_key_encoder at 96 x 128: the prefetched key encoder raises its flags in the side stream's
    ring; the fall-back count is the same in both modes"""
    net = _network(state_dict, f16_split=True, f16_split_key_encoder=True)
    cfg = synth.base_config(mem_every=3, f16_split=True, f16_split_key_encoder=True)
    fallbacks = _plain_and_prefetch(net, cfg, 96, 128, frames=5, seed=4)
    print('split fall-backs:', fallbacks)
    assert fallbacks['plain'] == fallbacks['prefetch']


# ------------------------------------------------------------------------------------------ f. a whole clip on a side stream
def _clip_products(net, root, on_stream):
    """the smoke clip (96 x 128, 5 objects) through `step` -> `FrameResultSaver` with a `VideoObjectScorer` hook, then the
    first frames of the automatic clip (a detection frame with the stand-in segmenter, `incorporate_detection`, plain
    steps) through `AutomaticProcessor`; everything inside `on_stream` -> what the run produced, on the host"""
    import numpy as np
    import prompt_case as PC
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.vos_quality import VideoObjectScorer
    from test_prompts_cpu import run_processor
    h, w, frames, objects = 96, 128, 4, [1, 2, 3, 4, 5]
    mask = synth.box_mask(h, w, len(objects))
    truth = [np.roll(mask.numpy(), (t, t), axis=(0, 1)).astype(np.uint8) for t in range(frames)]
    stream = synth.FrameStream(h, w, seed=1)
    images = [stream.next() for _ in range(frames)]
    clip_frames, rects = PC.clip()
    clip_frames, rects = clip_frames[:3], rects[:3]
    names = [f'{t:05d}.jpg' for t in range(len(clip_frames))]
    out = {}
    with on_stream:
        truth_dev = [torch.from_numpy(p).to(dev()) for p in truth]
        cfg = synth.base_config(mem_every=2)
        core = DEVAInferenceCore(net, cfg)
        scorer = VideoObjectScorer()
        scorer.start_video('clip', objects)
        saver = FrameResultSaver(str(root), 'clip', dataset='unsup_davis17', object_manager=core.object_manager,
                                 frame_hook=lambda name, result, annotation: scorer.add_frame(result, truth_dev[int(name[:-4])]))
        probs = []
        for t in range(frames):
            prob = core.step(images[t].to(dev()), mask.to(dev()) if t == 0 else None, objects if t == 0 else None)
            saver.save_mask(prob, f'{t:05d}.jpg')
            probs.append(prob)
        saver.end()
        assert saver.error is None
        scorer.end_video()
        res = scorer.result()
        out['probs'] = [p.cpu() for p in probs]
        out['counts'] = torch.from_numpy(np.ascontiguousarray(res['frames']['clip']['counts']).astype(np.int64))
        out['scores'] = repr(sorted(res['global'].items()))
        out['png'] = [open(os.path.join(str(root), 'clip', f'{t:05d}.png'), 'rb').read() for t in range(frames)]
        # the automatic loop: frame 0 is a detection frame (prompt points, proposals, assembly, incorporate_detection)
        np.random.seed(11)
        segmenter = PC.FakeSegmenter(clip_frames, rects)
        auto = DEVAInferenceCore(net, PC.loop_config('online'))
        produced, _, _ = run_processor(auto, segmenter, clip_frames, names)
        out['auto'] = [(name, p.cpu()) for name, p in produced]
        out['asked'] = [torch.from_numpy(a) for a in segmenter.asked()]
        out['ids'] = repr(sorted(int(o.id) if hasattr(o, 'id') else int(o) for o in auto.object_manager.all_historical_object_ids))
    return out


@needs_streams
def test_a_whole_clip_inside_a_side_stream_equals_the_default_stream_run(peaky_state_dict, tmp_path):
    """covers the event / pinned-copy code of detections.py, frame_results.py and the scorers: masks, records, PNG bytes and
    scores of a run inside `with torch.cuda.stream(s)` (s waits for the default stream and starts behind a delay) must
    equal the default-stream run"""
    from deva.model.network import DEVA
    net = DEVA(synth.base_config())
    net.load_weights(peaky_state_dict)
    net = net.to(dev()).eval()
    want = _clip_products(net, tmp_path / 'default', contextlib.nullcontext())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        SP.delay()
    got = _clip_products(net, tmp_path / 'side', torch.cuda.stream(s))
    s.synchronize()
    SP.release(s)
    assert len(want['auto']) == 3 and len(want['asked']) >= 1 and all(p.shape[0] >= 2 for _, p in want['auto'])
    assert want['png'] == got['png'], 'the PNG files differ'
    assert want['scores'] == got['scores'] and want['ids'] == got['ids']
    bad = SP.differences(SP.flatten({k: want[k] for k in ('probs', 'counts', 'auto', 'asked')}),
                         SP.flatten({k: got[k] for k in ('probs', 'counts', 'auto', 'asked')}))
    assert bad == [], bad


# ------------------------------------------------------------------------------------------ the log
def test_zz_probe_summary():
    """the calibration and the enqueue times of this run (kept under profiles/streams/); no probe was invalid"""
    for line in SP.summary():
        print(line)
    assert [r.name for r in SP.RECORDS if not r.blocked] == []
