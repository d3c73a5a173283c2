"""The table of tests/test_gpu_v_streams.py: one case per entry point that takes `void* stream` (include/*.h), through the
`ops` / `metrics` / `vos_metrics` wrappers at the smallest shape that reaches every launch of the launcher.

A case is `build(seed) -> (inputs, run)`: `inputs` a dict of HOST tensors (the probe keeps a real and a decoy set, built
from two seeds, on the device), `run(device inputs, mark) -> tensors`.  Whatever a kernel uses as an index (row lists,
skip_index, label planes, LUT channels, idx) is in range in every set, so that a launch that reads the decoys computes
a wrong answer and never a wild address.  Weights and tables that do not depend on the seed are made inside `build`
from a fixed generator and uploaded there.  In-place results are returned as clones (made on the current stream).

Every case names the entry points whose launches it reaches; tests/test_streams_cpu.py holds the union of those names,
plus `NOT_PROBED` with a reason per entry, against the three headers."""
import os
from collections import namedtuple

import numpy as np
import torch

import emu_ops
import gpu_util
from deva.hip import ops
from workload import synth

DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
Case = namedtuple('Case', 'name covers build raw')
CASES = []

# streamed entry points without a case, each with its reason
NOT_PROBED = {
    'deva_probe_mfma_f32': 'a clock probe for the tools (its result is a cycle count, not data): nothing to compare bit for bit',
}
# their launch is sized by a count the host reads back, so inside the wrappers they are enqueued behind the call's own
# wait, on an idle stream; the raw cases 'proposal_gather' and 'mask_rle_write' below give them the count of the CPU
# contract instead and probe them like every other launch
BEHIND_OWN_SYNC = ('deva_proposal_gather', 'deva_mask_rle_write')


# cases whose result does not depend on the inputs' VALUES: a misrouted launch shows by its order instead (the copy of the
# real inputs, queued behind the delay, lands on top of what it wrote too early)
INPUT_INDEPENDENT = ('usage_init',)


def install_contracts(monkeypatch):
    """the CPU contracts of everything the table calls beyond tests/emu_ops.py (which tests/conftest.py installs for a
    dry run): for DEVA_TEST_DRYRUN=1 and for tests/test_streams_cpu.py"""
    import emu_detections
    import emu_ensemble
    import emu_frame_result
    import emu_panoptic
    import emu_prompts
    import emu_proposals
    import emu_text
    import emu_vos
    import test_dense_read_cpu
    for m in (emu_detections, emu_ensemble, emu_frame_result, emu_panoptic, emu_prompts, emu_proposals, emu_text, emu_vos):
        m.install(monkeypatch)
    monkeypatch.setattr(ops, 'dense_read', test_dense_read_cpu.dense_read)
    monkeypatch.setattr(ops, 'affinity_last_read_flag', lambda device: 0)


def case(name, *covers, raw=False):
    """raw: the run calls the library directly (no wrapper is asynchronous end to end); not executed in the CPU dry run"""
    def deco(fn):
        CASES.append(Case(name, tuple(covers), fn, raw))
        return fn
    return deco


def G(seed):
    return torch.Generator().manual_seed(int(seed))


def D(x):
    return gpu_util.to_dev(x)


def rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def dev():
    return gpu_util.dev()


# ------------------------------------------------------------------------------------------ convolutions
def _conv(name, c0, cout, k, h, w, *, weights=(), amp=False, split=False, family, split_k, hot=False, legacy=False):
    """a `conv2d` call whose plan (deva_conv2d_plan, the function deva_conv2d plans with) is asserted in the builder"""
    def build(seed):
        gw, g = G(1000 + c0 + cout), G(seed)
        wt, b = rand(gw, cout, c0, k, k, scale=(2.0 / (c0 * k * k)) ** 0.5), rand(gw, cout, scale=0.1)
        if legacy:
            from test_gpu_a_conv import _legacy_pack
            pc = _legacy_pack(wt, b)
        else:
            pc = ops.pack_conv(wt, b, None, amp='f16' in weights, split='split' in weights, wino='wino' in weights)
        x = rand(g, 1, c0, h, w)
        if hot:
            x[0, 3, h // 2, w // 3] = 70000.0          # beyond fp16: the gated fp32 re-run is the second launch
        plan = emu_ops.plan_of(pc, x, None, 1, k // 2, amp=amp, split=split)
        assert plan.first.family == family and (plan.first.splits > 1) == split_k, (name, plan)
        assert (plan.rerun is not None) == (family == 'split'), (name, plan)
        pcd = D(pc)
        return dict(x=x), lambda i, mark: ops.conv2d(pcd, i['x'], pad=k // 2, amp=amp, split=split)
    case(name, 'deva_conv2d')(build)


_conv('conv_q4', 64, 64, 1, 8, 8, family='q4', split_k=False)
_conv('conv_q4_split_k', 64, 64, 3, 8, 8, family='q4', split_k=True)
_conv('conv_igemm_split_k', 256, 64, 1, 8, 8, family='igemm', split_k=True, legacy=True)
_conv('conv_wino', 64, 64, 3, 320, 128, weights=('wino',), family='wino', split_k=False)
_conv('conv_cout1_rows', 32, 1, 3, 4096, 4, family='cout1_rows', split_k=False)
_conv('conv_cout1_table', 32, 1, 3, 129, 127, family='cout1_table', split_k=False)
_conv('conv_f16_amp', 768, 64, 1, 8, 8, weights=('f16',), amp=True, family='f16', split_k=True)
_conv('conv_split_in_range', 768, 64, 1, 8, 8, weights=('split',), split=True, family='split', split_k=True)
_conv('conv_split_fp32_rerun', 768, 64, 1, 8, 8, weights=('split',), split=True, family='split', split_k=True, hot=True)


def _stem(name, hot):
    def build(seed):
        gw, g = G(77), G(seed)
        ps = ops.pack_stem(rand(gw, 64, 4, 7, 7, scale=(2.0 / (4 * 49)) ** 0.5), rand(gw, 64, scale=0.1), None, dev())
        image, masks = rand(g, 1, 3, 32, 48), torch.rand(2, 1, 32, 48, generator=g)
        if hot:
            image[0, 1, 20, 30] = 70000.0              # one tile is recomputed in fp32 inside the kernel
        return dict(image=image, masks=masks), lambda i, mark: ops.stem7x7(ps, i['image'], i['masks'], relu=True)
    case(name, 'deva_stem7x7')(build)


_stem('stem7x7', False)
_stem('stem7x7_recomputed_tile', True)


# ------------------------------------------------------------------------------------------ pointwise
@case('pad2d', 'deva_pad2d')
def _(seed):
    return dict(x=rand(G(seed), 2, 3, 29, 53)), lambda i, mark: ops.pad2d(i['x'], (1, 2, 3, 4))


@case('usage_init', 'deva_usage_init')
def _(seed):
    g = G(seed)

    def run(i, mark):
        ops.usage_init(i['use'], i['life'])
        return i['use'].clone(), i['life'].clone()
    return dict(use=rand(g, 1000), life=rand(g, 1000)), run


@case('gather_s2', 'deva_gather_s2')
def _(seed):
    return dict(x=rand(G(seed), 2, 5, 29, 53)), lambda i, mark: ops.gather_s2(i['x'], 3)


@case('maxpool3x3s2', 'deva_maxpool3x3s2')
def _(seed):
    return dict(x=rand(G(seed), 2, 5, 29, 53)), lambda i, mark: ops.maxpool3x3s2(i['x'])


@case('upsample2x_add', 'deva_upsample2x_add')
def _(seed):
    g = G(seed)
    return dict(x=rand(g, 2, 5, 12, 16), skip=rand(g, 1, 5, 24, 32)), lambda i, mark: ops.upsample2x_add(i['x'], i['skip'])


@case('upsample2x_add_ds2', 'deva_upsample2x_add_ds2')
def _(seed):
    g = G(seed)
    return dict(x=rand(g, 2, 5, 12, 16), skip=rand(g, 1, 5, 24, 32)), lambda i, mark: ops.upsample2x_add_ds2(i['x'], i['skip'])


def _map_inputs(seed):
    g = G(seed)
    index = torch.randint(0, 3, (2,), generator=g, dtype=torch.int32)      # in range in every set
    index[0] = seed % 3
    return dict(x=rand(g, 2, 5, 12, 16), skip=rand(g, 3, 5, 24, 32), skip_index=index)


@case('upsample2x_add_map', 'deva_upsample2x_add_map')
def _(seed):
    return _map_inputs(seed), lambda i, mark: ops.upsample2x_add_map(i['x'], i['skip'], i['skip_index'])


@case('upsample2x_add_ds2_map', 'deva_upsample2x_add_ds2_map')
def _(seed):
    return _map_inputs(seed), lambda i, mark: ops.upsample2x_add_ds2_map(i['x'], i['skip'], i['skip_index'])


@case('area_downsample', 'deva_area_downsample')
def _(seed):
    return dict(x=rand(G(seed), 2, 3, 24, 32)), lambda i, mark: ops.area_downsample(i['x'], 4)


@case('input_head', 'deva_input_head')
def _(seed):
    image = torch.randint(0, 256, (29, 53, 3), generator=G(seed), dtype=torch.uint8)
    return dict(image=image), lambda i, mark: ops.input_head(i['image'], (24, 32), pad=(1, 2, 3, 0))


@case('aggregate', 'deva_aggregate')
def _(seed):
    return dict(prob=torch.rand(3, 24, 32, generator=G(seed))), lambda i, mark: ops.aggregate(i['prob'])


@case('softmax_channels', 'deva_softmax_channels')
def _(seed):
    return dict(x=rand(G(seed), 4, 29, 53)), lambda i, mark: ops.softmax_channels(i['x'])


@case('upsample4x_softmax', 'deva_upsample4x_softmax')
def _(seed):
    return dict(x=rand(G(seed), 3, 12, 16)), lambda i, mark: ops.upsample4x_softmax(i['x'])


@case('cbam', 'deva_global_avgmax', 'deva_cbam_mlp', 'deva_cbam_channel_pool', 'deva_cbam_apply', 'deva_conv2d')
def _(seed):
    gw, c = G(6), 64
    hid = c // 16
    w1, b1 = rand(gw, hid, c, scale=c ** -0.5), rand(gw, hid, scale=0.1)
    w2, b2 = rand(gw, c, hid, scale=hid ** -0.5), rand(gw, c, scale=0.1)
    sp = ops.pack_conv(rand(gw, 1, 2, 7, 7, scale=0.2), rand(gw, 1, scale=0.1))
    args = [D(t) for t in (w1, b1, w2, b2, sp)]
    return dict(x=rand(G(seed), 2, c, 5, 7)), lambda i, mark: ops.cbam(i['x'], *args)


@case('gru_update', 'deva_gru_update')
def _(seed):
    g = G(seed)
    return dict(values=rand(g, 2, 24, 6, 8), h=rand(g, 2, 8, 6, 8)), lambda i, mark: ops.gru_update(i['values'], i['h'])


# ------------------------------------------------------------------------------------------ memory read
def _bank(n, hw, seed, n_long, scale=1.0):
    """token-major arenas split at n_long, queries and a zeroed usage counter"""
    mk, ms, qk, qe = synth.affinity_inputs(n, hw, seed=seed, key_scale=scale)
    rows, shr = mk.t().contiguous(), ms.reshape(-1).contiguous()
    return dict(kl=rows[:n_long].contiguous(), sl=shr[:n_long].contiguous(), kw=rows[n_long:].contiguous(),
                sw=shr[n_long:].contiguous(), qk=qk.contiguous(), qe=qe.clone().contiguous(),
                fix=torch.zeros(n, dtype=torch.int64))


def _topk(i, k, splits=None, prep=None, prep_key=None):
    n_long, n_work = i['kl'].shape[0], i['kw'].shape[0]
    i['fix'].zero_()
    idx, w = ops.affinity_topk(i['kl'] if n_long else None, i['sl'] if n_long else None, n_long, i['kw'], i['sw'], n_work,
                               i['qk'], i['qe'], k, i['fix'], splits, prep, prep_key)
    return idx, w, i['fix'].clone()


@case('affinity_topk_finalize', 'deva_affinity_topk', 'deva_affinity_finalize')
def _(seed):
    return _bank(999, 129, seed, 333), lambda i, mark: _topk(i, 30, splits=3)


def _candidates(i, k, splits):
    n_long, n_work = i['kl'].shape[0], i['kw'].shape[0]
    return ops.affinity_candidates(i['kl'], i['sl'], n_long, i['kw'], i['sw'], n_work, i['qk'], i['qe'], k, 1000, splits)


@case('affinity_select', 'deva_affinity_topk', 'deva_affinity_select')
def _(seed):
    return _bank(999, 129, seed, 333), lambda i, mark: _candidates(i, 30, 2)


@case('affinity_read', 'deva_affinity_read')
def _(seed):
    return _bank(999, 129, seed, 333), lambda i, mark: _candidates(i, 30, None)


@case('affinity_merge', 'deva_affinity_merge')
def _(seed):
    n, hw, k = 600, 129, 30
    mk, ms, qk, qe = synth.affinity_inputs(n, hw, seed=seed)
    rows, shr = mk.t().contiguous(), ms.reshape(-1).contiguous()
    shards = [emu_ops.affinity_candidates(None, None, 0, rows[a:a + 300].contiguous(), shr[a:a + 300].contiguous(), 300, qk, qe, k,
                                          token_offset=a) for a in (0, 300)]      # token indices below n in every set
    inputs = dict(keys=torch.stack([s[0] for s in shards]), counts=torch.stack([s[1] for s in shards]),
                  fix=torch.zeros(n, dtype=torch.int64))

    def run(i, mark):
        i['fix'].zero_()
        idx, w = ops.affinity_merge(i['keys'], i['counts'], k, i['fix'])
        return idx, w, i['fix'].clone()
    return inputs, run


@case('affinity_dense', 'deva_affinity_dense')
def _(seed):
    def run(i, mark):
        i['fix'].zero_()
        idx, w = ops.affinity_dense(i['kl'], i['sl'], 333, i['kw'], i['sw'], 666, i['qk'], i['qe'], 40, i['fix'])
        return idx, w, i['fix'].clone()
    return _bank(999, 129, seed, 333), run


PREFILTER_SHAPE = (8192, 1024, 30)     # of test_fp16_prefilter_falls_back_where_its_bound_does_not_hold: the library pre-filters


@case('affinity_read_prepared', 'deva_affinity_read_prepared')
def _(seed):
    n, hw, k = PREFILTER_SHAPE

    def run(i, mark):
        prep = ops.BankPrep()
        first = _topk(i, k, prep=prep, prep_key='bank')
        again = _topk(i, k, prep=prep, prep_key='bank')      # the prepared bank: the bank kernels are skipped
        return first, again
    return _bank(n, hw, seed, 0), run


def _falls_back(seed):
    n, hw, k = PREFILTER_SHAPE
    inputs = _bank(n, hw, seed, 0)
    inputs['qe'][3, 17] = -0.25       # outside the bound's premises: the device flag, then the fp32 kernels
    return inputs


@case('affinity_prefilter_fallback', 'deva_affinity_read_prepared')
def _(seed):
    return _falls_back(seed), lambda i, mark: _topk(i, PREFILTER_SHAPE[2])


@case('affinity_read_flag_stats', 'deva_affinity_read_flag', 'deva_affinity_read_stats')
def _(seed):
    """both synchronise the stream they are given: the read in front of them is the probed launch sequence, their
    answers (flag 2 on the real inputs, 0 on the decoys; the statistics of the real read) come from the hand-over buffer"""
    n, hw, k = PREFILTER_SHAPE
    inputs = _falls_back(seed) if seed % 2 == 0 else _bank(n, hw, seed, 0)

    def run(i, mark):
        import ctypes
        res = _topk(i, k)
        mark()
        flag = ops.affinity_last_read_flag(dev())
        stats = []
        if not DRYRUN:
            from deva.hip import check, lib
            out = (ctypes.c_int64 * 5)()
            ws = ops._AFF_WS[ops._stream_key(dev())]
            check(lib().deva_affinity_read_stats(ws.data_ptr(), n, hw, k, out, ops._stream()), 'deva_affinity_read_stats')
            stats = list(out)
        return res, flag, stats
    return inputs, run


@case('usage_update', 'deva_usage_update')
def _(seed):
    g = G(seed)
    inputs = dict(fix=torch.randint(0, 1 << 45, (500,), generator=g), use=torch.rand(300, generator=g),
                  life=torch.rand(300, generator=g) + 0.5)

    def run(i, mark):
        ops.usage_update(i['fix'], 100, i['use'], i['life'], 300)
        return i['fix'].clone(), i['use'].clone(), i['life'].clone()
    return inputs, run


@case('readout_sparse', 'deva_readout_sparse')
def _(seed):
    g = G(seed)
    n_long, n_work, hw, k, cv = 40, 160, 129, 30, 512
    w = torch.rand(hw, k, generator=g)
    inputs = dict(idx=torch.randint(0, n_long + n_work, (hw, k), generator=g, dtype=torch.int32), w=w / w.sum(1, keepdim=True),
                  vl=rand(g, n_long, cv), vw=rand(g, n_work, cv))

    def run(i, mark):
        out = torch.empty(cv, hw, device=i['w'].device)
        return ops.readout_sparse(i['idx'], i['w'], i['vl'], n_long, i['vw'], out)
    return inputs, run


def _dense_read(i, mark):
    n_long, n_work, hw = i['kl'].shape[0], i['kw'].shape[0], i['qk'].shape[1]
    i['fix'].zero_()
    out = torch.empty((2, 512, hw), device=i['qk'].device)
    ops.dense_read(i['kl'], i['sl'], n_long, i['kw'], i['sw'], n_work, i['qk'], i['qe'], [i['vl0'], i['vl1']],
                   [i['vw0'], i['vw1']], out, i['fix'])
    return out, i['fix'].clone()


def dense_inputs(seed, n=200, hw=129, n_long=60):
    inputs = _bank(n, hw, seed, n_long)
    vt = [v.t().contiguous() for v in synth.value_inputs(2, 512, n, seed=seed)]
    for o in range(2):
        inputs[f'vl{o}'], inputs[f'vw{o}'] = vt[o][:n_long].contiguous(), vt[o][n_long:].contiguous()
    return inputs


@case('dense_read_two_objects', 'deva_dense_read')
def _(seed):
    return dense_inputs(seed), _dense_read


# ------------------------------------------------------------------------------------------ bank upkeep
@case('bank_append', 'deva_bank_append')
def _(seed):
    g = G(seed)

    def run(i, mark):
        ops.bank_append(i['src'], i['arena'], 13)
        return i['arena'].clone()
    return dict(src=rand(g, 64, 77), arena=rand(g, 200, 64)), run


@case('bank_gather_rows', 'deva_bank_gather_rows')
def _(seed):
    g = G(seed)

    def run(i, mark):
        dst = torch.zeros(77, 64, device=i['src'].device)
        ops.bank_gather_rows(i['src'], i['rows'], dst, 77)
        return dst
    return dict(src=rand(g, 200, 64), rows=torch.randperm(200, generator=g)[:77].int()), run


@case('bank_export', 'deva_bank_export')
def _(seed):
    return dict(arena=rand(G(seed), 200, 64)), lambda i, mark: ops.bank_export(i['arena'], 150)


@case('rank_select_evict', 'deva_rank', 'deva_rank_select', 'deva_evict_select')
def _(seed):
    g = G(seed)
    n = 300

    def run(i, mark):
        r_desc, xn = ops.rank(i['use'], n, True, life=i['life'])
        sel = ops.rank_select(r_desc, 128)
        r_asc, _ = ops.rank(i['x'], n, False)
        idx, count = ops.evict_select(i['x'], r_asc, 100)
        return r_desc, xn, sel, r_asc, count          # (the rows of idx beyond count are not written)
    return dict(use=torch.rand(n, generator=g), life=torch.rand(n, generator=g) + 0.5,
                x=(torch.rand(n, generator=g) * 50).round() / 50), run


@case('similarity_softmax_columns', 'deva_similarity_dense', 'deva_softmax_columns')
def _(seed):
    g = G(seed)
    nc, p = 240, 32

    def run(i, mark):
        sim = ops.similarity_dense(i['key'], i['shr'], i['sel'], i['proto'], nc)
        return sim.clone(), ops.softmax_columns(sim, p)
    return dict(key=rand(g, nc, 64, scale=2.0), shr=torch.rand(nc, generator=g) + 1, sel=torch.rand(nc, 64, generator=g),
                proto=torch.randperm(nc, generator=g)[:p].int()), run


# ------------------------------------------------------------------------------------------ detection merging, masks
@case('label_histogram_merge_paint', 'deva_label_histogram', 'deva_merge_paint')
def _(seed):
    g, gt = G(seed), G(9)
    h, w, n_our, n_new, n_out = 29, 53, 3, 4, 3
    new_ids = (torch.randperm(5000, generator=gt)[:n_new] + 300).long()
    table = torch.cat([new_ids, torch.tensor([0, 77777])])
    our_order = torch.randint(-1, 6, (n_our + 1,), generator=gt).int()
    our_label = torch.randint(1, 400, (n_our + 1,), generator=gt)
    new_order = torch.randint(-1, 6, (n_new,), generator=gt).int()
    new_label = torch.randint(1, 400, (n_new,), generator=gt)
    out_ids = torch.unique(torch.cat([our_label, new_label]))[:n_out]
    static = [D(t) for t in (new_ids, our_order, our_label, new_order, new_label, out_ids)]
    inputs = dict(ours=torch.randint(0, n_our + 1, (h, w), generator=g),         # labels 0 .. n_our in every set
                  news=table[torch.randint(0, n_new + 2, (h, w), generator=g)])

    def run(i, mark):
        ids, oo, ol, no, nl, out = static
        return (ops.label_histogram(i['ours'], i['news'], ids, n_our),
                ops.merge_paint(i['ours'], i['news'], ids, oo, ol, no, nl, out))
    return inputs, run


@case('lut_remap', 'deva_lut_remap')
def _(seed):
    g = G(seed)
    return (dict(mask=torch.randint(0, 20, (29, 53), generator=g), lut=torch.randint(1, 1 << 40, (16,), generator=g)),
            lambda i, mark: ops.lut_remap(i['mask'], i['lut']))


def _soft(g, c, h, w):
    return torch.softmax(torch.randn(c, h, w, generator=g) * 2, dim=0)


@case('index_mask', 'deva_index_mask')
def _(seed):
    g = G(seed)
    return (dict(prob=_soft(g, 4, 24, 32), lut=torch.randint(1, 1 << 40, (4,), generator=g)),
            lambda i, mark: ops.index_mask(i['prob'], (29, 53), i['lut']))


@case('scores_u8', 'deva_scores_u8')
def _(seed):
    return dict(prob=_soft(G(seed), 3, 24, 32)), lambda i, mark: ops.scores_u8(i['prob'], (29, 53), flip=True)


@case('ensemble_index_mask', 'deva_ensemble_index_mask')
def _(seed):
    g = G(seed)
    return (dict(a=_soft(g, 3, 24, 32), b=_soft(g, 3, 29, 53), c=_soft(g, 3, 36, 60), lut=torch.randint(1, 1 << 40, (3,), generator=g)),
            lambda i, mark: (ops.ensemble_index_mask([i['a'], i['b'], i['c']], (29, 53), [False, True, False], i['lut']),
                             ops.ensemble_index_mask([i['a'], i['b']], (29, 53), [True, False], None, quantize=False)))


@case('flip_w', 'deva_flip_w')
def _(seed):
    g = G(seed)
    return (dict(x=rand(g, 2, 3, 29, 53), frame=torch.randint(0, 256, (29, 53, 3), generator=g, dtype=torch.uint8)),
            lambda i, mark: (ops.flip_w(i['x']), ops.flip_w(i['frame'])))


def _result_inputs(seed):
    g = G(seed)
    return dict(prob=_soft(g, 5, 24, 32), lut=torch.randint(1, 1 << 24, (5,), generator=g),
                colors=torch.randint(0, 256, (5, 3), generator=g, dtype=torch.uint8),
                image=torch.randint(0, 256, (29, 53, 3), generator=g, dtype=torch.uint8))


def _frame_result(i):
    return ops.frame_result(i['prob'], (29, 53), i['lut'], color_lut=i['colors'], image=i['image'],
                            want=('index', 'labels', 'stats', 'color', 'gray', 'blend'))


@case('frame_result', 'deva_frame_result')
def _(seed):
    return _result_inputs(seed), lambda i, mark: _frame_result(i)


@case('frame_result_mask_rle', 'deva_frame_result', 'deva_mask_rle_count', 'deva_mask_rle_write')
def _(seed):
    def run(i, mark):
        res = _frame_result(i)
        mark()                                         # mask_rle reads its counts back: the pair's own synchronisation
        n, bounds = ops.mask_rle(res.index, 5)
        return res.index, n, bounds
    return _result_inputs(seed), run


@case('mask_rle_count', 'deva_mask_rle_count', raw=True)
def _(seed):
    """the count launches (a memset and the kernels) without the read-back behind them"""
    index = torch.randint(0, 5, (29, 53), generator=G(seed), dtype=torch.int16)

    def run(i, mark):
        from deva.hip import check, lib
        nbytes = lib().deva_mask_rle_scratch(29, 53, 5)
        scratch = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=i['index'].device)
        n = torch.empty(5, dtype=torch.int32, device=i['index'].device)
        check(lib().deva_mask_rle_count(i['index'].data_ptr(), 29, 53, 5, scratch.data_ptr(), nbytes, n.data_ptr(), ops._stream()),
              'deva_mask_rle_count')
        return n
    return dict(index=index), run


@case('mask_rle_write', 'deva_mask_rle_count', 'deva_mask_rle_write', raw=True)
def _(seed):
    """count and write back to back, the host counts taken from the CPU contract instead of a read-back.  The scratch is
    an input of the probe (zeros in both sets: a plane without a boundary), so a write that runs before its count finds
    nothing to write -- the kernel indexes its cursors with what the scratch holds"""
    import emu_frame_result as E
    index = torch.randint(0, 5, (29, 53), generator=G(seed), dtype=torch.int16)
    n_host = E.mask_rle(index, 5)[0].to(torch.int32).contiguous()
    total = int(n_host.sum())
    words = 0
    if not DRYRUN:
        from deva.hip import lib
        words = (lib().deva_mask_rle_scratch(29, 53, 5) + 3) // 4

    def run(i, mark):
        from deva.hip import check, lib
        nbytes = lib().deva_mask_rle_scratch(29, 53, 5)
        n = torch.empty(5, dtype=torch.int32, device=i['index'].device)
        bounds = torch.full((total,), -1, dtype=torch.int32, device=i['index'].device)
        check(lib().deva_mask_rle_count(i['index'].data_ptr(), 29, 53, 5, i['scratch'].data_ptr(), nbytes, n.data_ptr(),
                                        ops._stream()), 'deva_mask_rle_count')
        check(lib().deva_mask_rle_write(29, 53, 5, i['scratch'].data_ptr(), nbytes, n_host.data_ptr(), bounds.data_ptr(), total,
                                        ops._stream()), 'deva_mask_rle_write')
        return n, bounds
    return dict(index=index, scratch=torch.zeros(max(words, 1), dtype=torch.int32)), run


# ------------------------------------------------------------------------------------------ detector output
def _detections(policy):
    def build(seed):
        import detection_case as DC
        n = 22
        inputs = dict(masks=DC.masks(24, 36, extra=4, seed=seed).to(torch.uint8), scores=DC.scores(n, seed))
        return inputs, lambda i, mark: ops.detection_assemble(i['masks'], (48, 72), policy, scores=i['scores'],
                                                              overlap_threshold=0.7, consistent_ids=policy == 'text')
    case('detection_assemble_' + policy, 'deva_detection_assemble')(build)


for _policy in ops.DETECTION_POLICIES:
    _detections(_policy)


def _proposal_inputs(seed, h=29, w=53):
    import proposal_case as PC
    a, b = PC.batch(h, w, 64, seed), PC.batch(h, w, 3, seed + 50)
    return dict(logits_a=a[0], iou_a=a[1], logits_b=b[0], iou_b=b[1])


@case('proposals', 'deva_proposal_begin', 'deva_proposal_batch', 'deva_proposal_finish', 'deva_proposal_gather')
def _(seed):
    import proposal_case as PC
    p = PC.params()
    nms = p.pop('box_nms_thresh')

    def run(i, mark):
        state = ops.proposal_state(29, 53, 128, dev())
        ops.proposal_begin(state)
        ops.proposal_batch(state, i['logits_a'], i['iou_a'], **p)
        ops.proposal_batch(state, i['logits_b'], i['iou_b'], **p)
        mark()                                         # proposal_finish reads its table back (the frame's one synchronisation)
        return ops.proposal_finish(state, nms)
    return _proposal_inputs(seed), run


@case('proposal_finish_table', 'deva_proposal_begin', 'deva_proposal_batch', 'deva_proposal_finish', raw=True)
def _(seed):
    """begin / batch / finish without the read-back: the result table as the device holds it"""
    import proposal_case as PC
    p = PC.params()
    nms = p.pop('box_nms_thresh')

    def run(i, mark):
        from deva.hip import check, lib
        state = ops.proposal_state(29, 53, 128, dev())
        ops.proposal_begin(state)
        ops.proposal_batch(state, i['logits_a'], i['iou_a'], **p)
        ops.proposal_batch(state, i['logits_b'], i['iou_b'], **p)
        state.result.zero_()
        check(lib().deva_proposal_finish(state.capacity, float(nms), state.scratch.data_ptr(), state.scratch_bytes,
                                         state.result.data_ptr(), ops._stream()), 'deva_proposal_finish')
        kept = state.result[:3].clone()
        return kept, state.result.clone()[:4]
    return _proposal_inputs(seed), run


@case('proposal_gather', 'deva_proposal_begin', 'deva_proposal_batch', 'deva_proposal_finish', 'deva_proposal_gather', raw=True)
def _(seed):
    """the whole frame without a read-back: the kept count comes from the CPU contract.  (The gather kernel skips a keep
    slot outside the arena, so it is safe on a keep list that is not written yet; its output is zero-filled on the
    stream, which wipes whatever a gather that ran too early wrote.)"""
    import emu_proposals as EP
    import proposal_case as PC
    p = PC.params()
    nms = p.pop('box_nms_thresh')
    inputs = _proposal_inputs(seed)
    host = EP.proposal_state(29, 53, 128, 'cpu')
    EP.proposal_begin(host)
    EP.proposal_batch(host, inputs['logits_a'], inputs['iou_a'], **p)
    EP.proposal_batch(host, inputs['logits_b'], inputs['iou_b'], **p)
    kept = int(EP.proposal_finish(host, nms).masks.shape[0])
    assert 0 < kept <= 128

    def run(i, mark):
        from deva.hip import check, lib
        state = ops.proposal_state(29, 53, 128, dev())
        ops.proposal_begin(state)
        ops.proposal_batch(state, i['logits_a'], i['iou_a'], **p)
        ops.proposal_batch(state, i['logits_b'], i['iou_b'], **p)
        check(lib().deva_proposal_finish(state.capacity, float(nms), state.scratch.data_ptr(), state.scratch_bytes,
                                         state.result.data_ptr(), ops._stream()), 'deva_proposal_finish')
        masks = torch.zeros((kept, 29, 53), dtype=torch.uint8, device=dev())
        check(lib().deva_proposal_gather(state.arena.data_ptr(), state.capacity, 29, 53, state.scratch.data_ptr(),
                                         state.scratch_bytes, kept, masks.data_ptr(), ops._stream()), 'deva_proposal_gather')
        return state.result[:3].clone(), masks
    return inputs, run


def _boxes(g, m, integer):
    xy = torch.rand(m, 2, generator=g) * 40
    wh = torch.rand(m, 2, generator=g) * 20 + 1
    boxes = torch.cat([xy, xy + wh], 1)
    return boxes.round().to(torch.int32) if integer else boxes.contiguous()


@case('box_nms', 'deva_box_nms')
def _(seed):
    g = G(seed)

    def run(i, mark):
        mark()                                         # the wrapper reads the count back
        return ops.box_nms(i['boxes'], i['scores'], 0.5)
    return dict(boxes=_boxes(g, 70, True), scores=torch.rand(70, generator=g)), run


@case('box_nms_list', 'deva_box_nms', raw=True)
def _(seed):
    g = G(seed)
    m = 70

    def run(i, mark):
        from deva.hip import check, lib
        keep = torch.full((m + 1,), -1, dtype=torch.int32, device=i['boxes'].device)
        nbytes = lib().deva_proposal_scratch(m)
        scratch = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device=i['boxes'].device)
        check(lib().deva_box_nms(i['boxes'].data_ptr(), i['scores'].data_ptr(), m, 0.5, scratch.data_ptr(), nbytes,
                                 keep.data_ptr(), keep.data_ptr() + 4 * m, ops._stream()), 'deva_box_nms')
        return keep[m:].clone()                        # (the list beyond the count is not written)
    return dict(boxes=_boxes(g, m, True), scores=torch.rand(m, generator=g)), run


@case('box_nms_xyxy', 'deva_box_nms_xyxy')
def _(seed):
    g = G(seed)
    m = 70

    def run(i, mark):
        packed = torch.full((m + 1,), -1, dtype=torch.int32, device=i['boxes'].device)
        ops.box_nms_xyxy(i['boxes'], i['scores'], 0.5, packed=packed)
        return packed[m:].clone()
    return dict(boxes=_boxes(g, m, False), scores=torch.rand(m, generator=g)), run


@case('box_mask_select', 'deva_box_mask_select')
def _(seed):
    g = G(seed)
    return (dict(logits=rand(g, 5, 3, 29, 53), scores=torch.rand(5, 3, generator=g)),
            lambda i, mark: ops.box_mask_select(i['logits'], i['scores'], 0.0))


@case('prompt_points', 'deva_prompt_points')
def _(seed):
    import prompt_case as PC

    def run(i, mark):
        points, labels, count = ops.prompt_points(i['mask'], i['grid'])
        return labels, count                           # (the rows of points beyond the count are not written)
    return dict(mask=PC.forward_mask(96, 128, seed), grid=PC.grid(8) * (0.9 + 0.1 * (seed % 2))), run


# ------------------------------------------------------------------------------------------ scorers
@case('panoptic_counts', 'deva_metrics_panoptic_counts')
def _(seed):
    import panoptic_case as NC
    from deva.hip import metrics
    gt_table, pred_table = NC.id_pool(20, 1), NC.id_pool(30, 2)
    gt = NC.blocky(29, 53, np.concatenate([[0], gt_table, [7777777]]), seed, cell=7).astype(np.int32)
    pred = NC.blocky(29, 53, np.concatenate([[0], pred_table, [424242, -5]]), seed + 1000, cell=9)
    tabs = [D(torch.from_numpy(t.astype(np.int32))) for t in (gt_table, pred_table)]
    return (dict(gt=torch.from_numpy(gt), pred=torch.from_numpy(pred)),
            lambda i, mark: metrics.panoptic_counts(i['gt'], tabs[0], i['pred'], tabs[1], validate=False))


@case('boundary_counts', 'deva_vos_boundary_counts')
def _(seed):
    import vos_case as VC
    from deva.hip import vos_metrics
    gt, pred, ids = VC.case(29, 53, 5, seed)
    table = D(torch.from_numpy(ids.astype(np.int32)))
    return (dict(gt=torch.from_numpy(gt.astype(np.int32)), pred=torch.from_numpy(pred)),
            lambda i, mark: vos_metrics.boundary_counts(i['gt'], i['pred'], table, validate=False))


def covered():
    return sorted({name for c in CASES for name in c.covers})
