"""top_k=None: the full-softmax memory read (csrc/dense_read.hip, ops.dense_read) against the CPU formula of the oracle
(get_similarity + dense_affinity(sim, None) + a dense fp64 read-out), and end to end through MemoryManager,
spatial_alignment and step_clips.  Weights and usage within 1e-5 relative, read-outs within 1e-5 of max |read-out|;
results independent of where the bank splits into long-term / working rows, bit for bit."""
import pytest
import torch

from deva.hip import ops
from gpu_util import dev, to_dev
from oracle import deva_oracle as O
from workload import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _read(mk, ms, qk, qe, vals, n_long, probs=False):
    """mk [64,N] channel-major, vals [objects, cv, N] -> token-major device arenas split at n_long, one dense read;
    -> (read-out [objects, cv, hw], usage [N] (float64), softmax [N, hw] or None) on the host"""
    n, hw = mk.shape[1], qk.shape[1]
    rows, shr = mk.t().contiguous(), ms.reshape(-1).contiguous()
    kl, sl = (to_dev(rows[:n_long].contiguous()), to_dev(shr[:n_long].contiguous())) if n_long else (None, None)
    kw, sw = to_dev(rows[n_long:].contiguous()), to_dev(shr[n_long:].contiguous())
    vt = [v.t().contiguous() for v in vals]
    vl = [to_dev(v[:n_long].contiguous()) if n_long else None for v in vt]
    vw = [to_dev(v[n_long:].contiguous()) for v in vt]
    out = torch.full((len(vals), vals.shape[1], hw), float('nan'), device=dev())
    fix = torch.zeros(n, dtype=torch.int64, device=dev())
    p = ops.dense_read(kl, sl, n_long, kw, sw, n - n_long, to_dev(qk), to_dev(qe), vl, vw, out, fix, return_probs=probs)
    torch.cuda.synchronize()
    return out.cpu(), fix.cpu().double() / 2**40, (p.cpu() if probs else None)


def _reference(mk, ms, qk, qe, vals, cols, chunk=1024):
    """the oracle's formula, column chunk by column chunk (fp32 scores as the oracle computes them, softmax and read-out
    in fp64): -> (softmax chunks {start: [N, c]}, usage [N], read-out of the columns `cols` [objects, cv, len(cols)])"""
    hw = qk.shape[1]
    usage = torch.zeros(mk.shape[1], dtype=torch.float64)
    aff_cols, probs = [], {}
    for c0 in range(0, hw, chunk):
        sim = O.get_similarity(mk, ms, qk[:, c0:c0 + chunk], qe[:, c0:c0 + chunk])
        aff, use = O.dense_affinity(sim.double(), None)
        usage += use
        probs[c0] = aff
        sel = [c - c0 for c in cols if c0 <= c < c0 + chunk]
        if sel:
            aff_cols.append(aff[:, sel])
    readout = torch.einsum('ocn,nq->ocq', vals.double(), torch.cat(aff_cols, 1))
    return probs, usage, readout


def _check(tag, out, usage, p, mk, ms, qk, qe, vals, cols, rtol=1e-5):
    ref_p, ref_u, ref_r = _reference(mk, ms, qk, qe, vals, cols)
    if p is not None:
        for c0, a in ref_p.items():
            got = p[:, c0:c0 + a.shape[1]].double()
            err = ((got - a).abs() - rtol * a.abs()).max().item()
            assert err <= 1e-10, f'{tag}: weights beyond {rtol} relative ({err:.3e})'
    uerr = ((usage - ref_u).abs() - rtol * ref_u.abs()).max().item()
    assert uerr <= qk.shape[1] * 2.0**-40, f'{tag}: usage beyond {rtol} relative ({uerr:.3e})'
    rerr = (out[:, :, cols].double() - ref_r).abs().max().item() / ref_r.abs().max().item()
    assert rerr <= rtol, f'{tag}: read-out error {rerr:.3e} of max |read-out|'
    print(f'{tag}: read-out err {rerr:.2e} (of max), usage ok')


@pytest.mark.parametrize('n,hw,objs', [(80, 40, 2), (999, 129, 2), (5000, 1620, 1), (10000, 8160, 1)])
def test_kernel_against_the_cpu_formula(n, hw, objs):
    mk, ms, qk, qe = synth.affinity_inputs(n, hw, seed=n + hw, key_scale=1.0)
    vals = synth.value_inputs(objs, 512, n, seed=n)
    cols = list(range(hw)) if hw <= 1620 else sorted(set(torch.randint(0, hw, (256,), generator=torch.Generator().manual_seed(1)).tolist()))
    runs = {}
    for n_long in (0, n // 3):
        runs[n_long] = _read(mk, ms, qk, qe, vals, n_long, probs=True)
    a, b = runs[0], runs[n // 3]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), 'depends on the split point'
    assert bool(torch.isfinite(a[0]).all())
    _check(f'n{n}hw{hw}', *a, mk, ms, qk, qe, vals, cols)


def test_large_scores_keep_the_max_subtraction():
    """scores around -400: exp without the max subtraction underflows to 0/0 (the top-k branch's NaN); here the weights
    stay finite and match the oracle.  One fp32 ulp of such a score is 3e-5, so the bound is 1e-4 relative here"""
    n, hw = 3000, 500
    mk, ms, qk, qe = synth.affinity_inputs(n, hw, seed=5, key_scale=6.0)
    assert not bool(torch.isfinite(O.get_similarity(mk, ms, qk, qe).exp().sum(0).reciprocal()).all())
    vals = synth.value_inputs(1, 512, n, seed=2)
    out, usage, p = _read(mk, ms, qk, qe, vals, n // 2, probs=True)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(out).all())
    _check('large scores', out, usage, p, mk, ms, qk, qe, vals, list(range(hw)), rtol=1e-4)


def test_4k_bank_on_sampled_columns_in_bounded_memory():
    """(50 000, 32 400): 6.5 GB as a dense matrix; the read runs in a bounded scratch (p one query chunk at a time)"""
    n, hw = 50000, 32400
    mk, ms, qk, qe = synth.affinity_inputs(n, hw, seed=3, key_scale=1.0)
    vals = synth.value_inputs(1, 512, n, seed=4)
    n_long = 10000
    rows, shr = mk.t().contiguous(), ms.reshape(-1).contiguous()
    kl, sl, kw, sw = (to_dev(rows[:n_long].contiguous()), to_dev(shr[:n_long].contiguous()),
                      to_dev(rows[n_long:].contiguous()), to_dev(shr[n_long:].contiguous()))
    vt = vals[0].t().contiguous()
    vl, vw = to_dev(vt[:n_long].contiguous()), to_dev(vt[n_long:].contiguous())
    qkd, qed = to_dev(qk), to_dev(qe)
    out = torch.empty((1, 512, hw), device=dev())
    fix = torch.zeros(n, dtype=torch.int64, device=dev())
    ops._DENSE_WS.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.dense_read(kl, sl, n_long, kw, sw, n - n_long, qkd, qed, [vl], [vw], out, fix)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f'4K dense read: peak extra device memory {extra / 2**20:.1f} MiB')
    assert extra <= 256 << 20
    cols = sorted(set(torch.randint(0, hw, (512,), generator=torch.Generator().manual_seed(2)).tolist()))
    sim = O.get_similarity(mk, ms, qk[:, cols], qe[:, cols])
    aff, _ = O.dense_affinity(sim.double(), None)
    ref = vals[0].double() @ aff
    err = (out[0].cpu()[:, cols].double() - ref).abs().max().item() / ref.abs().max().item()
    assert err <= 1e-5, err
    use = fix.cpu().double() / 2**40
    assert abs(use.sum().item() - hw) <= 1e-3 * hw  # every query's weights sum to one


def test_lockstep_teacher_forced(recipe_state_dict):
    """top_k=None end to end, every stage teacher-forced against the oracle with the same config"""
    import lockstep
    from deva.model.network import DEVA
    P, _ = recipe_state_dict
    net = DEVA(synth.base_config())
    net.load_weights(P)
    worst = lockstep.run(net.to(dev()).eval(), P, 192, 256, 2, 5, dev(), top_k=None)
    print('top_k=None teacher-forced lock-step, worst relative stage errors:', {k: f'{v:.2e}' for k, v in worst.items()})


def _clip_config():
    # long-term memory engages after the third memory frame (frames 0, 2, 4), frame 5 reads [long | work]
    return synth.base_config(top_k=None, mem_every=2, max_mid_term_frames=3, min_mid_term_frames=2, num_prototypes=64)


def test_free_running_480p_two_objects_with_long_term_memory(recipe_state_dict):
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    P, _ = recipe_state_dict
    cfg = _clip_config()
    net = DEVA(cfg)
    net.load_weights(P)
    net = net.to(dev()).eval()
    hip, orc = DEVAInferenceCore(net, cfg), O.OracleCore(P, cfg)
    stream = synth.FrameStream(480, 864, seed=4)
    mask = synth.box_mask(480, 864, 2)
    worst, lt = 0.0, False
    for t in range(6):
        img = stream.next()
        a = hip.step(img.to(dev()), mask.to(dev()) if t == 0 else None, [1, 2] if t == 0 else None).cpu()
        b = orc.step(img, mask if t == 0 else None, [1, 2] if t == 0 else None)
        worst = max(worst, (a - b).abs().max().item())
        top2 = b.topk(2, dim=0).values
        clear = (top2[0] - top2[1]) > 2e-3
        assert torch.equal(a.argmax(0)[clear], b.argmax(0)[clear]), f'frame {t}: argmax differs'
        lt = lt or hip.memory._long_term_mem_available()
    print(f'top_k=None 480p free-running: max abs prob error {worst:.2e}, long-term memory engaged: {lt}')
    assert lt and worst <= 1e-3


def test_spatial_alignment_against_the_oracle_read(recipe_state_dict):
    """spatial_alignment with top_k=None: its read equals the oracle's full softmax + dense read-out, restated here"""
    import scenarios
    from deva.inference.consensus_associated import spatial_alignment
    from deva.inference.image_feature_store import ImageFeatureStore
    from deva.model.network import DEVA
    P, _ = recipe_state_dict
    cfg = synth.base_config(top_k=None)
    net = DEVA(cfg)
    net.load_weights(P)
    net = net.to(dev()).eval()
    frames, masks = scenarios.alignment_inputs(scenarios.ALIGNMENT)
    src_img, src_mask, tar_img = frames[0].to(dev()), masks[0].to(dev()), frames[1].to(dev())
    out = spatial_alignment(0, src_img, src_mask, 1, tar_img, net, ImageFeatureStore(net, no_warning=True), cfg)
    # restatement: the same network stages, the memory read by the oracle's formula on the CPU
    store = ImageFeatureStore(net, no_warning=True)
    no, h, w = src_mask.shape
    src_ms = store.get_ms_features(0, src_img[None])
    src_key, src_shr, _ = store.get_key(0, src_img[None])
    tar_ms = store.get_ms_features(1, tar_img[None])
    tar_key, _, tar_sel = store.get_key(1, tar_img[None])
    sensory = torch.zeros((1, no, 512, h // 16, w // 16), device=dev())
    value, sensory = net.encode_mask(src_img[None], src_ms, sensory, src_mask[None], is_deep_update=True,
                                     chunk_size=cfg['chunk_size'])
    hw = (h // 16) * (w // 16)
    sim = O.get_similarity(src_key[0].reshape(64, hw).cpu(), src_shr[0].reshape(1, hw).cpu(),
                           tar_key[0].reshape(64, hw).cpu(), tar_sel[0].reshape(64, hw).cpu())
    aff, _ = O.dense_affinity(sim, None)
    readout = (value[0].reshape(no, 512, hw).cpu() @ aff).reshape(1, no, 512, h // 16, w // 16).to(dev())
    _, _, ref = net.segment(tar_ms, readout, sensory, src_mask[None], chunk_size=cfg['chunk_size'], update_sensory=False)
    err = (out - ref).abs().max().item()
    print(f'spatial_alignment top_k=None: max abs err {err:.2e}')
    assert out.shape == ref.shape and err <= 1e-3


def test_step_clips_matches_sequential_steps(recipe_state_dict):
    """two top_k=None clips through step_clips: each core matches its own sequential step (the read is per clip)"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.multi_clip import step_clips
    from deva.model.network import DEVA
    P, _ = recipe_state_dict
    cfg = _clip_config()
    net = DEVA(cfg)
    net.load_weights(P)
    net = net.to(dev()).eval()
    seq = [DEVAInferenceCore(net, cfg) for _ in range(2)]
    bat = [DEVAInferenceCore(net, cfg) for _ in range(2)]
    streams = [synth.FrameStream(192, 256, seed=11 + i) for i in range(2)]
    masks = [synth.box_mask(192, 256, 1 + i).to(dev()) for i in range(2)]
    objs = [[1], [1, 2]]
    worst = 0.0
    for t in range(6):
        imgs = [s.next().to(dev()) for s in streams]
        ms = [m if t == 0 else None for m in masks]
        ob = [o if t == 0 else None for o in objs]
        a = [c.step(imgs[i], ms[i], ob[i]) for i, c in enumerate(seq)]
        b = step_clips(bat, imgs, ms, ob)
        worst = max(worst, max((x - y).abs().max().item() for x, y in zip(a, b)))
    print(f'step_clips top_k=None vs sequential: max abs prob difference {worst:.2e}')
    assert worst <= 1e-4
