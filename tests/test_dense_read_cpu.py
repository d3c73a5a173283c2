"""top_k=None (the full-softmax memory read) without a GPU: configuration, the host wiring of MemoryManager on an
emulation of ops.dense_read (defined here, in the style of emu_ops), the refusal of the sharded modes, and the ABI."""
import pytest
import torch

import emu_ops
from oracle import deva_oracle as O
from workload import synth

torch.set_grad_enabled(False)


def dense_read(key_long, shr_long, n_long, key_work, shr_work, n_work, qk, qe, val_long, val_work, out, usage_fix=None,
               return_probs=False):
    """CPU statement of deva_dense_read: full softmax with max subtraction over the bank [long | work], usage as the sum
    over the queries of each weight in 2^40 fixed point (truncated per weight), read-out per object"""
    mk = emu_ops._bank(key_long, n_long, key_work, n_work)
    ms = emu_ops._bank(shr_long, n_long, shr_work, n_work)
    a_sq = mk.pow(2) @ qe
    two_ab = 2 * (mk @ (qk * qe))
    b_sq = (qe * qk.pow(2)).sum(0, keepdim=True)
    sim = (-a_sq + two_ab - b_sq) * ms[:, None] / 8.0
    e = torch.exp(sim - sim.max(0, keepdim=True)[0])
    p = e / e.sum(0, keepdim=True)
    n = p.shape[0]
    if usage_fix is not None:
        usage_fix[:n] += (p.double() * emu_ops.TWO40).long().sum(1)
    for o in range(len(val_work)):
        v = emu_ops._bank(val_long[o] if n_long else None, n_long, val_work[o], n_work)  # [n, cv]
        out[o].view(v.shape[1], -1).copy_(v.t() @ p)
    return p if return_probs else None


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    from deva.hip import ops
    monkeypatch.setattr(ops, 'dense_read', dense_read)


def test_top_k_none_constructs():
    from deva.inference.memory_manager import MemoryManager
    mm = MemoryManager(synth.base_config(top_k=None))
    assert mm.top_k is None
    mm.update_config(synth.base_config(top_k=None))
    assert mm.top_k is None
    mm.update_config(synth.base_config(top_k=30))
    assert mm.top_k == 30


def test_integer_limits_unchanged():
    from deva.inference.memory_manager import MemoryManager
    for bad in (0, 65):
        with pytest.raises(ValueError, match='top_k'):
            MemoryManager(synth.base_config(top_k=bad))
    assert MemoryManager(synth.base_config(top_k=64)).top_k == 64


def test_sharded_modes_refuse_top_k_none():
    from deva.inference.memory_manager import MemoryManager
    mm = MemoryManager(synth.base_config(top_k=None))
    with pytest.raises(ValueError, match='shard_queries: top_k=None'):
        mm.shard_queries()
    with pytest.raises(ValueError, match='shard_bank: top_k=None'):
        mm.shard_bank()
    # a sharded manager cannot switch to the full softmax either
    mm = MemoryManager(synth.base_config(top_k=30))
    mm._shard_group, mm._shard_mode = object(), 'queries'
    with pytest.raises(ValueError, match='top_k=None'):
        mm.update_config(synth.base_config(top_k=None))
    assert mm.top_k == 30


def test_emulation_matches_the_oracle_formula():
    """the emulation above against O.get_similarity + O.dense_affinity(sim, None), with the bank split in two"""
    n, hw = 300, 70
    mk, ms, qk, qe = synth.affinity_inputs(n, hw, seed=1)
    vals = synth.value_inputs(2, 16, n, seed=1)
    rows, shr = mk.t().contiguous(), ms.reshape(-1)
    vt = [v.t().contiguous() for v in vals]
    out = torch.empty(2, 16, hw)
    fix = torch.zeros(n, dtype=torch.int64)
    p = dense_read(rows[:100], shr[:100], 100, rows[100:], shr[100:], n - 100, qk, qe, [v[:100] for v in vt],
                   [v[100:] for v in vt], out, fix, return_probs=True)
    aff, use = O.dense_affinity(O.get_similarity(mk, ms, qk, qe), None)
    assert (p - aff).abs().max().item() <= 1e-6
    assert (fix.double() / 2**40 - use.double()).abs().max().item() <= 1e-5
    assert (out - torch.einsum('ocn,nq->ocq', vals, aff)).abs().max().item() <= 1e-4


def test_free_running_clip_with_long_term_memory_matches_the_oracle(emu, recipe_state_dict):
    """96x128, two objects, memory every other frame; long-term memory engages after the third memory frame and
    later frames read [long | work] with the full softmax"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    sd, _ = recipe_state_dict
    cfg = synth.base_config(top_k=None, mem_every=2, max_mid_term_frames=3, min_mid_term_frames=2, num_prototypes=32)
    net = DEVA(cfg)
    net.load_weights(sd)
    hip, orc = DEVAInferenceCore(net, cfg), O.OracleCore(sd, cfg)
    stream = synth.FrameStream(96, 128, seed=2)
    mask = synth.box_mask(96, 128, 2)
    worst, lt = 0.0, False
    for t in range(8):
        img = stream.next()
        a = hip.step(img, mask if t == 0 else None, [1, 2] if t == 0 else None)
        b = orc.step(img, mask if t == 0 else None, [1, 2] if t == 0 else None)
        worst = max(worst, (a - b).abs().max().item())
        lt = lt or hip.memory._long_term_mem_available()
    assert lt, 'long-term memory never engaged'
    assert worst <= 1e-3, worst


def test_abi_exports_the_dense_read():
    from deva import hip
    import __graft_entry__  # noqa: F401  (puts the package on the path)
    if not __import__('os').path.exists(hip.LIB_PATH):
        __graft_entry__.build()
    L = hip.lib()
    assert hip.ABI_VERSION == 11 and L.deva_hip_version() == 11
    assert 'deva_dense_read' in hip.SIGNATURES and 'deva_dense_read_scratch' in hip.SIGNATURES
    # bounded scratch: the 4K bank of 50 000 tokens x 32 400 queries stays under 256 MiB
    assert 0 < L.deva_dense_read_scratch(50000, 32400) <= 256 << 20
    assert L.deva_dense_read_scratch(10000, 8160) <= 256 << 20
    # argument validation before any launch
    assert L.deva_dense_read(None, None, 0, None, None, 0, None, None, 0, 0, None, None, 0, None, None, None, 0, None,
                             None) != 0
    assert b'deva_dense_read' in L.deva_hip_last_error()
    # a scratch smaller than deva_dense_read_scratch is refused before the first launch
    assert L.deva_dense_read(None, None, 0, 4096, 8192, 100, 4096, 8192, 64, 0, None, None, 0, None, None, 4096, 16, None,
                             None) != 0
    assert b'scratch' in L.deva_hip_last_error()
