"""Test-time ensemble without a GPU: the three entry points on the ABI, the CPU contracts of the ops
(tests/emu_ensemble.py) against a literal restatement of the reference protocol, `EnsembleInferenceCore` on the emulated
ops against the composition of per-variant oracle runs, and its argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import emu_ensemble
import emu_ops
import ensemble_case as EC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('deva_scores_u8', 'deva_ensemble_index_mask', 'deva_flip_w')


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    emu_ensemble.install(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)


def _network(state_dict, **extra):
    from deva.model.network import DEVA
    net = DEVA(EC.clip_config(**extra))
    net.load_weights(state_dict)
    return net


# ------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_exported_declared_and_bound():
    from deva import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'deva_hip.h')).read()
    for name in NAMES:
        assert hasattr(handle, name), f'{name} not exported'
        assert re.search(r'\bint ' + name + r'\s*\(', header), f'{name} not declared'
        assert name in hip.SIGNATURES
    assert hip.ABI_VERSION == 11 and hip.lib().deva_hip_version() == 11  # additive: the version does not move
    assert re.search(r'#define DEVA_HIP_ABI_VERSION 11\b', header)
    assert hip.ENSEMBLE_MAX_VARIANTS == 8 and re.search(r'#define DEVA_ENSEMBLE_MAX_VARIANTS 8\b', header)


def test_variant_mirror_has_the_c_layout(tmp_path):
    from deva.hip import EnsembleVariant
    import subprocess
    fields = [f[0] for f in EnsembleVariant._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_hip.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(deva_ensemble_variant));\n' +
                   ''.join(f'printf("%zu\\n", offsetof(deva_ensemble_variant, {f}));\n' for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(EnsembleVariant)
    assert vals[1:] == [getattr(EnsembleVariant, f).offset for f in fields]


def test_argument_errors_before_any_launch():
    """the launchers refuse bad arguments on the host: no variants, more than 8, differing channel counts, overlapping
    strides, an element size flip_w does not copy"""
    from deva import hip
    L = hip.lib()
    V = hip.EnsembleVariant
    ok = V(4096, 64 * 48, 64, 3, 48, 64, 0)                   # (pointers are never dereferenced: validation fails first)
    assert L.deva_ensemble_index_mask((V * 1)(ok), 0, 8, 8, 1, None, 0, 8192, None) != 0
    assert b'variants' in L.deva_hip_last_error()
    assert L.deva_ensemble_index_mask((V * 9)(*[ok] * 9), 9, 8, 8, 1, None, 0, 8192, None) != 0
    assert b'variants' in L.deva_hip_last_error()
    other = V(4096, 64 * 48, 64, 4, 48, 64, 1)
    assert L.deva_ensemble_index_mask((V * 2)(ok, other), 2, 8, 8, 1, None, 0, 8192, None) != 0
    assert b'channels' in L.deva_hip_last_error()
    overlapping = V(4096, 64 * 47, 64, 3, 48, 64, 0)
    assert L.deva_scores_u8(ctypes.byref(overlapping), 8, 8, 8192, None) != 0
    assert b'strides' in L.deva_hip_last_error()
    assert L.deva_flip_w(4096, 8192, 4, 4, 2, None) != 0 and b'1, 3, 4 or 8' in L.deva_hip_last_error()
    assert L.deva_flip_w(4096, 4096, 4, 4, 4, None) != 0


# ------------------------------------------------------------------------------------------ contracts
def _soft(g, c, h, w):
    p = torch.softmax(torch.randn(c, h, w, generator=g) * 2, dim=0)
    p[:, :3, :5] = 1.0 / c  # exact ties: the first maximum must win
    return p


@pytest.mark.parametrize('c,sizes,out', [(3, [(40, 56)], (40, 56)), (4, [(24, 32), (40, 56), (33, 47)], (40, 56)),
                                         (1, [(8, 8), (9, 7)], (20, 21)), (7, [(30, 44)] * 8, (61, 90))])
def test_contracts_match_the_protocol_restatement(c, sizes, out):
    g = torch.Generator().manual_seed(c * 100 + len(sizes))
    probs = [_soft(g, c, h, w) for h, w in sizes]
    flips = [bool(k % 2) for k in range(len(sizes))]
    lut = torch.tensor([0] + [100 + 7 * i for i in range(1, c)], dtype=torch.int64)
    vols = []
    for p, f in zip(probs, flips):
        want, _ = EC.restate_scores(p, out, f)
        got = emu_ensemble.scores_u8(p, out, f)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
        vols.append(want)
    got = emu_ensemble.ensemble_index_mask(probs, out, flips, lut, quantize=True)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), EC.restate_merge(vols, lut.numpy()))
    if all(s == out for s in sizes) and not any(flips):
        assert int(emu_ensemble.ensemble_index_mask(probs, out, flips)[:3, :5].abs().sum()) == 0  # ties -> channel 0
    # one unflipped fp32 variant is the single-run tail
    one = emu_ensemble.ensemble_index_mask(probs[:1], out, [False], lut, quantize=False)
    assert torch.equal(one, emu_ops.index_mask(probs[0], out, lut))
    assert torch.equal(emu_ensemble.ensemble_index_mask(probs[:1], out, [True], lut, quantize=False), one.flip(-1))


def test_flip_contract():
    g = torch.Generator().manual_seed(1)
    frame = torch.randint(0, 256, (5, 7, 3), generator=g, dtype=torch.uint8)
    assert torch.equal(emu_ensemble.flip_w(frame), torch.flip(frame, dims=[1]))
    planes = torch.randn(2, 5, 7, generator=g)
    assert torch.equal(emu_ensemble.flip_w(planes), torch.flip(planes, dims=[-1]))


# ------------------------------------------------------------------------------------------ end to end
def test_ensemble_core_matches_oracle_composition(emu, peaky_state_dict):
    """the smoke clip (96 x 128, 3 objects, mem_every=2, 4 frames, peaky recipe) at the native size and at 120, each
    with and without the flip (K = 4): the online ensemble on the emulated ops against one oracle run per variant
    merged by the protocol restatement"""
    oracle = EC.oracle_composition(peaky_state_dict)
    masks, scores, core = EC.run_ensemble(_network(peaky_state_dict), torch.device('cpu'))
    EC.check_end_to_end(masks, scores, core, oracle, 'emulated ops')
    assert len(core.cores) == 4 and core.variants == EC.VARIANTS


def test_step_without_scores_returns_the_same_mask(emu, peaky_state_dict):
    from deva.inference.ensemble import EnsembleInferenceCore
    net = _network(peaky_state_dict)
    a = EnsembleInferenceCore(net, EC.clip_config(), sizes=(-1,), flips=(False, True))
    b = EnsembleInferenceCore(net, EC.clip_config(), sizes=(-1,), flips=(False, True))
    mask = EC.clip_mask()
    for t, frame in enumerate(EC.clip_frames()[:2]):
        args = (frame, mask if t == 0 else None, EC.OBJECTS if t == 0 else None)
        plain = a.step(*args)
        with_scores, vols = b.step(*args, return_scores=True)
        assert torch.is_tensor(plain) and torch.equal(plain, with_scores) and len(vols) == 2
        assert tuple(plain.shape) == (EC.H, EC.W) and tuple(vols[0].shape) == (4, EC.H, EC.W)


# ------------------------------------------------------------------------------------------ errors
def test_more_than_eight_variants(peaky_state_dict):
    from deva.inference.ensemble import EnsembleInferenceCore
    net = _network(peaky_state_dict)
    with pytest.raises(ValueError):
        EnsembleInferenceCore(net, EC.clip_config(), sizes=(-1, 120, 140, 160, 180), flips=(False, True))
    with pytest.raises(ValueError):
        EnsembleInferenceCore(net, EC.clip_config(), sizes=(), flips=(False, True))
    assert len(EnsembleInferenceCore(net, EC.clip_config(), sizes=(-1, 120, 140, 160), flips=(False, True)).cores) == 8


def test_mismatched_object_tables(emu, peaky_state_dict):
    from deva.inference.ensemble import EnsembleInferenceCore
    core = EnsembleInferenceCore(_network(peaky_state_dict), EC.clip_config(), sizes=(-1,), flips=(False, True))
    core.cores[1].object_manager.all_historical_object_ids.add(2)  # variant 1 must draw another id for object 2
    with pytest.raises(RuntimeError, match='object table'):
        core.step(EC.clip_frames()[0], EC.clip_mask(), EC.OBJECTS)


def test_sharded_memory_is_refused(emu, peaky_state_dict):
    from deva.inference.ensemble import EnsembleInferenceCore
    core = EnsembleInferenceCore(_network(peaky_state_dict), EC.clip_config(), sizes=(-1,), flips=(False, True))
    core.cores[0].memory._shard_group = object()
    with pytest.raises(NotImplementedError):
        core.step(EC.clip_frames()[0], EC.clip_mask(), EC.OBJECTS)
