"""What the stream tests (tests/test_gpu_v_streams.py) rest on, checked without a GPU: every entry point of the three
headers that takes `void* stream` has a case in the probe table or a written reason; the table's builders, runs and
comparisons execute on the CPU contracts (a typo does not cost a GPU session); and the bookkeeping of the per-stream
scratch caches of deva/hip/ops.py -- key, bound, eviction, the fall-back count across evictions -- on CPU tensors with
made-up stream handles."""
import os
import re

import pytest
import torch

import abi_util
import emu_ops
import gpu_util
import stream_cases as SC
import stream_probe as SP
from deva.hip import DevaHipError, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('deva_hip.h', 'deva_metrics.h', 'deva_vos_metrics.h')
torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------ the headers
def streamed_entry_points():
    """the functions of include/*.h with a `void* stream` parameter (comments stripped like abi_util.declared)"""
    found = set()
    for header in HEADERS:
        text = open(os.path.join(ROOT, 'include', header)).read()
        text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
        text = re.sub(r'//[^\n]*', '', text)
        for name, params in re.findall(r'\b(deva_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S):
            if re.search(r'\bvoid\s*\*\s*stream\b', params):
                found.add(name)
    return found


def test_every_streamed_entry_point_has_a_case_or_a_reason():
    streamed = streamed_entry_points()
    assert len(streamed) >= 60 and 'deva_conv2d' in streamed and 'deva_vos_boundary_counts' in streamed
    declared = {n for h in HEADERS for n in abi_util.declared(os.path.join(ROOT, 'include', h))}
    assert streamed <= declared
    covered = set(SC.covered())
    assert not covered & set(SC.NOT_PROBED), 'an entry point is both covered and excused'
    assert all(len(reason) > 20 for reason in SC.NOT_PROBED.values())
    missing = streamed - covered - set(SC.NOT_PROBED)
    assert not missing, f'streamed entry points without a case in tests/stream_cases.py: {sorted(missing)}'
    unknown = (covered | set(SC.NOT_PROBED)) - streamed
    assert not unknown, f'the table names entry points that take no stream (or do not exist): {sorted(unknown)}'
    assert set(SC.BEHIND_OWN_SYNC) <= covered
    assert len({c.name for c in SC.CASES}) == len(SC.CASES)


def test_the_second_paths_the_table_must_hold():
    names = {c.name for c in SC.CASES}
    for wanted in ('conv_q4', 'conv_q4_split_k', 'conv_wino', 'conv_cout1_rows', 'conv_cout1_table', 'conv_f16_amp',
                   'conv_split_in_range', 'conv_split_fp32_rerun', 'stem7x7_recomputed_tile', 'affinity_prefilter_fallback',
                   'affinity_read_prepared', 'dense_read_two_objects', 'affinity_read_flag_stats', 'panoptic_counts',
                   'boundary_counts', 'detection_assemble_suppress_small', 'detection_assemble_prefer_small',
                   'detection_assemble_text'):
        assert wanted in names, wanted


# ------------------------------------------------------------------------------------------ the table, dry
@pytest.fixture
def dry(monkeypatch):
    """what DEVA_TEST_DRYRUN=1 sets up for the -m gpu files (tests/conftest.py), for this process"""
    emu_ops.install(monkeypatch)
    SC.install_contracts(monkeypatch)
    monkeypatch.setattr(gpu_util, 'dev', lambda: torch.device('cpu'))
    monkeypatch.setattr(SP, 'DRYRUN', True)
    monkeypatch.setattr(SC, 'DRYRUN', True)


@pytest.mark.parametrize('position', range(len(SC.CASES)), ids=[c.name for c in SC.CASES])
def test_the_table_runs_on_the_cpu_contracts(position, dry):
    c = SC.CASES[position]
    real, run = c.build(1000 + 2 * position)
    decoy, _ = c.build(1001 + 2 * position)
    SP.check_inputs(real, decoy)
    if c.raw:
        return                                   # (its run calls the library with device pointers)
    want = SP.probe(run, real, decoy, c.name)
    assert want and any(isinstance(v, torch.Tensor) and v.numel() for _, v in want)
    if c.name in SC.INPUT_INDEPENDENT:
        return
    # the decoys give another answer: a launch that read them would be seen
    other = SP.to_host(run({k: v.clone() for k, v in decoy.items()}, lambda: None))
    assert SP.differences(want, other), f'{c.name}: the decoy inputs give the same outputs as the real ones'


def test_the_comparison_is_bit_identity():
    a = [('out', torch.tensor([0.0, float('nan')])), ('n', 3)]
    assert SP.differences(a, [('out', torch.tensor([0.0, float('nan')])), ('n', 3)]) == []
    assert SP.differences(a, [('out', torch.tensor([-0.0, float('nan')])), ('n', 3)])          # the sign of zero is a bit
    assert SP.differences(a, [('out', torch.tensor([0.0, float('nan')])), ('n', 4)])
    assert SP.differences(a, [('out', torch.tensor([0.0, float('nan')]).double()), ('n', 3)])
    assert SP.differences(a, [('other', torch.tensor([0.0, float('nan')])), ('n', 3)])
    with pytest.raises(AssertionError, match='equal the real'):
        SP.check_inputs(dict(x=torch.ones(3)), dict(x=torch.ones(3)))


# ------------------------------------------------------------------------------------------ the caches
@pytest.fixture
def fake_streams(monkeypatch):
    """empty caches, small sizes, and a settable 'current stream' handle"""
    current = [0]
    for name in ('_WORKSPACE', '_SPLIT_FLAGS', '_SPLIT_EVICTED', '_AFF_WS', '_DENSE_WS'):
        monkeypatch.setattr(ops, name, {})
    monkeypatch.setattr(ops, '_WORKSPACE_ELEMS', 16)
    monkeypatch.setattr(ops, '_SPLIT_RING', 4)
    monkeypatch.setattr(ops, '_stream', lambda device=None: current[0])
    return current


def _raise_flag(device='cpu'):
    """what a split convolution whose input left the fp16 range does to the slot it was given"""
    ops._split_flag(device)
    ring, nxt = ops._SPLIT_FLAGS[ops._stream_key(device)]
    ring[nxt - 1] = 1


def test_the_key_is_the_device_index_and_the_stream(fake_streams, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    fake_streams[0] = 0x5151
    assert ops._stream_key(torch.device('cuda')) == ops._stream_key(torch.device('cuda:0')) == ops._stream_key('cuda:0') == (0, 0x5151)
    assert ops._stream_key(torch.device('cuda:1')) == (1, 0x5151)
    assert ops._stream_key('cpu') == (-1, 0x5151)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 1)
    assert ops._stream_key(torch.device('cuda')) == (1, 0x5151)


def test_caches_hold_at_most_the_bound_and_drop_the_oldest(fake_streams):
    bound = ops._MAX_STREAM_CACHES
    first = {}
    for s in range(1, bound + 4):
        fake_streams[0] = s
        ws, aff = ops._workspace('cpu'), ops._affinity_workspace(10, 'cpu')
        assert ops._workspace('cpu') is ws and ops._affinity_workspace(10, 'cpu') is aff     # one entry per stream, kept
        first.setdefault(s, (ws, aff))
        assert len(ops._WORKSPACE) == len(ops._AFF_WS) == min(s, bound)
    assert list(ops._WORKSPACE) == [(-1, s) for s in range(4, bound + 4)] == list(ops._AFF_WS)
    fake_streams[0] = 1                                            # an evicted stream gets a new buffer on demand
    assert ops._workspace('cpu') is not first[1][0] and len(ops._WORKSPACE) == bound
    big = ops._affinity_workspace(3 << 20, 'cpu')                  # growing an entry evicts nobody
    assert big.numel() >= 3 << 20 and len(ops._AFF_WS) == bound and (-1, 1) in ops._AFF_WS
    with pytest.raises(DevaHipError, match='no read has run'):
        fake_streams[0] = 99
        ops.affinity_last_read_flag('cpu')


def test_the_dense_read_scratch_is_bounded_like_its_neighbours(fake_streams):
    bound = ops._MAX_STREAM_CACHES
    qk = torch.zeros(64, 40)
    for s in range(1, bound + 4):
        fake_streams[0] = s
        with pytest.raises(DevaHipError):        # (host tensors: refused at the launch, after the scratch was set up)
            ops.dense_read(None, None, 0, torch.zeros(80, 64), torch.zeros(80), 80, qk, qk, [None], [torch.zeros(80, 512)],
                           torch.zeros(1, 512, 40))
        assert len(ops._DENSE_WS) == min(s, bound) and (-1, s) in ops._DENSE_WS
    assert list(ops._DENSE_WS) == [(-1, s) for s in range(4, bound + 4)]
    kept = ops._DENSE_WS[(-1, bound + 3)]
    with pytest.raises(DevaHipError):
        ops.dense_read(None, None, 0, torch.zeros(80, 64), torch.zeros(80), 80, qk, qk, [None], [torch.zeros(80, 512)],
                       torch.zeros(1, 512, 40))
    assert ops._DENSE_WS[(-1, bound + 3)] is kept and len(ops._DENSE_WS) == bound


def test_the_fallback_count_survives_wraps_evictions_and_releases(fake_streams):
    bound = ops._MAX_STREAM_CACHES
    raised = 0
    for s in range(1, bound + 4):
        fake_streams[0] = s
        for call in range(6):                    # a ring of 4 slots: wraps once per stream
            if (s + call) % 3 == 0:
                _raise_flag()
                raised += 1
            else:
                ops._split_flag('cpu')
        assert len(ops._SPLIT_FLAGS) == min(s, bound)
        assert ops.split_fallbacks('cpu') == raised, s
    assert sum(ops._SPLIT_EVICTED.values()) > 0 and set(ops._SPLIT_EVICTED) == {-1}
    assert list(ops._SPLIT_FLAGS) == [(-1, s) for s in range(4, bound + 4)]
    fake_streams[0] = 5
    ops._workspace('cpu'), ops._affinity_workspace(10, 'cpu')
    ops.release_stream_scratch('cpu')
    assert all((-1, 5) not in c for c in (ops._WORKSPACE, ops._AFF_WS, ops._DENSE_WS, ops._SPLIT_FLAGS))
    assert ops.split_fallbacks('cpu') == raised
    ops.release_stream_scratch('cpu')            # nothing left: a no-op
    assert ops.split_fallbacks('cpu') == raised
