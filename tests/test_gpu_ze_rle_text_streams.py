"""Do the launches and copies of `deva.hip.rle_text` go to the caller's stream?  The probe of tests/stream_probe.py as
tests/test_gpu_zb_mask_runs_streams.py uses it: the call runs on a side stream that is still blocked behind a delay kernel
and must be bit-identical to the default-stream run.  The probed buffers are the ones the call reads: the inputs are copied
over decoys (other valid inputs of the same shapes: the same masks in reverse order) in stream order before the call and
the decoys are put back after it, so a launch that left for the null stream would code or parse the decoys.  Neither
direction waits for anything before its `finish()`, which is called after the mark; `mask_runs.encode(text='device')` waits
once, for the total of the boundaries, and marks there."""
import os

import numpy as np
import pytest
import torch

import emu_rle_text as ET
import emu_runs as ER
import runs_case as RC
import stream_probe as SP
import rle_text_case as TC
from deva.hip import mask_runs, rle_text

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
H, W = 33, 67


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        ET.install(monkeypatch)
        ER.install(monkeypatch)


def _masks():
    return TC.blob_counts(H, W, 4) + TC.few_counts(H * W)[:3] + [TC.long_mask(TC.SCAN_CHUNK + 1, H * W, 5)]


def _same(got, want):
    flat = SP.flatten(want)
    assert [p for p, _ in got] == [p for p, _ in flat]
    assert all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b for (_, a), (_, b) in zip(got, flat))


def test_encode_text_on_a_blocked_side_stream():
    masks = _masks()
    real = dict(zip(('n', 'base', 'bounds'), (torch.from_numpy(a) for a in TC.to_bounds(masks))))
    decoy = dict(zip(('n', 'base', 'bounds'), (torch.from_numpy(a) for a in TC.to_bounds(masks[::-1]))))
    want = [TC.text_of(c) for c in masks]
    assert [TC.text_of(c) for c in masks[::-1]] != want

    def run(i, mark):
        pending = rle_text.encode_text(i['n'], i['base'], i['bounds'], (H, W), pending=True)
        mark()
        return pending.finish()
    _same(SP.probe(run, real, decoy, 'encode_text'), want)


def test_parse_on_a_blocked_side_stream():
    masks = _masks()

    def inputs(order):
        texts = [TC.text_of(c) for c in order]
        first = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
        return dict(chars=torch.frombuffer(bytearray(b''.join(texts)), dtype=torch.uint8), text_first=torch.from_numpy(first)), texts
    real, texts = inputs(masks)
    decoy, _ = inputs(masks[::-1])
    n, chars_len = len(masks), int(real['chars'].numel())
    words, flags = TC.run_words(texts, H * W)
    assert flags == 0 and not np.array_equal(words, TC.run_words([TC.text_of(c) for c in masks[::-1]], H * W)[0])

    def run(i, mark):
        device = i['chars'].device
        runs = torch.full((2 * n + 1 + chars_len,), -1, dtype=torch.int32, device=device)
        info = torch.full((2,), -1, dtype=torch.int64, device=device)
        scratch = torch.empty(2 * n, dtype=torch.int32, device=device)
        rle_text._launch_parse(i['chars'], chars_len, i['text_first'], n, H, W, scratch, runs, runs.numel(), info)
        return runs[:words.size], info
    _same(SP.probe(run, real, decoy, 'parse'), (torch.from_numpy(words), torch.tensor([0, words.size], dtype=torch.int64)))


@pytest.mark.parametrize('form', ['default', 'capacity'])
def test_encode_with_text_on_the_device_on_a_blocked_side_stream(form):
    planes = RC.byte_stack(H, W)[1]
    decoy = np.ascontiguousarray(planes[::-1, ::-1, ::-1])
    want = RC.records(planes, None, 'bytes', stats=True)
    assert RC.records(decoy, None, 'bytes', stats=True) != want
    total = RC.statement(planes)['total']

    def as_tensors(records):
        return [(r['counts'], r['area'], str(r['bbox'])) for r in records]

    def run(i, mark):
        if form == 'default':
            return as_tensors(mask_runs.encode(i['planes'], form='bytes', stats=True, text='device', before_wait=mark))
        pending = mask_runs.encode(i['planes'], form='bytes', stats=True, text='device', capacity=total + 7)
        mark()
        return as_tensors(pending.finish())
    _same(SP.probe(run, dict(planes=torch.from_numpy(planes)), dict(planes=torch.from_numpy(decoy)), f'encode, text on the device ({form})'),
          as_tensors(want))
