"""Does every launch of a call go to the caller's stream?  A helper of tests/test_gpu_v_streams.py (not a conftest).

`probe(run, real, decoy)` runs `run` once on the default stream (the expected outputs; the op's own test file already
holds those to their reference) and once on a fresh side stream that is still blocked behind a delay kernel while the
host enqueues, in this order: the delay, device-to-device copies of the real inputs over decoys, `run`, copies of the
decoys back, the read-back.  A launch that left for another stream (the null stream above all) cannot wait for the
delay: it reads the decoys, a second VALID input set from another seed, or runs before its producers, and the outputs
differ.  The decoys are never garbage and index-typed inputs stay in range: a misrouted kernel computes a wrong answer,
never a wild address.  The comparison is bit identity.

The delay is no tolerance: an event recorded right behind it must still be pending when `run` has returned on the host
(or, for a call that synchronises its stream itself, when it reaches that point and calls `mark()`), which shows that
every launch so far was enqueued while the stream was blocked.  A case whose event has fired is reported as
`ProbeInvalid`: a failure, never a skip.

With DEVA_TEST_DRYRUN=1 (no GPU: the emulated ops on the CPU) the stream machinery is a null context and the same
builders, runs and comparisons execute on host tensors."""
import contextlib
import os
import time
from collections import namedtuple

import torch

import gpu_util
from deva.hip import ops

DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
DELAY_MS = 50.0

Record = namedtuple('Record', 'name enqueue_ms blocked delay_ms')
RECORDS = []          # one per side-stream run of this process
_CALIBRATION = {}     # cycles_per_ms, measured_ms


class ProbeInvalid(AssertionError):
    """the delay was over before the host had enqueued the call: the run proves nothing"""


class Mismatch(AssertionError):
    """outputs of the side-stream run differ from the default-stream run"""


# ------------------------------------------------------------------------------------------ the delay
def calibrate():
    """-> cycles of torch.cuda._sleep per millisecond, from two events around the delay kernel alone"""
    if not _CALIBRATION:
        torch.cuda._sleep(1000000)                       # (loads the kernel)
        torch.cuda.synchronize()
        cycles = 20000000
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.5, f'the delay kernel took {ms} ms for {cycles} cycles: nothing to calibrate on'
        _CALIBRATION.update(cycles_per_ms=cycles / ms, measured_ms=ms, cycles=cycles)
    return _CALIBRATION['cycles_per_ms']


def delay(ms=DELAY_MS):
    """enqueue ~ms of spinning on the current stream -> an event recorded right behind it"""
    torch.cuda._sleep(int(calibrate() * ms))
    event = torch.cuda.Event()
    event.record()
    return event


# ------------------------------------------------------------------------------------------ buffers and outputs
def _device_buffer(t):
    """an uninitialised device tensor like t; fp32 ones carry the guard bands of ops._alloc (the vector gathers of the
    convolutions may touch and mask a few elements beyond the ends of their inputs)"""
    dev = gpu_util.dev()
    if t.dtype == torch.float32 and not DRYRUN:
        flat = torch.zeros(t.numel() + 2 * ops.GUARD, dtype=torch.float32, device=dev)
        return flat[ops.GUARD:ops.GUARD + t.numel()].view(*t.shape)
    return torch.empty(t.shape, dtype=t.dtype, device=dev)


def flatten(out, into=None, path='out'):
    """the tensors of a (nested) result as [(path, tensor)]; None and host scalars are kept as they are"""
    into = [] if into is None else into
    if isinstance(out, torch.Tensor) or out is None or isinstance(out, (int, float, str, bytes, bool)):
        into.append((path, out))
    elif isinstance(out, dict):
        for k in out:
            flatten(out[k], into, f'{path}[{k!r}]')
    elif hasattr(out, '_fields'):
        for k in out._fields:
            flatten(getattr(out, k), into, f'{path}.{k}')
    elif isinstance(out, (list, tuple)):
        for i, v in enumerate(out):
            flatten(v, into, f'{path}[{i}]')
    else:
        raise TypeError(f'{path}: a result of {type(out).__name__} cannot be compared')
    return into


def to_host(out):
    """flatten + copy to the host on the CURRENT stream (the read-back is part of the probed sequence)"""
    return [(p, v.cpu() if isinstance(v, torch.Tensor) else v) for p, v in flatten(out)]


def _bytes(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.numel() else t.reshape(0)


def differences(want, got):
    """bit identity of two `to_host` lists -> list of messages (empty: identical)"""
    if [p for p, _ in want] != [p for p, _ in got]:
        return [f'structure differs: {[p for p, _ in want]} vs {[p for p, _ in got]}']
    bad = []
    for (p, a), (_, b) in zip(want, got):
        if isinstance(a, torch.Tensor) != isinstance(b, torch.Tensor):
            bad.append(f'{p}: {type(a).__name__} vs {type(b).__name__}')
        elif not isinstance(a, torch.Tensor):
            if a != b:
                bad.append(f'{p}: {a!r} vs {b!r}')
        elif a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
            bad.append(f'{p}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}')
        elif not torch.equal(_bytes(a), _bytes(b)):
            n = int((_bytes(a) != _bytes(b)).sum())
            bad.append(f'{p}: {n} of {_bytes(a).numel()} bytes differ')
    return bad


def _fill(bufs, src):
    for k, t in bufs.items():
        t.copy_(src[k], non_blocking=True)


def check_inputs(real, decoy):
    assert set(real) == set(decoy), 'real and decoy inputs must have the same names'
    for k in real:
        a, b = real[k], decoy[k]
        assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor), f'{k}: inputs are tensors'
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), f'{k}: the decoy must have the shape of the real input'
    assert any(not torch.equal(real[k], decoy[k]) for k in real), 'the decoys equal the real inputs: nothing could be seen'


def release(stream=None):
    """hand back the per-stream scratch that ops keeps for `stream` (a probe's side stream is transient)"""
    if DRYRUN:
        return
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        ops.release_stream_scratch(gpu_util.dev())


# ------------------------------------------------------------------------------------------ the probe
def reference_run(run, real, decoy):
    """-> (host results of the default-stream run, bufs, real_d, decoy_d); the buffers hold the decoys afterwards"""
    check_inputs(real, decoy)
    real_d = {k: _device_buffer(v) for k, v in real.items()}
    decoy_d = {k: _device_buffer(v) for k, v in decoy.items()}
    bufs = {k: _device_buffer(v) for k, v in real.items()}
    for k in real:
        real_d[k].copy_(real[k])
        decoy_d[k].copy_(decoy[k])
    _fill(bufs, real_d)
    want = to_host(run(bufs, lambda: None))
    _fill(bufs, decoy_d)
    if not DRYRUN:
        torch.cuda.synchronize()        # (before the side stream exists: everything above has run)
    return want, bufs, real_d, decoy_d


def side_run(run, bufs, real_d, decoy_d, name, stream=None):
    """the blocked side-stream run -> (host results, Record); raises ProbeInvalid when the delay did not cover the
    host's enqueue time"""
    if DRYRUN:
        _fill(bufs, real_d)
        got = to_host(run(bufs, lambda: None))
        _fill(bufs, decoy_d)
        return got, Record(name, 0.0, True, 0.0)
    s = torch.cuda.Stream() if stream is None else stream
    s.wait_stream(torch.cuda.current_stream())
    state = {}

    def mark():
        if 'blocked' not in state:
            state['blocked'] = not event.query()
            state['ms'] = (time.perf_counter() - t0) * 1e3

    with torch.cuda.stream(s):
        event = delay()
        t0 = time.perf_counter()
        _fill(bufs, real_d)
        out = run(bufs, mark)
        mark()
        _fill(bufs, decoy_d)
        got = to_host(out)
    s.synchronize()
    record = Record(name, state['ms'], state['blocked'], DELAY_MS)
    RECORDS.append(record)
    if stream is None:
        release(s)
    if not record.blocked:
        raise ProbeInvalid(f'{name}: probe invalid -- the {DELAY_MS:.0f} ms delay was over after {record.enqueue_ms:.1f} ms of '
                           'host enqueue time (a hidden synchronisation inside the call, or a slow host)')
    return got, record


def probe(run, real, decoy, name='case'):
    """run(inputs: dict of device tensors, mark) -> (nested) tensors.  `mark()` is for a call that synchronises its own
    stream: it calls it right before that point (the launches up to there are the probed ones); otherwise the probe
    marks when `run` returns.  Raises Mismatch / ProbeInvalid; -> the host results of the default-stream run"""
    want, bufs, real_d, decoy_d = reference_run(run, real, decoy)
    got, _ = side_run(run, bufs, real_d, decoy_d, name)
    bad = differences(want, got)
    if bad:
        raise Mismatch(f'{name}: the side-stream run differs from the default-stream run: ' + '; '.join(bad))
    return want


def summary():
    """the lines of the log: calibration, enqueue times, invalid cases"""
    lines = []
    if _CALIBRATION:
        lines.append('delay kernel: {cycles} cycles took {measured_ms:.3f} ms -> {cycles_per_ms:.0f} cycles / ms; '
                     .format(**_CALIBRATION) + f'{DELAY_MS:.0f} ms = {int(_CALIBRATION["cycles_per_ms"] * DELAY_MS)} cycles')
    if RECORDS:
        slow = max(RECORDS, key=lambda r: r.enqueue_ms)
        lines.append(f'{len(RECORDS)} side-stream runs; slowest host enqueue {slow.enqueue_ms:.2f} ms ({slow.name}); '
                     f'invalid: {[r.name for r in RECORDS if not r.blocked]}')
        for r in RECORDS:
            lines.append(f'  {r.name}: enqueue {r.enqueue_ms:.2f} ms, blocked {r.blocked}')
    return lines
