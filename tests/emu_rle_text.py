"""TEST-ONLY CPU contract of the three library calls of `deva.hip.rle_text` (`_launch_encode_count`, `_launch_encode_write`,
`_launch_parse`), in the manner of tests/emu_runs.py: the per-value statement of tests/rle_text_case.py behind the binding's own
argument checks, chunking, capacity handling and host arithmetic, minus the refusal of host tensors.
`install(monkeypatch)` patches it over the ctypes wrappers; it also stands in for `rle.decode`, whose launch has no
wrapper of its own, so that `parse='device'` can be followed there.  Integers and bytes only: the device must agree exactly."""
import numpy as np
import torch

import rle_case as LC
import rle_text_case as TC
from deva.hip import rle as real_rle
from deva.hip import rle_text as real


def _launch_encode_count(n, base, bounds, bounds_len, h, w, text_len, text_base, text_total, first):
    start = 0 if first is None else int(first.reshape(-1)[0])
    want = TC.encode_statement(n.numpy(), base.numpy(), bounds.numpy()[:bounds_len], h * w, start)
    text_len.copy_(torch.from_numpy(want['text_len']))
    text_base.copy_(torch.from_numpy(want['text_base']))
    text_total.fill_(want['text_total'])


def _launch_encode_write(n, base, bounds, bounds_len, h, w, text_base, chars, capacity):
    want = TC.encode_statement(n.numpy(), base.numpy(), bounds.numpy()[:bounds_len], h * w)
    for at, text in zip(text_base.tolist(), want['texts']):
        room = max(0, min(int(capacity) - at, len(text)))          # C4: nothing at or beyond the capacity
        if room:
            chars[at:at + room] = torch.frombuffer(bytearray(text[:room]), dtype=torch.uint8)


def _launch_parse(chars, chars_len, text_first, n, h, w, scratch, runs, words_cap, info):
    assert scratch.numel() * 4 >= real.parse_scratch(n) and words_cap >= 2 * n + 1 + chars_len and runs.numel() >= words_cap
    body, first = bytes(chars.numpy()[:chars_len].tobytes()), text_first.tolist()
    words, flags = TC.run_words([body[first[k]:first[k + 1]] for k in range(n)], h * w)
    info[0], info[1] = flags, words.size
    if not flags:                                                   # (C7: with a flag the contents are unspecified)
        runs[:words.size] = torch.from_numpy(words)


def decode(rles, size=None, *, dtype=torch.uint8, out=None, source_size=None, device=None, max_masks=None, max_words=None, parse='host'):
    """tests/emu_rle.py's contract with the `parse` parameter: the planes come from the run arrays that `parse_checked` built"""
    fn = 'decode'
    real_rle._dtype_code(dtype, fn)
    parsed = real_rle.parse_checked(rles, source_size, fn, parse=parse, device='cpu', max_masks=max_masks, max_words=max_words)
    oh, ow = real_rle._sizes(parsed, size, fn)
    n = int(parsed.per_mask.size)
    real_rle._check_out(out, n, oh, ow, dtype, fn)
    if parsed.device is None:
        parts = real_rle.chunks(parsed.per_mask, *real_rle._limits(max_masks, max_words, fn), fn)
        arrays = [real_rle.run_array(parsed, lo, hi) for lo, hi in parts]
    else:
        parts, arrays = [(c.lo, c.hi) for c in parsed.device], [c.host for c in parsed.device]
    each = []
    for (lo, hi), words in zip(parts, arrays):
        real_rle.check(real_rle.lib().deva_rle_check(words.ctypes.data, words.size, hi - lo, parsed.height, parsed.width), 'deva_rle_check')
        first, starts = words[:hi - lo + 1], words[hi - lo + 1:]
        each += [np.diff(starts[first[k]:first[k + 1]]) for k in range(hi - lo)]
    res = torch.from_numpy(LC.decoded(each, parsed.height, parsed.width, (oh, ow))).to(dtype)
    if out is not None:
        out.copy_(res)
        return out
    return res


def install(monkeypatch):
    monkeypatch.setattr(real, '_launch_encode_count', _launch_encode_count)
    monkeypatch.setattr(real, '_launch_encode_write', _launch_encode_write)
    monkeypatch.setattr(real, '_launch_parse', _launch_parse)
    monkeypatch.setattr(real_rle, 'decode', decode)
