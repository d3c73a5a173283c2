"""TEST-ONLY CPU contract of `deva.hip.rle.decode`, in the manner of tests/emu_regions.py: the numpy statement of
tests/rle_case.py behind the binding's own parsing and argument checks (D2 included), minus the refusal of host tensors.
`install(monkeypatch)` patches it over the ctypes wrapper.  Zeros and ones only, so the device must agree bit for bit."""
import numpy as np
import torch

import rle_case as LC
from deva.hip import rle as real


def decode(rles, size=None, *, dtype=torch.uint8, out=None, source_size=None, device=None, max_masks=None, max_words=None):
    fn = 'decode'
    real._dtype_code(dtype, fn)
    parsed = real.parse_checked(rles, source_size, fn)
    oh, ow = real._sizes(parsed, size, fn)
    n = int(parsed.per_mask.size)
    real._check_out(out, n, oh, ow, dtype, fn)
    real.chunks(parsed.per_mask, *real._limits(max_masks, max_words, fn), fn)
    ends = np.cumsum(parsed.per_mask)
    each = [parsed.counts[e - m:e] for e, m in zip(ends.tolist(), parsed.per_mask.tolist())]
    res = torch.from_numpy(LC.decoded(each, parsed.height, parsed.width, (oh, ow))).to(dtype)
    if out is not None:
        if not out.is_contiguous():
            raise real.DevaHipError(f'{fn}: `out` must be a contiguous tensor on the HIP device')
        out.copy_(res)
        return out
    return res


def install(monkeypatch):
    monkeypatch.setattr(real, 'decode', decode)
