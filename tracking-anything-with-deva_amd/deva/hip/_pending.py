"""What the bindings with results in flight (`mask_runs`, `rle_text`, `rle_overlap`, `png`) share: the device check in
front of a launch, a preallocated output by name, the copy to pinned host memory and the event behind it.  `fn` is the
wrapper's name as it stands in front of every message."""
from typing import Optional

import torch

from . import DevaHipError


def require_on_device(t: torch.Tensor, name: str, fn: str) -> None:
    if not t.is_cuda:
        raise DevaHipError(f'{fn}: {name} must live on the HIP device (got {t.device}); there is no CPU path')


def out_tensor(out: Optional[dict], name: str, shape, dtype, device, fn: str) -> torch.Tensor:
    """out[name] when the caller gave one (checked), else a new tensor; it may be uninitialised"""
    t = None if out is None else out.get(name)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise DevaHipError(f'{fn}: out[{name!r}] must be a contiguous {dtype} {list(shape)}')
    return t


def to_pinned(t: torch.Tensor) -> torch.Tensor:
    """a copy in pinned host memory, in flight on the current stream (`record_event` after it).  A CPU tensor, which
    only the tests' CPU contract passes, is cloned: the result never aliases the argument."""
    if not t.is_cuda:
        return t.clone()
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    return host


def record_event(device) -> Optional['torch.cuda.Event']:
    """an event on the current stream of `device`; None for a CPU device, where nothing is in flight"""
    if torch.device(device).type != 'cuda':
        return None
    event = torch.cuda.Event()
    event.record(torch.cuda.current_stream(device))
    return event
