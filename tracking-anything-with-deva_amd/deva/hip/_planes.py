"""Argument handling that the scorers (`deva.hip.metrics`, `deva.hip.vos_metrics`, `deva.hip.pair_metrics`) share.  `fn` is the wrapper's
name as it stands in front of every message ('panoptic_counts', 'boundary_counts', 'pair_counts')."""
import numpy as np
import torch

from . import DevaHipError


def on_device(t: torch.Tensor, name: str, fn: str, align: int = 16) -> torch.Tensor:
    if not t.is_cuda:
        raise DevaHipError(f'{fn}: {name} must live on the HIP device (got {t.device}); there is no CPU path')
    t = t.contiguous()
    return t.clone() if t.data_ptr() % align else t   # (a view into the middle of a buffer)


def check_pred_lut(pred_lut: torch.Tensor, fn: str) -> None:
    if pred_lut.dim() != 1 or pred_lut.dtype != torch.uint16 or not 1 <= pred_lut.numel() <= 32767:
        raise DevaHipError(f'{fn}: pred_lut must be uint16 [channels], 1 to 32767 channels')


def check_out(out, shape, fn: str) -> None:
    if out is not None and (out.dtype != torch.uint32 or tuple(out.shape) != shape):
        raise DevaHipError(f'{fn}: `out` must be uint32 [{shape[0]},{shape[1]}]')


def check_out_on_device(out, fn: str) -> None:
    if out is not None and not (out.is_cuda and out.is_contiguous()):
        raise DevaHipError(f'{fn}: `out` must be a contiguous tensor on the HIP device')


def host_ids(ids, fn: str, what: str, *, allow_empty: bool, max_ids=None) -> np.ndarray:
    """a table of ids as the caller gives it -> int32 [n], checked: distinct, ascending, in 1 .. 2^31 - 1"""
    if isinstance(ids, torch.Tensor):
        ids = ids.cpu().numpy()
    a = np.asarray(ids if isinstance(ids, np.ndarray) or np.isscalar(ids) else list(ids), dtype=np.int64).reshape(-1)
    if max_ids is not None and a.size > max_ids:
        raise DevaHipError(f'{fn}: at most {max_ids} {what} (got {a.size})')
    if a.size == 0 and not allow_empty:
        raise DevaHipError(f'{fn}: at least one object id')
    if a.size and (a[0] < 1 or a[-1] > 2**31 - 1 or bool((np.diff(a) <= 0).any())):
        raise DevaHipError(f'{fn}: {what} must be distinct, ascending and in 1 .. 2^31 - 1')
    return a.astype(np.int32)


def device_ids(ids, device, fn: str, what: str, *, validate: bool, allow_empty: bool, max_ids=None,
               trusted_must_be_contiguous: bool):
    """-> (device int32 table, or None for an empty one, n).  The library cannot see from the host whether a table is
    ascending, so it is checked here (`host_ids`): for a device tensor that is a copy to the host, which `validate=False`
    leaves out.  What is taken on trust then differs between the two scorers and is kept as it was found: the panoptic
    one takes an empty table and sends a non-contiguous one to the checked path (allow_empty, trusted_must_be_contiguous);
    the DAVIS one wants an id and does not look at the strides (its caller makes the table contiguous afterwards)."""
    i32 = isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and ids.dim() == 1
    if not validate and i32 and (ids.is_contiguous() or not trusted_must_be_contiguous) and (ids.numel() or allow_empty):
        if max_ids is not None and ids.numel() > max_ids:
            raise DevaHipError(f'{fn}: at most {max_ids} {what} (got {ids.numel()})')
        return (ids if ids.numel() else None), ids.numel()
    host = host_ids(ids, fn, what, allow_empty=allow_empty, max_ids=max_ids)
    if host.size == 0:
        return None, 0
    if i32 and ids.is_cuda and ids.is_contiguous():
        return ids, host.size
    return torch.from_numpy(host).to(device), host.size
