"""TEST-ONLY CPU contract of the region kernels (`deva.hip.regions.label_components`, `remove_small_regions`), in the manner
of tests/emu_pairs.py: the numpy statement of tests/region_case.py behind the binding's own argument checks, minus the
refusal of host tensors.  `install(monkeypatch)` patches it over the ctypes wrappers.  Integers only, so the device must
agree bit for bit."""
import numpy as np
import torch

import region_case as RC
from deva.hip import regions as real


def label_components(planes, of_zeros=False, out=None, scratch=None):
    real._arguments(planes, 'label_components')
    real._check_labels(out, planes)
    res = torch.from_numpy(np.ascontiguousarray(RC.label_planes(planes.cpu().numpy(), of_zeros))).view(planes.shape)
    if out is not None:
        out.copy_(res)
        return out
    return res


def remove_small_regions(planes, min_area, *, scratch=None, records=None):
    fn = 'remove_small_regions'
    n, h, w, squeeze = real._arguments(planes, fn)
    min_area = real._min_area(min_area)
    real._check_records(records, n, squeeze)
    need = real.region_scratch_bytes(h, w, 1)          # (host-only library code)
    if scratch is not None and (scratch.dtype != torch.uint8 or scratch.dim() != 1 or scratch.numel() < need):
        raise real.DevaHipError(f'{fn}: `scratch` must be uint8 [{need}] or longer')
    if not planes.is_contiguous():
        raise real.DevaHipError(f'{fn}: planes must be contiguous')
    cleaned, recs = RC.clean(planes.cpu().numpy(), min_area)
    planes.copy_(torch.from_numpy(cleaned).view(planes.shape))
    recs = torch.from_numpy(np.ascontiguousarray(recs))
    if records is not None:
        records.copy_(recs)
        return planes, records
    return planes, recs


def region_buffers(height, width, capacity, device):
    return None


def clean_and_suppress(masks, min_area, nms_thresh, buffers):
    import emu_proposals as EP
    _, records = remove_small_regions(masks, min_area)
    rec = records.numpy()
    keep = torch.tensor(EP.nms(rec[:, 4:8], (1 - rec[:, 0]).astype(np.float32), nms_thresh), dtype=torch.int64)
    return records.clone(), keep, keep.clone()


def install(monkeypatch):
    monkeypatch.setattr(real, 'region_buffers', region_buffers)
    monkeypatch.setattr(real, 'clean_and_suppress', clean_and_suppress)
    monkeypatch.setattr(real, 'label_components', label_components)
    monkeypatch.setattr(real, 'remove_small_regions', remove_small_regions)
