"""TEST-ONLY CPU contract of the three library calls of `deva.hip.lowres` (`_launch_upsample`, `_launch_select`,
`_launch_proposal_batch`), in the manner of tests/emu_rle_text.py: the numpy statement of tests/lowres_case.py behind the
binding's own argument checks, minus the refusal of host tensors.  `install(monkeypatch)` patches it over the ctypes
wrappers; the filter's state is tests/emu_proposals.py's, so install that one too.  The statement is fp32 operation by
operation: the device must agree bit for bit."""
import numpy as np
import torch

import emu_proposals as EP
import lowres_case as LC
from deva.hip import lowres as real


def _sizes(geo):
    return geo.model_size, (geo.in_h, geo.in_w), (geo.out_h, geo.out_w)


def _launch_upsample(low, geo, out):
    out.copy_(torch.from_numpy(LC.upsample(low.cpu().numpy(), *_sizes(geo))).view(out.shape))


def _launch_select(low, scores, geo, threshold, out, chosen):
    planes, picks = LC.select(low.cpu().numpy(), None if scores is None else scores.cpu().numpy(), *_sizes(geo), threshold=threshold)
    out.copy_(torch.from_numpy(planes).view(out.shape))
    chosen.copy_(torch.from_numpy(picks))


def _launch_proposal_batch(state, low, iou_preds, geo, thresholds):
    """L5: rules 1-4 on the planes of L3.  A plane that is not live is never evaluated: it is handed on as zeros, which
    rule 1 of tests/emu_proposals.py never reads."""
    iou = iou_preds.cpu().numpy()
    t_iou = np.float32(thresholds['pred_iou_thresh'])
    live = np.ones(len(iou), dtype=bool) if not thresholds['pred_iou_thresh'] > 0.0 else iou > t_iou
    planes = np.zeros((len(iou), geo.out_h, geo.out_w), dtype=np.float32)
    if live.any():
        planes[live] = LC.upsample(low.cpu().numpy()[live], *_sizes(geo))
    EP.proposal_batch(state, torch.from_numpy(planes), iou_preds, **thresholds)


def install(monkeypatch):
    for name in ('_launch_upsample', '_launch_select', '_launch_proposal_batch'):
        monkeypatch.setattr(real, name, globals()[name])
