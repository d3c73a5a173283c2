"""Multi-scale / horizontal-flip test-time ensemble as one online object (an extension of the interface; the
arithmetic is the reference protocol's).

The reference produces its ensemble results in three places: `evaluation/eval_vos.py --flip` (lines 162-164, 176-177)
mirrors image and mask before `step` and mirrors the resized probabilities back; `--save_scores` (lines 188-211)
writes `(prob * 255).astype(np.uint8)` per frame and run plus, on the last frame, the tmp-id -> object-id table; and
`scripts/merge_multi_scale.py:44-66` sums the runs' uint8 volumes as float32, takes `np.argmax` over channels and
maps the ids through that table.  `EnsembleInferenceCore` runs the variants side by side on the device instead: one
`DEVAInferenceCore` per (size, flip), one `step_clips` call per frame (variants of equal padded size -- a flip pair in
particular -- share the batched network passes), and one fused output tail (`ops.ensemble_index_mask`) that resizes,
mirrors, quantises, sums, takes the argmax and applies the table without writing a score volume.  H*W labels leave the
device per frame; the uint8 volumes are produced (`ops.scores_u8`) only when asked for.

Exactness: with `quantize=True` the returned mask equals `lut[argmax_c(sum_k scores_k)]` of the uint8 volumes that
`return_scores=True` returns, bit for bit (integer sums, first maximum), which is what the offline script computes from
the saved files.  `quantize=False` sums the fp32 resized probabilities in variant order instead.
"""
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from deva.hip import ENSEMBLE_MAX_VARIANTS, ops
from deva.inference.inference_core import DEVAInferenceCore
from deva.inference.multi_clip import step_clips
from deva.model.network import DEVA
from deva.utils.tensor_utils import frame_to_network_input, network_input_size, unpad


class EnsembleInferenceCore:
    def __init__(self, network: DEVA, config: Dict, sizes: Sequence[int] = (-1,), flips: Sequence[bool] = (False, True),
                 quantize: bool = True):
        """sizes: `--size` of every scale (shorter side of the network input; <= 0: the frame's own size); flips:
        which of {False, True} to run at every scale.  Variant order: sizes outermost."""
        self.variants = [(int(s), bool(f)) for s in sizes for f in flips]
        if not 1 <= len(self.variants) <= ENSEMBLE_MAX_VARIANTS:
            raise ValueError(f'EnsembleInferenceCore: 1 to {ENSEMBLE_MAX_VARIANTS} (size, flip) variants, '
                             f'got {len(self.variants)}')
        self.network = network
        self.config = config
        self.quantize = bool(quantize)
        self.cores = [DEVAInferenceCore(network, config) for _ in self.variants]
        self._lut = None
        self._lut_ids = None

    def tmp_to_obj_mapping(self) -> Dict[int, int]:
        """{object id: tmp id}: what the reference saves as backward.hkl (eval_vos.py:203-206)"""
        return self.cores[0].object_manager.get_tmp_to_obj_mapping()

    def _variant_mask(self, mask: torch.Tensor, size, flip: bool) -> torch.Tensor:
        """the readers' nearest-neighbour resize of an index mask to a variant's input size, mirrored for a flipped one
        (annotated frames only)"""
        if tuple(mask.shape) != tuple(size):
            mask = F.interpolate(mask[None, None].double(), size, mode='nearest')[0, 0].to(torch.int64)
        return ops.flip_w(mask.contiguous()) if flip else mask

    def _table(self, device) -> torch.Tensor:
        """variant 0's tmp-id -> object-id table on the device, rebuilt only when the objects change; every variant
        receives the same objects in the same order, so the tables must agree (the merge script uses one backward.hkl)"""
        ids = [c.object_manager.all_obj_ids for c in self.cores]
        if any(other != ids[0] for other in ids[1:]):
            raise RuntimeError(f'EnsembleInferenceCore: the variants disagree on the object table: {ids}')
        if self._lut is None or self._lut_ids != ids[0] or self._lut.device != device:
            self._lut = self.cores[0].object_manager._tmp_to_obj_table(device)
            self._lut_ids = list(ids[0])
        return self._lut

    def step(self, frame_u8_hwc, mask: Optional[torch.Tensor] = None, objects: Optional[List[int]] = None, *,
             end: bool = False, return_scores: bool = False):
        """One frame.  frame_u8_hwc: the decoded uint8 H*W*3 frame (numpy array or tensor); mask: H*W index mask of an
        annotated frame with the ids `objects`, else None.  Returns the int64 H*W object-id mask on the device, at the
        frame's own resolution; with return_scores=True also the list of the variants' uint8 (num_objects+1)*H*W score
        volumes (the `--save_scores` files of the runs)."""
        frame = frame_u8_hwc if torch.is_tensor(frame_u8_hwc) else torch.from_numpy(frame_u8_hwc)
        if not frame.is_cuda:
            frame = frame.cuda()
        frame = frame.contiguous()
        h, w = frame.shape[:2]
        if mask is not None:
            if objects is None:
                raise ValueError('EnsembleInferenceCore.step: an index mask needs its object ids')
            mask = mask.to(frame.device)

        mirrored = None
        images, pads, masks = [], [], []
        for size, flip in self.variants:
            if flip and mirrored is None:
                mirrored = ops.flip_w(frame)
            image, pad = frame_to_network_input(mirrored if flip else frame, size, pad_to=16)
            images.append(image)
            pads.append(pad)
            masks.append(None if mask is None else self._variant_mask(mask, network_input_size(h, w, size), flip))
        each_objects = [None if mask is None else list(objects) for _ in self.variants]
        probs = step_clips(self.cores, images, masks, each_objects, end=[end] * len(self.variants))
        probs = [unpad(p, pad) for p, pad in zip(probs, pads)]

        flips = [flip for _, flip in self.variants]
        out = ops.ensemble_index_mask(probs, (h, w), flips, self._table(frame.device), self.quantize)
        if not return_scores:
            return out
        return out, [ops.scores_u8(p, (h, w), flip) for p, flip in zip(probs, flips)]
