"""`DEVAInferenceCore`: the per-frame state machine of the reference
(deva/inference/inference_core.py:17-290) on the HIP network / memory modules of this package.

Public surface kept verbatim: constructor, attributes (`network, mem_every, enable_long_term,
chunk_size, max_missed_detection_count, max_num_objects, config, curr_ti, last_mem_ti, memory,
object_manager, image_feature_store, last_mask, frame_buffer, pad`) and the methods `step`,
`incorporate_detection`, `add_to_temporary_buffer`, `vote_in_temporary_buffer`, `clear_buffer`,
`enabled_long_id`, `_segment`, `_add_memory`.
"""
import struct
import warnings
from typing import Dict, Iterable, List, Literal, Optional, Tuple

import torch

from deva.hip import ops
from deva.inference.image_feature_store import ImageFeatureStore
from deva.inference.memory_manager import MemoryManager
from deva.inference.object_info import ObjectInfo
from deva.inference.object_manager import ObjectManager, pack_objects, unpack_objects
from deva.model.network import DEVA
from deva.utils.tensor_utils import pad_divide_by, unpad


class DEVAInferenceCore:
    def __init__(self, network: DEVA, config: Dict, *, image_feature_store: ImageFeatureStore = None):
        self.network = network
        self.mem_every = config['mem_every']
        self.enable_long_term = config['enable_long_term']
        self.chunk_size = config['chunk_size']
        self.max_missed_detection_count = config.get('max_missed_detection_count')
        self.max_num_objects = config.get('max_num_objects')
        self.config = config

        self.curr_ti = -1
        self.last_mem_ti = 0
        self.memory = MemoryManager(config=config)
        self.object_manager = ObjectManager()
        self.image_feature_store = (ImageFeatureStore(self.network)
                                    if image_feature_store is None else image_feature_store)
        self.last_mask = None
        self.pad = None
        self._map16 = (None, None, None)  # (h/16, w/16, device) of the current frame: the shape of what a broadcast delivers
        self.frame_buffer = []  # online / semi-online processing

    def enabled_long_id(self) -> None:
        # short ids 1..255 (palette PNG) by default; long ids 256..255**3 for panoptic RGB masks
        self.object_manager.use_long_id = True

    @property
    def use_long_id(self):
        return self.object_manager.use_long_id

    # ------------------------------------------------------------------ one clip on several GPUs: frame-owner mode
    # `MemoryManager.shard_queries(group, owner=r)` / `shard_bank(group, owner=r)`: every rank of the group
    # makes the same `step` / `incorporate_detection` / `vote_in_temporary_buffer` calls with the same host-side arguments;
    # only the owner runs the key encoder, the mask decoder and the value encoder, and only the owner reads pixels
    # (`mask`, `new_mask`, `segments_info`, `forward_mask`: the other ranks may pass anything there, but None where the
    # owner passes None).  Per frame the owner broadcasts the query key / selection, every rank matches and reads out its
    # share against its replica of the bank, the read-out is gathered to the owner and the integer usage counters
    # all-reduced; on memory frames the owner broadcasts the new key / shrinkage / selection / value rows and every rank
    # appends them (consolidation and eviction then run redundantly on identical inputs with deterministic kernels, so
    # the replicas cannot diverge); after a detection the owner broadcasts its object table.  The frame state machine
    # depends on host-side state only, which is identical on all ranks.  The owner returns what the unsharded call
    # returns, the other ranks None.  Below this shows as `own` (`MemoryManager.is_frame_owner`: True on an unsharded
    # manager) and the manager's broadcasts, which hand their arguments back outside this mode.

    # ------------------------------------------------------------------ the pieces of a frame (shared with multi_clip.py)
    def _advance(self, image: torch.Tensor, image_ti_override=None):
        """advance the clock and pad the frame to a multiple of 16 -> (frame index used for the feature cache,
        1*3*H'*W' image)"""
        self.curr_ti += 1
        frame_ti = image_ti_override if image_ti_override is not None else self.curr_ti
        padded, self.pad = pad_divide_by(image, 16)
        self._map16 = (padded.shape[-2] // 16, padded.shape[-1] // 16, image.device)
        return frame_ti, padded.unsqueeze(0)

    def _begin_frame(self, image: torch.Tensor, image_ti_override):
        """`_advance` and fetch (or compute) the frame's features on the owner: -> (frame index, 1*3*H'*W' image,
        ms_features, key, shrinkage, selection), the last five None on the other ranks"""
        frame_ti, batch = self._advance(image, image_ti_override)
        if not self.memory.is_frame_owner:
            return frame_ti, None, None, None, None, None
        store = self.image_feature_store
        return (frame_ti, batch, store.get_ms_features(frame_ti, batch), *store.get_key(frame_ti, batch))

    def _plan(self, mask, objects: Optional[List[int]], hard_mask: bool, end: bool):
        """what the frame after `_advance` does -> (the annotation's object ids, commit a memory frame?, propagate?)"""
        annotated = mask is not None
        if annotated and objects is None:
            assert not hard_mask
            objects = list(range(1, mask.shape[0] + 1))
        due = self.curr_ti - self.last_mem_ti >= self.mem_every
        # propagate unless the annotation covers every object known so far
        om = self.object_manager
        return objects, (annotated or due) and not end, (not annotated) or (om.num_obj > 0 and not om.has_all(objects))

    def _segment(self, key: torch.Tensor, selection: torch.Tensor, ms_features: Iterable[torch.Tensor],
                 update_sensory: bool = True) -> torch.Tensor:
        """memory read + decode for every live object (inference_core.py:89-113);
        returns (num_objects+1)*H*W probabilities"""
        mem, om = self.memory, self.object_manager
        own = mem.is_frame_owner
        if not mem.engaged:
            warnings.warn('Trying to segment without any memory!', RuntimeWarning)
            return (torch.zeros((1, key.shape[-2] * 16, key.shape[-1] * 16), device=key.device, dtype=key.dtype)
                    if own else None)
        readout = mem.match_memory(*mem.broadcast_query(key, selection, *self._map16))
        if not own:
            return None
        ids = om.all_obj_ids
        readout = om.realize_dict(readout).unsqueeze(0)
        sensory, _, prob = self.network.segment(ms_features, readout, mem.get_sensory(ids),
                                                self.last_mask, chunk_size=self.chunk_size,
                                                update_sensory=update_sensory)
        if update_sensory:
            mem.update_sensory(sensory, ids)
        return prob[0]

    def _blend_annotation(self, prediction: torch.Tensor, mask: torch.Tensor, objects: List[int],
                          new_tmp_ids: List[int], hard_mask: bool) -> torch.Tensor:
        """an annotation that covers only some objects on top of the propagated prediction
        ((no+1)*H*W): annotated pixels win, channels of newly introduced objects are appended
        (inference_core.py:251-272, including its channel indexing).  For soft masks the reference
        compares the (values, indices) pair of `mask.max(0)` with 0.5 and indexes the annotation by tmp
        id (a TypeError on every call); here the values are compared and channel `pos` of the annotation
        is taken, which is what that code means."""
        fg = prediction[1:]
        annotated = (mask > 0) if hard_mask else (mask.max(0).values > 0.5)
        fg[:, annotated] = 0
        appended = []
        for pos, tmp_id in enumerate(new_tmp_ids):
            channel = (mask == objects[pos]).type_as(fg) if hard_mask else mask[pos].type_as(fg)
            if tmp_id < fg.shape[0]:
                fg[tmp_id + 1] = channel
            else:
                appended.append(channel.unsqueeze(0))
        return torch.cat([fg, *appended], dim=0)

    def _annotate(self, prob: Optional[torch.Tensor], mask, objects: List[int], hard_mask: bool, propagate: bool):
        """register the annotation's objects (mask None: no annotation) and lay it over the propagated probabilities
        -> the frame's (num_objects+1)*H*W probabilities, whose object channels become `last_mask`"""
        own = self.memory.is_frame_owner
        if mask is not None:
            new_tmp_ids, _ = self.object_manager.add_new_objects(objects)
            if own:
                mask, _ = pad_divide_by(mask, 16)
                if propagate:
                    mask = self._blend_annotation(prob, mask, objects, new_tmp_ids, hard_mask)
                elif hard_mask:
                    mask = torch.stack([mask == o for o in objects], dim=0)  # index mask -> one-hot
                prob = ops.softmax_channels(self.network.aggregate(mask, dim=0))
        if own:
            self.last_mask = prob[1:].unsqueeze(0)
        return prob

    def _memory_frame_ids(self, prob: Optional[torch.Tensor], key) -> Optional[List[int]]:
        """the objects of a memory frame made from `prob` (1*num_objects*H*W; None on a rank that does not own the frame,
        so frame-owner mode decides by the object table, identical on all ranks), their sensory state initialised;
        None, with the reference's warning, when there are none"""
        mem = self.memory
        ids = self.object_manager.all_obj_ids
        if (not ids) if mem.frame_owner_mode else prob.shape[1] == 0:
            warnings.warn('Empty object mask!', RuntimeWarning)
            return None
        if mem.is_frame_owner:
            mem.initialize_sensory_if_needed(key, ids)
        return ids

    def _commit_value(self, key, shrinkage, selection, value, sensory, ids: List[int]) -> None:
        """append the memory frame whose value (1*num_objects*CV*h*w) the caller encoded, on every rank, and keep the
        deep-updated sensory state (None: there is none)"""
        mem = self.memory
        key, shrinkage, value, selection = mem.broadcast_memory_frame(key, shrinkage, value, selection, ids, *self._map16)
        mem.add_memory(key, shrinkage, value, ids, selection=selection)
        self.last_mem_ti = self.curr_ti
        if sensory is not None:
            mem.update_sensory(sensory, ids)

    def _add_memory(self, image: torch.Tensor, ms_features: Iterable[torch.Tensor], prob: torch.Tensor,
                    key: torch.Tensor, shrinkage: torch.Tensor, selection: torch.Tensor, *,
                    is_deep_update: bool = True) -> None:
        """encode (image, masks) into a memory value and append it (inference_core.py:55-87).
        image 1*3*H*W; prob 1*num_objects*H*W in [0,1]"""
        ids = self._memory_frame_ids(prob, key)
        if ids is None:
            return
        value = sensory = None
        if self.memory.is_frame_owner:
            value, sensory = self.network.encode_mask(image, ms_features, self.memory.get_sensory(ids), prob,
                                                      is_deep_update=is_deep_update,
                                                      chunk_size=self.chunk_size)
        self._commit_value(key, shrinkage, selection, value, sensory if is_deep_update else None, ids)

    # ------------------------------------------------------------------ semi-online buffer
    def add_to_temporary_buffer(self, frame_info) -> None:
        self.frame_buffer.append(frame_info)

    def vote_in_temporary_buffer(
            self, keyframe_selection: Literal['last', 'middle', 'score', 'first'] = 'first'
    ) -> Tuple[int, torch.Tensor, List[ObjectInfo]]:
        """consensus of the buffered window -> (keyframe time index, H*W index mask, merged segments).  Frame-owner
        mode: the owner votes (its feature store holds the window's features; the spatial alignments read one-frame
        memories, not the sharded bank) and broadcasts the keyframe index and the segment list; the other ranks return
        (keyframe index, None, segments)."""
        # consensus voting (deva/inference/consensus_automatic.py:82) is a caller of this path, not
        # part of it; it is resolved from whichever `deva` tree provides it.
        from deva.inference.consensus_automatic import find_consensus_auto_association
        mem = self.memory
        result = payload = None
        if mem.is_frame_owner:
            result = find_consensus_auto_association(self.frame_buffer, network=self.network,
                                                     store=self.image_feature_store, config=self.config,
                                                     keyframe_selection=keyframe_selection)
            if not mem.frame_owner_mode:
                return result
            payload = struct.pack('<q', int(result[0])) + pack_objects(result[2])
        data = mem.broadcast_bytes(payload, self.frame_buffer[0].image.device)
        if result is not None:
            return result
        return struct.unpack_from('<q', data, 0)[0], None, unpack_objects(data, 8)[0]

    def clear_buffer(self) -> None:
        for f in self.frame_buffer:
            self.image_feature_store.delete(f.ti)
        self.frame_buffer = []

    # ------------------------------------------------------------------ detections
    def _broadcast_decisions(self, kept: Optional[List[int]]) -> Optional[List[int]]:
        """frame-owner mode, detection frame: the owner's object table after merging and purging, plus the kept list
        of the purge (None: nothing was purged), travel as bytes -- int32 length of the kept list (-1 for None), the
        kept ids (int64), then `ObjectManager.encode_state`; the other ranks adopt the table.  -> the kept list"""
        mem, om = self.memory, self.object_manager
        if not mem.frame_owner_mode:
            return kept
        payload = None
        if mem.is_frame_owner:
            ids = [] if kept is None else [int(i) for i in kept]
            payload = struct.pack(f'<i{len(ids)}q', -1 if kept is None else len(ids), *ids) + om.encode_state()
        data = mem.broadcast_bytes(payload, self._map16[2])
        if mem.is_frame_owner:
            return kept
        n = struct.unpack_from('<i', data, 0)[0]
        kept = None if n < 0 else list(struct.unpack_from(f'<{n}q', data, 4))
        om.load_state(data, 4 + 8 * max(n, 0))
        return kept

    def incorporate_detection(self, image: torch.Tensor, new_mask: torch.Tensor,
                              segments_info: List[ObjectInfo], *, image_ti_override: bool = None,
                              forward_mask: torch.Tensor = None, incremental: bool = False) -> torch.Tensor:
        """merge an image-level detection into the propagated state (inference_core.py:137-198):
        propagate (unless the caller did), match detected segments with tracked objects by IoU, retire
        objects that went unseen for too long, and commit the merged masks as a memory frame.
        Frame-owner mode: without a forward mask every rank takes part in the read of an engaged memory; the owner
        alone merges (`match_and_merge`: ids may be drawn from np.random), applies `max_num_objects` / `incremental`
        and purges, then broadcasts the object table and the kept list; every rank purges its memory (value-sharded
        storage: its share of the rows) and appends the merged masks as a memory frame."""
        from deva.inference.segment_merging import match_and_merge
        mem, om = self.memory, self.object_manager
        own = mem.is_frame_owner
        frame_ti, batch, ms_features, key, shrinkage, selection = self._begin_frame(image, image_ti_override)
        if own:
            new_mask, _ = pad_divide_by(new_mask, 16)
        if forward_mask is None:
            if mem.engaged:  # identical on every rank: memory frames and purges are applied everywhere
                prob = self._segment(key, selection, ms_features)
                if own:  # argmax over the propagated probabilities in one pass (the output-tail kernel without resize / LUT)
                    forward_mask = ops.index_mask(prob.contiguous())
            elif own:
                forward_mask = torch.zeros_like(new_mask)

        kept = None
        if own:
            merged = match_and_merge(forward_mask, new_mask, om, segments_info,
                                     max_num_objects=self.max_num_objects, incremental_mode=incremental)
            anything_purged, tmp_kept, obj_kept = om.purge_inactive_objects(self.max_missed_detection_count)
            if anything_purged:
                kept = obj_kept
                merged = merged[[t - 1 for t in tmp_kept]]  # tmp ids are 1-based channel numbers
            self.last_mask = merged.unsqueeze(0).type_as(key)
        kept = self._broadcast_decisions(kept)
        if kept is not None:
            mem.purge_except(kept)

        self._add_memory(batch, ms_features, self.last_mask, key, shrinkage, selection)
        if not own:
            return None
        self.image_feature_store.delete(frame_ti)
        return unpad(self.network.aggregate(self.last_mask[0], dim=0), self.pad)

    # ------------------------------------------------------------------ propagation
    def step(self, image: torch.Tensor, mask: torch.Tensor = None, objects: Optional[List[int]] = None, *,
             hard_mask: bool = True, end: bool = False, image_ti_override: bool = None,
             delete_buffer: bool = True) -> torch.Tensor:
        """One frame (inference_core.py:200-290).

        image: 3*H*W, ImageNet-normalised.  mask: H*W index mask, or len(objects)*H*W soft masks with
        hard_mask=False, or None to propagate only.  objects: ids in mask order (None with soft masks
        means 1..mask.shape[0]).  end: last frame of the sequence -- nothing is written to the memories.
        Returns (num_objects+1)*H*W probabilities at the input size, channel 0 = background."""
        own = self.memory.is_frame_owner
        frame_ti, batch, ms_features, key, shrinkage, selection = self._begin_frame(image, image_ti_override)
        objects, commit, propagate = self._plan(mask, objects, hard_mask, end)
        prob = self._segment(key, selection, ms_features, update_sensory=not end) if propagate else None
        prob = self._annotate(prob, mask, objects, hard_mask, propagate)
        if commit:
            self._add_memory(batch, ms_features, self.last_mask, key, shrinkage, selection)
        if own and delete_buffer:
            self.image_feature_store.delete(frame_ti)
        return unpad(prob, self.pad) if own else None
