"""Several independent clips stepped through one batched network pass (an extension; the reference's drivers are
per-video loops).

`step_clips(cores, images, ...)` leaves every `cores[i]` in the state `cores[i].step(images[i], masks[i], objects[i],
hard_mask=hard_mask, end=end[i])` would leave, and returns the same probabilities to fp32 round-off; so it mixes freely
with `step`, `incorporate_detection` and the semi-online buffer on the same cores, and clips may differ in config, start,
annotations, object count and length.  Per call and per padded frame size:

1. the key encoder and key projection run once over the clips whose feature store lacks the frame (batch B); each
   clip's store receives per-clip views of the batched outputs;
2. each clip reads its own memory (`MemoryManager.match_memory`, unchanged);
3. the mask decoder runs once over all propagating objects of all clips: the image-only parts (the fuser's image term,
   the skips of the up-sampling blocks) once per clip, handed to each object by its clip index;
4. annotations, aggregate and the output soft-max per clip, exactly as `step`;
5. the value encoder once over the objects of the clips that commit a memory frame, then `add_memory` /
   `update_sensory` per clip.

A group of one clip is routed to `core.step` itself (bit-identical).  Batching changes the kernel choice of the batched
convolutions (Winograd threshold, split-K, tile policy), so a batched clip matches its sequential run to round-off, not bit
for bit.
"""
from typing import Dict, List, Optional

import torch

from deva.hip import ops
from deva.inference.inference_core import DEVAInferenceCore
from deva.utils.tensor_utils import unpad


def _batch_of(items: List[torch.Tensor]) -> torch.Tensor:
    """[1,C,h,w] items -> [B,C,h,w]: a batch-strided view when the items are equally spaced in one storage (the views
    the batched key encoder stored), otherwise a guard-banded copy"""
    t0 = items[0]
    if len(items) == 1:
        return t0
    step = items[1].data_ptr() - t0.data_ptr()
    item_bytes = t0.numel() * t0.element_size()
    same = all(it.is_contiguous() and it.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr()
               and it.data_ptr() - t0.data_ptr() == k * step for k, it in enumerate(items))
    if same and step >= item_bytes and step % t0.element_size() == 0:
        return t0.as_strided((len(items), *t0.shape[1:]), (step // t0.element_size(), *t0.stride()[1:]),
                             t0.storage_offset())
    return _cat(items)


def _cat(items: List[torch.Tensor]) -> torch.Tensor:
    """torch.cat along dim 0 into a guard-banded tensor (the convolutions' vector gathers read a little past their inputs)"""
    out = ops._alloc((sum(t.shape[0] for t in items), *items[0].shape[1:]), items[0].device)
    torch.cat([t.float() for t in items], 0, out=out)
    return out


def _chunk(cores) -> Optional[int]:
    """objects per batched pass: the smallest chunk_size >= 1 among the clips (the memory-saving meaning of the flag)"""
    sizes = [c.chunk_size for c in cores if c.chunk_size is not None and c.chunk_size >= 1]
    return min(sizes) if sizes else None


def step_clips(cores: List[DEVAInferenceCore], images: List[torch.Tensor],
               masks: Optional[List[Optional[torch.Tensor]]] = None,
               objects: Optional[List[Optional[List[int]]]] = None, *,
               hard_mask: bool = True, end: Optional[List[bool]] = None) -> List[torch.Tensor]:
    """One frame of each clip; arguments per clip as `DEVAInferenceCore.step` takes them.  Returns the per-clip
    (num_objects+1)*H*W probabilities at the input size."""
    n = len(cores)
    masks = [None] * n if masks is None else list(masks)
    objects = [None] * n if objects is None else list(objects)
    end = [False] * n if end is None else [bool(e) for e in end]
    if not (len(images) == len(masks) == len(objects) == len(end) == n):
        raise ValueError('step_clips: one image, mask, object list and end flag per core')
    if n == 0:
        return []
    if any(c.network is not cores[0].network for c in cores):
        raise ValueError('step_clips: all cores must share one DEVA network object')
    if len({id(c) for c in cores}) != n:
        raise ValueError('step_clips: a core may appear once per call')
    if any(c.memory._shard_group is not None for c in cores):
        raise NotImplementedError('step_clips: sharded memories (shard_queries / shard_bank) are not supported')
    groups: Dict[tuple, List[int]] = {}
    for i, img in enumerate(images):
        h, w = img.shape[-2:]
        groups.setdefault((-(-h // 16), -(-w // 16)), []).append(i)
    out: List[Optional[torch.Tensor]] = [None] * n
    for members in groups.values():
        if len(members) == 1:
            i = members[0]
            out[i] = cores[i].step(images[i], masks[i], objects[i], hard_mask=hard_mask, end=end[i])
            continue
        probs = _step_group([cores[i] for i in members], [images[i] for i in members], [masks[i] for i in members],
                            [objects[i] for i in members], hard_mask, [end[i] for i in members])
        for i, p in zip(members, probs):
            out[i] = p
    return out


class _Clip:
    """one clip's frame inside a batched call: what `_step_group` carries from one batched pass to the next"""

    def __init__(self, core, image, mask, objects, end):
        self.core, self.mask, self.objects, self.end = core, mask, objects, end
        self.frame_ti, self.batch = core._advance(image)
        self.prob = None


def _step_group(cores, images, masks, objects, hard_mask, end) -> List[torch.Tensor]:
    net = cores[0].network
    g = net.graph()
    clips = [_Clip(*a) for a in zip(cores, images, masks, objects, end)]

    # 1. key encoder + key projection over the clips whose store lacks the frame
    todo = [c for c in clips if c.frame_ti not in c.core.image_feature_store]
    if todo:
        frames = _cat([c.batch for c in todo]) if len(todo) > 1 else _f32c(todo[0].batch)
        ms, feat = g.encode_image(frames)  # batch-major NCHW: item i of every output is clip i's tensor (a view)
        key, shrinkage, selection = g.transform_key(feat, True, True)  # (the convolutions take feat's batch stride)
        for i, c in enumerate(todo):
            c.core.image_feature_store.put(c.frame_ti, tuple(t[i:i + 1] for t in ms), feat[i:i + 1], key[i:i + 1],
                                           shrinkage[i:i + 1], selection[i:i + 1])
    for c in clips:
        store = c.core.image_feature_store
        c.ms = store.get_ms_features(c.frame_ti, c.batch)
        c.key, c.shrinkage, c.selection = store.get_key(c.frame_ti, c.batch)
        c.objects, c.commit, c.propagate = c.core._plan(c.mask, c.objects, hard_mask, c.end)

    # 2. + 3. memory read per clip, one decoder pass over the objects of all propagating clips
    decoding = []
    for c in clips:
        if not c.propagate:
            continue
        mem, om = c.core.memory, c.core.object_manager
        if not mem.engaged or not om.all_obj_ids:
            c.prob = c.core._segment(c.key, c.selection, c.ms, update_sensory=not c.end)  # (warns like `step`)
            continue
        c.ids = om.all_obj_ids
        c.readout = om.realize_dict(mem.match_memory(c.key, c.selection))
        c.sensory = mem.get_sensory(c.ids)[0]
        decoding.append(c)
    if decoding:
        _decode(net, decoding)

    # 4. annotations per clip
    for c in clips:
        c.prob = c.core._annotate(c.prob, c.mask, c.objects, hard_mask, c.propagate)

    # 5. value encoder over the objects of the committing clips
    committing = []
    for c in clips:
        if c.commit:
            c.ids = c.core._memory_frame_ids(c.core.last_mask, c.key)
            if c.ids is not None:
                committing.append(c)
    if committing:
        _encode_values(net, committing)

    for c in clips:
        c.core.image_feature_store.delete(c.frame_ti)
    return [unpad(c.prob, c.core.pad) for c in clips]


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _object_rows(clips):
    """(clip index of every object, [(first, end) object row of each clip])"""
    clip, spans, at = [], [], 0
    for p, c in enumerate(clips):
        clip += [p] * len(c.ids)
        spans.append((at, at + len(c.ids)))
        at += len(c.ids)
    return clip, spans


def _decode(net, clips) -> None:
    """`DEVA.segment` of every clip, the network passes batched over all their objects"""
    clip, spans = _object_rows(clips)
    ms = tuple(_batch_of([c.ms[k] for c in clips]) for k in range(3))
    new_sens, obj_logits = net.decode_objects(ms, _cat([c.readout for c in clips]), _cat([c.sensory for c in clips]),
                                              _cat([c.core.last_mask[0] for c in clips]), any(not c.end for c in clips),
                                              _chunk([c.core for c in clips]), clip)
    for c, (a, b) in zip(clips, spans):
        _, c.prob = net.soft_aggregate(obj_logits[a:b])
        if not c.end:
            c.core.memory.update_sensory(new_sens[a:b].unsqueeze(0), c.ids)


def _encode_values(net, clips) -> None:
    """`DEVAInferenceCore._add_memory` of every clip, the value encoder batched over all their objects"""
    clip, spans = _object_rows(clips)
    sensory = _cat([c.core.memory.get_sensory(c.ids)[0] for c in clips])
    value, new_sens = net.encode_objects(_cat([c.batch for c in clips]), _batch_of([c.ms[0] for c in clips]), sensory,
                                         _cat([c.core.last_mask[0] for c in clips]), True,
                                         _chunk([c.core for c in clips]), clip)
    for c, (a, b) in zip(clips, spans):
        c.core._commit_value(c.key, c.shrinkage, c.selection, value[a:b].unsqueeze(0), new_sens[a:b].unsqueeze(0), c.ids)
