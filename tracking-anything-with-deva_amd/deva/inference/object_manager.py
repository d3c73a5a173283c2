"""Object id bookkeeping (interface of deva/inference/object_manager.py:8-168).

Real object ids never change; temporary ids are the 1-based channel positions of the objects in
the network tensors and are re-packed when objects are removed."""
import struct
from typing import Dict, List, Sequence, Set, Tuple, Union

import numpy as np
import torch

from deva.inference.object_info import ObjectInfo

# ---------------------------------------------------------------------- byte form (frame-owner mode, several GPUs)
# Little-endian, no padding.  An object: id (int64), thing flag (uint8: 0 None, 1 False, 2 True), missed-detection
# counter (int32), then its category votes and its score votes, each as a count (uint32) followed by one entry per
# vote: a flag byte (0 = None) and, when set, the value (int64 category / float64 score).  21 bytes per object, plus
# 9 per vote of either list (1 for a None vote).
_THING_CODE = {None: 0, False: 1, True: 2}
_THING_OF = {0: None, 1: False, 2: True}


def _pack_votes(values: Sequence, fmt: str) -> bytes:
    out = [struct.pack('<I', len(values))]
    for v in values:
        out.append(b'\x00' if v is None else b'\x01' + struct.pack(fmt, v))
    return b''.join(out)


def _unpack_votes(data: bytes, at: int, fmt: str, size: int) -> Tuple[List, int]:
    (n,), at = struct.unpack_from('<I', data, at), at + 4
    out = []
    for _ in range(n):
        present, at = data[at], at + 1
        if present:
            out.append(struct.unpack_from(fmt, data, at)[0])
            at += size
        else:
            out.append(None)
    return out, at


def pack_objects(objects: Sequence[ObjectInfo]) -> bytes:
    """ObjectInfo list -> bytes (count, then the objects in order; categories travel as int, scores as float)"""
    out = [struct.pack('<I', len(objects))]
    for o in objects:
        out.append(struct.pack('<qBi', int(o.id), _THING_CODE[o.isthing], int(o.poke_count)))
        out.append(_pack_votes([None if c is None else int(c) for c in o.category_ids], '<q'))
        out.append(_pack_votes([None if s is None else float(s) for s in o.scores], '<d'))
    return b''.join(out)


def unpack_objects(data: bytes, at: int = 0) -> Tuple[List[ObjectInfo], int]:
    """inverse of `pack_objects` -> (objects, offset after them)"""
    (n,), at = struct.unpack_from('<I', data, at), at + 4
    objects = []
    for _ in range(n):
        oid, thing, poke = struct.unpack_from('<qBi', data, at)
        at += 13
        o = ObjectInfo(id=oid, isthing=_THING_OF[thing])
        o.poke_count = poke
        o.category_ids, at = _unpack_votes(data, at, '<q', 8)
        o.scores, at = _unpack_votes(data, at, '<d', 8)
        objects.append(o)
    return objects, at


class ObjectManager:
    def __init__(self):
        self.obj_to_tmp_id: Dict[ObjectInfo, int] = {}
        self.tmp_id_to_obj: Dict[int, ObjectInfo] = {}
        self.obj_id_to_obj: Dict[int, ObjectInfo] = {}
        self.all_historical_object_ids: Set[int] = set()  # removed ids stay reserved
        self.use_long_id = False

    def _reindex(self) -> None:
        self.obj_id_to_obj = {obj.id: obj for obj in self.obj_to_tmp_id}

    def _fresh_id(self, wanted: int) -> int:
        """keep `wanted` unless it collides (or is a short id in long-id mode); then draw random
        ids from the active id space until one is free (object_manager.py:40-55)"""
        new_id = wanted
        for _ in range(5001):
            if new_id not in self.all_historical_object_ids and not (self.use_long_id and new_id < 256):
                return new_id
            new_id = np.random.randint(256, 256**3) if self.use_long_id else np.random.randint(1, 256)
        raise ValueError('We cannot find a new ID for this object. Perhaps you should use long ID?')

    def add_new_objects(self, objects: Union[List[ObjectInfo], ObjectInfo, List[int]]) -> Tuple[List[int], List[int]]:
        if not isinstance(objects, list):
            objects = [objects]
        tmp_ids, obj_ids = [], []
        for obj in objects:
            if isinstance(obj, int):
                obj = ObjectInfo(id=obj)
            new_obj = ObjectInfo(id=self._fresh_id(obj.id))
            new_obj.copy_meta_info(obj)
            tmp = len(self.obj_to_tmp_id) + 1
            self.obj_to_tmp_id[new_obj] = tmp
            self.tmp_id_to_obj[tmp] = new_obj
            self.all_historical_object_ids.add(new_obj.id)
            tmp_ids.append(tmp)
            obj_ids.append(new_obj.id)
        self._reindex()
        assert tmp_ids == sorted(tmp_ids), 'tmp id assignment bugged'
        return tmp_ids, obj_ids

    def delete_object(self, obj_ids_to_remove: Union[int, List[int]]) -> None:
        if isinstance(obj_ids_to_remove, int):
            obj_ids_to_remove = [obj_ids_to_remove]
        survivors = [self.tmp_id_to_obj[t] for t in range(1, len(self.obj_to_tmp_id) + 1)
                     if self.tmp_id_to_obj[t].id not in obj_ids_to_remove]
        self.obj_to_tmp_id = {obj: i + 1 for i, obj in enumerate(survivors)}
        self.tmp_id_to_obj = {i + 1: obj for i, obj in enumerate(survivors)}
        self._reindex()

    def purge_inactive_objects(self, max_missed_detection_count: int) -> Tuple[bool, List[int], List[int]]:
        """drop objects missed more than the allowed number of detections; returns
        (anything purged, tmp ids kept (old numbering), object ids kept)"""
        gone = [o.id for o in self.obj_to_tmp_id if o.poke_count > max_missed_detection_count]
        tmp_keep = [t for o, t in self.obj_to_tmp_id.items() if o.poke_count <= max_missed_detection_count]
        obj_keep = [o.id for o in self.obj_to_tmp_id if o.poke_count <= max_missed_detection_count]
        if gone:
            self.delete_object(gone)
        return len(gone) > 0, tmp_keep, obj_keep

    def _tmp_to_obj_table(self, device) -> torch.Tensor:
        table = [0] * (max(self.tmp_id_to_obj, default=0) + 1)
        for tmp_id, obj in self.tmp_id_to_obj.items():
            table[tmp_id] = int(obj.id)
        return torch.tensor(table, dtype=torch.int64, device=device)

    def prob_to_obj_cls(self, prob: torch.Tensor, size=None) -> torch.Tensor:
        """(no+1)*H*W probabilities of `DEVAInferenceCore.step` -> object-id index mask, optionally at
        another resolution: the drivers' F.interpolate(bilinear) -> argmax -> tmp_to_obj_cls tail
        (eval_vos.py:170-181, result_utils.py:98-102) as one kernel, so that H*W labels leave the
        device instead of (no+1)*H*W floats (not part of the reference's interface)"""
        from deva.hip import ops
        return ops.index_mask(prob.contiguous(), size, self._tmp_to_obj_table(prob.device))

    def frame_result(self, prob: torch.Tensor, size=None, *, image=None, rle: bool = False, color=None,
                     labels: bool = False):
        """everything a frame's consumer needs from the probabilities of `DEVAInferenceCore.step`, in one device pass
        (plus the run-length kernels with rle=True) instead of the per-object host passes of the reference's saver
        (result_utils.py:98-242): a `FrameResult` with the gray or colour id plane, the overlay on `image` and, if
        asked, the object-id labels of `prob_to_obj_cls` still on the device, and one host-side record per object of
        `get_current_segments_info()` with area, bbox and (rle=True) the COCO dict (deva/inference/frame_results.py;
        not part of the reference's interface)"""
        from deva.inference.frame_results import launch_frame
        return launch_frame(self, prob, size, image=image, rle=rle, color=color, labels=labels).finish()

    def tmp_to_obj_cls(self, mask) -> torch.Tensor:
        """tmp-id index mask -> object-id index mask"""
        if mask.is_cuda and mask.dtype == torch.int64 and self.tmp_id_to_obj:
            # one relabelling pass on the device instead of one masked assignment per object
            from deva.hip import ops
            return ops.lut_remap(mask.contiguous(), self._tmp_to_obj_table(mask.device))
        new_mask = torch.zeros_like(mask)  # host-side masks (e.g. in the result savers)
        for tmp_id, obj in self.tmp_id_to_obj.items():
            new_mask[mask == tmp_id] = obj.id
        return new_mask

    def get_tmp_to_obj_mapping(self) -> Dict[int, int]:
        # {object id: tmp id}, the table scripts/merge_multi_scale.py:61-64 reads back.  NB the reference unpacks the
        # items of tmp_id_to_obj as (obj, tmp_id) (object_manager.py:119-121) and so raises AttributeError on an int
        # as soon as an object exists; the intended mapping is returned here instead of raising.
        return {obj.id: tmp_id for tmp_id, obj in self.tmp_id_to_obj.items()}

    def realize_dict(self, obj_dict: Dict[int, torch.Tensor]) -> torch.Tensor:
        """{object id: tensor} -> stacked tensor in tmp-id order"""
        stack, order = getattr(obj_dict, 'stack', None), getattr(obj_dict, 'order', None)
        if stack is not None and order == [obj.id for obj in self.tmp_id_to_obj.values()]:
            return stack  # MemoryManager.match_memory already produced the rows in this order: no copy
        rows = []
        for obj in self.tmp_id_to_obj.values():
            if obj.id not in obj_dict:
                raise NotImplementedError
            rows.append(obj_dict[obj.id])
        return torch.stack(rows, dim=0)

    def make_one_hot(self, cls_mask: torch.Tensor) -> torch.Tensor:
        planes = [cls_mask == obj.id for obj in self.tmp_id_to_obj.values()]
        if not planes:
            return torch.zeros((0, *cls_mask.shape), dtype=torch.bool, device=cls_mask.device)
        return torch.stack(planes, dim=0)

    def get_current_segments_info(self) -> List[Dict]:
        return [{'category_id': obj.vote_category_id(), 'id': int(obj.id), 'score': obj.vote_score()}
                for obj in self.obj_to_tmp_id]

    @property
    def all_obj_ids(self) -> List[int]:
        return [k.id for k in self.obj_to_tmp_id]

    @property
    def num_obj(self) -> int:
        return len(self.obj_to_tmp_id)

    def has_all(self, objects: List[int]) -> bool:
        # NB the reference compares ints against ObjectInfo keys, which raises AttributeError for an
        # id that is already registered (object_manager.py:161-165 + object_info.py:58); asking
        # about registered ids is answered here instead of raising.
        return all(o in self.obj_id_to_obj for o in objects)

    def find_object_by_id(self, obj_id) -> ObjectInfo:
        return self.obj_id_to_obj[obj_id]

    # ------------------------------------------------------------------ one clip on several GPUs
    def encode_state(self) -> bytes:
        """the whole table as bytes, the same bytes for the same table: use_long_id (1 B), the reserved ids (count +
        sorted int64), then the objects in tmp-id order (`pack_objects`).  Frame-owner mode: the owner's decisions of a
        detection frame travel to the other ranks in this form (`DEVAInferenceCore.incorporate_detection`)."""
        hist = sorted(int(i) for i in self.all_historical_object_ids)
        objects = [self.tmp_id_to_obj[t] for t in range(1, len(self.tmp_id_to_obj) + 1)]
        return struct.pack(f'<?I{len(hist)}q', bool(self.use_long_id), len(hist), *hist) + pack_objects(objects)

    def load_state(self, data: bytes, at: int = 0) -> int:
        """replace this table with the one `encode_state` wrote into `data` at offset `at`; -> offset after it"""
        use_long_id, n = struct.unpack_from('<?I', data, at)
        hist = struct.unpack_from(f'<{n}q', data, at + 5)
        objects, end = unpack_objects(data, at + 5 + 8 * n)
        self.use_long_id = use_long_id
        self.all_historical_object_ids = set(hist)
        self.obj_to_tmp_id = {obj: i + 1 for i, obj in enumerate(objects)}
        self.tmp_id_to_obj = {i + 1: obj for i, obj in enumerate(objects)}
        self._reindex()
        return end
