"""The byte form in which frame-owner mode sends the owner's decisions to the other ranks
(`ObjectManager.encode_state` / `load_state`, `pack_objects` / `unpack_objects`; DESIGN §5 counts its size): it
round-trips every field the tracker keeps, is the same for the same table whatever the history of its sets, and has
the size DESIGN states."""
from deva.inference.object_info import ObjectInfo
from deva.inference.object_manager import ObjectManager, pack_objects, unpack_objects

import owner_mode


def _manager(reserved_order):
    om = ObjectManager()
    om.use_long_id = True
    om.add_new_objects([ObjectInfo(300, category_id=3, isthing=True, score=0.75),
                        ObjectInfo(4000, category_id=None, isthing=False, score=None),
                        ObjectInfo(70000, category_id=7, isthing=None, score=0.5)])
    first = om.find_object_by_id(300)
    first.merge(ObjectInfo(1, category_id=None, score=0.125))
    first.merge(ObjectInfo(2, category_id=3, score=1 / 3))
    first.poke()
    om.find_object_by_id(70000).poke()
    om.find_object_by_id(70000).poke()
    om.delete_object(4000)  # its id stays reserved
    om.all_historical_object_ids = set(reserved_order) | om.all_historical_object_ids
    return om


def test_object_table_round_trips_with_every_field():
    om = _manager([5000, 256])
    data = om.encode_state()
    other = ObjectManager()
    assert other.load_state(b'\x07' + data, 1) == len(data) + 1  # read at an offset, returns the end
    assert owner_mode.table(other) == owner_mode.table(om)
    assert [o.vote_category_id() for o in other.obj_to_tmp_id] == [o.vote_category_id() for o in om.obj_to_tmp_id]
    assert [o.vote_score() for o in other.obj_to_tmp_id] == [o.vote_score() for o in om.obj_to_tmp_id]
    assert other.find_object_by_id(70000).poke_count == 2 and other.use_long_id
    assert other.encode_state() == data


def test_object_table_bytes_are_deterministic_and_sized_as_documented():
    a, b = _manager([5000, 256, 9999]), _manager([9999, 256, 5000])
    assert a.encode_state() == b.encode_state()
    # 5 + 8 x reserved ids + 4 + per object 21 + 9 per vote (1 per None vote)
    size = 5 + 8 * len(a.all_historical_object_ids) + 4
    for o in a.obj_to_tmp_id:
        votes = o.category_ids + o.scores
        size += 21 + sum(1 if v is None else 9 for v in votes)
    assert len(a.encode_state()) == size
    assert len(ObjectManager().encode_state()) == 9


def test_segment_list_round_trips():
    segs = [ObjectInfo(1, category_id=2, isthing=True, score=0.9), ObjectInfo(2), ObjectInfo(3, isthing=False, score=0.7)]
    segs[0].merge(segs[2])
    data = b'xyz' + pack_objects(segs)
    got, end = unpack_objects(data, 3)
    assert end == len(data)
    assert [(o.id, o.isthing, o.category_ids, o.scores, o.poke_count) for o in got] == \
        [(o.id, o.isthing, o.category_ids, o.scores, o.poke_count) for o in segs]
