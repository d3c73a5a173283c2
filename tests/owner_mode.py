"""Detection frames and the semi-online voting buffer of ONE clip in frame-owner mode (`shard_queries(owner=0)` /
`shard_bank(owner=0)`: rank 0 alone runs the network), run next to the unsharded clip.  Shared by
tests/test_owner_detections_gloo.py (2 and 3 CPU ranks over gloo, emulated ops) and tests/test_gpu_l_owner_detections.py
(a 1-rank RCCL group on the HIP library).

Every rank drives the same scenario of tests/scenarios.py / tests/driver_loops.py through the public interface; where
the core returns None (the probabilities on a non-owner rank) the driver gets a zero map of the frame's size instead
(`Rank`), as the `Recording` class of tests/test_sharded_read_gloo.py does for `step`."""
from typing import Dict, List, Optional

import numpy as np
import torch

import driver_loops
import scenarios
from workload import synth

MODES = ('owner', 'owner_bank')
RUNS = ('detection', 'consistent', 'edge', 'semionline')
# the host-side observables of tests/scenarios.py:run_edge_cases (the rest are probabilities, recorded by `Rank`)
EDGE_HOST_KEYS = ('no_memory_warned', 'soft_ids', 'soft_work_size', 'empty_detection_warned', 'empty_detection_objects',
                  'vanish_counts', 'vanish_engaged_after_purge')


def shard(core, mode: str):
    if mode == 'owner':
        core.memory.shard_queries(owner=0)
    elif mode == 'owner_bank':
        core.memory.shard_bank(owner=0)
    else:
        raise ValueError(mode)
    return core


class Rank:
    """a `DEVAInferenceCore` as a driver loop sees it on any rank: every output of `step` / `incorporate_detection` is
    recorded (None on a non-owner rank), and a zero 1*H*W map stands in for a None; everything else is the core's"""

    def __init__(self, core):
        self.core, self.outs = core, []

    def __getattr__(self, name):
        return getattr(self.core, name)

    def _keep(self, image, prob):
        self.outs.append(None if prob is None else prob.detach().float().cpu())
        return prob if prob is not None else torch.zeros((1, *image.shape[-2:]), device=image.device)

    def step(self, image, *args, **kwargs):
        return self._keep(image, self.core.step(image, *args, **kwargs))

    def incorporate_detection(self, image, *args, **kwargs):
        return self._keep(image, self.core.incorporate_detection(image, *args, **kwargs))


def run(name: str, net, mode: Optional[str], golden_dir: str, device='cpu'):
    """one scenario, unsharded (mode=None) or in a frame-owner mode -> (outputs of every step / detection of every
    core the scenario built, in call order; the cores; host-side results of the scenario)"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.object_info import ObjectInfo
    built: List[Rank] = []

    def make(cfg):
        core = DEVAInferenceCore(net, cfg)
        built.append(Rank(shard(core, mode) if mode is not None else core))
        return built[-1]

    np.random.seed(0)  # ids drawn on collisions (ObjectManager._fresh_id): the owner draws what the plain run draws
    extra = {}
    if name == 'detection':
        scenarios.run_detection_scenario(make, ObjectInfo, scenarios.DETECTION, device=device)
    elif name == 'consistent':  # the detections the reference recorded: matches, new buckets, purges, consolidations
        _, dets = scenarios.load_consistent_golden(golden_dir)
        scenarios.run_consistent_detection_scenario(make, ObjectInfo, scenarios.CONSISTENT, device=device, replay=dets)
    elif name == 'edge':  # items 4 and 5: empty detection, "Empty object mask!", everything purged, then a detection
        got = scenarios.run_edge_cases(make, device=device, make_info=ObjectInfo)
        extra = {k: got[k] for k in EDGE_HOST_KEYS}
    elif name == 'semionline':
        frames, dets = driver_loops.semionline_clip()
        cfg = synth.base_config(mem_every=2, max_missed_detection_count=2, max_num_objects=-1)
        masks, alive = driver_loops.semionline_loop(make, cfg, frames, dets, lambda **kw: ObjectInfo(**kw),
                                                    num_voting_frames=3, detection_every=5, device=device)
        extra = dict(alive=alive, masks=masks)
    else:
        raise ValueError(name)
    return [p for r in built for p in r.outs], [r.core for r in built], extra


def table(om) -> Dict:
    """the whole object table: ids in tmp order, tmp ids, votes, missed-detection counters, reserved ids, id mode"""
    objs = list(om.obj_to_tmp_id)
    return dict(ids=[int(o.id) for o in objs], tmp=[int(t) for t in om.obj_to_tmp_id.values()],
                tmp_order=[int(o.id) for o in om.tmp_id_to_obj.values()], poke=[int(o.poke_count) for o in objs],
                cats=[[None if c is None else int(c) for c in o.category_ids] for o in objs],
                scores=[[None if s is None else float(s) for s in o.scores] for o in objs],
                isthing=[o.isthing for o in objs], reserved=sorted(int(i) for i in om.all_historical_object_ids),
                long_id=bool(om.use_long_id))


def bank(mem) -> Dict:
    """bank sizes, bucket membership, usage counters and long-term keys of every bucket (CPU copies)"""
    st = {'engaged': bool(mem.engaged)}
    for b, objs in mem.work_mem.buckets.items():
        st[f'work{b}'] = (mem.work_mem.size(b), list(objs))
        if mem.use_long_term:
            st[f'use{b}'] = mem.work_mem.get_usage(b).cpu().clone()
            if mem.long_mem.engaged(b):
                st[f'long{b}'] = mem.long_mem.size(b)
                st[f'lkey{b}'] = mem.long_mem.key[b].cpu().clone()
                if mem.long_mem.save_usage:
                    st[f'luse{b}'] = mem.long_mem.get_usage(b).cpu().clone()
    return st


def bank_difference(want: Dict, got: Dict) -> float:
    """inf if sizes / buckets / membership differ, else the largest relative difference of the tensors"""
    if want.keys() != got.keys():
        return float('inf')
    worst = 0.0
    for k, a in want.items():
        b = got[k]
        if not torch.is_tensor(a):
            if a != b:
                return float('inf')
        elif a.shape != b.shape:
            return float('inf')
        elif a.numel():
            worst = max(worst, ((a - b).abs() / (1 + a.abs())).max().item())
    return worst
