"""Shared case of the scoring tests on the device (tests/test_gpu_t_panoptic.py): planes for the joint count, and the
semi-online clip of tests/driver_loops.py with a synthetic ground truth derived from its detections, run through
`FrameResultSaver('vipseg', id_postprocessor=StuffMerger(...))` with the scorer fed online from the saver's hook."""
import json
import os

import numpy as np
import torch
from PIL import Image

import driver_loops

CATEGORIES = [{'id': 0, 'name': 'wall', 'isthing': 0}, {'id': 2, 'name': 'door', 'isthing': 1},
              {'id': 5, 'name': 'floor', 'isthing': 0}, {'id': 8, 'name': 'person', 'isthing': 1}]
THING_GT, STUFF_GT, CROWD_GT = 66051, 131844, 900     # (ids using all three colour bytes)


# ------------------------------------------------------------------------------------------ planes for the count
def id_pool(n, seed):
    """n distinct ids in 1 .. 2^24 - 1, ascending, some in each colour byte"""
    rng = np.random.default_rng(seed)
    low = np.arange(1, min(n, 200) + 1)
    rest = rng.choice(np.arange(256, 2**24), size=max(n - low.size, 0) + 8, replace=False)
    return np.unique(np.concatenate([low, rest]))[:n].astype(np.int64) if n else np.zeros(0, dtype=np.int64)


def blocky(h, w, ids, seed, cell=9):
    """a plane of runs: cells of `cell` x `cell` pixels drawn from `ids`, with single pixels of other draws sprinkled in"""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, dtype=np.int64)
    coarse = rng.integers(0, ids.size, size=((h + cell - 1) // cell, (w + cell - 1) // cell))
    plane = ids[np.kron(coarse, np.ones((cell, cell), dtype=np.int64))[:h, :w]]
    noise = rng.random((h, w)) < 0.03
    plane[noise] = ids[rng.integers(0, ids.size, size=int(noise.sum()))]
    return plane


def planes(h, w, n_gt, n_pred, seed):
    """-> (gt ids int32 [h,w], gt table, predicted ids int64 [h,w], predicted table): both planes hold id 0, the ids of
    their tables and a few ids that no table lists (the prediction also a negative one and one above 2^31)"""
    gt_table, pred_table = id_pool(n_gt, seed), id_pool(n_pred, seed + 1)
    stray_gt = np.setdiff1d(np.array([7777777, 12345, 16777215]), gt_table)
    stray_pred = np.setdiff1d(np.array([424242, 999]), pred_table)
    gt = blocky(h, w, np.concatenate([[0], gt_table[:300], stray_gt]), seed + 2, cell=7)
    pred = blocky(h, w, np.concatenate([[0], pred_table[:300], stray_pred, [-5, 2**31 + 3]]), seed + 3, cell=9)
    if n_gt > 300:      # every id of a long table somewhere
        gt.reshape(-1)[:n_gt - 300] = gt_table[300:][:gt.size]
    if n_pred > 300:
        pred.reshape(-1)[-(n_pred - 300):] = pred_table[300:][:pred.size]
    return gt.astype(np.int32), gt_table, pred, pred_table


def rgb(plane):
    plane = np.asarray(plane).astype(np.int64)
    return np.stack([plane % 256, plane // 256 % 256, plane // 65536 % 256], axis=-1).astype(np.uint8)


def channel_form(pred, pred_table, seed):
    """the tracker's form of a predicted id plane: (int16 channel plane, uint16 channel -> slot table).  Every distinct
    id gets a channel; the first listed id gets a second one that takes every other of its pixels (a shared slot); an
    unlisted id's entry is >= P; a few pixels carry a negative channel and one beyond the table, standing for unlisted
    ids.  -> (index, lut, the id plane that the form stands for)"""
    rng = np.random.default_rng(seed)
    pred = np.array(pred, dtype=np.int64)
    ids = np.unique(pred)
    ids = ids[ids != 0]
    p = len(pred_table) + 2
    index = ((np.searchsorted(ids, pred) + 1) * (pred != 0)).astype(np.int64)
    at = np.clip(np.searchsorted(pred_table, ids), 0, max(len(pred_table) - 1, 0))
    listed = (np.asarray(pred_table)[at] == ids) if len(pred_table) else np.zeros(ids.size, dtype=bool)
    slots = np.where(listed, at + 2, 1)
    lut = np.concatenate([[0], slots]).astype(np.int64)
    unlisted = np.nonzero(lut == 1)[0]
    if unlisted.size:
        lut[unlisted[0]] = p + 3                       # an entry >= P counts as slot 1
    first = np.nonzero(lut >= 2)[0]
    if first.size:                                     # a second channel for the first listed id
        lut = np.concatenate([lut, [lut[first[0]]]])
        mask = index == first[0]
        mask.reshape(-1)[::2] = False
        index[mask] = lut.size - 1
    stands_for = pred.copy()
    stray = rng.random(pred.shape) < 0.01
    index[stray] = np.where(rng.random(int(stray.sum())) < 0.5, -1, lut.size + 5)
    stands_for[stray] = -1
    return index.astype(np.int16), lut.astype(np.uint16), stands_for


# ------------------------------------------------------------------------------------------ the end-to-end clip
def ground_truth(dets):
    """a ground truth derived from the clip's detections: the drifting thing box as one track, the stuff box where it is
    detected, a crowd strip of the thing's category on the right edge and a VOID strip at the bottom
    -> ([H,W] int32 planes, segments_info per frame)"""
    out, infos = [], []
    for t, (mask, info) in enumerate(dets):
        h, w = mask.shape
        plane = np.zeros((h, w), dtype=np.int32)
        plane[56:92, 60:126] = STUFF_GT
        thing = (mask == 7 + 10 * t).numpy()
        plane[np.roll(thing, 3, axis=1)] = THING_GT      # (not quite where the detector saw it)
        plane[0:40, w - 8:] = CROWD_GT
        plane[h - 2:] = 0
        out.append(plane)
        infos.append([dict(id=i, category_id=c, iscrowd=k, area=int((plane == i).sum()))
                      for i, c, k in ((THING_GT, 2, 0), (STUFF_GT, 5, 0), (CROWD_GT, 2, 1)) if (plane == i).any()])
    return out, infos


def semionline_with_saver(make_processor, config, frames_u8, detections, make_info, save, num_voting_frames=3,
                          detection_every=5, device='cuda', seed=0):
    """the schedule of driver_loops.semionline_loop (eval_with_detections.py:150-297) with the driver's saver call
    `save(prob, frame name)` left to the caller"""
    np.random.seed(seed)
    vid_length = frames_u8.shape[0]
    processor = make_processor(driver_loops._count_usage(config, vid_length))
    next_voting_frame = num_voting_frames - 1
    processor.enabled_long_id()
    for ti in range(vid_length):
        det_mask, det_info = detections[ti]
        image = driver_loops.to_network_input(frames_u8[ti]).unsqueeze(0).to(device)[0]
        mask = det_mask.unsqueeze(0).to(device)[0]
        info = {'frame': [f'{ti:05d}.jpg'], 'shape': None, 'need_resize': [False], 'save': [True], 'path_to_image': [None]}
        frame_info = driver_loops.FrameInfo(image, mask, [make_info(**i) for i in det_info], ti, info)
        if ti + num_voting_frames > next_voting_frame:
            processor.add_to_temporary_buffer(frame_info)
            if ti == next_voting_frame:
                first = processor.frame_buffer[0]
                _, vmask, new_segments_info = processor.vote_in_temporary_buffer(keyframe_selection='first')
                prob = processor.incorporate_detection(first.image, vmask, new_segments_info)
                next_voting_frame += detection_every
                if next_voting_frame >= vid_length:
                    next_voting_frame = vid_length + num_voting_frames
                save(processor, prob, first.name)
                for fi in processor.frame_buffer[1:]:
                    prob = processor.step(fi.image, None, None, end=(fi.ti == vid_length - 1))
                    save(processor, prob, fi.name)
                processor.clear_buffer()
        else:
            prob = processor.step(image, None, None, end=(ti == vid_length - 1))
            save(processor, prob, info['frame'][0])
    return processor


def write_truth(root, video, gt_planes, gt_infos):
    """the truth tree and the ground-truth JSON of one video -> (truth dir, JSON path)"""
    truth = os.path.join(root, 'truth')
    os.makedirs(os.path.join(truth, video), exist_ok=True)
    images, annos = [], []
    for t, (plane, info) in enumerate(zip(gt_planes, gt_infos)):
        name = f'{t:05d}.png'
        Image.fromarray(rgb(plane)).save(os.path.join(truth, video, name))
        images.append({'file_name': name})
        annos.append({'file_name': name, 'segments_info': info})
    gt_json = os.path.join(root, 'gt.json')
    with open(gt_json, 'w') as f:
        json.dump({'categories': CATEGORIES, 'videos': [{'video_id': video, 'images': images}],
                   'annotations': [{'video_id': video, 'annotations': annos}]}, f)
    return truth, gt_json
