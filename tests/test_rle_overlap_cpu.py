"""The run-length overlap without a GPU: libdeva_rle_overlap.so on its ABI, the argument errors before any launch, the plan's
and the walk's host code under the host sanitizers, the kernels' static resources, the binding's chunks, rules O1-O7 and
`iou` by hand, and the binding's host half behind the numpy statement (tests/overlap_case.py, tests/emu_overlap.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_util
import emu_overlap as EO
import overlap_case as OC
import rle_case as LC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_rle_overlap.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
OVERLAP_SRC = os.path.join(CSRC, 'rle_overlap')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_overlap_check', 'deva_overlap_intersections', 'deva_overlap_last_error', 'deva_overlap_limits', 'deva_overlap_plan',
        'deva_overlap_scratch', 'deva_overlap_version']


def _built():
    from deva.hip import rle_overlap
    return abi_util.built(rle_overlap)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    ro = _built()
    exported, _ = abi_util.exported(ro.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(ro.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_OVERLAP_ABI_VERSION 1\b', header)
    assert ro.ABI_VERSION == 1 and ro.lib().deva_overlap_version() == 1
    for name, value in (('MAX_MASKS', ro.MAX_MASKS), ('MAX_WORDS', ro.MAX_WORDS), ('D_CHUNK', ro.D_CHUNK), ('LDS_RUNS', ro.LDS_RUNS),
                        ('SCAN_CHUNK', ro.SCAN_CHUNK), ('DT', ro.DT), ('GT', ro.GT)):
        assert re.search(rf'#define DEVA_OVERLAP_{name} {value}\b', header), name
    for rule in ('O1', 'O2', 'O3', 'O4', 'O5', 'O6', 'O7', 'O8', 'O9'):
        assert re.search(rf'^ \*   {rule}  ', header, flags=re.M), rule
    assert ro.overlap_limits() == ro.LimitInfo(ro.MAX_MASKS, ro.MAX_WORDS, 256, ro.D_CHUNK, ro.LDS_RUNS, ro.SCAN_CHUNK)
    from deva.hip import rle
    assert rle.intersections is ro.intersections and rle.iou is ro.iou                # re-exports only
    assert not any('overlap' in name for name in rle.SIGNATURES)
    assert (ro.MAX_MASKS, ro.MAX_WORDS) == (rle.MAX_MASKS, rle.MAX_WORDS)             # "as in deva_rle_limits"


def test_no_symbol_is_shared_and_the_other_libraries_have_not_moved():
    from deva import hip
    from deva.hip import mask_runs, metrics, pair_metrics, regions, rle, vos_metrics
    ro = _built()
    exported, mine = abi_util.exported(ro.LIB_PATH)
    assert all(name.startswith('deva_overlap_') for name in exported)
    others = (hip, metrics, vos_metrics, pair_metrics, regions, rle, mask_runs)
    for other in others:
        theirs_exported, theirs = abi_util.exported(other.LIB_PATH)
        assert not any(n.startswith('deva_overlap') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other.LIB_PATH, shared)
    for name in ('deva_hip.h', 'deva_metrics.h', 'deva_vos_metrics.h', 'deva_pair_metrics.h', 'deva_regions.h', 'deva_rle.h',
                 'deva_mask_runs.h'):
        assert 'deva_overlap' not in open(os.path.join(ROOT, 'include', name)).read(), name
    abi_util.inference_entry_points([])       # libdeva_hip.so stays at its ABI version
    assert rle.ABI_VERSION == 1 and rle.lib().deva_rle_version() == 1 and len(rle.SIGNATURES) == 6
    assert mask_runs.ABI_VERSION == 1 and mask_runs.lib().deva_runs_version() == 1 and len(mask_runs.SIGNATURES) == 7
    counts = {m.__name__: (m.ABI_VERSION, len(m.SIGNATURES)) for m in (metrics, vos_metrics, pair_metrics, regions)}
    for m in (metrics, vos_metrics, pair_metrics, regions):
        exported_there, _ = abi_util.exported(m.LIB_PATH)
        assert len(exported_there) == counts[m.__name__][1] == len(m.SIGNATURES), m.__name__
    libs = sorted(f for f in os.listdir(os.path.dirname(ro.LIB_PATH)) if re.fullmatch(r'libdeva_\w+\.so', f))
    assert len(libs) == 8 and 'libdeva_rle_overlap.so' in libs


def test_struct_mirrors_have_the_c_layout(tmp_path):
    ro = _built()
    assert [f[0] for f in ro.Plan._fields_] == list(ro.PlanInfo._fields) and [f[0] for f in ro.Limits._fields_] == list(ro.LimitInfo._fields)
    lines = []
    for tag, mirror in (('deva_overlap_plan', ro.Plan), ('deva_overlap_limits', ro.Limits)):
        lines.append(f'printf("%zu\\n", sizeof(struct {tag}));\n')
        lines += [f'printf("%zu\\n", offsetof(struct {tag}, {f[0]}));\n' for f in mirror._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_rle_overlap.h"\nint main(void){\n' + ''.join(lines) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for mirror in (ro.Plan, ro.Limits):
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert vals == want


def test_plan_is_host_side():
    ro = _built()
    lds = 2 * (ro.LDS_RUNS + 1) * 4 + 2 * ro.D_CHUNK * 4
    assert lds <= 16 * 1024
    assert ro.overlap_plan(64, 64, 64 + 1 + 64 * 301) == ro.PlanInfo(128, 8 * 64, 8, lds, 4 * 64 * 301)
    assert ro.overlap_plan(20, 5, 5 + 1 + 5 * 11) == ro.PlanInfo(25, 15, 3, lds, 4 * 55)
    assert ro.overlap_plan(ro.D_CHUNK, 1, 4).d_chunks == 1 and ro.overlap_plan(ro.D_CHUNK + 1, 1, 4).d_chunks == 2
    assert ro.overlap_plan(0, 0, 1) == ro.PlanInfo(0, 0, 0, lds, 0)
    assert ro.overlap_plan(65536, 65536, 65537 + 2 * 65536).pair_grid == 65536       # capped: the rest is a grid-stride loop
    assert ro.overlap_scratch(5 + 1 + 5 * 11, 5) == 4 * 55 and ro.overlap_scratch(1, 0) == 0
    with pytest.raises(ro.DevaHipError, match='dt: 0 to 65536 masks'):
        ro.overlap_plan(65537, 1, 4)
    with pytest.raises(ro.DevaHipError, match='gt: 0 to 65536 masks'):
        ro.overlap_plan(1, -1, 4)
    with pytest.raises(ro.DevaHipError, match=r'gt: a run array of 3 to 67108864 words \(got 2\)'):
        ro.overlap_plan(1, 2, 2)
    assert ro.overlap_scratch(ro.MAX_WORDS + 1, 1) == -1 and ro.overlap_scratch(ro.MAX_WORDS, 1) == 4 * (ro.MAX_WORDS - 2)


def test_the_threshold_shapes_of_the_gpu_tests():
    """the frame of tests/test_gpu_zc_rle_overlap.py for the LDS threshold: the smallest that holds L + 1 runs"""
    ro = _built()
    h, w = OC.threshold_frame(ro.LDS_RUNS)
    assert h * w == ro.LDS_RUNS + 1
    for r in (ro.LDS_RUNS - 1, ro.LDS_RUNS, ro.LDS_RUNS + 1):
        c = OC.run_counts(r, h, w)
        assert len(c) == r and LC.valid(c, h, w) and LC.counts_of(LC.plane(c, h, w)) == c


# ------------------------------------------------------------------------------------------ refusals before any launch
def test_wrapper_refusals_happen_before_any_launch(monkeypatch):
    ro = _built()
    monkeypatch.setattr(ro, '_launch', lambda *a: pytest.fail('a launch was reached'))
    ok = [{'size': [2, 3], 'counts': [2, 4]}, {'size': [2, 3], 'counts': [6]}]
    kw = dict(device='cpu')
    with pytest.raises(ro.DevaHipError, match='intersections: dt: a list of masks expected'):
        ro.intersections(ok[0], ok, **kw)
    with pytest.raises(ro.DevaHipError, match='intersections: gt: a list of masks expected'):
        ro.intersections(ok, 'abc', **kw)
    with pytest.raises(ro.DevaHipError, match=r'intersections: gt: mask 1: the counts sum to 5, H \* W is 6'):
        ro.intersections(ok, [ok[0], {'size': [2, 3], 'counts': [2, 3]}], **kw)
    with pytest.raises(ro.DevaHipError, match='intersections: dt: mask 0: a count is negative'):
        ro.intersections([{'size': [2, 3], 'counts': [-1, 7]}], ok, **kw)
    with pytest.raises(ro.DevaHipError, match=r"intersections: gt: mask 0: size 3 x 2, the call's is 2 x 3"):
        ro.intersections(ok, [{'size': [3, 2], 'counts': [6]}], **kw)
    with pytest.raises(ro.DevaHipError, match='intersections: dt: no mask carries its size'):
        ro.intersections([[6]], [], **kw)
    with pytest.raises(ro.DevaHipError, match="character"):
        ro.intersections([{'size': [2, 3], 'counts': 'a~'}], ok, **kw)
    for bad in (dict(max_masks=0), dict(max_words=3), dict(max_masks=ro.MAX_MASKS + 1), dict(max_words=ro.MAX_WORDS + 1)):
        with pytest.raises(ro.DevaHipError, match='limits of 1 to 65536 masks and 4 to 67108864 words'):
            ro.intersections(ok, ok, **bad, **kw)
    with pytest.raises(ro.DevaHipError, match=r'intersections: dt: mask 0: 2 runs are above the limit of one call \(4 words\)'):
        ro.intersections(ok, ok, max_words=4, **kw)
    with pytest.raises(ro.DevaHipError, match='`stream` must be a torch.cuda.Stream'):
        ro.intersections(ok, ok, stream=0, **kw)
    with pytest.raises(ro.DevaHipError, match=r"out\['inter'\] must be a contiguous torch.int32 \[2, 2\]"):
        ro.intersections(ok, ok, out={'inter': torch.zeros(2, 2, dtype=torch.int64)}, **kw)
    with pytest.raises(ro.DevaHipError, match=r"out\['area_g'\] must be a contiguous torch.int32 \[2\]"):
        ro.intersections(ok, ok, out={'area_g': torch.zeros(3, dtype=torch.int32)}, **kw)
    with pytest.raises(ro.DevaHipError, match='iscrowd has 1 entries for 2'):
        ro.iou(ok, ok, [0], **kw)


def test_host_tensors_are_refused_there_is_no_cpu_path():
    ro = _built()
    ok = [{'size': [2, 3], 'counts': [2, 4]}]
    with pytest.raises(ro.DevaHipError, match='must live on the HIP device'):
        ro.intersections(ok, ok, device='cpu')
    with pytest.raises(ro.DevaHipError, match='must live on the HIP device'):
        ro.intersections(ok, ok, out={'inter': torch.zeros(1, 1, dtype=torch.int32)})
    with pytest.raises(ro.DevaHipError, match='must live on the HIP device'):
        ro.iou(ok, ok, device='cpu')


A = 1 << 40   # made-up device addresses: validation fails before anything is dereferenced or launched
DT_DEV, GT_DEV, SCRATCH, INTER, AREA_D, AREA_G = (A + (k << 30) for k in range(6))


def _call(L, dt, gt, d=2, g=2, h=2, w=3, dt_dev=DT_DEV, gt_dev=GT_DEV, box_d=None, box_g=None, scratch=SCRATCH, nbytes=20, inter=INTER,
          pitch=2, area_d=AREA_D, area_g=AREA_G):
    a, b = np.asarray(dt, dtype=np.int32), np.asarray(gt, dtype=np.int32)
    return L.deva_overlap_intersections(a.ctypes.data, dt_dev, a.size, d, b.ctypes.data, gt_dev, b.size, g, h, w, box_d, box_g, scratch, nbytes,
                                        inter, pitch, area_d, area_g, None)


def test_library_refusals_before_any_launch():
    ro = _built()
    L = ro.lib()
    err = L.deva_overlap_last_error
    ok = [0, 3, 5, 0, 2, 6, 0, 6]
    for kw, text in ((dict(h=0), b'bad size 0 x 3'), (dict(h=46341, w=46341), b'bad size'), (dict(d=-1), b'dt: 0 to 65536 masks'),
                     (dict(g=65537), b'gt: 0 to 65536 masks'), (dict(dt_dev=None), b'dt: null or misaligned'),
                     (dict(gt_dev=GT_DEV + 2), b'gt: null or misaligned'), (dict(box_d=A + 512), b"give both sides' or neither"),
                     (dict(box_d=A + 513, box_g=A + 1024), b'boxes: misaligned'), (dict(scratch=None), b'scratch: null or not 4-byte aligned'),
                     (dict(scratch=SCRATCH + 2), b'scratch: null or not 4-byte aligned'),
                     (dict(nbytes=19), b'scratch_bytes: 19 given, deva_overlap_scratch asks for 20'), (dict(inter=None), b'inter: null or misaligned'),
                     (dict(pitch=1), b'pitch: 1 elements for rows of 2'), (dict(area_d=None), b'area_d: null'), (dict(area_g=AREA_G + 1), b'area_g: null or misaligned'),
                     (dict(area_g=AREA_D + 4), b'area_d overlaps area_g'), (dict(inter=SCRATCH + 16), b'scratch overlaps inter'),
                     (dict(scratch=DT_DEV + 28), b'scratch overlaps the dt run array'), (dict(area_d=GT_DEV), b'area_d overlaps the gt run array'),
                     (dict(d=3), b'dt mask 1: its starts end at word 5 of 4'), (dict(h=3, w=3), b'dt mask 0: the counts sum to 6, H * W is 9')):
        assert _call(L, ok, ok, **kw) == 2 and text in err() and b'deva_overlap_intersections' in err(), (kw, err())
    assert _call(L, ok, [0, 3, 5, 0, 4, 6, 0, 5]) == 2 and b'gt mask 1: the counts sum to 5' in err()
    assert _call(L, [0, 3, 5, 0, 4, 3, 0, 6], ok) == 2 and b'dt mask 0: count 1 is negative (-1)' in err()
    assert _call(L, ok, ok, d=0, dt_dev=None, scratch=None, inter=None, area_d=None, area_g=None) == 0           # O7: no work
    assert _call(L, ok, ok, g=0, gt_dev=None, scratch=None, inter=None, area_d=None, area_g=None) == 0
    bad = np.asarray([0, 3, 5, 0, 2, 6, 0, 7], dtype=np.int32)
    assert L.deva_overlap_check(bad.ctypes.data, 8, 2, 2, 3, ro.GT) == 2 and b'deva_overlap_check: gt mask 1: the counts sum to 7' in err()
    assert L.deva_overlap_check(bad.ctypes.data, 8, 2, 2, 3, 2) == 2 and b'side must be' in err()
    assert L.deva_overlap_limits(None) == 2 and b'null limits' in err()
    assert L.deva_overlap_plan(1, 1, 4, None) == 2 and b'null plan' in err()


def test_chunks_cover_every_pair_exactly_once():
    ro = _built()
    from deva.hip import rle
    rng = np.random.default_rng(5)
    for _ in range(100):
        per_d, per_g = rng.integers(1, 40, int(rng.integers(0, 30))), rng.integers(1, 40, int(rng.integers(0, 30)))
        max_masks, max_words = int(rng.integers(1, 12)), int(rng.integers(43, 200))
        blocks = ro.pair_chunks(per_d, per_g, max_masks, max_words)
        seen = np.zeros((per_d.size, per_g.size), dtype=np.int64)
        for (lo_d, hi_d), (lo_g, hi_g) in blocks:
            seen[lo_d:hi_d, lo_g:hi_g] += 1
            for per, lo, hi in ((per_d, lo_d, hi_d), (per_g, lo_g, hi_g)):
                assert 1 <= hi - lo <= max_masks and 2 * (hi - lo) + 1 + int(per[lo:hi].sum()) <= max_words
        assert (seen == 1).all()
        assert [b[0] for b in blocks] == [pd for pd in rle.chunks(per_d, max_masks, max_words) for _ in rle.chunks(per_g, max_masks, max_words)]
    assert ro.pair_chunks(np.zeros(0, dtype=np.int64), np.array([3]), 4, 100) == []


# ------------------------------------------------------------------------------------------ O-rules and iou by hand
def test_o_rules_by_hand_on_a_2x2_and_a_1x9_mask(monkeypatch):
    ro = _built()
    EO.install(monkeypatch)
    # 2 x 2, positions p = x * 2 + y: 0 = (0,0), 1 = (1,0), 2 = (0,1), 3 = (1,1)
    dt = [[1, 2, 1], [0, 0, 0, 4, 0, 0], [4]]                  # ones at {1, 2}; everywhere (zero counts first, inside, last); nowhere
    gt = [[0, 2, 2], [4], [0, 4], [1, 2, 1], [3, 1, 0]]        # {0, 1}; none; all; {1, 2} again; {3}
    want = (np.array([[1, 0, 2, 2, 0], [2, 0, 4, 2, 1], [0, 0, 0, 0, 0]]), np.array([2, 4, 0]), np.array([2, 0, 4, 2, 1]))
    for got in (OC.statement(dt, gt, 2, 2), OC.statement(dt, gt, 2, 2, direct=False)):
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    got = ro.intersections(OC.as_rles(dt, 2, 2), OC.as_rles(gt, 2, 2), device='cpu')
    assert all(t.dtype == torch.int32 and np.array_equal(t.numpy(), b) for t, b in zip(got, want))
    assert OC.boxes_of(dt, 2, 2).tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [-1, -1, -1, -1]]
    from deva.hip import rle
    for side, h, w in ((dt, 2, 2), (gt, 2, 2), ([[4], [1, 1, 2], [4], [4]], 2, 2), ([[9], [9]], 1, 9), ([[0, 9]], 9, 1)):   # empty masks first, between, last
        parsed = rle.parse_checked([list(c) for c in side], (h, w))
        boxes, areas = ro.boxes_and_areas(rle.run_array(parsed, 0, len(side)), len(side), h)
        assert boxes.tolist() == OC.boxes_of(side, h, w).tolist() and areas.tolist() == OC.statement(side, [], h, w)[1].tolist()
    # 1 x 9: a row, the scan runs along it
    dt9, gt9 = [[2, 3, 4]], [[4, 5], [0, 3, 0, 0, 6], [5, 4]]  # ones at 2..4 against 4..8, 0..2, 5..8: one pixel, one pixel, touching but apart
    want9 = (np.array([[1, 1, 0]]), np.array([3]), np.array([5, 3, 4]))
    assert all(np.array_equal(a, b) for a, b in zip(OC.statement(dt9, gt9, 1, 9), want9))
    got = ro.intersections([c for c in dt9], [c for c in gt9], source_size=(1, 9), device='cpu', pending=True).finish()
    assert all(a.dtype == np.int64 and np.array_equal(a, b) for a, b in zip(got, want9))
    # O7: an empty side launches nothing and the other side's areas are still there
    monkeypatch.setattr(ro, '_launch', lambda *a: pytest.fail('a launch was reached'))
    inter, area_d, area_g = ro.intersections([], OC.as_rles(gt, 2, 2), device='cpu')
    assert tuple(inter.shape) == (0, 5) and area_d.numel() == 0 and area_g.tolist() == [2, 0, 4, 2, 1]
    inter, area_d, area_g = ro.intersections(OC.as_rles(dt, 2, 2), [], device='cpu')
    assert tuple(inter.shape) == (3, 0) and area_d.tolist() == [2, 4, 0] and area_g.numel() == 0
    assert tuple(ro.intersections([], [], device='cpu')[0].shape) == (0, 0)


def test_iou_with_crowd_flags_and_empty_masks_by_hand(monkeypatch):
    ro = _built()
    EO.install(monkeypatch)
    dt = [[2, 3, 4], [9], [0, 9]]                              # ones at 2..4; empty; full
    gt = [[4, 5], [9], [0, 3, 6]]                              # ones at 4..8; empty; 0..2
    rles_d, rles_g = [{'size': [1, 9], 'counts': c} for c in dt], [{'size': [1, 9], 'counts': c} for c in gt]
    plain = ro.iou(rles_d, rles_g, device='cpu')
    assert plain.dtype == np.float64 and plain.shape == (3, 3)
    assert plain.tolist() == [[1 / 7, 0.0, 1 / 5], [0.0, 0.0, 0.0], [5 / 9, 0.0, 3 / 9]]      # two empty masks: 0, not NaN
    crowd = ro.iou(rles_d, rles_g, [1, 0, 1], device='cpu')
    assert crowd.tolist() == [[1 / 3, 0.0, 1 / 3], [0.0, 0.0, 0.0], [5 / 9, 0.0, 3 / 9]]      # inter / a_d where the gt is a crowd
    inter, a_d, a_g = OC.statement(dt, gt, 1, 9)
    assert np.array_equal(OC.iou(inter, a_d, a_g), plain) and np.array_equal(OC.iou(inter, a_d, a_g, [1, 0, 1]), crowd)
    assert ro.iou([], rles_g, device='cpu').shape == (0, 3) and ro.iou(rles_d, [], device='cpu').shape == (3, 0)


@pytest.mark.parametrize('size', OC.GEOMETRIES[:5], ids=lambda s: f'{s[0]}x{s[1]}')
def test_the_bindings_host_half_behind_the_statement(size, monkeypatch):
    """parsing, run arrays, boxes and chunked calls of the binding, with the library call replaced by the statement: the
    single call and the call with limits forced small give the statement's tables"""
    ro = _built()
    from deva.hip import rle
    EO.install(monkeypatch)
    h, w = size
    dt, gt = OC.geometry_case(h, w)
    want = OC.statement(dt, gt, h, w)
    rles_d, rles_g = OC.as_rles(dt, h, w), OC.as_rles(gt, h, w)
    most = max(len(c) for c in dt + gt)
    for kw in ({}, dict(max_masks=3), dict(max_words=most + 3), dict(max_masks=4, max_words=2 * most + 5)):
        got = ro.intersections(rles_d, rles_g, device='cpu', **kw)
        assert all(np.array_equal(t.numpy(), b) for t, b in zip(got, want)), kw
    parsed = rle.parse_checked(rles_g, (h, w))
    boxes, areas = ro.boxes_and_areas(rle.run_array(parsed, 0, len(gt)), len(gt), h)             # the boxes the binding sends are the planes'
    assert np.array_equal(boxes, OC.boxes_of(gt, h, w)) and np.array_equal(areas, want[2])
    assert np.array_equal(boxes, rle.records(rles_g).bbox) and np.array_equal(areas, rle.records(rles_g).area)
    assert np.array_equal(ro.iou(rles_d, rles_g, device='cpu'), OC.iou(*want))
    launches = []
    monkeypatch.setattr(ro, '_launch', lambda dt_, gt_, *a: launches.append((dt_.n, gt_.n)))
    ro.intersections(rles_d, rles_g, device='cpu', max_masks=3)
    assert sum(a * b for a, b in launches) == len(dt) * len(gt) and len(launches) == -(-len(dt) // 3) * -(-len(gt) // 3)


def test_the_run_array_the_binding_sends_reads_back_as_its_counts(monkeypatch):
    ro = _built()
    seen = []
    monkeypatch.setattr(ro, '_launch', lambda dt, gt, *a: seen.append((dt, gt)))
    dt, gt = OC.geometry_case(9, 1)
    ro.intersections(OC.as_rles(dt, 9, 1), OC.as_rles(gt, 9, 1), device='cpu')
    (side_d, side_g), = seen
    assert EO.counts_of_side(side_d) == dt and EO.counts_of_side(side_g) == gt
    assert side_d.host.numpy()[side_d.words:].reshape(-1, 4).tolist() == OC.boxes_of(dt, 9, 1).tolist()
    assert side_d.host.numel() == side_d.words + 4 * len(dt) and side_d.words == 2 * len(dt) + 1 + sum(len(c) for c in dt)


# ------------------------------------------------------------------------------------------ the sanitizers
def test_plan_code_under_host_sanitizers(tmp_path):
    """csrc/rle_overlap/rle_overlap_plan.cpp and the walk of csrc/rle_overlap/overlap_walk.h in a stand-alone program with
    its own main (tests/rle_overlap_plan_sanitize_main.cpp); nothing is loaded into Python and no GPU is involved"""
    exe = tmp_path / 'rle_overlap_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', OVERLAP_SRC, os.path.join(OVERLAP_SRC, 'rle_overlap_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'rle_overlap_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 30000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
SOURCES = sorted(f for f in os.listdir(OVERLAP_SRC) if f.endswith('.hip')) if os.path.isdir(OVERLAP_SRC) else []
KERNELS = {'overlap_scan_kernel': (16, 8), 'overlap_pair_kernel': (16384, 7)}    # name -> (LDS bytes at most, waves a SIMD at least)


def test_the_listing_is_not_empty():
    assert SOURCES == ['rle_overlap.hip']
    assert sorted(f for f in os.listdir(OVERLAP_SRC) if f.endswith('.cpp')) == ['rle_overlap_plan.cpp']
    for name in ('rle_overlap_plan.cpp', 'rle_overlap_plan.h', 'overlap_walk.h'):
        text = open(os.path.join(OVERLAP_SRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name        # the plan and the walk are host code too
    make = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'OVERLAP_OUT := ../deva/hip/libdeva_rle_overlap.so' in make and '$(eval $(call LIBRARY,OVERLAP_OUT,rle_overlap/))' in make
    assert re.search(r'^clean:\n\trm -f .*\$\(OVERLAP_OUT\)', make, flags=re.M) and re.search(r'^all: .*\$\(OVERLAP_OUT\)', make, flags=re.M)
    kernel = open(os.path.join(OVERLAP_SRC, 'rle_overlap.hip')).read()
    assert kernel.count('hipLaunchKernelGGL') == 2                           # two launches
    for word in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFree'):
        assert word not in kernel, word                                      # nothing allocated, copied or synchronised


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    kernels = abi_util.kernel_resources(os.path.join(OVERLAP_SRC, src))
    assert len(kernels) == len(KERNELS)
    for name, r in kernels.items():
        bound = [v for k, v in KERNELS.items() if k in name]
        assert len(bound) == 1, name
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0 and r.get('SGPRs Spill', 0) == 0, (name, r)
        assert r.get('LDS Size', 0) <= bound[0][0], (name, r)
        assert r['Occupancy'] >= bound[0][1], (name, r)
