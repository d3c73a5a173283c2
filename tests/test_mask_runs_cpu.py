"""The run-length encoder without a GPU: libdeva_mask_runs.so on its ABI, the argument errors before any launch, the plan's
host code under the host sanitizers, the kernels' static resources, the wrapper's chunks, rules E3 and E4 by hand, the numpy
statement (tests/runs_case.py) against the per-pixel encoder of tests/emu_frame_result.py, where the scans take a second
step, and the recorder's file read back."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_util
import emu_frame_result as EF
import emu_runs as ER
import rle_case as LC
import runs_case as RC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_mask_runs.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
RUNS_SRC = os.path.join(CSRC, 'mask_runs')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_runs_count', 'deva_runs_last_error', 'deva_runs_limits', 'deva_runs_plan', 'deva_runs_scratch', 'deva_runs_version',
        'deva_runs_write']


def _built():
    from deva.hip import mask_runs
    return abi_util.built(mask_runs)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    mr = _built()
    exported, _ = abi_util.exported(mr.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(mr.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_RUNS_ABI_VERSION 1\b', header)
    assert mr.ABI_VERSION == 1 and mr.lib().deva_runs_version() == 1
    for name, value in (('TILE', mr.TILE), ('MAX_MASKS', mr.MAX_MASKS), ('MAX_SCRATCH', mr.MAX_SCRATCH), ('SCAN_CHUNK', mr.SCAN_CHUNK),
                        ('MASK_CHUNK', mr.MASK_CHUNK), ('U8', mr.DTYPES[torch.uint8]), ('F32', mr.DTYPES[torch.float32])):
        assert re.search(rf'#define DEVA_RUNS_{name} {value}\b', header), name
    for rule in ('E1', 'E2', 'E3', 'E4', 'E5', 'E6', 'E7'):
        assert re.search(rf'^ \*   {rule}  ', header, flags=re.M), rule
    assert mr.runs_limits() == mr.LimitInfo(mr.MAX_MASKS, mr.TILE, 256, mr.SCAN_CHUNK, mr.MASK_CHUNK, 0, mr.MAX_SCRATCH)
    from deva.hip import rle
    assert rle.encode is mr.encode and rle.encode_labels is mr.encode_labels          # re-exports only
    assert not any('runs' in name for name in rle.SIGNATURES)


def test_no_symbol_is_shared_and_the_other_libraries_have_not_moved():
    from deva import hip
    from deva.hip import metrics, pair_metrics, regions, rle, vos_metrics
    mr = _built()
    exported, mine = abi_util.exported(mr.LIB_PATH)
    assert all(name.startswith('deva_runs_') for name in exported)
    for other in (hip.LIB_PATH, metrics.LIB_PATH, vos_metrics.LIB_PATH, pair_metrics.LIB_PATH, regions.LIB_PATH, rle.LIB_PATH):
        theirs_exported, theirs = abi_util.exported(other)
        assert not any(n.startswith('deva_runs') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other, shared)
    for name in ('deva_hip.h', 'deva_metrics.h', 'deva_vos_metrics.h', 'deva_pair_metrics.h', 'deva_regions.h', 'deva_rle.h'):
        assert 'deva_runs' not in open(os.path.join(ROOT, 'include', name)).read(), name
    abi_util.inference_entry_points([])       # libdeva_hip.so stays at its ABI version
    assert rle.ABI_VERSION == 1 and rle.lib().deva_rle_version() == 1 and len(rle.SIGNATURES) == 6


def test_struct_mirrors_have_the_c_layout(tmp_path):
    mr = _built()
    assert [f[0] for f in mr.Plan._fields_] == list(mr.PlanInfo._fields) and [f[0] for f in mr.Limits._fields_] == list(mr.LimitInfo._fields)
    lines = []
    for tag, mirror in (('deva_runs_plan', mr.Plan), ('deva_runs_limits', mr.Limits)):
        lines.append(f'printf("%zu\\n", sizeof(struct {tag}));\n')
        lines += [f'printf("%zu\\n", offsetof(struct {tag}, {f[0]}));\n' for f in mirror._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_mask_runs.h"\nint main(void){\n' + ''.join(lines) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for mirror in (mr.Plan, mr.Limits):
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert vals == want


def test_plan_is_host_side():
    mr = _built()
    assert mr.runs_plan(3, (480, 854)) == mr.PlanInfo(14, 8, 854 * 8, 4, 1, 3 * 14 * 8, 3 * 27, 0, 3 * 854 * 8 * 12)
    p = mr.runs_plan(64, (1080, 1920))
    assert (p.tiles_x, p.tiles_y, p.segments, p.scan_chunks, p.scratch_bytes) == (30, 17, 1920 * 17, 16, 64 * 1920 * 17 * 12)
    assert p.scratch_bytes // 64 == 391680                        # about 392 KB a mask at 1080p
    assert mr.runs_plan(1, (1, 1)) == mr.PlanInfo(1, 1, 1, 1, 1, 1, 1, 0, 12)
    assert mr.runs_plan(0, (5, 5)).count_grid == 0 and mr.runs_scratch(0, (5, 5)) == 0
    assert mr.runs_plan(4096, (480, 854)).count_grid == 65536    # capped: the rest is a grid-stride loop
    for bad in ((0, 5), (5, -1), (46341, 46341)):                 # the last: 2^31 pixels and more
        with pytest.raises(mr.DevaHipError, match='bad height x width'):
            mr.runs_plan(1, bad)
        assert mr.runs_scratch(1, bad) == -1
    assert mr.runs_plan(1, (46340, 46341)).tiles_x == 725         # 2^31 - 47 045 pixels: the largest plane there is
    with pytest.raises(mr.DevaHipError, match='n: 0 to 65536 masks'):
        mr.runs_plan(65537, (4, 4))
    with pytest.raises(mr.DevaHipError, match='bytes of scratch, a call takes 1073741824'):
        mr.runs_plan(4096, (1080, 1920))
    assert mr.runs_scratch(4096, (1080, 1920)) == -1


def test_where_the_scans_take_a_second_step():
    """the shapes of tests/test_gpu_zb_mask_runs.py, derived from the plan (as tests/full_frame_shapes.py does for the
    frame kernels): the smallest plane with two steps of the per-mask scan, the smallest stack with two of the other"""
    mr = _built()
    h, w = RC.SCAN_GEOMETRY
    assert h * w == mr.SCAN_CHUNK + 1 and mr.runs_plan(1, (h, w)).scan_chunks == 2
    smaller = [(a, b) for a in range(1, 70) for b in range(1, h * w) if a * b < h * w and b * ((a + 63) // 64) > mr.SCAN_CHUNK]
    assert smaller == [] and mr.runs_plan(1, (1, w - 1)).scan_chunks == 1 and mr.runs_plan(1, (64, w - 1)).scan_chunks == 1
    assert RC.SCAN_MASKS == mr.MASK_CHUNK + 1
    assert mr.runs_plan(RC.SCAN_MASKS, RC.SCAN_MASKS_SIZE).mask_chunks == 2 and mr.runs_plan(RC.SCAN_MASKS - 1, RC.SCAN_MASKS_SIZE).mask_chunks == 1
    # the geometries of the table: 65 x 129 has 258 segments, two tile rows; 480 x 854 takes four scan steps
    assert mr.runs_plan(1, (65, 129)).segments == 258 and mr.runs_plan(1, (480, 854)).scan_chunks == 4
    assert RC.GEOMETRIES[:4] + RC.GEOMETRIES[4:7] + RC.GEOMETRIES[8:] == LC.GEOMETRIES and RC.GEOMETRIES[7] == (128, 144)


# ------------------------------------------------------------------------------------------ refusals before any launch
def test_wrapper_refusals_happen_before_any_launch(monkeypatch):
    mr = _built()
    monkeypatch.setattr(mr, '_launch_count', lambda *a: pytest.fail('a launch was reached'))
    monkeypatch.setattr(mr, '_launch_write', lambda *a: pytest.fail('a launch was reached'))
    ok = torch.zeros(2, 4, 5, dtype=torch.uint8)
    for fn in (mr.encode, mr.count):
        for dtype in (torch.int32, torch.int64, torch.float16, torch.float64, torch.int8):
            with pytest.raises(mr.DevaHipError, match='planes must be torch.uint8, torch.bool or torch.float32'):
                fn(ok.to(dtype))
        with pytest.raises(mr.DevaHipError, match='float32 planes need a `threshold`'):
            fn(ok.float())
        with pytest.raises(mr.DevaHipError, match='`threshold` is for float32 planes'):
            fn(ok, threshold=0.5)
        with pytest.raises(mr.DevaHipError, match=r'planes must be an \[N,H,W\] tensor'):
            fn(ok[0])
        with pytest.raises(mr.DevaHipError, match='bad height x width 0 x 5'):
            fn(ok[:, :0])
        with pytest.raises(mr.DevaHipError, match='bad height x width 46341 x 46341'):
            fn(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(1, 46341, 46341))
    with pytest.raises(mr.DevaHipError, match='form must be one of'):
        mr.encode(ok, form='text')
    with pytest.raises(mr.DevaHipError, match='capacity must not be negative'):
        mr.encode(ok, capacity=-1)
    for kw in (dict(max_masks=0), dict(max_scratch=11), dict(max_masks=mr.MAX_MASKS + 1), dict(max_scratch=mr.MAX_SCRATCH + 1)):
        with pytest.raises(mr.DevaHipError, match='limits of 1 to 65536 masks and 12 to 1073741824 bytes of scratch'):
            mr.encode(ok, **kw)
    with pytest.raises(mr.DevaHipError, match=r'one mask of 4 x 5 needs 60 bytes of scratch, above the limit of one call \(59\)'):
        mr.encode(ok, max_scratch=59)
    with pytest.raises(mr.DevaHipError, match='`first` must be an int64 tensor of one element'):
        mr.count(ok, first=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(mr.DevaHipError, match=r"out\['n'\] must be a contiguous torch.int32 \[2\]"):
        mr.count(ok, out={'n': torch.zeros(2, dtype=torch.int64)})
    with pytest.raises(mr.DevaHipError, match='above the limits of one call'):
        mr.count(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(4096, 1080, 1920))
    counted = mr.Counted(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), None,
                         torch.zeros(30, dtype=torch.int32), 4, 5)
    with pytest.raises(mr.DevaHipError, match='`bounds` must be a contiguous int32 vector'):
        mr.write(counted, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(mr.DevaHipError, match='capacity 5 is outside `bounds`'):
        mr.write(counted, torch.zeros(4, dtype=torch.int32), 5)
    for fn in (mr.encode_labels,):
        with pytest.raises(mr.DevaHipError, match='labels must be an int64, int32 or int16'):
            fn(torch.zeros(4, 5, dtype=torch.uint8), [1])
        with pytest.raises(mr.DevaHipError, match='the ids must be distinct'):
            fn(torch.zeros(4, 5, dtype=torch.int64), [1, 2, 1])


def test_host_tensors_are_refused_there_is_no_cpu_path():
    mr = _built()
    ok = torch.zeros(2, 4, 5, dtype=torch.uint8)
    with pytest.raises(mr.DevaHipError, match='planes must live on the HIP device'):
        mr.encode(ok)
    with pytest.raises(mr.DevaHipError, match='planes must live on the HIP device'):
        mr.encode(ok.float(), threshold=0.0, capacity=10)
    assert mr.encode(ok[:0]) == []


A = 1 << 40   # made-up device addresses: validation fails before anything is dereferenced or launched
PLANES, SCRATCH, N_OUT, BASE, TOTAL, STATS, BOUNDS = (A + (k << 30) for k in range(7))
H, W = 7, 5


def _count(L, planes=PLANES, dtype=0, n=2, h=H, w=W, scratch=SCRATCH, nbytes=None, n_out=N_OUT, base=BASE, total=TOTAL, first=None, stats=STATS):
    nbytes = 12 * n * w * ((h + 63) // 64) if nbytes is None else nbytes
    return L.deva_runs_count(planes, dtype, 0.0, n, h, w, scratch, nbytes, n_out, base, total, first, stats, None)


def _write(L, n=2, h=H, w=W, scratch=SCRATCH, nbytes=120, base=BASE, bounds=BOUNDS, capacity=10):
    return L.deva_runs_write(n, h, w, scratch, nbytes, base, bounds, capacity, None)


def test_library_refusals_before_any_launch():
    mr = _built()
    L = mr.lib()
    err = L.deva_runs_last_error
    for kw, text in ((dict(dtype=2), b'dtype must be'), (dict(n=-1), b'n: 0 to 65536 masks'), (dict(n=65537), b'n: 0 to 65536 masks'),
                     (dict(h=0), b'bad height x width 0 x 5'), (dict(h=46341, w=46341), b'bad height x width'),
                     (dict(n=4096, h=1080, w=1920), b'bytes of scratch, a call takes'), (dict(planes=None), b'planes: null or misaligned'),
                     (dict(planes=PLANES + 2, dtype=1), b'planes: null or misaligned'), (dict(scratch=None), b'scratch: null or not 4-byte aligned'),
                     (dict(scratch=SCRATCH + 2), b'scratch: null or not 4-byte aligned'),
                     (dict(nbytes=119), b'scratch_bytes: 119 given, deva_runs_scratch asks for 120'), (dict(n_out=None), b'n_out: null or misaligned'),
                     (dict(n_out=N_OUT + 2), b'n_out: null or misaligned'), (dict(base=None), b'base: null or misaligned'),
                     (dict(base=BASE + 4), b'base: null or misaligned'), (dict(total=None), b'total: null or misaligned'),
                     (dict(first=TOTAL), b'first: it must not be `total` itself'), (dict(first=BASE + 4), b'first: misaligned'),
                     (dict(stats=STATS + 1), b'stats: misaligned'), (dict(scratch=PLANES + 68), b'scratch overlaps the planes'),
                     (dict(total=BASE + 8), b'overlaps'), (dict(stats=N_OUT + 4), b'overlaps'), (dict(first=BASE), b'base overlaps first')):
        assert _count(L, **kw) == 2 and text in err() and b'deva_runs_count' in err(), (kw, err())
    assert _count(L, n=0, planes=None, scratch=None, n_out=None, base=None, total=None, stats=None) == 0   # no masks: no work
    for kw, text in ((dict(capacity=-1), b'capacity: negative'), (dict(bounds=None), b'bounds: null or misaligned'),
                     (dict(bounds=BOUNDS + 2), b'bounds: null or misaligned'), (dict(scratch=None), b'scratch: null'),
                     (dict(scratch=SCRATCH + 1), b'scratch: null or not 4-byte aligned'), (dict(nbytes=116), b'scratch_bytes: 116 given'),
                     (dict(base=None), b'base: null or misaligned'), (dict(w=0), b'bad height x width'),
                     (dict(bounds=SCRATCH + 116), b'bounds overlaps scratch'), (dict(bounds=BASE + 8), b'bounds overlaps base')):
        assert _write(L, **kw) == 2 and text in err() and b'deva_runs_write' in err(), (kw, err())
    assert _write(L, n=0, scratch=None, base=None, bounds=None, capacity=0) == 0
    assert L.deva_runs_limits(None) == 2 and b'null limits' in err()
    assert L.deva_runs_plan(1, 4, 4, None) == 2 and b'null plan' in err()


def test_chunks_stay_within_the_limits_and_cover_every_mask():
    mr = _built()
    rng = np.random.default_rng(3)
    for _ in range(200):
        n, h, w = int(rng.integers(1, 400)), int(rng.integers(1, 300)), int(rng.integers(1, 300))
        per_mask = mr.runs_scratch(1, (h, w))
        max_masks, max_scratch = int(rng.integers(1, 50)), per_mask * int(rng.integers(1, 20)) + int(rng.integers(0, 12))
        parts = mr.chunks(n, (h, w), max_masks, max_scratch)
        assert [lo for lo, _ in parts] == [0] + [hi for _, hi in parts[:-1]] and parts[-1][1] == n
        for lo, hi in parts:
            assert 1 <= hi - lo <= max_masks and 0 < mr.runs_scratch(hi - lo, (h, w)) <= max_scratch
            if hi < n and hi - lo < max_masks:               # greedy: one more mask did not fit
                assert mr.runs_scratch(hi - lo + 1, (h, w)) > max_scratch
    assert mr.chunks(0, (4, 4), 4, 100) == []
    top = mr.runs_limits()
    parts = mr.chunks(100, (1080, 1920), top.max_masks, top.max_scratch)          # the library takes every chunk of a large call
    assert len(parts) == 1 and mr.runs_scratch(100, (1080, 1920)) > 0
    parts = mr.chunks(5000, (1080, 1920), top.max_masks, top.max_scratch)
    assert len(parts) == 2 and all(mr.runs_scratch(hi - lo, (1080, 1920)) > 0 for lo, hi in parts)


# ------------------------------------------------------------------------------------------ E3, E4 by hand; the statement
def test_e3_and_e4_by_hand_on_the_2x2_row(monkeypatch):
    mr = _built()
    ER.install(monkeypatch)
    names, planes = RC.row_planes(2, 2)
    assert names == ['empty', 'full', 'corners', 'checkerboard', 'column-stripes', 'row-stripes', 'blobs-1', 'blobs-2', 'zero-counts']
    top = RC.INT32_MAX
    by_hand = {'empty': ([], [4], [0, top, top, -1, -1]), 'full': ([0], [0, 4], [4, 0, 0, 1, 1]), 'corners': ([0], [0, 4], [4, 0, 0, 1, 1]),
               'checkerboard': ([1, 2, 3], [1, 1, 1, 1], [2, 0, 1, 1, 1]),          # positions 1 and 3: (y, x) = (1, 0) and (1, 1)
               'column-stripes': ([2], [2, 2], [2, 1, 0, 1, 1]), 'row-stripes': ([1, 2, 3], [1, 1, 1, 1], [2, 0, 1, 1, 1]),
               'zero-counts': ([0, 2], [0, 2, 2], [2, 0, 0, 0, 1])}                  # the shortest counts of [0, 2, 0, 0, 2, 0]
    want = RC.statement(planes)
    got = mr.encode(torch.from_numpy(planes.copy()), form='counts', stats=True)
    for name, (bounds, counts, stats) in by_hand.items():
        k = names.index(name)
        assert RC.bounds_of(planes[k]).tolist() == bounds and RC.counts_from(bounds, 2, 2) == counts, name
        assert want['stats'][k].tolist() == stats and int(want['n'][k]) == len(bounds), name
        assert got[k] == {'size': [2, 2], 'counts': counts, 'area': stats[0], 'bbox': stats[1:] if stats[0] else None}, name
    assert want['base'].tolist() == (np.cumsum(want['n']) - want['n']).tolist() and want['total'] == int(want['n'].sum())
    assert RC.statement(planes, first=9)['base'][0] == 9 and RC.statement(planes, first=9)['total'] == want['total'] + 9
    # E1 by hand
    values = np.array([[[np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45]]], dtype=np.float32)
    assert RC.pixels(values, 0.0).tolist() == [[[False, True, False, False, False, True, False]]]
    assert RC.pixels(values, -np.inf).tolist() == [[[False, True, False, True, True, True, True]]]
    assert RC.pixels(np.array([0, 1, 2, 255], dtype=np.uint8)).tolist() == [False, True, True, True]


def test_the_statement_equals_the_per_pixel_encoder(monkeypatch):
    """tests/runs_case.py against `coco_encode` / `coco_string` of tests/emu_frame_result.py (a per-pixel loop over the COCO
    API's algorithm) and against `rle_case.counts_of`, on every row; the binding's host arithmetic on the same rows"""
    mr = _built()
    ER.install(monkeypatch)
    for h, w in RC.GEOMETRIES[:-1]:
        names, planes = RC.row_planes(h, w)
        all_counts = LC.row(h, w)[1]
        _, bytes_ = RC.byte_stack(h, w)
        assert np.array_equal(bytes_ != 0, planes != 0) and {2, 255} <= set(np.unique(bytes_).tolist()) | ({2, 255} if h * w < 4 else set())
        texts = mr.encode(torch.from_numpy(bytes_))
        for k, name in enumerate(names):
            counts = RC.counts_from(RC.bounds_of(planes[k] != 0), h, w)
            assert counts == LC.counts_of(planes[k]) and 0 not in counts[1:], (h, w, name)
            if h * w <= 64 * 64:
                slow = EF.coco_encode(planes[k] != 0)
                assert slow['size'] == [h, w] and slow['counts'] == EF.coco_string(counts), (h, w, name)
            assert texts[k] == {'size': [h, w], 'counts': EF.coco_string(counts)}, (h, w, name)
            assert np.array_equal(LC.plane(counts, h, w), planes[k]), (h, w, name)
            if name == 'zero-counts':                             # the shortest counts, not the ones the row was written with
                assert counts != list(all_counts[k]) and len(counts) < len(all_counts[k])
        for threshold in RC.THRESHOLDS:
            _, logits = RC.float_stack(h, w, threshold)
            assert np.isnan(logits).any() or h * w < 4
            assert mr.encode(torch.from_numpy(logits), threshold=threshold) == texts
        assert mr.encode(torch.from_numpy(planes != 0), form='bytes') == [dict(t, counts=t['counts'].encode()) for t in texts]
    special = RC.float_stack(65, 129, 0.0)[1]
    assert np.isposinf(special).any() and np.isneginf(special).any() and (special == 0).any() and np.signbit(special[special == 0]).any()


# ------------------------------------------------------------------------------------------ the sanitizers
def test_plan_code_under_host_sanitizers(tmp_path):
    """csrc/mask_runs/mask_runs_plan.cpp in a stand-alone program with its own main
    (tests/mask_runs_plan_sanitize_main.cpp); nothing is loaded into Python and no GPU is involved"""
    exe = tmp_path / 'mask_runs_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', RUNS_SRC, os.path.join(RUNS_SRC, 'mask_runs_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'mask_runs_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 30000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
SOURCES = sorted(f for f in os.listdir(RUNS_SRC) if f.endswith('.hip')) if os.path.isdir(RUNS_SRC) else []
KERNELS = {'runs_count_kernelIh': 520, 'runs_count_kernelIf': 520, 'runs_stats_init_kernel': 0, 'runs_scan_kernel': 16, 'runs_base_kernel': 32,
           'runs_write_kernel': 0}


def test_the_listing_is_not_empty():
    assert SOURCES == ['mask_runs.hip']
    assert sorted(f for f in os.listdir(RUNS_SRC) if f.endswith('.cpp')) == ['mask_runs_plan.cpp']
    for name in ('mask_runs_plan.cpp', 'mask_runs_plan.h'):
        text = open(os.path.join(RUNS_SRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name        # the plan is host code
    make = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'RUNS_OUT := ../deva/hip/libdeva_mask_runs.so' in make and '$(eval $(call LIBRARY,RUNS_OUT,mask_runs/))' in make
    assert re.search(r'^clean:\n\trm -f .*\$\(RUNS_OUT\)', make, flags=re.M) and re.search(r'^all: .*\$\(RUNS_OUT\)', make, flags=re.M)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    kernels = abi_util.kernel_resources(os.path.join(RUNS_SRC, src))
    assert len(kernels) == len(KERNELS)
    for name, r in kernels.items():
        lds = [v for k, v in KERNELS.items() if k in name]
        assert len(lds) == 1, name
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0 and r.get('SGPRs Spill', 0) == 0, (name, r)
        assert r.get('LDS Size', 0) == lds[0], (name, r)
        assert r['Occupancy'] >= 8, (name, r)


# ------------------------------------------------------------------------------------------ the recorder
def _recorded_frames(monkeypatch):
    from deva.inference.detections import DetectionRecorder
    from deva.inference.object_info import ObjectInfo
    ER.install(monkeypatch)
    EF.install(monkeypatch)
    labels, ids = RC.disjoint(33, 67)
    infos = [ObjectInfo(i, category_id=(None if k == 1 else 10 + k), score=float(np.float32(0.3 + 0.1 * k))) for k, i in enumerate(ids)]
    recorder = DetectionRecorder()
    recorder.add('00000.jpg', torch.from_numpy(labels), infos)
    recorder.add('00001.jpg', torch.zeros(33, 67, dtype=torch.int64), [])                  # nothing detected: nothing written
    recorder.add('00002.jpg', torch.from_numpy(labels.T.copy()), infos[:2])
    planes = RC.many_small(4, 33, 67)
    recorder.add_planes('00003.jpg', torch.from_numpy(planes), [0.9, 0.8, 0.7, 0.6], category_ids=[1, None, 3, 4])
    return recorder, labels, ids, infos, planes


def test_the_recorders_file_is_read_back_by_coco_results(tmp_path, monkeypatch):
    from deva.inference.detections import CocoResults
    recorder, labels, ids, infos, planes = _recorded_frames(monkeypatch)
    with pytest.raises(ValueError, match='no path was given'):
        recorder.write()
    path = recorder.write(str(tmp_path / 'detections.json'))
    entries = json.load(open(path))
    assert entries == recorder.annotations and len(entries) == len(ids) + 2 + 4
    results = CocoResults(path)
    assert results.image_ids() == ['00000.jpg', '00002.jpg', '00003.jpg'] and '00001.jpg' not in results
    first = results.annotations('00000.jpg')
    assert [a['id'] for a in first] == ids and [a['score'] for a in first] == [o.scores[0] for o in infos]
    assert [a.get('category_id') for a in first] == [10, None, 12, 13, 14] and 'category_id' not in first[1]
    for a, i in zip(first, ids):
        assert set(a) - {'category_id'} == {'image_id', 'id', 'score', 'segmentation'}
        assert a['segmentation'] == {'size': [33, 67], 'counts': EF.coco_string(LC.counts_of(labels == i))}
    assert first[-1]['segmentation']['counts'] == EF.coco_string([33 * 67])                  # the id that no pixel holds
    assert results.annotations('00002.jpg')[0]['segmentation']['size'] == [67, 33]
    raw = results.annotations('00003.jpg')
    assert [a['id'] for a in raw] == [1, 2, 3, 4] and [a.get('category_id') for a in raw] == [1, None, 3, 4]
    assert [a['segmentation'] for a in raw] == RC.records(planes)
    with pytest.raises(ValueError, match='4 planes, 3 scores'):
        recorder.add_planes('x', torch.from_numpy(planes), [0.1, 0.2, 0.3])


def test_policy_recorded_gives_the_recorded_pair_and_refuses_what_it_cannot_read(tmp_path, monkeypatch):
    import emu_rle
    from deva.inference import detections as D
    recorder, labels, ids, infos, planes = _recorded_frames(monkeypatch)
    emu_rle.install(monkeypatch)
    results = D.CocoResults(recorder.annotations)
    mask, objects = results.detections('00000.jpg', policy='recorded', device='cpu')
    assert mask.dtype == torch.int64 and np.array_equal(mask.numpy(), labels)
    assert [(o.id, o.category_ids, o.scores) for o in objects] == [(o.id, o.category_ids, o.scores) for o in infos]
    mask, objects = results.detections('00001.jpg', (33, 67), policy='recorded', device='cpu')        # a frame the file does not mention
    assert tuple(mask.shape) == (33, 67) and not mask.any() and objects == []
    with pytest.raises(ValueError, match='no `size`'):
        results.detections('00001.jpg', policy='recorded')
    broken = [dict(a) for a in recorder.annotations[:3]]
    del broken[2]['id']
    with pytest.raises(ValueError, match=r"entry 2 carries no 'id'"):
        D.rle_detections(broken, policy='recorded', device='cpu')
    with pytest.raises(ValueError, match='policy must be one of'):
        D.rle_detections(broken, policy='replayed')
    assert D._RLE_POLICIES == ('text', 'large', 'small', 'recorded')


def test_recorded_processor_has_no_keys_of_its_own():
    from deva.inference.automatic import FrameLoop, RecordedProcessor

    class Core:
        config = {'temporal_setting': 'online', 'num_voting_frames': 3}
    processor = RecordedProcessor(Core(), results=object(), incorporate_keywords={'incremental': True})
    assert isinstance(processor, FrameLoop) and RecordedProcessor.config_keys == () and processor.recorder is None
    assert processor.incorporate_keywords == {'incremental': True} and RecordedProcessor(Core(), None).incorporate_keywords == {}
    assert FrameLoop(Core()).recorder is None and FrameLoop.incorporate_keywords == {}
