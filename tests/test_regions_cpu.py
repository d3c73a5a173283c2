"""The region library without a GPU: libdeva_regions.so on its ABI, its argument errors and its launch plan; the plan's host
code and the kernels' merging loop under the host sanitizers; the kernels' static resources; the numpy statement of the
rules (tests/region_case.py) against scipy where that is installed, on hand cases with known answers, and the coverage of
the planes the GPU test runs on."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_util
import region_case as RC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_regions.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
REGION_SRC = os.path.join(CSRC, 'regions')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_regions_clean', 'deva_regions_label', 'deva_regions_last_error', 'deva_regions_plan', 'deva_regions_scratch_bytes',
        'deva_regions_version']


def _built():
    from deva.hip import regions
    return abi_util.built(regions)


def _parse(text):
    return np.array([[int(c) for c in row] for row in text.split('/')], dtype=np.uint8)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    rg = _built()
    exported, _ = abi_util.exported(rg.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(rg.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_REGIONS_ABI_VERSION 1\b', header)
    assert rg.ABI_VERSION == 1 and rg.lib().deva_regions_version() == 1
    for name, value in (('TILE', rg.TILE), ('FIELDS', rg.FIELDS), ('MAX_PLANES', rg.MAX_PLANES)):
        assert re.search(rf'#define DEVA_REGIONS_{name} {value}\b', header), name
    for rule in ('R1', 'R2', 'R3', 'R4', 'R5', 'R6', 'R7'):
        assert re.search(rf'^ \*   {rule}  ', header, flags=re.M), rule
    assert rg.region_plan(29, 53, 1).tile == rg.TILE         # what the GPU test reads its geometry from


def test_no_symbol_is_shared_and_no_other_header_declares_the_entry_points():
    from deva import hip
    from deva.hip import metrics, pair_metrics, vos_metrics
    rg = _built()
    exported, mine = abi_util.exported(rg.LIB_PATH)
    assert all(name.startswith('deva_regions_') for name in exported)
    for other in (hip.LIB_PATH, metrics.LIB_PATH, vos_metrics.LIB_PATH, pair_metrics.LIB_PATH):
        theirs_exported, theirs = abi_util.exported(other)
        assert not any(n.startswith('deva_regions') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other, shared)
    for name in ('deva_hip.h', 'deva_metrics.h', 'deva_vos_metrics.h', 'deva_pair_metrics.h'):
        assert 'deva_regions' not in open(os.path.join(ROOT, 'include', name)).read(), name


def test_plan_mirror_has_the_c_layout(tmp_path):
    rg = _built()
    fields = [f[0] for f in rg.Plan._fields_]
    assert fields == list(rg.PlanInfo._fields)
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_regions.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(struct deva_regions_plan));\n' +
                   ''.join(f'printf("%zu\\n", offsetof(struct deva_regions_plan, {f}));\n' for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(rg.Plan) and vals[1:] == [getattr(rg.Plan, f).offset for f in fields]


# ------------------------------------------------------------------------------------------ refusals
A = 1 << 40   # made-up addresses: validation fails before anything is dereferenced or launched
PLANES, OUT, SCRATCH = (A + (k << 34) for k in (0, 1, 2))
N, H, W = 5, 29, 53


def _clean(L, planes=PLANES, n=N, h=H, w=W, min_area=12, records=OUT, scratch=SCRATCH, scratch_bytes=1 << 30):
    return L.deva_regions_clean(planes, n, h, w, min_area, records, scratch, scratch_bytes, None)


def _label(L, planes=PLANES, n=N, h=H, w=W, of_zeros=0, labels=OUT):
    return L.deva_regions_label(planes, n, h, w, of_zeros, labels, None, 0, None)


def test_argument_errors_before_any_launch():
    rg = _built()
    L = rg.lib()
    err = L.deva_regions_last_error
    one = rg.region_scratch_bytes(H, W)
    assert one == 2 * ((4 * H * W + 255) // 256 * 256) + 256 == 13056
    for call, name in ((_clean, b'deva_regions_clean'), (_label, b'deva_regions_label')):
        for kw in (dict(h=0), dict(w=-3), dict(h=32769, w=32768)):        # the last: above 2^30 pixels
            assert call(L, **kw) == 2 and b'bad plane size' in err() and name in err(), kw
        for n in (-1, 65537):
            assert call(L, n=n) == 2 and b'0 to 65536 planes' in err()
        assert call(L, planes=None) == 2 and b'null planes' in err()
    for min_area in (0, -1, -2**31):
        assert _clean(L, min_area=min_area) == 2 and b'min_area must be positive' in err()                  # R6
    assert _clean(L, records=None) == 2 and b'null or misaligned records' in err()
    assert _clean(L, records=OUT + 2) == 2 and b'null or misaligned records' in err()
    assert _clean(L, scratch=None) == 2 and b'null or misaligned scratch' in err()
    assert _clean(L, scratch=SCRATCH + 8) == 2 and b'null or misaligned scratch' in err()
    for short in (one - 1, 0, -5):
        assert _clean(L, scratch_bytes=short) == 2 and b'%d are needed for one plane' % one in err(), short
    assert _label(L, labels=None) == 2 and b'null or misaligned labels' in err()
    assert _label(L, labels=OUT + 2) == 2 and b'null or misaligned labels' in err()
    # an output over the planes' last byte or the scratch's (the part a call with this budget uses), the scratch over the planes
    assert _clean(L, records=PLANES + N * H * W - 1 & ~3) == 2 and b'records overlaps an input' in err()
    assert _clean(L, planes=OUT + 4 * 8 * N - 1) == 2 and b'records overlaps an input' in err()
    assert _clean(L, records=SCRATCH + 2 * one - 4, scratch_bytes=2 * one) == 2 and b'records overlaps an input' in err()
    assert _clean(L, scratch=PLANES + 16 * 100) == 2 and b'scratch overlaps an input' in err()
    assert _label(L, labels=PLANES + 4 * 100) == 2 and b'labels overlaps an input' in err()
    assert _label(L, planes=OUT + 4 * N * H * W - 1) == 2 and b'labels overlaps an input' in err()
    plan, nbytes = rg.Plan(), ctypes.c_int64()
    assert L.deva_regions_plan(H, W, N, one, None) == 2 and b'deva_regions_plan: null plan' in err()
    assert L.deva_regions_plan(H, W, N, one - 1, ctypes.byref(plan)) == 2 and b'%d are needed for one plane' % one in err()
    assert L.deva_regions_plan(H, W, N, -1, ctypes.byref(plan)) == 2 and b'budget' in err()
    assert L.deva_regions_plan(0, W, N, one, ctypes.byref(plan)) == 2 and b'bad plane size' in err()
    assert L.deva_regions_scratch_bytes(H, W, 1, None) == 2 and b'null bytes' in err()
    assert L.deva_regions_scratch_bytes(H, -1, 1, ctypes.byref(nbytes)) == 2 and b'bad plane size' in err()
    # R6: no planes is no work, whatever the pointers
    assert _clean(L, n=0, planes=None, records=None, scratch=None, scratch_bytes=0) == 0
    assert _label(L, n=0, planes=None, labels=None) == 0


def test_wrapper_errors_before_any_launch():
    from deva.hip import DevaHipError
    rg = _built()
    planes = torch.zeros(3, 4, 6, dtype=torch.uint8)
    with pytest.raises(DevaHipError, match=r'planes must be uint8 \[K,H,W\] or \[H,W\]'):
        rg.remove_small_regions(planes.float(), 5)
    with pytest.raises(DevaHipError, match=r'planes must be uint8 \[K,H,W\] or \[H,W\]'):
        rg.label_components(planes[0, 0])
    with pytest.raises(DevaHipError, match='planes must be a tensor'):
        rg.remove_small_regions(planes.numpy(), 5)
    with pytest.raises(DevaHipError, match='bad plane size 0 x 6'):
        rg.remove_small_regions(planes[:, :0], 5)
    for bad in (0, -2, 2.5, True, 2**31):
        with pytest.raises(DevaHipError, match='min_area must be positive'):
            rg.remove_small_regions(planes, bad)
    with pytest.raises(DevaHipError, match=r'`records` must be int32 \[3, 8\]'):
        rg.remove_small_regions(planes, 5, records=torch.zeros(3, 7, dtype=torch.int32))
    with pytest.raises(DevaHipError, match=r'`records` must be int32 \[8\]'):
        rg.remove_small_regions(planes[0], 5, records=torch.zeros(1, 8, dtype=torch.int32))
    need = rg.region_scratch_bytes(4, 6)
    with pytest.raises(DevaHipError, match=rf'`scratch` must be uint8 \[{need}\] or longer'):
        rg.remove_small_regions(planes, 5, scratch=torch.zeros(need - 1, dtype=torch.uint8))
    with pytest.raises(DevaHipError, match=r'`out` must be int32 \[3, 4, 6\]'):
        rg.label_components(planes, out=torch.zeros(3, 4, 6, dtype=torch.int64))
    with pytest.raises(DevaHipError, match='HIP device'):
        rg.remove_small_regions(planes, 5)
    with pytest.raises(DevaHipError, match='HIP device'):
        rg.label_components(planes)


def test_filter_arguments():
    from deva.hip import DevaHipError
    from deva.inference.proposals import ProposalFilter
    flt = ProposalFilter(8, 12, capacity=4)
    assert flt.min_mask_region_area == 0 and flt.region_nms_thresh == flt.box_nms_thresh == 0.7 and flt.last_regions is None
    flt = ProposalFilter(8, 12, capacity=4, min_mask_region_area=25, box_nms_thresh=0.6)
    assert flt.min_mask_region_area == 25 and flt.region_nms_thresh == 0.6
    assert ProposalFilter(8, 12, capacity=4, min_mask_region_area=25, region_nms_thresh=0.5).region_nms_thresh == 0.5
    for bad in (-1, 2.5, True):
        with pytest.raises(DevaHipError, match='min_mask_region_area'):
            ProposalFilter(8, 12, capacity=4, min_mask_region_area=bad)
    with pytest.raises(TypeError):
        ProposalFilter(8, 12, 4, 0.88, 0.95, 1.0, 0.0, 0.7, None, 25)         # keyword-only


# ------------------------------------------------------------------------------------------ the plan
def test_plan_is_host_side_monotone_and_bounded_by_the_budget():
    rg = _built()
    one = rg.region_scratch_bytes(480, 854)
    assert one == 2 * 4 * 480 * 854 + 256 == 3279616                     # (4 H W is a multiple of 256 here)
    # 480 x 854: 15 x 27 tiles; seams: 26 x 480 + 14 x 854 = 24 436 pixels; 409 920 pixels, 1 602 chunks of 256
    assert rg.region_plan(480, 854, 3) == rg.PlanInfo(32, 256, 27, 15, 3, 1, 3 * 405, (3 * 24436 + 255) // 256, 3 * 1602, 0, one, 3 * one)
    assert rg.region_plan(1, 1, 1) == rg.PlanInfo(32, 256, 1, 1, 1, 1, 1, 0, 1, 0, 768, 768)
    assert rg.region_plan(32, 32, 1).border_grid == 0 and rg.region_plan(32, 33, 1).border_grid == 1
    assert rg.region_plan(29, 53, 0, 0)[4:] == (0, 0, 0, 0, 0, 0, 13056, 0)
    big = rg.region_plan(32768, 32768, 2)                                # capped: the rest is a grid-stride loop
    assert (big.local_grid, big.border_grid, big.pixel_grid, big.plane_bytes) == (65536, 65536, 65536, (1 << 33) + 256)
    sizes = [(1, 1), (8, 12), (96, 128), (480, 854), (1080, 1920), (2160, 3840)]
    plans = [rg.region_plan(h, w, 4) for h, w in sizes]
    for a, b in zip(plans, plans[1:]):        # monotone in the plane
        assert a.local_grid <= b.local_grid and a.border_grid <= b.border_grid and a.pixel_grid <= b.pixel_grid
        assert a.plane_bytes < b.plane_bytes and a.scratch_bytes < b.scratch_bytes
    counts = [rg.region_plan(96, 128, n) for n in (1, 2, 5, 64)]
    for a, b in zip(counts, counts[1:]):      # and in the planes
        assert a.local_grid < b.local_grid and a.pixel_grid < b.pixel_grid and a.scratch_bytes < b.scratch_bytes and a.plane_bytes == b.plane_bytes
    # the budget: passes x planes per pass >= n, the scratch used never above the budget; one plane's worth works, a byte less does not
    one = rg.region_scratch_bytes(96, 128)
    for n in (1, 2, 5, 7, 64):
        for budget in (one, one + 1, 2 * one, 3 * one - 1, 5 * one, 64 * one, 1 << 40):
            p = rg.region_plan(96, 128, n, budget)
            assert p.planes_per_pass == min(n, budget // one) and p.passes * p.planes_per_pass >= n > (p.passes - 1) * p.planes_per_pass
            assert p.scratch_bytes == p.planes_per_pass * one <= budget
        assert rg.region_plan(96, 128, n, one).passes == n
        with pytest.raises(rg.DevaHipError, match=f'holds {one - 1} bytes, {one} are needed for one plane'):
            rg.region_plan(96, 128, n, one - 1)
    assert rg.region_scratch_bytes(96, 128, 5) == 5 * one and rg.region_scratch_bytes(96, 128, 0) == 0
    with pytest.raises(rg.DevaHipError, match='bad plane size'):
        rg.region_plan(0, 5, 1)


def test_plan_and_union_code_under_host_sanitizers(tmp_path):
    """csrc/regions/region_plan.cpp and the merging loop of csrc/regions/region_union.h (on host threads) in a stand-alone
    program with its own main (tests/region_plan_sanitize_main.cpp); nothing is loaded into Python and no GPU is involved"""
    exe = tmp_path / 'region_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-pthread',
                    '-I', os.path.join(ROOT, 'include'), '-I', REGION_SRC, os.path.join(REGION_SRC, 'region_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'region_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 50000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
SOURCES = sorted(f for f in os.listdir(REGION_SRC) if f.endswith('.hip')) if os.path.isdir(REGION_SRC) else []


def test_the_listing_is_not_empty():
    assert SOURCES == ['regions.hip']
    assert sorted(f for f in os.listdir(REGION_SRC) if f.endswith('.cpp')) == ['region_plan.cpp']
    for name in ('region_plan.cpp', 'region_plan.h', 'region_union.h'):
        text = open(os.path.join(REGION_SRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name        # the plan and the union loop are host code too


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    kernels = abi_util.kernel_resources(os.path.join(REGION_SRC, src))
    for stage, count in (('init', 1), ('local', 1), ('border', 1), ('flatten', 2), ('decide', 1), ('rewrite', 1), ('record', 1)):
        assert sum(f'regions_{stage}_kernel' in name for name in kernels) == count, stage
    assert len(kernels) == 8
    for name, r in kernels.items():
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0 and r.get('SGPRs Spill', 0) == 0, (name, r)
        assert r.get('LDS Size', 0) <= 160 * 1024, (name, r)
        assert r['Occupancy'] >= 4, (name, r)


# ------------------------------------------------------------------------------------------ the statement against scipy
SHAPES = ((1, 9), (9, 1), (2, 2), (29, 53), (33, 67), (67, 33), (32, 32), (31, 31))


def _reference_helper(ndimage, mask, area_thresh, mode):
    """the ten lines of the helper the reference's generator calls (segment_anything.utils.amg.remove_small_regions, which
    the reference imports and does not carry), with scipy's labelling in the place of OpenCV's
    connectedComponentsWithStats(..., 8).  Among equal largest islands OpenCV's order is its algorithm's; scipy numbers
    components by their first pixel in row-major order (checked below), which is the rule R3 states."""
    correct_holes = mode == 'holes'
    working_mask = correct_holes ^ mask
    regions, n_labels = ndimage.label(working_mask, structure=np.ones((3, 3)))
    n_labels += 1
    sizes = np.bincount(regions.ravel(), minlength=n_labels)[1:]
    small_regions = [i + 1 for i, s in enumerate(sizes) if s < area_thresh]
    if len(small_regions) == 0:
        return mask, False
    fill_labels = [0] + small_regions
    if not correct_holes:
        fill_labels = [i for i in range(n_labels) if i not in fill_labels]
        if len(fill_labels) == 0:
            fill_labels = [int(np.argmax(sizes)) + 1]
    mask = np.isin(regions, fill_labels)
    return mask, True


def test_the_statement_against_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    for h, w in SHAPES:
        names, planes, min_area = RC.row(h, w)
        for name, plane in zip(names, planes):
            for of_zeros in (False, True):
                kind = (plane != 0) != of_zeros
                theirs, count = ndimage.label(kind, structure=np.ones((3, 3)))
                mine = RC.labels(kind)
                # scipy numbers components in row-major order of their first pixel
                firsts = [int(np.flatnonzero(theirs.ravel() == c)[0]) for c in range(1, count + 1)]
                assert firsts == sorted(firsts), (h, w, name)
                lut = np.array([0] + [f + 1 for f in firsts], dtype=np.int32)
                assert np.array_equal(mine, lut[theirs]), (h, w, name, of_zeros)
            for area in (1, 2, min_area, h * w, h * w + 1):
                mask, changed = _reference_helper(ndimage, plane.astype(bool), area, 'holes')
                mask, changed_too = _reference_helper(ndimage, mask, area, 'islands')
                out, record = RC.clean(plane, area)
                assert np.array_equal(out.astype(bool), mask) and record[0] == int(changed or changed_too), (h, w, name, area)


# ------------------------------------------------------------------------------------------ hand cases
def test_labels_of_small_planes_by_hand():
    plane = _parse('1100/0010/0001/1000')
    assert RC.labels(plane != 0).tolist() == [[1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [13, 0, 0, 0]]
    assert RC.labels(plane == 0).tolist() == [[0, 0, 3, 3], [3, 3, 0, 3], [3, 3, 3, 0], [0, 3, 3, 3]]     # one, through (0, 2)-(1, 1)
    # two bars closed diagonally at both ends: one mask component, and the inside is one with the outside through the corners
    bars = _parse('0111110/1000001/0111110')
    assert np.unique(RC.labels(bars != 0)).tolist() == [0, 2] and np.unique(RC.labels(bars == 0)).tolist() == [0, 1]
    board = RC.checkerboard(6, 7)
    assert np.unique(RC.labels(board != 0)).tolist() == [0, 1] and np.unique(RC.labels(board == 0)).tolist() == [0, 2]
    for name in ('serpentine', 'comb', 'spiral'):
        for h, w in ((33, 67), (67, 33), (9, 12)):
            assert len(np.unique(RC.labels(RC.PATTERNS[name](h, w) != 0))) == 2, (name, h, w)      # one chain, however it winds
    assert len(np.unique(RC.labels(RC.spiral(33, 67) == 0))) == 2                                       # and one between its arms
    for o in range(4):
        pair = RC.diag_touch(40, 40, (32, 32), o)
        assert pair.sum() == 17 and len(np.unique(RC.labels(pair != 0))) == 2 and len(np.unique(RC.labels(pair == 0))) == 2


def test_clean_of_small_planes_by_hand():
    ring = _parse('01110/10001/10001/10001/01110')               # corners touch only diagonally: it encloses nothing
    out, rec = RC.clean(ring, 100)
    assert out.all() and rec.tolist() == [1, 13, 0, 25, 0, 0, 4, 4]  # the one complement component (13 < 100) fills; 25 < 100 is all there is: kept
    assert RC.clean(ring, 13)[1].tolist() == [1, 0, 0, 12, 0, 0, 4, 4]      # 13 pixels stay unfilled; the ring's 12 are small, and kept
    assert RC.clean(ring, 12)[1].tolist() == [0, 0, 0, 12, 0, 0, 4, 4]
    closed = _parse('11111/10001/10001/10001/11111')
    assert RC.clean(closed, 10)[1].tolist() == [1, 9, 0, 25, 0, 0, 4, 4] and RC.clean(closed, 9)[1][0] == 0
    island = np.zeros((8, 9), dtype=np.uint8)
    island[3:5, 4:6] = 1
    out, rec = RC.clean(island, 10)                              # a lone small island is kept, and changed (R4)
    assert np.array_equal(out, island) and rec.tolist() == [1, 0, 0, 4, 4, 3, 5, 4]
    out, rec = RC.clean(RC.full_minus_corner(4, 5), 3)
    assert out.all() and rec.tolist() == [1, 1, 0, 20, 0, 0, 4, 3]
    for plane in (RC.empty(4, 5), RC.full(4, 5)):                # unchanged (R2): 20 pixels are not below 20
        out, rec = RC.clean(plane * 255, 20)
        assert np.array_equal(out, plane) and rec[:4].tolist() == [0, 0, 0, int(plane.sum())]
    assert RC.clean(RC.empty(4, 5), 21)[1].tolist() == [1, 20, 0, 20, 0, 0, 4, 3]     # a plane smaller than min_area is one small hole


def test_an_area_of_exactly_min_area_stays():
    for size, stays in ((6, True), (5, False)):
        plane = np.zeros((9, 14), dtype=np.uint8)
        plane[1:8, 1:8] = 1
        plane[3, 2:2 + size] = 0                                 # a hole
        out, rec = RC.clean(plane, 6)
        assert bool(out[3, 2] == 0) == stays and rec[:3].tolist() == [int(not stays), 0 if stays else size, 0]
        plane = np.zeros((9, 14), dtype=np.uint8)
        plane[1:8, 1:8] = 1
        plane[1, 9:9 + size // 2] = plane[2, 9:9 + size - size // 2] = 1     # an island
        out, rec = RC.clean(plane, 6)
        assert bool(out[1, 9] == 1) == stays and rec[:3].tolist() == [int(not stays), 0, 0 if stays else size]


def test_equal_largest_islands_the_row_major_first_stays():
    plane = np.zeros((9, 14), dtype=np.uint8)
    plane[1, 9:12] = 1          # first in row-major order, though it starts in a higher column
    plane[5, 1:4] = 1
    plane[7, 6:8] = 1
    out, rec = RC.clean(plane, 50)
    assert out[1, 9:12].all() and out.sum() == 3 and rec.tolist() == [1, 0, 5, 3, 9, 1, 11, 1]
    assert RC.kind_of(plane, 50) == 'keep-largest'
    plane[5, 4] = 1             # now the later one is the largest
    out, rec = RC.clean(plane, 50)
    assert out[5, 1:5].all() and out.sum() == 4 and rec.tolist() == [1, 0, 5, 4, 1, 5, 4, 5]
    # filling a hole can join islands, so R3 runs on the result of R2: two halves of 8 with a column of 3 holes between them
    halves = np.zeros((7, 12), dtype=np.uint8)
    halves[1:4, 2:7] = 1
    halves[1:4, 4] = 0
    halves[0, 2:7] = halves[4, 2:7] = 0
    out, rec = RC.clean(halves, 10)
    assert rec.tolist() == [1, 0, 6, 6, 2, 1, 3, 3]              # the column is open at both ends: two islands of 6, the first stays
    halves[0, 3:6] = halves[4, 3:6] = 1                          # closed: the column of 3 fills and the halves are one island of 21
    out, rec = RC.clean(halves, 10)
    assert rec.tolist() == [1, 3, 0, 21, 2, 0, 6, 4]


# ------------------------------------------------------------------------------------------ the GPU test's planes
def test_every_geometry_row_holds_every_outcome():
    """a condition on the generator, asked of the statement alone: unchanged, only-filled, only-removed, keep-largest and
    both passes acting occur in every row (2 x 2 holds one mask component at most under 8-connectivity, so nothing can
    be removed beside something kept there: three outcomes)"""
    for h, w in SHAPES:
        present = RC.check_row(h, w)
        assert present >= ({'unchanged', 'only-filled', 'keep-largest'} if (h, w) == (2, 2) else set(RC.KINDS)), (h, w)
        names, planes, min_area = RC.row(h, w)
        assert len(set(names)) == len(names) and set(RC.PATTERNS) <= set(names)
        if min(h, w) >= 8:
            assert sum(n.startswith('diag_touch') for n in names) % 4 == 0 and any(n.startswith('diag_touch') for n in names)
    # the pairs of the tiled rows sit on the tile corners
    assert any(n.startswith('diag_touch(32, 64)') for n in RC.row(33, 67)[0]) and any(n.startswith('diag_touch(64, 32)') for n in RC.row(67, 33)[0])
    # thresholded noise would not do: it is changed wherever one looks
    noise = np.random.default_rng(0).random((50, 29, 53)) < 0.5
    assert sum(RC.kind_of(p, 12) != 'unchanged' for p in noise) == 50

