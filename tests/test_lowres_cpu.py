"""The filter from low-resolution logits without a GPU: libdeva_lowres.so on its ABI, the plan by hand, the refusals of rule L7
before any launch, the plan's host code under the host sanitizers, the kernels' static resources, the statement
(tests/lowres_case.py) against ATen's chain on the CPU, and `ProposalFilter.add_lowres`, `lowres.select_masks` and both
processors on the CPU contract (tests/emu_lowres.py) against the full-resolution route on the statement's planes."""
import ctypes
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import abi_util
import emu_detections as ED
import emu_lowres as EL
import emu_ops
import emu_proposals as EP
import emu_text as ET
import lowres_case as LC
import prompt_case
import text_case as TC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_lowres.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
LOWRES_SRC = os.path.join(CSRC, 'lowres')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_lowres_last_error', 'deva_lowres_limits', 'deva_lowres_plan', 'deva_lowres_proposal_batch', 'deva_lowres_select',
        'deva_lowres_upsample', 'deva_lowres_version']
LOW, M, INPUT = (16, 16), 64, (36, 64)


def _built():
    from deva.hip import lowres
    return abi_util.built(lowres)


def _install(monkeypatch):
    emu_ops.install(monkeypatch)
    ED.install(monkeypatch)
    EP.install(monkeypatch)
    ET.install(monkeypatch)
    EL.install(monkeypatch)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    lr = _built()
    exported, _ = abi_util.exported(lr.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(lr.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_LOWRES_ABI_VERSION 1\b', header)
    assert lr.ABI_VERSION == 1 and lr.lib().deva_lowres_version() == 1
    for name, value in (('MAX_SIDE', lr.MAX_SIDE), ('MAX_PER_BOX', lr.MAX_PER_BOX), ('LDS_BUDGET', lr.LDS_BUDGET),
                        ('MAX_TILE_ROWS', lr.MAX_TILE_ROWS), ('PATH_TILE', lr.PATH_TILE), ('PATH_POINT', lr.PATH_POINT)):
        assert re.search(rf'#define DEVA_LOWRES_{name} {value}\b', header), name
    assert re.search(r'#define DEVA_LOWRES_MAX_PIXELS \(1 << 30\)', header) and lr.MAX_PIXELS == 1 << 30
    for rule in ('L1', 'L2', 'L3', 'L4', 'L5', 'L6', 'L7'):
        assert re.search(rf'^ \* {rule}\. ', header, flags=re.M), rule
    assert 'Not ATen bit for bit' in header and 'torchvision' in header
    assert lr.limits() == lr.LimitInfo(lr.MAX_SIDE, lr.MAX_PIXELS, lr.MAX_PER_BOX, 256, lr.LDS_BUDGET, lr.MAX_TILE_ROWS)
    from deva.hip import ops
    assert lr.MAX_PER_BOX == ops.BOX_MAX_PER_BOX
    assert os.path.basename(os.path.dirname(lr.LIB_PATH)) == 'lowres_lib'


def test_no_symbol_is_shared_and_the_other_libraries_have_not_moved():
    from deva import hip
    from deva.hip import mask_runs, metrics, pair_metrics, regions, rle, rle_overlap, rle_text, vos_metrics
    lr = _built()
    exported, mine = abi_util.exported(lr.LIB_PATH)
    assert all(name.startswith('deva_lowres_') for name in exported)
    others = (hip, metrics, vos_metrics, pair_metrics, regions, rle, mask_runs, rle_overlap, rle_text)
    for other in others:
        theirs_exported, theirs = abi_util.exported(abi_util.built(other).LIB_PATH)
        assert not any(n.startswith('deva_lowres') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other.LIB_PATH, shared)
    for name in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if name != 'deva_lowres.h':
            assert 'deva_lowres' not in open(os.path.join(ROOT, 'include', name)).read(), name
    abi_util.inference_entry_points([])       # libdeva_hip.so stays at its ABI version
    assert [m.ABI_VERSION for m in others[1:]] == [1] * 8


def test_struct_mirrors_have_the_c_layout(tmp_path):
    lr = _built()
    assert [f[0] for f in lr.Plan._fields_] == list(lr.PlanInfo._fields) and [f[0] for f in lr.Limits._fields_] == list(lr.LimitInfo._fields)
    mirrors = (('deva_lowres_plan', lr.Plan), ('deva_lowres_limits', lr.Limits), ('deva_lowres_geometry', lr.Geometry))
    lines = []
    for tag, mirror in mirrors:
        lines.append(f'printf("%zu\\n", sizeof(struct {tag}));\n')
        lines += [f'printf("%zu\\n", offsetof(struct {tag}, {f[0]}));\n' for f in mirror._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_lowres.h"\nint main(void){\n' + ''.join(lines) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, mirror in mirrors:
        want += [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    assert vals == want


# ------------------------------------------------------------------------------------------ the plan by hand
def test_plan_by_hand():
    """rows of the source that c destination rows touch at most: floor(c * n_in / n_out) + 4, capped at n_in; a band is the
    tallest of 16 .. 1 rows (at most 16384 pixels) whose patch fits 60 KB; tile path iff that patch holds at most 3 values
    of mid per output pixel of the band"""
    lr = _built()
    sam = dict(low_size=(256, 256), input_size=(576, 1024))
    # 1080p: 8 rows of 1920 (16384 // 1920), 9 covered: floor(9 * 576 / 1080) + 4 = 8 rows of mid, floor(8 / 4) + 4 = 6 of low
    assert lr.plan(size=(1080, 1920), **sam) == lr.PlanInfo(lr.PATH_TILE, 8, 1920, 9, 8, 6, 4 * (8 * 1024 + 6 * 256), 256, 135, 65535,
                                                            8 * 1024, 8 * 1920)
    # 480 x 854: 16 rows would cover 17 -> 24 rows of mid, 96 KB; 8 rows: 14 rows of mid + 7 of low = 63 KB; 7 rows: 13 + 7
    assert lr.plan(size=(480, 854), **sam) == lr.PlanInfo(lr.PATH_TILE, 7, 854, 8, 13, 7, 4 * (13 * 1024 + 7 * 256), 256, 69, 65535,
                                                          13 * 1024, 7 * 854)
    # 4K: 4 rows of 3840, 5 covered: floor(5 * 576 / 2160) + 4 = 5
    p = lr.plan(size=(2160, 3840), **sam)
    assert (p.path, p.tile_rows, p.mid_rows, p.low_rows, p.grid_x) == (lr.PATH_TILE, 4, 5, 5, 540)
    # the small geometry of the GPU tests: 16 rows of 70, 17 covered: floor(17 * 36 / 33) + 4 = 22; low: floor(22 / 4) + 4 = 9
    assert lr.plan(LOW, INPUT, (33, 70), model_size=M) == lr.PlanInfo(lr.PATH_TILE, 16, 70, 17, 22, 9, 4 * (22 * 64 + 9 * 16), 256, 3, 65535,
                                                                      22 * 64, 16 * 70)
    # strong minification: 5 rows of 9 touch all 36 rows of mid, 2304 values for 45 pixels -> point path, nothing in LDS
    assert lr.plan(LOW, INPUT, (5, 9), model_size=M) == lr.PlanInfo(lr.PATH_POINT, 5, 9, 5, 0, 0, 0, 256, 1, 65535, 4 * 45, 45)
    assert lr.plan(LOW, INPUT, (1, 9), model_size=M).path == lr.PATH_POINT
    # a 33 x 70 frame from SAM's own sizes: ratio 14 and more
    assert lr.plan((256, 256), lr.sam_input_size(33, 70), (33, 70)).path == lr.PATH_POINT
    # a plane one pixel wide: a 16-byte piece reaches 15 rows down
    p = lr.plan(LOW, (64, 1), (100, 1), model_size=M)
    assert (p.tile_rows, p.cover_rows) == (16, 31)
    assert lr.plan(LOW, INPUT, (1, 1 << 30), model_size=M).tile_rows == 1
    assert lr.sam_input_size(1080, 1920) == (576, 1024) and lr.sam_input_size(1920, 1080) == (1024, 576)
    assert lr.sam_input_size(480, 854) == (576, 1024) and lr.sam_input_size(33, 70, 64) == (30, 64)


# ------------------------------------------------------------------------------------------ L7: refusals before any launch
A = 1 << 40   # made-up device addresses: validation fails before anything is dereferenced or launched


def test_library_refusals_before_any_launch():
    lr = _built()
    L = lr.lib()
    err = L.deva_lowres_last_error
    geo = lambda **over: ctypes.byref(lr.Geometry(**dict(dict(low_h=16, low_w=16, model_size=64, in_h=36, in_w=64, out_h=33, out_w=70,
                                                               reserved=0), **over)))
    plan = lr.Plan()
    for over, text in ((dict(low_h=0), b'low-resolution planes of 1 to 4096'), (dict(low_w=4097), b'low-resolution planes of 1 to 4096'),
                       (dict(model_size=4097), b'a model_size of 1 to 4096'), (dict(in_h=65), b'within 1 .. model_size = 64'),
                       (dict(in_w=0), b'within 1 .. model_size = 64'), (dict(out_h=0), b'bad output size'),
                       (dict(out_h=32769, out_w=32768), b'bad output size'), (dict(reserved=1), b'reserved must be 0')):
        assert L.deva_lowres_plan(geo(**over), ctypes.byref(plan)) == 2 and text in err(), over
        assert L.deva_lowres_upsample(A, 1, geo(**over), A + 4096, None) == 2 and text in err(), over
        assert L.deva_lowres_select(A, A + 4096, 1, 3, geo(**over), 0.0, A + 8192, None, None) == 2 and text in err(), over
        assert L.deva_lowres_proposal_batch(A, A + 4096, 1, geo(**over), 0.88, 0.95, 1.0, 0.0, A + 8192, 8, A + (1 << 20), 1 << 30, None) == 2
        assert text in err(), over
    assert L.deva_lowres_plan(None, ctypes.byref(plan)) == 2 and b'null geometry' in err()
    assert L.deva_lowres_plan(geo(), None) == 2 and b'null plan' in err()
    assert L.deva_lowres_limits(None) == 2 and b'null limits' in err()
    assert L.deva_lowres_upsample(A, -1, geo(), A, None) == 2 and b'negative batch' in err()
    assert L.deva_lowres_upsample(None, 1, geo(), A, None) == 2 and b'null or misaligned low-resolution logits' in err()
    assert L.deva_lowres_upsample(A, 1, geo(), A + 2, None) == 2 and b'null or misaligned output' in err()
    assert L.deva_lowres_upsample(None, 0, geo(), None, None) == 0                      # nothing to do, nothing launched
    assert L.deva_lowres_select(A, A, 1, 0, geo(), 0.0, A, None, None) == 2 and b'1 to 16 planes per box (got 0)' in err()
    assert L.deva_lowres_select(A, A, 1, 17, geo(), 0.0, A, None, None) == 2 and b'1 to 16 planes per box (got 17)' in err()
    assert L.deva_lowres_select(A, None, 1, 3, geo(), 0.0, A, None, None) == 2 and b'null scores with 3 planes per box' in err()
    assert L.deva_lowres_select(A, A, 1, 3, geo(), float('nan'), A, None, None) == 2 and b'threshold is not a number' in err()
    assert L.deva_lowres_select(A, A, 1, 3, geo(), 0.0, None, None, None) == 2 and b'null output' in err()
    assert L.deva_lowres_select(A, A, 1 << 30, 2, geo(), 0.0, A, None, None) == 2 and b'at most 2^30 planes' in err()
    assert L.deva_lowres_select(None, None, 0, 3, geo(), 0.0, None, None, None) == 0
    batch = lambda **o: L.deva_lowres_proposal_batch(*[dict(dict(low=A, iou=A + 4096, b=1, g=geo(), t0=0.88, t1=0.95, t2=1.0, t3=0.0, arena=A + 8192,
                                                                 cap=8, scratch=A + (1 << 20), nbytes=1 << 30, stream=None), **o)[k]
                                                       for k in ('low', 'iou', 'b', 'g', 't0', 't1', 't2', 't3', 'arena', 'cap', 'scratch', 'nbytes', 'stream')])
    assert batch(b=-1) == 2 and b'negative batch' in err()
    assert batch(t1=float('nan')) == 2 and b'a threshold is not a number' in err()
    assert batch(cap=0) == 2 and b'a capacity of 1 to 4096 masks (got 0)' in err()
    assert batch(cap=4097) == 2 and b'a capacity of 1 to 4096' in err()
    assert batch(nbytes=100) == 2 and b'deva_proposal_scratch asks for' in err()
    assert batch(scratch=A + 8) == 2 and b'16-byte aligned' in err()
    assert batch(arena=None) == 2 and b'null arena' in err()
    assert batch(low=None) == 2 and b'null or misaligned low-resolution logits' in err()
    assert batch(iou=None) == 2 and b'null or misaligned predicted IoUs' in err()
    from deva import hip
    assert hip.lib().deva_proposal_scratch(8) <= 1 << 30                                # (what `nbytes` stands for above)


def test_wrapper_refusals_happen_before_any_launch(monkeypatch):
    lr = _built()
    for name in ('_launch_upsample', '_launch_select', '_launch_proposal_batch'):
        monkeypatch.setattr(lr, name, lambda *a: pytest.fail('a launch was reached'))
    low = torch.zeros(2, 16, 16)
    with pytest.raises(lr.DevaHipError, match=r'\[B,LH,LW\] logits expected'):
        lr.upsample_logits(low[0], INPUT, (33, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match='an input_size within 1 .. model_size = 64'):
        lr.upsample_logits(low, (65, 64), (33, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match='a model_size of 1 to 4096'):
        lr.upsample_logits(low, INPUT, (33, 70), model_size=4097)
    with pytest.raises(lr.DevaHipError, match='bad output size'):
        lr.upsample_logits(low, INPUT, (0, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match='bad output size'):
        lr.upsample_logits(low, INPUT, (32769, 32768), model_size=M)
    with pytest.raises(lr.DevaHipError, match='low-resolution planes of 1 to 4096'):
        lr.upsample_logits(torch.zeros(1, 1, 4097), INPUT, (33, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match='`out` must be fp32'):
        lr.upsample_logits(low, INPUT, (33, 70), model_size=M, out=torch.zeros(2, 33, 71))
    with pytest.raises(lr.DevaHipError, match='sizes are pairs of integers'):
        lr.upsample_logits(low, None, (33, 70), model_size=M)
    cand = torch.zeros(2, 3, 16, 16)
    with pytest.raises(lr.DevaHipError, match=r'\[B,M,LH,LW\] logits expected'):
        lr.select_masks(low, None, INPUT, (33, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match='1 to 16 planes per box'):
        lr.select_masks(torch.zeros(1, 17, 16, 16), torch.zeros(1, 17), INPUT, (33, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match='scores may be None only with one plane per box'):
        lr.select_masks(cand, None, INPUT, (33, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match=r'scores must be fp32 \[2,3\]'):
        lr.select_masks(cand, torch.zeros(2, 2), INPUT, (33, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match='threshold is not a number'):
        lr.select_masks(cand, torch.zeros(2, 3), INPUT, (33, 70), model_size=M, threshold=float('nan'))
    with pytest.raises(lr.DevaHipError, match='`out` must be uint8'):
        lr.select_masks(cand, torch.zeros(2, 3), INPUT, (33, 70), model_size=M, out=torch.zeros(2, 33, 70))
    state = SimpleNamespace(height=33, width=70)
    t = dict(pred_iou_thresh=0.88, stability_score_thresh=0.95, stability_score_offset=1.0, mask_threshold=0.0)
    with pytest.raises(lr.DevaHipError, match=r'\[B,LH,LW\] low-resolution logits expected'):
        lr.proposal_batch(state, cand, torch.zeros(2), INPUT, model_size=M, **t)
    with pytest.raises(lr.DevaHipError, match=r'iou_preds must be fp32 \[2\]'):
        lr.proposal_batch(state, low, torch.zeros(3), INPUT, model_size=M, **t)
    with pytest.raises(lr.DevaHipError, match='a threshold is not a number'):
        lr.proposal_batch(state, low, torch.zeros(2), INPUT, model_size=M, **dict(t, mask_threshold=float('nan')))
    with pytest.raises(lr.DevaHipError, match='an input_size within'):
        lr.proposal_batch(state, low, torch.zeros(2), (36, 65), model_size=M, **t)


def test_host_tensors_are_refused_there_is_no_cpu_path():
    lr = _built()
    low = torch.zeros(2, 16, 16)
    with pytest.raises(lr.DevaHipError, match='low must live on the HIP device'):
        lr.upsample_logits(low, INPUT, (33, 70), model_size=M)
    with pytest.raises(lr.DevaHipError, match='low must live on the HIP device'):
        lr.select_masks(low[:, None], None, INPUT, (33, 70), model_size=M)
    state = SimpleNamespace(height=33, width=70)
    with pytest.raises(lr.DevaHipError, match='low must live on the HIP device'):
        lr.proposal_batch(state, low, torch.zeros(2), INPUT, model_size=M, pred_iou_thresh=0.88, stability_score_thresh=0.95,
                          stability_score_offset=1.0, mask_threshold=0.0)


# ------------------------------------------------------------------------------------------ the sanitizers
def test_plan_code_under_host_sanitizers(tmp_path):
    """csrc/lowres/lowres_plan.cpp in a stand-alone program with its own main (tests/lowres_plan_sanitize_main.cpp); nothing
    is loaded into Python and no GPU is involved"""
    exe = tmp_path / 'lowres_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', LOWRES_SRC, os.path.join(LOWRES_SRC, 'lowres_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'lowres_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 1000000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
SOURCES = sorted(f for f in os.listdir(LOWRES_SRC) if f.endswith('.hip')) if os.path.isdir(LOWRES_SRC) else []
# static LDS bytes: the tally's [4][6] int32, the decide kernel's wave sums; the patch of the tile path is dynamic
KERNELS = {'lowres_upsample_kernel': 0, 'lowres_select_kernel': 0, 'lowres_stats_kernel': 96, 'lowres_binarize_kernel': 0,
           'prop_decide_kernel': 64}


def test_the_listing_is_not_empty():
    assert SOURCES == ['lowres.hip']
    assert sorted(f for f in os.listdir(LOWRES_SRC) if f.endswith('.cpp')) == ['lowres_plan.cpp']
    for name in ('lowres_plan.cpp', 'lowres_plan.h'):
        text = open(os.path.join(LOWRES_SRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name        # the plan is host code
    for name in ('proposal_plan.h', 'host_args.h'):                          # and so is what it includes
        text = open(os.path.join(CSRC, name)).read()
        assert 'hip/' not in text and '__global__' not in text, name
    make = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'LOWRES_OUT := ../deva/hip/lowres_lib/libdeva_lowres.so' in make and '$(eval $(call LIBRARY,LOWRES_OUT,lowres/))' in make
    assert re.search(r'^clean:\n\trm -f .*\$\(LOWRES_OUT\)', make, flags=re.M) and re.search(r'^all: .*\$\(LOWRES_OUT\)', make, flags=re.M)
    assert 'lowres/lowres.o: CXXFLAGS += -ffp-contract=off' in make
    # one text of the decide kernel and the tally, compiled by both translation units
    shared = open(os.path.join(CSRC, 'proposal_device.h')).read()
    for name in ('struct PropArgs', 'prop_live', 'struct PropTally', 'prop_take', 'prop_decide_kernel'):
        assert name in shared, name
    for src in (os.path.join(CSRC, 'proposals.hip'), os.path.join(LOWRES_SRC, 'lowres.hip')):
        text = open(src).read()
        assert 'proposal_device.h"' in text and 'struct PropArgs' not in text and 'prop_decide_kernel(PropArgs a) {' not in text


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    kernels = abi_util.kernel_resources(os.path.join(LOWRES_SRC, src), ['-ffp-contract=off'])
    assert len(kernels) == 2 * 4 + 1                                          # both paths of the four kernels, and decide
    for name, r in kernels.items():
        lds = [v for k, v in KERNELS.items() if k in name]
        assert len(lds) == 1, name
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0 and r.get('SGPRs Spill', 0) == 0, (name, r)
        assert r.get('LDS Size', 0) == lds[0], (name, r)
        assert r['Occupancy'] >= 4, (name, r)                                # (a workgroup is 4 waves, one per SIMD)


# ------------------------------------------------------------------------------------------ the statement
def test_l1_by_hand():
    i0, i1, l0, l1 = LC.axis(16, 64)                                         # scale 0.25: s = 0.25 d - 0.375
    assert i0[:7].tolist() == [0, 0, 0, 0, 0, 0, 1] and i1[:7].tolist() == [1, 1, 1, 1, 1, 1, 2]
    assert l1[:6].tolist() == [0.0, 0.0, 0.125, 0.375, 0.625, 0.875] and l0[2] == 0.875
    assert i0[-1] == 15 and i1[-1] == 15                                     # clamped at the edge, the weight stays
    i0, i1, _, _ = LC.axis(36, 5)                                            # stage 2 clamps at the crop's edge
    assert i1.max() <= 35 and i0.tolist() == [3, 10, 17, 24, 31]
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(LC.resize(x, (3, 4), (3, 4)), x)                   # the identity
    assert LC.resize(x, (2, 2), (1, 1))[0, 0] == np.float32(2.5)             # the crop: 0, 1, 4, 5


@pytest.mark.parametrize('case', LC.ATEN_CASES, ids=[f'{c[3][0]}x{c[3][1]}' for c in LC.ATEN_CASES])
def test_the_statement_against_aten_on_the_cpu(case):
    """values within 4 x the measured bound; bytes equal wherever ATen's value is further than that from the threshold, and
    far fewer than 1 % of the pixels are that close"""
    low_size, m, input_size, size = case
    bound = LC.ATEN_FACTOR * LC.ATEN_BOUND
    low = LC.smooth_logits(5, 3, low_size)
    ours = LC.upsample(low, m, input_size, size)
    aten = LC.aten_chain(torch.from_numpy(low), m, input_size, size).numpy()
    worst = float(np.abs(ours - aten).max())
    print(f'{case}: worst |statement - ATen| = {worst:.3e} (measured bound {LC.ATEN_BOUND:.3e}, asserted {bound:.3e})')
    assert worst <= bound
    for t in (0.0, 1.0, -1.0):
        near = np.abs(aten - t) <= bound
        assert near.mean() <= LC.ATEN_EXCUSED_MAX / 10
        assert np.array_equal((ours > t)[~near], (aten > t)[~near])


def test_special_values_follow_ieee():
    low = LC.logits(3, 4, LOW)
    out = LC.upsample(low, M, INPUT, (33, 70))
    aten = LC.aten_chain(torch.from_numpy(low), M, INPUT, (33, 70)).numpy()
    assert np.isnan(out[1]).all() and np.isinf(out[2]).any() and np.isnan(out[2]).any()       # 0 * inf at the patch's rim
    assert np.array_equal(np.isnan(out), np.isnan(aten)) and np.array_equal(np.isposinf(out), np.isposinf(aten))
    assert np.array_equal(np.isneginf(out), np.isneginf(aten))


# ------------------------------------------------------------------------------------------ the filter on the CPU contract
def _frame(seed, n=24):
    iou = LC.iou_preds(seed, n)
    iou[:4] = 0.99
    return [(LC.logits(seed, n, LOW), iou), (LC.logits(seed + 1, 5, LOW), np.full(5, 0.5, dtype=np.float32)),
            (np.zeros((0,) + LOW, dtype=np.float32), np.zeros(0, dtype=np.float32))]


def _same(found, want):
    assert found.index.tolist() == want.index.tolist() and found.boxes.tolist() == want.boxes.tolist()
    assert torch.equal(found.iou_preds.view(torch.int32), want.iou_preds.view(torch.int32))
    assert torch.equal(found.stability.view(torch.int32), want.stability.view(torch.int32))
    assert torch.equal(found.masks, want.masks)


@pytest.mark.parametrize('size', [(33, 70), (5, 9), (1, 1)])
@pytest.mark.parametrize('stability', [0.95, 0.7, 0.0])
def test_add_lowres_is_add_on_the_statements_planes(size, stability, monkeypatch):
    from deva.inference.proposals import ProposalFilter
    _install(monkeypatch)
    a = ProposalFilter(*size, capacity=64, stability_score_thresh=stability)
    b = ProposalFilter(*size, capacity=64, stability_score_thresh=stability)
    for low, iou in _frame(21):
        a.add_lowres(torch.from_numpy(low), torch.from_numpy(iou), INPUT, model_size=M)
        b.add(torch.from_numpy(LC.upsample(low, M, INPUT, size)).view(-1, *size), torch.from_numpy(iou))
    accounts = (dict(a._state.account), dict(b._state.account))
    found, want = a.finish(), b.finish()
    _same(found, want)
    assert accounts[0] == accounts[1] and accounts[0]['dropped_by_iou'] >= 5
    assert size != (33, 70) or stability == 0.95 or found.masks.shape[0] > 0


def test_add_lowres_overflow_raises_as_add_does(monkeypatch):
    from deva.hip import DevaHipError
    from deva.inference.proposals import ProposalFilter
    _install(monkeypatch)
    size = (33, 70)
    texts = []
    for route in ('lowres', 'full'):
        flt = ProposalFilter(*size, capacity=3, stability_score_thresh=0.0)
        for low, iou in _frame(21):
            if route == 'lowres':
                flt.add_lowres(torch.from_numpy(low), torch.from_numpy(iou), INPUT, model_size=M)
            else:
                flt.add(torch.from_numpy(LC.upsample(low, M, INPUT, size)).view(-1, *size), torch.from_numpy(iou))
        with pytest.raises(DevaHipError, match=r'masks passed the filter, the arena holds 3') as caught:
            flt.finish()
        texts.append(str(caught.value))
    assert texts[0] == texts[1]


def test_select_masks_is_box_mask_select_on_the_statements_planes(monkeypatch):
    from deva.hip import lowres, ops
    _install(monkeypatch)
    low = LC.logits(11, 12, LOW).reshape(4, 3, *LOW)
    scores = torch.tensor([[0.1, 0.9, 0.5], [float('nan'), 0.2, 0.3], [0.5, 0.5, 0.5], [0.0, -0.0, -1.0]])
    for size in ((33, 70), (5, 9)):
        planes, chosen = lowres.select_masks(torch.from_numpy(low), scores, INPUT, size, model_size=M, threshold=0.5)
        full = torch.from_numpy(LC.upsample(low, M, INPUT, size)).view(4, 3, *size)
        want, picks = ops.box_mask_select(full, scores, 0.5)
        assert chosen.tolist() == picks.tolist() == [1, 0, 0, 0] and torch.equal(planes, want)


# ------------------------------------------------------------------------------------------ the processors
class LowresPointSegmenter:
    """a stand-in with both routes: every point yields three low-resolution planes from the generator (steep, so that some
    pass the stability drop), the same ones however the points are batched; `predict_points` is the statement's resize of
    them"""
    model_size = M

    def __init__(self, lowres=True):
        self.calls, self.shape, self.input_size = [], None, None
        if not lowres:
            self.predict_points_lowres = None

    def set_image(self, image_np):
        from deva.hip import lowres
        self.shape = image_np.shape[:2]
        self.input_size = lowres.sam_input_size(*self.shape, M)

    def _planes(self, points_px):
        pts = points_px.cpu().numpy()
        seeds = [int(x) * 1000 + int(y) for x, y in pts]
        low = np.concatenate([LC.smooth_logits(s, 3, LOW, scale=60.0) for s in seeds])
        iou = np.concatenate([np.array([0.96, 0.5, 0.9], dtype=np.float32) + np.float32(0.0001 * (s % 97)) for s in seeds])
        return low, iou

    def predict_points_lowres(self, points_px):
        self.calls.append('lowres')
        low, iou = self._planes(points_px)
        return torch.from_numpy(low), torch.from_numpy(iou)

    def predict_points(self, points_px):
        self.calls.append('full')
        low, iou = self._planes(points_px)
        return torch.from_numpy(LC.upsample(low, M, self.input_size, self.shape)).view(-1, *self.shape), torch.from_numpy(iou)


def test_automatic_processor_takes_the_lowres_route(monkeypatch):
    from deva.hip import DevaHipError
    from deva.inference.automatic import AutomaticProcessor
    _install(monkeypatch)
    core = SimpleNamespace(config=prompt_case.loop_config('online', SAM_NUM_POINTS_PER_SIDE=4, SAM_NUM_POINTS_PER_BATCH=5))
    image = np.zeros((36, 64, 3), dtype=np.uint8)
    results = {}
    for name, seg, kw in (('auto', LowresPointSegmenter(), {}), ('forced', LowresPointSegmenter(), dict(lowres=True)),
                          ('off', LowresPointSegmenter(), dict(lowres=False)), ('full only', LowresPointSegmenter(lowres=False), {})):
        processor = AutomaticProcessor(core, seg, capacity=64, **kw)
        mask, info = processor.segment(image, None, device='cpu')
        results[name] = (mask, [(o.id, o.scores) for o in info])
        assert set(seg.calls) == ({'lowres'} if name in ('auto', 'forced') else {'full'}) and len(seg.calls) == 4
        assert processor.lowres == (name in ('auto', 'forced'))
    assert len(results['auto'][1]) >= 1 and 0 < int((results['auto'][0] > 0).sum()) < 36 * 64   # something came through
    for name in ('forced', 'off', 'full only'):
        assert torch.equal(results[name][0], results['auto'][0]) and results[name][1] == results['auto'][1]
    with pytest.raises(DevaHipError, match='lowres=True: the segmenter has no `predict_points_lowres`'):
        AutomaticProcessor(core, LowresPointSegmenter(lowres=False), lowres=True)


class LowresBoxSegmenter(TC.FakeBoxSegmenter):
    """`predict_boxes_lowres`: three candidates per box from the generator; `predict_boxes`: the statement's resize of them"""
    model_size = M

    def __init__(self, lowres=True):
        super().__init__()
        self.input_size = None
        if not lowres:
            self.predict_boxes_lowres = None

    def set_image(self, image_np):
        from deva.hip import lowres
        super().set_image(image_np)
        self.input_size = lowres.sam_input_size(*self.shape, M)

    def _answer(self, boxes_px):
        boxes = boxes_px.cpu().numpy()
        low = np.stack([LC.smooth_logits(int(b[0]) * 100 + int(b[1]), 3, LOW) for b in boxes])
        scores = np.stack([np.roll(np.array([0.9, 0.5, 0.7], dtype=np.float32), int(b[0]) % 3) for b in boxes])
        return low, scores

    def predict_boxes_lowres(self, boxes_px):
        self.calls.append(('predict_boxes_lowres', None))
        low, scores = self._answer(boxes_px)
        return torch.from_numpy(low), torch.from_numpy(scores)

    def predict_boxes(self, boxes_px):
        self.calls.append(('predict_boxes', None))
        low, scores = self._answer(boxes_px)
        return torch.from_numpy(LC.upsample(low, M, self.input_size, self.shape)).view(-1, 3, *self.shape), torch.from_numpy(scores)


def test_text_detections_take_the_lowres_route(monkeypatch):
    from deva.hip import DevaHipError
    from deva.inference import detections
    from deva.inference.with_text import TextPromptedProcessor
    _install(monkeypatch)
    h, w = 36, 64
    boxes = np.array([[2, 3, 30, 20], [31, 5, 60, 30], [10, 18, 40, 34], [3, 3, 29, 21], [50, 1, 63, 12]], dtype=np.float32)
    conf = np.array([0.9, 0.8, 0.7, 0.6, 0.5], dtype=np.float32)
    classes = [0, 1, 0, None, 2]
    results = {}
    for name, seg, lowres in (('auto', LowresBoxSegmenter(), None), ('forced', LowresBoxSegmenter(), True), ('off', LowresBoxSegmenter(), False),
                              ('full only', LowresBoxSegmenter(lowres=False), None)):
        seg.set_image(np.zeros((h, w, 3), dtype=np.uint8))
        mask, info = detections.text_detections(boxes, conf, classes, seg, (h, w), (h, w), nms_threshold=0.5, boxes_per_batch=2,
                                                device='cpu', lowres=lowres)
        results[name] = (mask, [(o.id, o.category_ids, o.scores) for o in info])
        kinds = {c[0] for c in seg.calls} - {'set_image'}
        assert kinds == ({'predict_boxes_lowres'} if name in ('auto', 'forced') else {'predict_boxes'})
    assert int(results['auto'][0].max()) >= 3 and len(results['auto'][1]) >= 3
    for name in ('forced', 'off', 'full only'):
        assert torch.equal(results[name][0], results['auto'][0]) and results[name][1] == results['auto'][1]
    with pytest.raises(DevaHipError, match='lowres=True: the segmenter has no `predict_boxes_lowres`'):
        detections.text_detections(boxes, conf, classes, LowresBoxSegmenter(lowres=False), (h, w), (h, w), nms_threshold=0.5, device='cpu', lowres=True)
    core = SimpleNamespace(config=dict(size=-1, temporal_setting='online', num_voting_frames=3, detection_every=5, prompt='a.b',
                                       DINO_THRESHOLD=0.3, DINO_NMS_THRESHOLD=0.5))
    assert TextPromptedProcessor(core, object(), LowresBoxSegmenter()).lowres is True
    assert TextPromptedProcessor(core, object(), LowresBoxSegmenter(lowres=False)).lowres is False
    assert TextPromptedProcessor(core, object(), LowresBoxSegmenter(), lowres=False).lowres is False
