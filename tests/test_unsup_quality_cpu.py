"""Scoring an unsupervised DAVIS run without a GPU: libdeva_pair_metrics.so on its ABI, its argument errors and its launch
plan; the plan's host code under the host sanitizers; the kernels' static resources; `assign` against brute force (and
scipy where it is installed); `deva.inference.unsup_quality` on the CPU contract of the pair counts (tests/emu_pairs.py,
the numpy statement of tests/pair_case.py) against the from-scratch restatement of the protocol (tests/unsup_case.py); the
limiter against recorded output of the reference's own `limit_max_id` (tests/golden/unsup_limit.npz)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import abi_util
import emu_pairs as EP
import pair_case as PC
import unsup_case as UC
import vos_case as VC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deva_pair_metrics.h')
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')
PAIR_SRC = os.path.join(CSRC, 'pair_metrics')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = os.environ.get('DEVA_HOST_CXX', '/opt/rocm/llvm/bin/clang++')
WANT = ['deva_pair_counts', 'deva_pair_last_error', 'deva_pair_plan', 'deva_pair_scratch_bytes', 'deva_pair_version']


@pytest.fixture()
def emu(monkeypatch):
    EP.install(monkeypatch)


def _built():
    from deva.hip import pair_metrics
    return abi_util.built(pair_metrics)


# ------------------------------------------------------------------------------------------ ABI
def test_exports_header_and_binding_are_one_list():
    pm = _built()
    exported, _ = abi_util.exported(pm.LIB_PATH)
    assert exported == abi_util.declared(HEADER) == sorted(pm.SIGNATURES) == WANT
    header = open(HEADER).read()
    assert re.search(r'#define DEVA_PAIR_ABI_VERSION 1\b', header)
    assert pm.ABI_VERSION == 1 and pm.lib().deva_pair_version() == 1
    for name, value in (('U8', pm.U8), ('I32', pm.I32), ('I64', pm.I64), ('INDEX16', pm.INDEX16), ('MAX_OBJECTS', pm.MAX_OBJECTS),
                        ('MAX_RADIUS', pm.MAX_RADIUS), ('FIELDS', pm.FIELDS), ('SINGLE_FIELDS', pm.SINGLE_FIELDS), ('STRIP', pm.STRIP),
                        ('INNER_RADIUS', pm.INNER_RADIUS)):
        assert re.search(rf'#define DEVA_PAIR_{name} {value}\b', header), name
    from deva.hip import vos_metrics as vm      # P1: the encodings and their numbers are those of the DAVIS counts
    assert (pm.U8, pm.I32, pm.I64, pm.INDEX16, pm.MAX_RADIUS) == (vm.U8, vm.I32, vm.I64, vm.INDEX16, vm.MAX_RADIUS)
    for rule in ('P1', 'P2', 'P3', 'P4', 'P5'):
        assert re.search(rf'^ \*   {rule}  ', header, flags=re.M), rule
    # P2 is R2, word for word
    vos_header = open(os.path.join(ROOT, 'include', 'deva_vos_metrics.h')).read()
    r2 = re.search(r'R2  (boundary map:.*?)\n \*   R3', vos_header, flags=re.S).group(1)
    p2 = re.search(r'P2  (boundary map:.*?)\n \*   P3', header, flags=re.S).group(1)
    assert r2 == p2


def test_no_symbol_is_shared_with_the_other_three_libraries():
    from deva import hip
    from deva.hip import metrics, vos_metrics
    pm = _built()
    exported, mine = abi_util.exported(pm.LIB_PATH)
    assert all(name.startswith('deva_pair_') for name in exported)
    for other in (hip.LIB_PATH, metrics.LIB_PATH, vos_metrics.LIB_PATH):
        theirs_exported, theirs = abi_util.exported(other)
        assert not any(n.startswith('deva_pair') for n in theirs_exported)
        shared = {s for s in mine & theirs if 'deva' in s}
        assert not shared, (other, shared)


def test_plan_mirror_has_the_c_layout(tmp_path):
    pm = _built()
    fields = [f[0] for f in pm.Plan._fields_]
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deva_pair_metrics.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(struct deva_pair_plan));\n' +
                   ''.join(f'printf("%zu\\n", offsetof(struct deva_pair_plan, {f}));\n' for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(pm.Plan) and vals[1:] == [getattr(pm.Plan, f).offset for f in fields]


# ------------------------------------------------------------------------------------------ refusals
A = 1 << 30   # made-up addresses: validation fails before anything is dereferenced or launched
GT, PRED, GIDS, PIDS, LUT, SCRATCH, ONE, TWO = (A + (k << 26) for k in (0, 1, 2, 3, 4, 5, 7, 8))


def _counts(L, gt=GT, gt_enc=0, gids=GIDS, n_gt=3, pred=PRED, pred_enc=0, pids=PIDS, n_pred=5, lut=None, channels=0, h=8, w=12,
            radius=2, scratch=SCRATCH, scratch_bytes=16 * 8 * 12, singles=ONE, pairs=TWO):
    return L.deva_pair_counts(gt, gt_enc, gids, n_gt, pred, pred_enc, pids, n_pred, lut, channels, h, w, radius, scratch,
                              scratch_bytes, singles, pairs, None)


def test_argument_errors_before_any_launch():
    pm = _built()
    L = pm.lib()
    err = L.deva_pair_last_error
    assert _counts(L, h=0) == 2          # (the good call below would launch: every call here is refused)
    for enc in (2, 3, -1, 4, 256, 257, 512):        # there is no binary form
        assert _counts(L, gt_enc=enc) == 2 and b'ground truth is U8 (0) or I32 (1)' in err(), enc
    for enc in (-1, 4, 256, 256 + 3, 512):
        assert _counts(L, pred_enc=enc) == 2 and b'unknown encoding' in err(), enc
    for n in (0, -1, 65):
        assert _counts(L, n_gt=n) == 2 and b'1 to 64 ground-truth objects' in err()
        assert _counts(L, n_pred=n) == 2 and b'1 to 64 proposals' in err()
    for radius in (-1, 129):
        assert _counts(L, radius=radius) == 2 and b'radius 0 to 128' in err()
    assert _counts(L, h=0) == 2 and b'bad plane size' in err()
    assert _counts(L, w=-3) == 2 and b'bad plane size' in err()
    assert _counts(L, h=32769, w=32768, scratch_bytes=1 << 40) == 2 and b'bad plane size' in err()     # above 2^30 pixels
    assert _counts(L, gt=None) == 2 and b'ground-truth plane' in err()
    assert _counts(L, gt=GT + 8) == 2 and b'misaligned ground-truth plane' in err()
    assert _counts(L, pred=None) == 2 and b'predicted plane' in err()
    assert _counts(L, pred=PRED + 4) == 2 and b'misaligned predicted plane' in err()
    assert _counts(L, gids=None) == 2 and b'ground-truth id table' in err()
    assert _counts(L, gids=GIDS + 2) == 2 and b'misaligned ground-truth id table' in err()
    assert _counts(L, pids=None) == 2 and b'proposal id table' in err()
    assert _counts(L, pids=PIDS + 2) == 2 and b'misaligned proposal id table' in err()
    fast = dict(pred_enc=3, lut=LUT, channels=7)
    assert _counts(L, **dict(fast, lut=None)) == 2 and b'channel table' in err()
    assert _counts(L, **dict(fast, lut=LUT + 1)) == 2 and b'channel table' in err()
    for channels in (0, -1, 32768):
        assert _counts(L, **dict(fast, channels=channels)) == 2 and b'1 to 32767 channels' in err()
    assert _counts(L, scratch=None) == 2 and b'scratch' in err()
    assert _counts(L, scratch=SCRATCH + 8) == 2 and b'misaligned scratch' in err()
    assert _counts(L, scratch_bytes=16 * 8 * 12 - 1) == 2 and b'1536 are needed' in err()
    assert _counts(L, singles=None) == 2 and b'singles' in err()
    assert _counts(L, singles=ONE + 2) == 2 and b'misaligned singles' in err()
    assert _counts(L, pairs=None) == 2 and b'pairs' in err()
    assert _counts(L, pairs=TWO + 2) == 2 and b'misaligned pairs' in err()
    # an output over an input: a plane's last byte, either table's last entry, the channel table, the scratch, the other output
    for name, text in (('singles', b'singles overlaps an input'), ('pairs', b'pairs overlaps an input')):
        assert _counts(L, **{name: GT + 8 * 12 - 4}) == 2 and text in err()
        assert _counts(L, pred_enc=2, **{name: PRED + 8 * 12 * 8 - 4}) == 2 and text in err()
        assert _counts(L, **{name: GIDS + 8}) == 2 and text in err()
        assert _counts(L, **{name: PIDS + 16}) == 2 and text in err()
        assert _counts(L, **dict(fast, **{name: LUT + 12})) == 2 and text in err()
        assert _counts(L, **{name: SCRATCH + 16 * 8 * 12 - 4}) == 2 and text in err()
    assert _counts(L, gt=ONE + 16) == 2 and b'singles overlaps an input' in err()
    assert _counts(L, pairs=ONE + 4 * 2 * 8 - 4) == 2 and b'singles and pairs overlap' in err()
    assert _counts(L, singles=TWO + 4 * 4 * 15 - 4) == 2 and b'singles and pairs overlap' in err()
    assert _counts(L, scratch=GT + 16 * 5) == 2 and b'scratch overlaps an input' in err()
    assert all(b'deva_pair_counts' in (_counts(L, **kw), err())[1] for kw in (dict(h=0), dict(gt=None), dict(n_gt=0)))
    plan, nbytes = pm.Plan(), ctypes.c_int64()
    assert L.deva_pair_plan(8, 12, 3, 5, 2, None) == 2 and b'deva_pair_plan: null plan' in err()
    assert L.deva_pair_plan(8, 12, 65, 5, 2, ctypes.byref(plan)) == 2 and b'1 to 64 ground-truth objects' in err()
    assert L.deva_pair_plan(8, 12, 3, 0, 2, ctypes.byref(plan)) == 2 and b'1 to 64 proposals' in err()
    assert L.deva_pair_plan(8, 12, 3, 5, 129, ctypes.byref(plan)) == 2 and b'radius 0 to 128' in err()
    assert L.deva_pair_plan(0, 12, 3, 5, 2, ctypes.byref(plan)) == 2 and b'bad plane size' in err()
    assert L.deva_pair_scratch_bytes(8, 12, None) == 2 and b'null bytes' in err()
    assert L.deva_pair_scratch_bytes(8, -1, ctypes.byref(nbytes)) == 2 and b'bad plane size' in err()


def test_wrapper_errors_before_any_launch():
    from deva.hip import DevaHipError
    pm = _built()
    gt, pred = torch.zeros(4, 6, dtype=torch.int32), torch.zeros(4, 6, dtype=torch.int64)
    with pytest.raises(DevaHipError, match='gt must be an .H,W. plane of torch.uint8, torch.int32'):
        pm.pair_counts(pred, pred, [1], [1])
    with pytest.raises(DevaHipError, match='pred must be an .H,W. plane'):
        pm.pair_counts(gt, pred.float(), [1], [1])
    with pytest.raises(DevaHipError, match=r'gt is \(4, 6\) and pred \(4, 5\)'):
        pm.pair_counts(gt, pred[:, :5], [1], [1])
    with pytest.raises(DevaHipError, match='go together'):
        pm.pair_counts(gt, pred.to(torch.int16), [1], [1])
    with pytest.raises(DevaHipError, match='go together'):
        pm.pair_counts(gt, pred, [1], [1], pred_lut=torch.zeros(3, dtype=torch.uint16))
    with pytest.raises(DevaHipError, match='pred_ids is needed'):
        pm.pair_counts(gt, pred, [1])
    for bad in ([3, 2], [2, 2], [0, 1], [-4], [2**31]):
        with pytest.raises(DevaHipError, match='gt_ids must be distinct, ascending'):
            pm.pair_counts(gt, pred, bad, [1])
        with pytest.raises(DevaHipError, match='pred_ids must be distinct, ascending'):
            pm.pair_counts(gt, pred, [1], bad)
    with pytest.raises(DevaHipError, match='at least one object id'):
        pm.pair_counts(gt, pred, [], [1])
    with pytest.raises(DevaHipError, match=r'at most 64 gt_ids \(got 65\)'):
        pm.pair_counts(gt, pred, list(range(1, 66)), [1])
    with pytest.raises(DevaHipError, match=r'at most 64 pred_ids \(got 65\)'):
        pm.pair_counts(gt, pred, [1], list(range(1, 66)))
    with pytest.raises(DevaHipError, match='radius 0 to 128'):
        pm.pair_counts(gt, pred, [1], [1], radius=129)
    with pytest.raises(DevaHipError, match='an integer'):
        pm.pair_counts(gt, pred, [1], [1], bound_th=2.5)
    with pytest.raises(DevaHipError, match=r'`out` must be uint32 \[3,2\]'):
        pm.pair_counts(gt, pred, [1, 2], [1], out=(torch.zeros(2, 2, dtype=torch.int32).view(torch.uint32), None))
    with pytest.raises(DevaHipError, match=r'`out\[1\]` must be uint32 \[2,1,4\]'):
        pm.pair_counts(gt, pred, [1, 2], [1], out=(torch.zeros(3, 2, dtype=torch.int32).view(torch.uint32), torch.zeros(2, 1, 4)))
    with pytest.raises(DevaHipError, match=r'`scratch` must be uint8 \[384\]'):
        pm.pair_counts(gt, pred, [1, 2], [1], scratch=torch.zeros(383, dtype=torch.uint8))
    with pytest.raises(DevaHipError, match='HIP device'):
        pm.pair_counts(gt, pred, [1], [1])


# ------------------------------------------------------------------------------------------ the plan
def test_plan_is_host_side_monotone_and_capped():
    pm = _built()
    # 480 x 854: 107 strips of 8 a row, 51 360 strips; 409 920 pixels, 6 405 chunks of 64 for at most 1024 x 4 waves
    assert pm.pair_plan(480, 854, 5, 20, 8) == pm.PlanInfo(201, 1024, 256, 4 * (50 + 100), 4 * (128 + 200), 3, 1, 8, 16 * 480 * 854)
    assert pm.pair_plan(240, 427, 5, 20, 4).match_grid == 401          # 102 480 pixels: 1 602 chunks, a wave each
    assert pm.pair_scratch_bytes(480, 854) == 16 * 480 * 854
    assert pm.pair_plan(1, 1, 1, 1, 0) == pm.PlanInfo(1, 1, 256, 20, 520, 0, 0, 0, 16)
    assert [pm.pair_plan(9, 1, 2, 2, r)[5:7] for r in (2, 3, 4, 128)] == [(2, 0), (3, 0), (3, 1), (3, 1)]
    full = pm.pair_plan(96, 128, 64, 64, 8)      # the LDS tables at their largest: 32.5 KB of 160
    assert full.match_lds_bytes == 4 * (128 + 2 * 64 * 64) == 33280 and full.label_lds_bytes == 4 * (256 + 4096)
    assert max(full.match_lds_bytes, full.label_lds_bytes) <= 160 * 1024
    big = pm.pair_plan(32768, 32768, 1, 1, 36)             # capped: the rest is a grid-stride loop
    assert (big.label_grid, big.match_grid, big.scratch_bytes) == (2048, 1024, 1 << 34)
    sizes = [(1, 1), (8, 12), (96, 128), (480, 854), (1080, 1920), (2160, 3840)]
    plans = [pm.pair_plan(h, w, 5, 20, 8) for h, w in sizes]
    for a, b in zip(plans, plans[1:]):        # monotone in the plane
        assert a.label_grid <= b.label_grid and a.match_grid <= b.match_grid and a.scratch_bytes < b.scratch_bytes
    tables = [pm.pair_plan(96, 128, g, p, 8) for g, p in ((1, 1), (1, 20), (5, 20), (20, 20), (64, 20), (64, 64))]
    for a, b in zip(tables, tables[1:]):      # and in the tables
        assert a.label_lds_bytes < b.label_lds_bytes and a.match_lds_bytes < b.match_lds_bytes and a[:3] == b[:3]
    for g, p, text in ((0, 1, 'ground-truth objects'), (65, 1, 'ground-truth objects'), (1, 0, 'proposals'), (1, 65, 'proposals')):
        with pytest.raises(pm.DevaHipError, match='1 to 64 ' + text):
            pm.pair_plan(480, 854, g, p, 8)
    with pytest.raises(pm.DevaHipError, match='bad plane size'):
        pm.pair_plan(0, 5, 1, 1, 1)


def test_plan_code_under_host_sanitizers(tmp_path):
    """csrc/pair_metrics/pair_plan.cpp in a stand-alone program with its own main (tests/pair_plan_sanitize_main.cpp);
    nothing is loaded into Python and no GPU is involved"""
    exe = tmp_path / 'pair_sanitize'
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', PAIR_SRC, os.path.join(PAIR_SRC, 'pair_plan.cpp'),
                    os.path.join(ROOT, 'tests', 'pair_plan_sanitize_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, run.stderr[-4000:]
    checks, refused, failures = (int(v) for v in re.findall(r'\d+', run.stdout))
    assert checks > 100000 and 0 < refused < checks and failures == 0


# ------------------------------------------------------------------------------------------ static resources
SOURCES = sorted(f for f in os.listdir(PAIR_SRC) if f.endswith('.hip')) if os.path.isdir(PAIR_SRC) else []


def test_the_listing_is_not_empty():
    assert SOURCES == ['pair_counts.hip']
    assert sorted(f for f in os.listdir(PAIR_SRC) if f.endswith('.cpp')) == ['pair_plan.cpp']
    text = open(os.path.join(PAIR_SRC, 'pair_plan.cpp')).read() + open(os.path.join(PAIR_SRC, 'pair_plan.h')).read()
    assert 'hip/' not in text and '__global__' not in text        # the plan is host only


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
@pytest.mark.parametrize('src', SOURCES)
def test_no_kernel_spills_or_uses_scratch(src):
    kernels = abi_util.kernel_resources(os.path.join(PAIR_SRC, src))
    # 2 ground-truth encodings x 4 predicted, and the disk search
    assert sum('pair_label_kernel' in name for name in kernels) == 8 and sum('pair_match_kernel' in name for name in kernels) == 1
    for name, r in kernels.items():
        assert r.get('ScratchSize', 0) == 0, (name, r)
        assert r.get('VGPRs Spill', 0) == 0, (name, r)
        assert r.get('LDS Size', 0) <= 160 * 1024, (name, r)
        assert r['Occupancy'] >= 4, (name, r)


# ------------------------------------------------------------------------------------------ the contract itself
def test_the_statement_reproduces_the_davis_counts_on_one_table():
    """P5's identity, on the two numpy statements: the same table on both sides gives record i of `vos_case.counts`"""
    gt, pred, ids = VC.case(24, 40, 4, 5)
    singles, pairs = PC.counts(gt, pred, ids, ids, 2)
    want = VC.counts(gt, pred, ids, 2)
    for i in range(len(ids)):
        assert np.array_equal(PC.record(singles, pairs, i, i), want[i].astype(np.int64))
    assert not pairs[..., 3].any() and pairs[..., 0].sum() == (np.isin(gt, ids) & np.isin(pred, ids)).sum()


# ------------------------------------------------------------------------------------------ assign
def _check_assign(score):
    from deva.inference.unsup_quality import assign
    got = assign(score)
    best, maps = UC.brute_force(score)
    assert len(got) == score.shape[1] == len(set(got)) and all(0 <= p < score.shape[0] for p in got)
    total = sum(score[p, g] for g, p in enumerate(got))
    assert abs(total - best) <= 1e-12 * max(1, score.shape[1]), (total, best)
    if len(maps) == 1:            # unique by more than 1e-9: the map itself
        assert tuple(got) == maps[0]
    return len(maps) == 1


def test_assign_against_brute_force():
    rng = np.random.default_rng(2024)
    unique = 0
    shapes = [(g + extra, g) for g in (1, 2, 3, 4) for extra in (0, 1, 2) if g + extra <= 6]
    for k in range(200):
        p, g = shapes[k % len(shapes)]
        unique += _check_assign(rng.random((p, g)))
    assert unique == 200            # every seeded matrix has its optimum to itself: the maps were compared, not only the totals
    for p, g in ((1, 1), (6, 1), (4, 4), (6, 4), (5, 5)):
        assert _check_assign(rng.random((p, g)))


def test_assign_with_exact_ties_and_misuse():
    from deva.inference.unsup_quality import assign
    for score in (np.ones((4, 3)), np.zeros((2, 2)), np.array([[1.0, 1.0], [1.0, 1.0], [0.5, 0.5]]),
                  np.array([[0.5, 0.5, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 1.0]])):
        assert not _check_assign(score)             # several optima: the total alone
    assert assign(np.zeros((3, 0))) == []
    assert assign(np.array([[0.2], [0.9], [0.4]])) == [1]
    with pytest.raises(ValueError, match='P >= G'):
        assign(np.zeros((2, 3)))
    with pytest.raises(ValueError, match='finite'):
        assign(np.array([[np.nan]]))


def test_assign_against_scipy():
    optimize = pytest.importorskip('scipy.optimize')
    from deva.inference.unsup_quality import assign
    rng = np.random.default_rng(7)
    for p, g in ((20, 5), (20, 10), (12, 12), (3, 1)):
        score = rng.random((p, g))
        rows, cols = optimize.linear_sum_assignment(score, maximize=True)
        got = assign(score)
        assert abs(score[rows, cols].sum() - sum(score[q, k] for k, q in enumerate(got))) <= 1e-12 * g
        assert got == rows[np.argsort(cols)].tolist()


# ------------------------------------------------------------------------------------------ the scorer on the contract
H, W, T = 24, 40, 5


def _boxes(t, boxes, dtype=np.int64):
    out = np.zeros((H, W), dtype=dtype)
    for label, y0, y1, x0, x1 in boxes:
        out[y0:y1, x0 + t:x1 + t] = label
    return out


def _videos():
    """name -> (gts, preds, gt ids)"""
    gt3 = [_boxes(t, [(1, 2, 10, 2, 12), (2, 12, 22, 4, 16), (3, 4, 18, 20, 32)]) for t in range(T)]
    perm = [PC.rename(np.roll(g, (1, -1), axis=(0, 1)), [1, 2, 3], [31, 7, 19]) for g in gt3]      # other ids, another order
    split = [p.copy() for p in perm]
    for p in split:                 # object 3 in two halves (19 and 40); objects 1 and 2 merged into one proposal (7)
        p[11:, 20:] = np.where(p[11:, 20:] == 19, 40, p[11:, 20:])
        p[p == 31] = 7
    few = [np.where(g == 1, 9, 0) for g in gt3]                                   # P = 1 < G = 3: two padded rows
    few_gt = [g.copy() for g in gt3]
    for t in (1, 3):
        few_gt[t][few_gt[t] == 2] = 0                                            # object 2 absent there: J = F = 1 against an empty proposal
    late = [np.where(p == 19, 0, p) if t < 3 else p for t, p in enumerate(perm)]  # proposal 19 first appears in frame 3
    return {'perm': (gt3, perm, [1, 2, 3]), 'split': (gt3, split, [1, 2, 3]), 'few': (few_gt, few, [1, 2, 3]), 'late': (gt3, late, [1, 2, 3])}


@pytest.fixture(scope='module')
def videos():
    return _videos()


@pytest.fixture(scope='module')
def restated(videos):
    return {name: UC.video(g, p, ids) for name, (g, p, ids) in videos.items()}


def _feed(scorer, videos, names, form=lambda pred: pred.astype(np.int64)):
    for name in names:
        gts, preds, ids = videos[name]
        scorer.start_video(name, ids)
        for g, p in zip(gts, preds):
            scorer.add_frame(form(p), g.astype(np.uint8))
        scorer.end_video()
    return scorer.result()


def _same_as_restated(res, name, want, videos):
    fr = res['frames'][name]
    gts, preds, ids = videos[name]
    assert fr['proposals'] == want['proposals'] and fr['ids'] == ids
    # the integers: the record of every pair on every frame is the per-plane statement's, exactly
    radius = VC.radius_of(H, W)
    for a, p in enumerate(want['proposals']):
        for b, g in enumerate(ids):
            for t in range(T):
                pm = np.zeros((H, W), dtype=bool) if p is None else preds[t] == p
                rec = VC.counts(gts[t] == g, pm, [1], radius)[0]
                assert np.array_equal(fr['counts'][a, b, t], rec.astype(np.int64)), (name, p, g, t)
    # floats: the tolerance of the existing scorer's tests for the same quantities
    assert np.allclose(fr['score'], want['score'], rtol=0, atol=1e-12)
    # the optimum is unique up to swapping padded (empty) rows, which are one and the same proposal: None
    assert len({tuple(want['proposals'][p] for p in m) for m in want['maps']}) == 1
    assert [fr['assignment'][g] for g in ids] == [want['proposals'][p] for p in want['maps'][0]]
    assert np.allclose(fr['J'], want['J'], rtol=0, atol=1e-12) and np.allclose(fr['F'], want['F'], rtol=0, atol=1e-12)


def test_scorer_against_the_restated_protocol(videos, restated, emu):
    from deva.inference.unsup_quality import UnsupervisedVideoScorer
    from deva.inference.vos_quality import GLOBAL_HEADER
    names = ['perm', 'split', 'few', 'late']
    scorer = UnsupervisedVideoScorer()
    res = _feed(scorer, videos, names)
    for name in names:
        _same_as_restated(res, name, restated[name], videos)
    table, per_object = UC.table([(n, restated[n]) for n in names])
    assert list(res['global']) == GLOBAL_HEADER
    assert np.allclose([res['global'][k] for k in GLOBAL_HEADER], table, rtol=0, atol=1e-12)
    assert list(res['sequences']) == [f'{n}_{k}' for n in names for k in (1, 2, 3)]
    for name, k, j, f in per_object:
        seq = res['sequences'][f'{name}_{k}']
        assert seq['J-Mean'] == pytest.approx(np.mean(j), abs=1e-12) and seq['F-Mean'] == pytest.approx(np.mean(f), abs=1e-12)
    # what the cases are there for
    assert res['frames']['perm']['assignment'] == {1: 31, 2: 7, 3: 19} and res['frames']['perm']['score'].shape == (3, 3)
    split = res['frames']['split']
    assert split['proposals'] == [7, 19, 40] and sorted(split['assignment'].values()) == [7, 19, 40]
    few = res['frames']['few']
    assert few['proposals'] == [9, None, None] and few['assignment'][1] == 9 and few['assignment'][2] is None is few['assignment'][3]
    j2 = few['J'][1]      # object 2 against an empty proposal: 0 where it is present, 1 (and F = 1) where both are empty
    assert j2.tolist() == [0.0, 1.0, 0.0, 1.0, 0.0] == few['F'][1].tolist()
    late = res['frames']['late']
    assert late['assignment'][3] == 19 and not late['counts'][late['proposals'].index(19), :, :3, 2].any()
    assert late['counts'][late['proposals'].index(19), 2, 3:, 0].all()
    # the two CSV texts are those of VideoObjectScorer
    texts = scorer.texts()
    assert texts['global_results.csv'].splitlines()[1] == ','.join('%.3f' % v for v in table)
    assert texts['per-sequence_results.csv'].splitlines()[1:] == ['%s_%d,%.3f,%.3f' % (n, k, np.mean(j), np.mean(f)) for n, k, j, f in per_object]


def test_skip_ends_and_too_many_proposals(videos, emu):
    from deva.inference.unsup_quality import UnsupervisedVideoScorer
    res = _feed(UnsupervisedVideoScorer(skip_ends=True), videos, ['split'])
    want = UC.video(*videos['split'], skip_ends=True)
    assert res['frames']['split']['J'].shape == (3, T - 2) and np.allclose(res['frames']['split']['score'], want['score'], rtol=0, atol=1e-12)
    crowd = np.zeros((H, W), dtype=np.int64)
    crowd[:3, :7] = np.arange(1, 22).reshape(3, 7)                     # 21 proposals of one pixel each
    for feed in ([crowd], [np.where(crowd <= 11, crowd, 0), np.where(crowd > 11, crowd, 0)]):
        scorer = UnsupervisedVideoScorer()
        scorer.start_video('crowd', [1])
        with pytest.raises(ValueError, match='more than 20 proposals'):
            for p in feed:
                scorer.add_frame(p, (crowd == 1).astype(np.uint8))
            scorer.end_video()
        with pytest.raises(ValueError):
            UC.video([crowd == 1] * len(feed), feed, [1])
    ok = UnsupervisedVideoScorer(max_proposals=21)
    ok.start_video('crowd', [1])
    ok.add_frame(crowd, (crowd == 1).astype(np.uint8))
    ok.end_video()
    assert ok.result()['frames']['crowd']['assignment'] == {1: 1}


class _Result:
    """shaped like `FrameResult`: the channel plane and the id of every channel"""

    def __init__(self, index, channel_ids):
        self.index, self.channel_ids = torch.from_numpy(index), channel_ids


def test_frame_result_form_equals_the_planes(videos, emu):
    from deva.inference.unsup_quality import UnsupervisedVideoScorer
    names = ['split', 'late', 'few']
    planes = _feed(UnsupervisedVideoScorer(), videos, names)
    seeds = iter(range(100))

    def as_result(pred):
        ids = np.unique(pred[pred > 0])
        index, lut, channel_ids = VC.channel_form(pred, ids, next(seeds))      # two channels share the first id; 99999 and 88888 hold no pixel
        assert np.array_equal(channel_ids[index], pred)
        return _Result(index, channel_ids)
    fast = _feed(UnsupervisedVideoScorer(), videos, names, as_result)
    assert fast['global'] == planes['global'] and fast['sequences'] == planes['sequences']
    for name in names:
        a, b = fast['frames'][name], planes['frames'][name]
        assert np.array_equal(a['counts'], b['counts']) and a['assignment'] == b['assignment'] and a['proposals'] == b['proposals']
    for form in (lambda p: p.astype(np.uint8), lambda p: torch.from_numpy(p.astype(np.int32)), lambda p: torch.from_numpy(p)):
        other = _feed(UnsupervisedVideoScorer(), videos, ['split'], form)
        assert np.array_equal(other['frames']['split']['counts'], planes['frames']['split']['counts'])
    # `keep`: the limiter's set drops a proposal through the table
    scorer = UnsupervisedVideoScorer()
    gts, preds, ids = videos['split']
    scorer.start_video('split', ids)
    for g, p in zip(gts, preds):
        scorer.add_frame(as_result(p), g.astype(np.uint8), keep={7, 19})
    scorer.end_video()
    dropped = scorer.result()['frames']['split']
    assert dropped['proposals'] == [7, 19, None]
    assert np.array_equal(dropped['counts'][:2], planes['frames']['split']['counts'][:2])


def test_scorer_misuse(emu):
    from deva.inference.unsup_quality import UnsupervisedVideoScorer
    scorer = UnsupervisedVideoScorer()
    with pytest.raises(RuntimeError, match='start_video'):
        scorer.add_frame(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8))
    with pytest.raises(RuntimeError, match='start_video'):
        scorer.end_video()
    scorer.start_video('a', [2, 1, 2])
    assert scorer._ids.tolist() == [1, 2]
    with pytest.raises(RuntimeError, match='end_video'):
        scorer.start_video('b', [1])
    with pytest.raises(ValueError, match=r'gt is \(4, 4\) and pred \(4, 5\)'):
        scorer.add_frame(np.zeros((4, 5), np.uint8), np.zeros((4, 4), np.uint8))
    scorer.add_frame(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8))        # nothing proposed, nothing to find
    scorer.end_video()
    fr = scorer.result()['frames']['a']
    assert fr['proposals'] == [None, None] and fr['J'].tolist() == [[1.0], [1.0]] == fr['F'].tolist()


# ------------------------------------------------------------------------------------------ the limiter
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'unsup_limit.npz')
LIMIT_CASES = {'quirk': ['a'], 'tie': ['a'], 'crowded': ['a', 'b'], 'default': ['a'], 'rgb': ['a']}


def _write_case(golden, name, root):
    for video in LIMIT_CASES[name]:
        os.makedirs(os.path.join(root, video))
        for t, p in enumerate(golden[f'{name}/{video}/in']):
            if bool(golden[f'{name}/rgb']):
                img = Image.fromarray(np.stack([p >> 16, (p >> 8) & 255, p & 255], axis=2).astype(np.uint8))
            else:
                img = Image.fromarray(p.astype(np.uint8), mode='P')
                img.putpalette([v for i in range(256) for v in (i, i, i)])
            img.save(os.path.join(root, video, '%05d.png' % t))


@pytest.mark.parametrize('name', list(LIMIT_CASES))
def test_limiter_against_the_reference_recording(name, tmp_path):
    from deva.inference.unsup_quality import ProposalLimiter, davis_palette, limit_directory
    golden = np.load(GOLDEN)
    limit = int(golden[f'{name}/max'])
    assert {n: int(golden[f'{n}/max']) for n in LIMIT_CASES} == {'quirk': 4, 'tie': 20, 'crowded': 3, 'default': 20, 'rgb': 4}
    _write_case(golden, name, str(tmp_path / 'in'))
    maps = limit_directory(str(tmp_path / 'in'), str(tmp_path / 'out'), limit)
    for video in LIMIT_CASES[name]:
        planes, want = golden[f'{name}/{video}/in'], golden[f'{name}/{video}/out']
        for t in range(len(planes)):
            img = Image.open(tmp_path / 'out' / video / ('%05d.png' % t))
            assert img.mode == 'P' and np.array_equal(np.array(img), want[t]), (video, t)
            assert bytes(img.getpalette()) == bytes(golden['palette'].tolist()) == davis_palette()
        # the online form, fed with areas alone
        online = ProposalLimiter(limit)
        kept = [online.add_frame(dict(zip(*(a.tolist() for a in np.unique(p, return_counts=True))))) for p in planes]
        assert online.mapping() == maps[video]
        for t, p in enumerate(planes):
            relabelled = np.zeros_like(p)
            for old, new in online.mapping().items():
                relabelled[p == old] = new
            assert np.array_equal(relabelled, want[t])
            assert kept[t] <= set(online.mapping())
        assert all(a <= b for a, b in zip(kept, kept[1:]))                  # the kept set only grows


def test_the_quirk_and_its_repair():
    from deva.inference.unsup_quality import ProposalLimiter
    golden = np.load(GOLDEN)
    planes = golden['quirk/a/in']
    areas = [dict(zip(*(a.tolist() for a in np.unique(p, return_counts=True)))) for p in planes]
    as_reference, distinct = ProposalLimiter(4), ProposalLimiter(4, distinct=True)
    for a in areas:
        as_reference.add_frame(a)
        distinct.add_frame(a)
    assert as_reference.listed == [7, 3, 7, 3] and as_reference.mapping() == {7: 3, 3: 4} and as_reference.full
    assert distinct.listed == [7, 3, 9] and distinct.mapping() == {7: 1, 3: 2, 9: 3} and not distinct.full
    # five objects in every frame: the list of 20 is full after four frames and a sixth is never kept
    five = ProposalLimiter()
    for t in range(6):
        kept = five.add_frame({k: 10 + k for k in range(1, 6)} if t < 5 else {k: 10 + k for k in range(1, 7)})
    assert kept == {1, 2, 3, 4, 5} and sorted(five.mapping().values()) == [16, 17, 18, 19, 20]
    # the tie: equal areas go by label, the larger first
    tie = ProposalLimiter()
    tie.add_frame({2: 12, 5: 12, 4: 12, 1: 6, 0: 50})
    assert tie.listed == [5, 4, 2, 1]
    # where the two agree: no label ever repeats
    for d in (False, True):
        lim = ProposalLimiter(3, distinct=d)
        lim.add_frame({1: 4, 2: 24, 3: 20, 4: 6, 5: 12})
        assert lim.mapping() == {2: 1, 3: 2, 5: 3}


def test_score_directory(videos, emu, tmp_path):
    from deva.inference.unsup_quality import UnsupervisedVideoScorer, score_directory
    for name in ('perm', 'split'):
        gts, preds, ids = videos[name]
        for kind, planes in (('truth', gts), ('run', preds)):
            os.makedirs(tmp_path / kind / name)
            for t, plane in enumerate(planes):
                img = Image.fromarray(plane.astype(np.uint8), mode='P' if kind == 'truth' else 'L')
                if kind == 'truth':        # (a palette-less P image is remapped on saving)
                    img.putpalette([v for i in range(256) for v in (i, 255 - i, (7 * i) % 256)])
                img.save(tmp_path / kind / name / ('%05d.png' % t))
    offline = score_directory(str(tmp_path / 'run'), str(tmp_path / 'truth'))
    online = _feed(UnsupervisedVideoScorer(), videos, ['perm', 'split'])
    assert offline['global'] == online['global'] and offline['sequences'] == online['sequences']
    assert offline['frames']['split']['assignment'] == online['frames']['split']['assignment']
    # an RGB-coded run: ids beyond a byte
    gts, preds, ids = videos['perm']
    os.makedirs(tmp_path / 'rgb' / 'perm')
    for t, p in enumerate(preds):
        p = PC.rename(p, [31, 7, 19], [70000, 300, 65536])
        Image.fromarray(np.stack([p >> 16, (p >> 8) & 255, p & 255], axis=2).astype(np.uint8)).save(tmp_path / 'rgb' / 'perm' / ('%05d.png' % t))
    rgb = score_directory(str(tmp_path / 'rgb'), str(tmp_path / 'truth'), ['perm'])
    assert rgb['frames']['perm']['assignment'] == {1: 70000, 2: 300, 3: 65536}
    assert np.array_equal(rgb['frames']['perm']['J'], online['frames']['perm']['J'])
