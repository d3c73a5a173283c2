"""The JPEG coder (csrc/jpeg/jpeg_encode.hip) on the device against the numpy statement of rules J1-J10
(tests/jpeg_case.py): byte for byte, `info` included, at the sizes around the MCU, at block counts around the 256 blocks
an interval's workgroup codes in a step, at restart intervals whose counter wraps, at four qualities on the crafted image
that reaches the corners of the code space, at every base alignment, into sentinel-poisoned outputs from a poisoned
scratch; the overflow path; the worst-case capacity; whole frames through `PIL.Image.open` against PIL's own files; and
`FrameResultSaver(jpeg='device')` end to end from `DEVAInferenceCore.step` against `jpeg='host'`.

Every byte-for-byte case goes through `_device_scan`: its scratch and its output are poisoned, the output has a guard
band behind `capacity`, and the band must come back untouched."""
import functools
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import emu_jpeg as EJPEG
import emu_png as EPNG
import gpu_util
import jpeg_case as JC
from deva.hip import jpeg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
GUARD = 256
SUBS = ('4:2:0', '4:4:4')


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        import emu_frame_result
        emu_frame_result.install(monkeypatch)
        EPNG.install(monkeypatch)
        EJPEG.install(monkeypatch)


def _on_device(plane, shift=0):
    """the plane on the device, its first byte `shift` bytes behind a 256-byte boundary"""
    flat = torch.from_numpy(np.ascontiguousarray(plane)).reshape(-1)
    buf = torch.empty(flat.numel() + 256, dtype=torch.uint8, device=gpu_util.dev())
    at = (-buf.data_ptr()) % 256 + shift if buf.is_cuda else shift
    buf[at:at + flat.numel()] = flat.to(buf.device)
    return buf[at:at + flat.numel()].view(*plane.shape)


def _device_scan(plane, quality=75, subsampling='4:2:0', restart=0, capacity=None, poison=0xA5, shift=0, out_shift=0):
    """deva_jpeg_scan on poisoned buffers -> (out[:min(total, capacity)] as bytes, info as a list); asserts J10's capacity"""
    dev = gpu_util.dev()
    h, w = plane.shape[:2]
    p = jpeg.plan(h, w, subsampling, restart)
    room = p.worst_case if capacity is None else capacity
    scratch = torch.full((p.scratch_bytes,), poison, dtype=torch.uint8, device=dev)
    whole = torch.full((out_shift + room + GUARD,), poison ^ 0xFF, dtype=torch.uint8, device=dev)
    out = whole[out_shift:out_shift + room + GUARD]
    info = torch.full((4,), -1, dtype=torch.int64, device=dev)
    jpeg._launch_scan(_on_device(plane, shift), h, w, quality, jpeg.SUBSAMPLINGS[subsampling], restart, scratch, out, room, info)
    info = info.cpu().tolist()
    host = whole.cpu().numpy()
    assert (host[:out_shift] == poison ^ 0xFF).all() and (host[out_shift + room:] == poison ^ 0xFF).all(), 'a byte at or beyond capacity changed'
    return host[out_shift:out_shift + min(info[0], room)].tobytes(), info


def _equals_the_statement(plane, quality=75, subsampling='4:2:0', restart=0, **kw):
    want, info = JC.scan(plane, quality, subsampling, restart)
    got, got_info = _device_scan(plane, quality, subsampling, restart, **kw)
    assert got_info == info, (got_info, info)
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        first = int(np.nonzero(a != b)[0][0])
        pytest.fail(f'{int((a != b).sum())} of {len(want)} bytes differ, the first at {first}: {got[first:first + 8].hex()} vs {want[first:first + 8].hex()}')
    return got, got_info


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, (*shape, 3)).astype(np.uint8)


def _picture(shape, seed):
    """half overlay, half noise: long runs of zeros and blocks with many coefficients in one picture"""
    image = JC.overlay(*shape, seed)
    noise = _noise(shape, seed + 1)
    image[:, shape[1] // 2:] = noise[:, shape[1] // 2:]
    return image


# ------------------------------------------------------------------------------------------ byte for byte
@pytest.mark.parametrize('subsampling', SUBS)
@pytest.mark.parametrize('shape', [(1, 1), (7, 9)] + [(h, w) for h in (15, 16, 17) for w in (15, 16, 17)] + [(33, 47)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_shapes_around_the_mcu(shape, subsampling):
    """J2: a picture that ends before, on and after an MCU's edge, in both directions"""
    _equals_the_statement(_picture(shape, 10 + shape[0] + shape[1]), 75, subsampling)
    _equals_the_statement(_noise(shape, 11), 100, subsampling, restart=1)


STEP_CASES = [('4:4:4', (8, 2040), 0, 765), ('4:4:4', (8, 2048), 0, 768), ('4:4:4', (8, 2056), 0, 771), ('4:4:4', (8, 2048), 85, 255),
              ('4:4:4', (8, 2048), 86, 258), ('4:2:0', (16, 2032), 0, 762), ('4:2:0', (16, 2048), 0, 768), ('4:2:0', (16, 2064), 0, 774),
              ('4:2:0', (16, 2048), 42, 252), ('4:2:0', (16, 2048), 43, 258)]


@pytest.mark.parametrize('subsampling,shape,restart,blocks', STEP_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_blocks_per_interval_around_the_workgroups_step(subsampling, shape, restart, blocks):
    """a lane owns a block and a workgroup codes 256 a step: intervals that end just before, on and just behind a step
    (252, 255, 258 blocks; 762 .. 774 around three steps).  Noise at quality 95: a step's bytes take several stuffing
    passes, and bits are carried from step to step"""
    p = jpeg.plan(*shape, subsampling, restart)
    assert p.block == 256 and p.restart * p.blocks_per_mcu == blocks
    image = _noise(shape, 20 + blocks)
    got, _ = _equals_the_statement(image, 95, subsampling, restart)
    print(f'{len(got) / p.blocks:.1f} bytes a block')
    assert len(got) > 32 * p.blocks      # more than 8192 bytes a step of 256 blocks: at least two stuffing passes of 4096
    _equals_the_statement(_picture(shape, 21 + blocks), 50, subsampling, restart)


@pytest.mark.parametrize('subsampling', SUBS)
def test_restart_intervals(subsampling):
    """`restart` 1, 3, 0 and the whole image, with 8, 9 and 17 intervals: the marker's counter stops short of, reaches and
    passes its wrap"""
    side = 16 if subsampling == '4:2:0' else 8
    for mcus_x, mcus_y, restart, intervals in ((4, 2, 1, 8), (3, 3, 1, 9), (17, 1, 1, 17), (6, 4, 3, 8), (9, 3, 3, 9), (3, 8, 0, 8),
                                               (3, 9, 0, 9), (2, 17, 0, 17), (5, 4, 20, 1), (5, 4, 65535, 1), (5, 5, 3, 9)):
        shape = (mcus_y * side - 3, mcus_x * side - 5)
        assert jpeg.plan(*shape, subsampling, restart).intervals == intervals
        got, info = _equals_the_statement(_picture(shape, 30 + intervals), 75, subsampling, restart)
        assert info[3] == intervals and sum(got.count(bytes([0xFF, 0xD0 + m])) for m in range(8)) >= intervals - 1


@functools.lru_cache(maxsize=None)
def _crafted():
    return JC.crafted()


@pytest.mark.parametrize('subsampling', SUBS)
@pytest.mark.parametrize('quality', [1, 50, 75, 100])
def test_qualities_on_the_crafted_image(quality, subsampling):
    """tests/test_jpeg_cpu.py asserts what this image holds at quality 100: DC category 11, AC category 10, ZRL, blocks
    without EOB, stuffed FFs, more than 8 intervals"""
    got, info = _equals_the_statement(_crafted(), quality, subsampling)
    assert info[3] > 8
    file = jpeg.file_bytes(got, *_crafted().shape[:2], quality=quality, subsampling=subsampling)
    assert file == JC.file_bytes(got, *_crafted().shape[:2], quality, subsampling, 0)
    assert JC.psnr(np.array(Image.open(io.BytesIO(file))), _crafted()) > (35 if quality == 100 else 8)


@pytest.mark.parametrize('shift', range(1, 16))
def test_base_addresses_off_by_1_to_15_bytes(shift):
    plane = _picture((19, 150), 40)
    want = _equals_the_statement(plane, 90)[0]
    assert _equals_the_statement(plane, 90, shift=shift, out_shift=16 - shift)[0] == want
    _equals_the_statement(plane[:, :133].copy(), 90, '4:4:4', shift=shift, out_shift=shift)


def test_poisoned_scratch_and_output():
    plane = _picture((40, 70), 50)
    total = len(JC.scan(plane)[0])
    results = [_device_scan(plane, capacity=total + 5, poison=p) for p in (0x00, 0xFF, 0xA5)]
    assert results[0] == results[1] == results[2] and results[0][0] == JC.scan(plane)[0]
    results = [_device_scan(plane, capacity=total, poison=p) for p in (0x00, 0xFF)]      # exactly full: no overflow
    assert results[0] == results[1] and results[0][1][2] == 0 and results[0][0] == JC.scan(plane)[0]


# ------------------------------------------------------------------------------------------ overflow, capacity
def test_overflow_sets_the_flag_and_finish_still_returns_the_file():
    plane = _picture((120, 200), 5)
    want, info = JC.scan(plane)
    cut = len(want) // 2
    got, got_info = _device_scan(plane, capacity=cut)           # (the guard band behind `cut` is checked in there)
    assert got_info == [info[0], info[1], 1, info[3]] and got == want[:cut]
    for cap in (0, 1, 2, 3, len(want) - 1):
        got, got_info = _device_scan(plane, capacity=cap)
        assert got_info[0] == len(want) and got_info[2] == 1 and got == want[:cap], cap
    pending = jpeg.encode(_on_device(plane), capacity=cut)
    file = pending.finish()
    assert pending.overflowed and pending.total == len(want) and file == JC.file_bytes(want, 120, 200)
    assert np.array(Image.open(io.BytesIO(file))).shape == plane.shape
    fits = jpeg.scan(_on_device(plane), capacity=len(want))
    assert fits.finish() == want and not fits.overflowed and (fits.blocks, fits.intervals) == (info[1], info[3])
    assert jpeg.scan(_on_device(plane)) == want
    assert jpeg.encode(_on_device(plane), quality=30, subsampling='4:4:4', restart=7) == JC.encode(plane, 30, '4:4:4', 7)


@pytest.mark.parametrize('subsampling', SUBS)
def test_the_worst_case_is_a_capacity(subsampling):
    """random bytes at quality 100: the longest data a picture of the size gives in practice stays below the plan's bound"""
    plane = _noise((64, 300), 3)
    worst = JC.plan(64, 300, subsampling)['worst_case']
    assert len(JC.scan(plane, 100, subsampling)[0]) <= worst == jpeg.plan(64, 300, subsampling).worst_case          # on the statement first
    got, info = _equals_the_statement(plane, 100, subsampling)
    assert info[0] <= worst and info[2] == 0
    print(f'{subsampling}: {info[0]} bytes of {worst}')


# ------------------------------------------------------------------------------------------ whole frames
@pytest.mark.parametrize('size', [(480, 854), (1080, 1920)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_whole_frames_through_pil(size):
    """an overlay at the saver's settings: byte for byte the statement, opened by PIL, and within the margins of
    tests/test_jpeg_cpu.py of PIL's own file of the same frame"""
    image = JC.overlay(*size, seed=size[0])
    got, info = _equals_the_statement(image)
    file = jpeg.encode(_on_device(image))
    assert file == JC.file_bytes(got, *size)
    opened = Image.open(io.BytesIO(file))
    assert opened.size == (size[1], size[0]) and opened.mode == 'RGB'
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format='JPEG', quality=75, subsampling='4:2:0', restart_marker_blocks=JC.geometry(*size)[1])
    mine, theirs = JC.psnr(np.array(opened), image), JC.psnr(np.array(Image.open(io.BytesIO(buf.getvalue()))), image)
    print(f'{size}: {len(file)} bytes vs PIL {len(buf.getvalue())}, {mine:.3f} vs {theirs:.3f} dB, {info[3]} intervals')
    assert len(file) <= 1.10 * len(buf.getvalue()) and mine >= theirs - 0.2


# ------------------------------------------------------------------------------------------ end to end
def test_clip_through_the_saver_on_both_jpeg_and_both_png_paths(peaky_state_dict, tmp_path):
    """the smoke-size clip of tests/test_gpu_zg_png.py as a `demo` run: `DEVAInferenceCore.step` -> four savers on the same
    probabilities.  The `jpeg='device'` files are the statement's bytes of the saver's own overlay and decode to within
    0.2 dB of what PIL's files decode to; the PNGs and the JSON do not depend on the JPEG path"""
    import ensemble_case as EC
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    from workload import synth

    def reader(frame_u8):   # the reader's transform of a decoded frame (ToTensor + Normalize), on the host
        mean, std = torch.tensor(EC.MEAN).view(3, 1, 1), torch.tensor(EC.STD).view(3, 1, 1)
        return (frame_u8.permute(2, 0, 1).float() / 255 - mean) / std
    dev = gpu_util.dev()
    net = DEVA(EC.clip_config())
    net.load_weights(peaky_state_dict)
    core = DEVAInferenceCore(net.to(dev).eval(), EC.clip_config())
    om = core.object_manager
    om.use_long_id = True
    wanted = [70000, 66051]
    overlays = []
    modes = [(p, j) for p in ('host', 'device') for j in ('host', 'device')]
    savers = {(p, j): FrameResultSaver(str(tmp_path / f'{p}_{j}'), 'clip', dataset='demo', object_manager=om, png=p, jpeg=j,
                                       frame_hook=(lambda name, result, ann: overlays.append(result.blend.cpu().numpy())) if (p, j) == modes[0] else None)
              for p, j in modes}
    mask = torch.tensor([0] + wanted)[synth.box_mask(EC.H, EC.W, 2)]
    for t, frame in enumerate(EC.clip_frames()[:3]):
        prob = core.step(reader(frame).to(dev), mask.to(dev) if t == 0 else None, wanted if t == 0 else None)
        for saver in savers.values():
            saver.save_mask(prob, f'{t:05d}.jpg', image_np=frame.numpy())
    for saver in savers.values():
        saver.end()
        assert saver.queue.empty() and not saver.thread.is_alive() and saver.error is None
    files = lambda mode: sorted(os.path.relpath(os.path.join(b, f), tmp_path / mode) for b, _, fs in os.walk(tmp_path / mode) for f in fs)
    assert len(overlays) == 3
    for p, j in modes:
        assert files(f'{p}_{j}') == files('host_host') and len(files('host_host')) == 6
        assert savers[(p, j)].video_json == savers[modes[0]].video_json
        assert (savers[(p, j)].jpeg_largest > 0) == (j == 'device') and (savers[(p, j)].png_largest > 0) == (p == 'device')
        for t in range(3):
            png_file = Image.open(tmp_path.joinpath(f'{p}_{j}', 'Annotations', 'clip', f'{t:05d}.png'))
            assert np.array_equal(np.array(png_file), np.array(Image.open(tmp_path.joinpath('host_host', 'Annotations', 'clip', f'{t:05d}.png'))))
            data = open(tmp_path.joinpath(f'{p}_{j}', 'Visualizations', 'clip', f'{t:05d}.jpg'), 'rb').read()
            host_data = open(tmp_path.joinpath('host_host', 'Visualizations', 'clip', f'{t:05d}.jpg'), 'rb').read()
            if j == 'host':
                assert data == host_data
                continue
            assert data == JC.encode(overlays[t])
            mine, theirs = (JC.psnr(np.array(Image.open(io.BytesIO(d))), overlays[t]) for d in (data, host_data))
            print(f'png={p} frame {t}: {len(data)} bytes vs PIL {len(host_data)}, {mine:.3f} vs {theirs:.3f} dB')
            assert mine >= theirs - 0.2
    assert savers[('host', 'device')].jpeg_capacity == 2 * savers[('host', 'device')].jpeg_largest
