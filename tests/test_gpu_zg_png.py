"""The PNG coder (csrc/png/png_encode.hip) on the device against the numpy statement of rules Z1-Z8 (tests/png_case.py):
byte for byte, `info` included, at the sizes where the walk changes (a row string that ends on, before and after a
1024-byte step; segment counts around R), on runs of the lengths where Z3 changes its tokens, at every base alignment,
into sentinel-poisoned outputs from a poisoned scratch; at full-frame sizes against zlib and PIL; the overflow path; and
`FrameResultSaver(png='device')` end to end from `DEVAInferenceCore.step` against `png='host'`.

Every byte-for-byte case goes through `_device_stream`: its scratch and its output are poisoned, the output has a guard
band behind `capacity`, and the band must come back untouched."""
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import emu_png as EPNG
import gpu_util
import png_case as PC
from deva.hip import png

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
GUARD = 256


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        import emu_frame_result
        emu_frame_result.install(monkeypatch)
        EPNG.install(monkeypatch)


def _on_device(plane, shift=0):
    """the plane on the device, its first byte `shift` bytes behind a 256-byte boundary"""
    flat = torch.from_numpy(np.ascontiguousarray(plane)).reshape(-1)
    buf = torch.empty(flat.numel() + 256, dtype=torch.uint8, device=gpu_util.dev())
    at = (-buf.data_ptr()) % 256 + shift if buf.is_cuda else shift
    buf[at:at + flat.numel()] = flat.to(buf.device)
    return buf[at:at + flat.numel()].view(*plane.shape)


def _device_stream(plane, capacity=None, poison=0xA5, shift=0, out_shift=0):
    """deva_png_deflate on poisoned buffers -> (out[:min(total, capacity)] as bytes, info as a list); asserts Z7"""
    dev = gpu_util.dev()
    h, w = plane.shape[:2]
    bpp = 3 if plane.ndim == 3 else 1
    p = png.plan(h, w, bpp)
    room = p.worst_case if capacity is None else capacity
    scratch = torch.full((p.scratch_bytes,), poison, dtype=torch.uint8, device=dev)
    whole = torch.full((out_shift + room + GUARD,), poison ^ 0xFF, dtype=torch.uint8, device=dev)
    out = whole[out_shift:out_shift + room + GUARD]
    info = torch.full((4,), -1, dtype=torch.int64, device=dev)
    png._launch_deflate(_on_device(plane, shift), h, w, bpp, scratch, out, room, info)
    info = info.cpu().tolist()
    host = whole.cpu().numpy()
    assert (host[:out_shift] == poison ^ 0xFF).all() and (host[out_shift + room:] == poison ^ 0xFF).all(), 'a byte at or beyond capacity changed'
    return host[out_shift:out_shift + min(info[0], room)].tobytes(), info


def _equals_the_statement(plane, **kw):
    want, info = PC.stream(plane)
    got, got_info = _device_stream(plane, **kw)
    assert got_info == info, (got_info, info)
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        first = int(np.nonzero(a != b)[0][0])
        pytest.fail(f'{int((a != b).sum())} of {len(want)} bytes differ, the first at {first}: {got[first:first + 8].hex()} vs {want[first:first + 8].hex()}')
    assert zlib.decompress(got) == PC.row_strings(plane).tobytes()
    return got, got_info


def _few_values(shape, seed, values=(0, 0, 0, 0, 1, 2, 143, 144, 255)):
    """planes whose filtered rows hold runs: few values, drawn per pixel"""
    rng = np.random.default_rng(seed)
    return np.asarray(values, dtype=np.uint8)[rng.integers(0, len(values), shape)]


# ------------------------------------------------------------------------------------------ byte for byte
@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (3, 1022), (3, 1023), (3, 1024), (3, 1025), (3, 341, 3), (3, 342, 3), (2, 2047), (2, 2048)])
def test_sizes_around_a_step(shape):
    """a row string of n + 1 bytes ends before, on and after a 1024-byte step"""
    assert [png.plan(1, w, b).steps_per_row for w, b in ((1022, 1), (1023, 1), (1024, 1), (341, 3), (342, 3))] == [1, 1, 2, 1, 2]
    _equals_the_statement(_few_values(shape, 11))
    _equals_the_statement(np.random.default_rng(12).integers(0, 256, shape).astype(np.uint8))


def test_segment_counts_around_r():
    r = png.plan(1, 1).rows_per_segment
    assert r == PC.R
    for h in (r - 1, r, r + 1, 2 * r + 1):
        _, info = _equals_the_statement(_few_values((h, 37), 20 + h))
        assert info[3] == -(-h // r)


@pytest.mark.parametrize('width', [2100, 3000])
def test_run_lengths_where_the_tokens_change(width):
    """rows made of runs of 1, 2, 3, 4, 258 .. 262, 516, 517 and 519 bytes: the literal, 1 and 2 more literals, the shortest
    match, a full match and what follows it; at these widths many of them span two steps"""
    plane = PC.run_rows(width)
    strings = PC.row_strings(plane)
    for k, m in enumerate((1, 2, 3, 4, 258, 259, 260, 261, 262, 516, 517, 519), start=1):
        _, lengths, _ = PC.runs(strings[k:k + 1])
        assert (lengths[1:-1] == m).all() and lengths.size > 2, m
    _equals_the_statement(plane)


def test_a_run_that_spans_two_steps_and_one_that_spans_a_row():
    plane = np.zeros((4, 2600), dtype=np.uint8)
    plane[0, 1000:1100] = 7         # strings 1001 .. 1100: across the first step's end
    plane[1, 1000:1100] = 7
    plane[1, 5:2590] = 200          # a run of 2585 bytes over three steps, 9-bit literals
    plane[2] = 9                    # the whole row after the filter byte
    _equals_the_statement(plane)


def test_an_all_zero_plane():
    got, info = _equals_the_statement(np.zeros((480, 854), dtype=np.uint8))
    assert info[0] == PC.stream_size(np.zeros((480, 854), dtype=np.uint8))


def test_first_data_byte_2_joins_the_filter_byte_and_values_around_143():
    plane = np.zeros((6, 40), dtype=np.uint8)
    plane[0, :5] = 2                                   # row string 02 02 02 02 02 02 00 ..: one run of six
    plane[1, 0] = 4                                    # 4 - 2 = 2 again, then 0 - 2 = 254
    plane[2, :] = np.arange(124, 164, dtype=np.uint8)  # both sides of 143 / 144
    plane[3, :] = 143
    plane[4, :] = 31                                   # 31 - 143 = 144
    values, lengths, _ = PC.runs(PC.row_strings(plane)[:1])
    assert values[0] == 2 and lengths[0] == 6
    _equals_the_statement(plane)


def test_the_worst_case_is_a_capacity():
    plane = np.random.default_rng(3).integers(0, 256, (64, 300)).astype(np.uint8)
    worst = PC.plan(64, 300, 1)['worst_case']
    assert len(PC.stream(plane)[0]) <= worst == png.plan(64, 300, 1).worst_case          # on the statement first
    got, info = _equals_the_statement(plane)
    assert info[0] <= worst and info[2] == 0


@pytest.mark.parametrize('shift', range(1, 16))
def test_base_addresses_off_by_1_to_15_bytes(shift):
    plane = _few_values((9, 1100), 40)
    want = _equals_the_statement(plane)[0]
    assert _equals_the_statement(plane, shift=shift, out_shift=16 - shift)[0] == want
    rgb = _few_values((9, 400, 3), 41)
    _equals_the_statement(rgb, shift=shift)


def test_poisoned_scratch_and_output():
    plane = _few_values((20, 700), 50)
    total = len(PC.stream(plane)[0])
    results = [_device_stream(plane, capacity=total + 5, poison=p) for p in (0x00, 0xFF, 0xA5)]
    assert results[0] == results[1] == results[2] and results[0][0] == PC.stream(plane)[0]
    results = [_device_stream(plane, capacity=total, poison=p) for p in (0x00, 0xFF)]      # exactly full: no overflow
    assert results[0] == results[1] and results[0][1][2] == 0 and results[0][0] == PC.stream(plane)[0]


# ------------------------------------------------------------------------------------------ full frames
@pytest.mark.parametrize('rgb', [False, True])
@pytest.mark.parametrize('size', [(1080, 1920), (2160, 3840)])
def test_full_frames_against_zlib_and_pil(size, rgb):
    plane = PC.blobs(*size, objects=14, seed=size[0], rgb=rgb)
    assert len(np.unique(plane.reshape(-1, 3 if rgb else 1), axis=0)) >= 10
    got, info = _device_stream(plane)
    assert zlib.decompress(got) == PC.row_strings(plane).tobytes()
    assert info[0] == len(got) == PC.stream_size(plane) and info[1] == zlib.adler32(PC.row_strings(plane).tobytes())
    assert info[2] == 0 and info[3] == -(-size[0] // PC.R)
    palette = None if rgb else bytes(range(256)) * 3
    file = png.encode(_on_device(plane), palette=palette)
    assert file == png.file_bytes(got, *size, 3 if rgb else 1, palette)
    image = Image.open(io.BytesIO(file))
    assert image.mode == ('RGB' if rgb else 'P') and np.array_equal(np.array(image), plane)
    if not rgb:
        assert bytes(image.getpalette()[:768]) == palette
    print(f'{size} rgb={rgb}: {len(file)} bytes')


# ------------------------------------------------------------------------------------------ overflow
def test_overflow_sets_the_flag_and_finish_still_returns_the_file():
    plane = PC.blobs(120, 200, objects=6, seed=5)
    want, info = PC.stream(plane)
    cut = len(want) // 2
    got, got_info = _device_stream(plane, capacity=cut)           # (the guard band behind `cut` is checked in there)
    assert got_info == [info[0], info[1], 1, info[3]] and got == want[:cut]
    for cap in (0, 1, 2, 3, len(want) - 6, len(want) - 1):
        got, got_info = _device_stream(plane, capacity=cap)
        assert got_info[0] == len(want) and got_info[2] == 1 and got == want[:cap], cap
    pending = png.encode(_on_device(plane), capacity=cut)
    file = pending.finish()
    assert pending.overflowed and pending.total == len(want) and file == png.file_bytes(want, 120, 200)
    assert np.array_equal(np.array(Image.open(io.BytesIO(file))), plane)
    fits = png.deflate(_on_device(plane), capacity=len(want))
    assert fits.finish() == want and not fits.overflowed
    assert png.deflate(_on_device(plane)) == want


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('dataset', ['demo', 'burst'])
def test_clip_through_the_saver_on_both_png_paths(dataset, peaky_state_dict, tmp_path):
    """the smoke-size clip of tests/test_gpu_o_frame_result.py: `DEVAInferenceCore.step` -> two savers on the same
    probabilities; the files of `png='device'` decode to what those of `png='host'` decode to, and the JSON is the same"""
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
    long_id = dataset == 'demo'
    om.use_long_id = long_id
    wanted = [70000, 66051] if long_id else [1, 2]
    palette = None if long_id else bytes(range(255, -1, -1)) * 3
    savers = {mode: FrameResultSaver(str(tmp_path / mode), 'clip', dataset=dataset, object_manager=om, palette=palette, png=mode)
              for mode in ('host', 'device')}
    mask = torch.tensor([0] + wanted)[synth.box_mask(EC.H, EC.W, 2)]
    for t, frame in enumerate(EC.clip_frames()[:3]):
        prob = core.step(reader(frame).to(dev), mask.to(dev) if t == 0 else None, wanted if t == 0 else None)
        for saver in savers.values():
            saver.save_mask(prob, f'{t:05d}.jpg', image_np=frame.numpy())
    for saver in savers.values():
        saver.end()
        assert saver.queue.empty() and not saver.thread.is_alive() and saver.error is None
    assert savers['host'].video_json == savers['device'].video_json
    assert savers['device'].png_largest > 0 and savers['device'].png_capacity == 2 * savers['device'].png_largest
    sub = ('Annotations', 'clip') if dataset == 'demo' else ('clip',)
    for t in range(3):
        a = Image.open(tmp_path.joinpath('host', *sub, f'{t:05d}.png'))
        b = Image.open(tmp_path.joinpath('device', *sub, f'{t:05d}.png'))
        assert a.mode == b.mode == ('RGB' if long_id else 'P') and np.array_equal(np.array(a), np.array(b))
        assert len(np.unique(np.array(b).reshape(-1, 3 if long_id else 1), axis=0)) == 3
        if not long_id:
            assert a.getpalette() == b.getpalette()
    files = lambda mode: sorted(os.path.relpath(os.path.join(b, f), tmp_path / mode) for b, _, fs in os.walk(tmp_path / mode) for f in fs)
    assert files('host') == files('device')
