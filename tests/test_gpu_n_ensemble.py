"""Test-time ensemble kernels (csrc/ensemble.hip) and `EnsembleInferenceCore` on the device: `scores_u8`,
`ensemble_index_mask` and `flip_w` against the CPU restatement of the reference protocol (tests/ensemble_case.py),
the identities with the single-run tail `index_mask`, and the smoke clip end to end against the composition of
per-variant oracle runs.  With DEVA_TEST_DRYRUN=1 the same code runs on the CPU contracts (tests/emu_ensemble.py)."""
import os

import pytest
import torch

import ensemble_case as EC
import gpu_util
from deva.hip import ops
from gpu_util import to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        import emu_ensemble
        emu_ensemble.install(monkeypatch)
        monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)


def _soft(g, c, h, w):
    p = torch.softmax(torch.randn(c, h, w, generator=g) * 2, dim=0)
    p[:, :3, :5] = 1.0 / c  # exact ties: the first maximum must win
    return p


def _lut(c):
    return torch.tensor([0] + [100 + 7 * i for i in range(1, c)], dtype=torch.int64)


def _own_merge(vols, lut):
    """lut[argmax(sum of the kernel's own bytes)] in torch, on the bytes' device"""
    total = sum(v.to(torch.int32) for v in vols)
    return lut.to(total.device)[torch.argmax(total, dim=0)]


# the shape list of test_index_mask_resize_argmax_lut (tests/test_gpu_c_bank.py)
SHAPES = [(3, 40, 56, None), (6, 480, 864, (1080, 1920)), (2, 33, 47, (97, 61)), (4, 96, 128, (48, 64)),
          (1, 8, 8, (20, 20))]


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('c,h,w,size', SHAPES)
def test_scores_u8_against_the_restatement(c, h, w, size, flip):
    """bit-equal without a resize; with one a byte may differ by 1, and only where 255 * r_cpu lies within 255e-6 of an
    integer (the 1e-6 tie margin on resized probabilities of test_index_mask_resize_argmax_lut, times 255)"""
    g = torch.Generator().manual_seed(c * 1000 + h)
    prob = _soft(g, c, h, w)
    got = ops.scores_u8(to_dev(prob), size, flip)
    differing, total = EC.check_bytes(got, prob, size, flip)
    print(f'scores_u8 {c}x{h}x{w} -> {size} flip={flip}: {differing} of {total} bytes differ from the CPU restatement')


SOURCE_SIZES = [None, (24, 32), (40, 56), (33, 47), (64, 90), (17, 90), (50, 31), (96, 128)]  # None: the output size


def _mixed_variants(g, k, c, out):
    """k sources of mixed sizes (the first at the output size; every third an un-padded view of a padded tensor: rows
    and planes strided) and mixed flips -> (device tensors, the same on the CPU, flips)"""
    dev_probs, cpu_probs, flips = [], [], []
    for i in range(k):
        h, w = SOURCE_SIZES[i] or out
        p = _soft(g, c, h, w)
        if i % 3 == 1:
            padded = torch.zeros(c, h + 5, w + 7)
            padded[:, 2:2 + h, 3:3 + w] = p
            dev_probs.append(to_dev(padded)[:, 2:2 + h, 3:3 + w])
        else:
            dev_probs.append(to_dev(p))
        cpu_probs.append(p)
        flips.append(i % 2 == 1 or i == 4)
    return dev_probs, cpu_probs, flips


CASES = [(1, 7, (37, 52)), (2, 2, (45, 61)), (5, 7, (64, 90)), (8, 1, (30, 44)), (8, 7, (50, 63)), (5, 2, (33, 48))]


@pytest.mark.parametrize('k,c,out', CASES)
def test_quantised_merge_equals_the_sum_of_its_own_bytes(k, c, out):
    """ensemble_index_mask(quantize=True) == lut[argmax(sum_k scores_u8(variant k))] from the kernel's own bytes, bit for
    bit (integer sums, first maximum); against the CPU restatement a label may differ only where moving every byte
    whose 255 * r_cpu is within 255e-6 of an integer by one makes it a first maximum"""
    g = torch.Generator().manual_seed(100 * k + c)
    dev_probs, cpu_probs, flips = _mixed_variants(g, k, c, out)
    lut = _lut(c)
    vols = [ops.scores_u8(p, out, f) for p, f in zip(dev_probs, flips)]
    got = ops.ensemble_index_mask(dev_probs, out, flips, to_dev(lut))
    assert got.dtype == torch.int64 and tuple(got.shape) == tuple(out)
    assert torch.equal(got, _own_merge(vols, lut))
    idx = ops.ensemble_index_mask(dev_probs, out, flips)  # no table: channel indices
    assert torch.equal(got.cpu(), lut[idx.cpu()])
    for v, p, f in zip(vols, cpu_probs, flips):
        EC.check_bytes(v, p, out, f)
    differing = EC.check_labels_attainable(idx, cpu_probs, out, flips)
    print(f'K={k} C={c} -> {out}: {differing} labels differ from the CPU restatement (all attainable)')


@pytest.mark.parametrize('c,h,w,size', SHAPES)
def test_one_fp32_variant_is_the_single_run_tail(c, h, w, size):
    """K = 1, quantize=False: index_mask bit for bit; flipped: its mirror image"""
    g = torch.Generator().manual_seed(c * 1000 + h)
    prob, lut = to_dev(_soft(g, c, h, w)), to_dev(_lut(c))
    out = (h, w) if size is None else size
    want = ops.index_mask(prob, size, lut)
    assert torch.equal(ops.ensemble_index_mask([prob], out, [False], lut, quantize=False), want)
    assert torch.equal(ops.ensemble_index_mask([prob], out, [True], lut, quantize=False), want.flip(-1))


def test_fp32_merge_sums_in_variant_order():
    """quantize=False against the CPU contract; a differing label only where the summed top-2 margin is within
    2K * 1e-6 (the 1e-6 tie margin on one resized probability, K of them on each of two channels)"""
    import emu_ensemble
    g = torch.Generator().manual_seed(7)
    out, k, c = (45, 62), 5, 4
    dev_probs, cpu_probs, flips = _mixed_variants(g, k, c, out)
    got = ops.ensemble_index_mask(dev_probs, out, flips, quantize=False).cpu()
    total = sum(EC.resized(p, out, f) for p, f in zip(cpu_probs, flips))
    want = emu_ensemble.ensemble_index_mask(cpu_probs, out, flips, quantize=False)
    diff = got != want
    if diff.any():
        top2 = total.topk(2, dim=0)[0]
        assert (top2[0] - top2[1])[diff].max().item() <= 2 * k * 1e-6


@pytest.mark.parametrize('shape,dtype', [((37, 53, 3), torch.uint8), ((5, 31), torch.uint8), ((3, 17, 29), torch.float32),
                                         ((33, 47), torch.int64), ((1, 1), torch.int64), ((480, 854, 3), torch.uint8)])
def test_flip_w(shape, dtype):
    """1-, 3-, 4- and 8-byte elements, odd widths: torch.flip bit for bit, nothing written outside the destination"""
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(shape, generator=g) if dtype.is_floating_point
         else torch.randint(0, 200, shape, generator=g).to(dtype))
    frame = dtype == torch.uint8 and len(shape) == 3
    want = torch.flip(x, dims=[1] if frame else [-1])
    got = ops.flip_w(to_dev(x))
    assert got.dtype == dtype and torch.equal(got.cpu(), want)
    if DRYRUN:
        return
    # the C entry point into the middle of a sentinel-filled buffer
    from deva.hip import check, lib
    nbytes = x.numel() * x.element_size()
    guard = 256
    buf = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=gpu_util.dev())
    src = to_dev(x)
    rows, width, elem = (shape[0], shape[1], 3) if frame else (x.numel() // shape[-1], shape[-1], x.element_size())
    check(lib().deva_flip_w(src.data_ptr(), buf.data_ptr() + guard, rows, width, elem, ops._stream()), 'deva_flip_w')
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:guard] == 0xA5).all()) and bool((host[guard + nbytes:] == 0xA5).all())
    assert torch.equal(host[guard:guard + nbytes], want.contiguous().view(-1).view(torch.uint8))


def test_wrapper_errors():
    from deva.hip import DevaHipError
    g = torch.Generator().manual_seed(3)
    a, b = to_dev(_soft(g, 3, 8, 8)), to_dev(_soft(g, 4, 8, 8))
    with pytest.raises(DevaHipError):
        ops.ensemble_index_mask([a, b], (8, 8), [False, False])      # channel counts differ
    with pytest.raises(DevaHipError):
        ops.ensemble_index_mask([a] * 9, (8, 8), [False] * 9)        # more than 8 variants
    with pytest.raises(DevaHipError):
        ops.ensemble_index_mask([a], (8, 8), [False, True])


def test_full_size_output():
    """480 x 864 and 384 x 688 sources, each with and without the flip -> (1080, 1920), 6 channels: the 16-byte label
    stores and the packed byte stores at full size, contract level"""
    g = torch.Generator().manual_seed(11)
    out, c = (1080, 1920), 6
    cpu_probs = [_soft(g, c, 480, 864), _soft(g, c, 480, 864), _soft(g, c, 384, 688), _soft(g, c, 384, 688)]
    flips = [False, True, False, True]
    probs, lut = [to_dev(p) for p in cpu_probs], _lut(c)
    vols = [ops.scores_u8(p, out, f) for p, f in zip(probs, flips)]
    got = ops.ensemble_index_mask(probs, out, flips, to_dev(lut))
    assert torch.equal(got, _own_merge(vols, lut))
    EC.check_bytes(vols[3], cpu_probs[3], out, True)
    idx = ops.ensemble_index_mask(probs, out, flips)
    differing = EC.check_labels_attainable(idx, cpu_probs, out, flips)
    print(f'K=4 C=6 -> {out}: {differing} labels differ from the CPU restatement (all attainable)')


# ------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def oracle(peaky_state_dict):
    return EC.oracle_composition(peaky_state_dict)


@pytest.mark.parametrize('mode', ['fp32', 'f16_split'])
def test_ensemble_core_matches_oracle_composition(mode, oracle, peaky_state_dict):
    """the smoke clip (96 x 128, 3 objects, mem_every=2, 4 frames, peaky recipe) at the native size and at 120, each
    with and without the flip (K = 4), on the HIP library -- fp32 and --f16_split --f16_split_key_encoder -- against
    one oracle run per variant merged by the protocol restatement (ensemble_case.check_end_to_end: (i) bytes within 1,
    (ii) mask == lut[argmax(sum of the returned bytes)], (iii) mask == the oracle's where its summed top-2 margin
    exceeds 2K, at most 15 % of a frame left out, (iv) the tmp -> object mapping)"""
    from deva.model.network import DEVA
    extra = dict(f16_split=True, f16_split_key_encoder=True) if mode == 'f16_split' else {}
    net = DEVA(EC.clip_config(**extra))
    net.load_weights(peaky_state_dict)
    net = net.to(gpu_util.dev()).eval()
    masks, scores, core = EC.run_ensemble(net, gpu_util.dev())
    EC.check_end_to_end(masks, scores, core, oracle, mode)
