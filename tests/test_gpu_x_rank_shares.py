"""The N-rank halves of the sharded memory read on the HIP kernels, every rank played in turn by ONE process on one device
(no torch.distributed: `shard_values(rank, world)` takes plain integers, the row maps are ordinary tensors and the
collectives in between are sums and concatenations the test does itself).  What the 1-rank RCCL tests cannot reach --
row maps with -1 entries, arenas that hold a subset, a rank without rows, the ragged K of one rank's prototype GEMM, token
shards large enough for the fp16 pre-filter -- runs here for W = 2, 3, 8; RCCL itself does not.

Bounds, all asserted elsewhere in this suite for the same operation: read-out against fp64 1e-4 * max(1, |ref|max)
(test_against_reference_golden); partial read-outs summed against the unsharded read-out 1e-5 * max(1,
|full|max) (test_token_sharded_read_merges_to_the_unsharded_result); prototype GEMM 1e-5 * max(1, |ref|max)
(test_similarity_dense_and_softmax_columns).  Helpers, ownership and references: tests/rank_shares.py."""
import functools
import os

import pytest
import torch

import rank_shares as RS
from deva.hip import ops
from gpu_util import dev, max_err, to_dev
from workload import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# bit-identity across differently shaped launches is a property of the kernels, not of the PyTorch emulation of the dry run
kernel_property = pytest.mark.skipif(os.environ.get('DEVA_TEST_DRYRUN') == '1',
                                     reason='checks a property of the HIP kernels; the dry run emulates them')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case_id(shape):
    return 'hw{}-k{}-cv{}-long{}-work{}-W{}'.format(*shape)


# ------------------------------------------------------------------------------------------ 1. read-out with row maps
@pytest.mark.parametrize('shape', RS.READ_CASES, ids=_case_id)
def test_partial_readouts_through_row_maps(shape):
    """every rank's partial read-out through its row maps and local arenas (NaN around and behind the owned rows, a
    one-row NaN arena where the rank owns nothing): finite, exactly 0 where the rank owns no term, the fp64 sum over its
    terms, nothing written outside the output; the W partials add up to the unsharded kernel's read-out; identity maps
    (W == 1) change no bit"""
    c = RS.read_case(*shape)
    RS.assert_conditions(c)
    full = RS.launch(c, c.vl_d, c.vw_d)
    ref = c.reference()
    scale = max(1.0, ref.abs().max().item())
    err_full = (full.double() - ref).abs().max().item()
    assert err_full <= 1e-4 * scale, (shape, err_full)
    total, worst = torch.zeros_like(full), err_full / scale
    for r in range(c.world):
        got = RS.partial(c, r)
        worst = max(worst, RS.check_partial(c, r, got))
        total += got
    err_sum = max_err(total, full)
    print(f'read-out {shape}: worst err against fp64 / max(1, |ref|max) {worst:.3e} (bound 1e-4); sum of the {c.world} '
          f'partials against the unsharded read-out {err_sum:.3e} (bound {1e-5 * max(1.0, full.abs().max().item()):.3e})')
    assert err_sum <= 1e-5 * max(1.0, full.abs().max().item())
    one = torch.zeros_like(c.owner)   # a 1-rank group: identity maps over the whole arenas
    ident = RS.launch(c, c.vl_d, c.vw_d, row_map_long=to_dev(RS.row_map(one[:c.n_long], 0)) if c.n_long else None,
                      row_map_work=to_dev(RS.row_map(one[c.n_long:], 0)))
    assert torch.equal(_bits(ident), _bits(full)), f'{shape}: identity row maps change the read-out'


@kernel_property
@pytest.mark.parametrize('shape', RS.READ_CASES, ids=_case_id)
def test_partial_readout_is_the_unsharded_kernel_with_the_other_ranks_weights_zeroed(shape):
    """isolates the remap from the arithmetic: the kernel accumulates the live terms in index order, and adding
    0 * finite leaves an accumulator unchanged -- so rank r's partial must equal, bit for bit, the same kernel on the same
    idx with the WHOLE arenas, no maps, and weight 0 for the terms rank r does not own"""
    c = RS.read_case(*shape)
    for r in range(c.world):
        masked = RS.launch(c, c.vl_d, c.vw_d, weight=to_dev(torch.where(c.owned(r), c.w, torch.zeros(()))))
        assert torch.equal(_bits(RS.partial(c, r)), _bits(masked)), f'{shape} rank {r}: the row maps change the arithmetic'


def test_control_a_swapped_map_entry_is_seen():
    """negative control of check 3: two owned entries of one rank's map exchanged (both rows exist and are finite) -- the
    fp64 reference must refuse the partial"""
    c = RS.read_case(*RS.READ_CASES[4])
    r = c.world - 1
    RS.check_partial(c, r, RS.partial(c, r))
    with pytest.raises(AssertionError, match='differs from the fp64 sum'):
        RS.check_partial(c, r, RS.partial(c, r, maps=RS.swapped_maps(c, r)))


def test_control_b_gathered_stand_in_row_is_seen():
    """negative control of check 1: the partial formed the way the emulation used to (weight zeroed, row 0 of the arena
    still gathered) on a rank whose long-term arena is one row of NaN -- 0 * NaN must be caught"""
    c = RS.read_case(*RS.READ_CASES[4])
    r = 0
    assert int((c.own_long == r).sum()) == 0 and bool(torch.isnan(c.arenas(r)[0]).all())
    assert bool(((c.idx.long() < c.n_long) & ~c.owned(r)).any()), 'no long-term term of another rank in this case'
    RS.check_partial(c, r, RS.partial(c, r))
    with pytest.raises(AssertionError, match='NaN / inf in the partial read-out'):
        RS.check_partial(c, r, RS.partial_like_the_old_emulation(c, r))


# ------------------------------------------------------------------------------------------ 2. the value-sharded store
def _usage_counters(g, n, offset):
    """seeded fixed-point usage counters (2^-40 units) of n tokens at `offset` of a scratch buffer, as after a merged
    read: identical on every rank"""
    fix = torch.zeros(offset + n + 3, dtype=torch.int64)
    fix[offset:offset + n] = torch.randint(0, 1 << 44, (n,), generator=g)
    return fix


@pytest.mark.parametrize('world', [2, 3, 8])
def test_value_sharded_stores_follow_the_unsharded_store(world):
    """W value-sharded stores and one unsharded store through the same memory events (frames of 35 tokens -- not
    divisible by 2, 3 or 8 -- and one of 5, fewer than 8 ranks); the stores are compared after EVERY event
    (rank_shares.check_stores), then one real read of the unsharded bank is read out by every rank through its row map"""
    g = torch.Generator().manual_seed(100 + world)
    plain, shards = RS.make_stores(world)
    stores = [plain] + shards

    def event(tag, call):
        for s in stores:
            call(s)
        torch.cuda.synchronize()
        RS.check_stores(plain, shards, f'W={world} after {tag}')

    def add(tag, n, objects, **kw):
        key, val, shr, sel = RS.frame(g, n, objects, token_major=kw.get('token_major', False))
        event(tag, lambda s: s.add(key, val, shr, sel, **kw))

    def usage(tag, offset):
        for b in list(plain.buckets):
            fix = _usage_counters(g, plain.size(b), offset)
            event(f'{tag} (bucket {b})', lambda s: s.apply_usage_fix(b, to_dev(fix.clone()), offset))

    for i in range(3):
        add(f'frame {i}', RS.FRAME, [1, 2])
    add('a frame of 5 tokens', RS.SMALL_FRAME, [1, 2])
    add('a third object opens bucket 1', RS.FRAME, [1, 2, 3])
    add('frame 5', RS.FRAME, [1, 2, 3])
    assert plain.size(0) == 180 and plain.size(1) == 70 and plain.buckets == {0: [1, 2], 1: [3]}
    usage('usage counters', 7)
    event('remove_obsolete_features(0, 120)', lambda s: s.remove_obsolete_features(0, 120))
    assert plain.size(0) == 120
    event('remove_old_memory(1, 10, 40)', lambda s: s.remove_old_memory(1, 10, 40))
    assert plain.size(1) == 40
    event('sieve_by_range(0, 35, -35)', lambda s: s.sieve_by_range(0, RS.FRAME, -RS.FRAME, min_size=50))
    assert plain.size(0) == 70
    add('prototypes into bucket 0 (token-major)', RS.SMALL_FRAME, [1, 2], supposed_bucket_id=0, token_major=True)
    add('prototypes into a new bucket 7 (token-major)', RS.FRAME, [9], supposed_bucket_id=7, token_major=True)
    add('a frame after the compactions', RS.FRAME, [1, 2, 3])
    usage('usage counters again', 0)
    event('remove_obsolete_features(1, 50)', lambda s: s.remove_obsolete_features(1, 50))
    event('purge_except([1, 3])', lambda s: s.purge_except([1, 3]))
    assert plain.buckets == {0: [1], 1: [3]} and 9 not in plain and all(9 not in s for s in shards)

    # one real read of the unsharded bank, read out by every rank through ITS row map and value arena
    n, k, hw, obj = plain.size(0), 30, 45, 1
    assert n >= k
    qk, qe = to_dev(torch.randn(RS.CK, hw, generator=g)), to_dev(torch.rand(RS.CK, hw, generator=g))
    idx, w = ops.affinity_topk(None, None, 0, plain.key_arena(0), plain.shrinkage_arena(0), n, qk, qe, k)
    full = ops.readout_sparse(idx, w, None, 0, plain.value_arena(obj), torch.empty(RS.CV, hw, device=dev()))
    torch.cuda.synchronize()
    rows64 = plain.value_arena(obj)[:n].cpu().double()[idx.cpu().long()]                   # [hw, k, CV]
    total = torch.zeros_like(full)
    worst = 0.0
    for r, s in enumerate(shards):
        part = ops.readout_sparse(idx, w, None, 0, s.value_arena(obj), torch.empty(RS.CV, hw, device=dev()),
                                  row_map_work=s.row_map(0))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(part).all()), (world, r)
        mine = (s.row_map(0)[:n].cpu() >= 0)[idx.cpu().long()]                             # [hw, k]
        assert bool((part.cpu()[:, mine.sum(1) == 0] == 0.0).all()), (world, r)
        ref = torch.einsum('qk,qkc->cq', torch.where(mine, w.cpu(), torch.zeros(())).double(), rows64)
        err, scale = (part.cpu().double() - ref).abs().max().item(), max(1.0, ref.abs().max().item())
        worst = max(worst, err / scale)
        assert err <= 1e-4 * scale, (world, r, err)
        total += part
    err_sum = max_err(total, full)
    print(f'store W={world}: {n} tokens; worst partial read-out err against fp64 / max(1, |ref|max) {worst:.3e} (bound 1e-4); '
          f'sum of the partials against the unsharded read-out {err_sum:.3e} (bound {1e-5 * max(1.0, full.abs().max().item()):.3e})')
    assert err_sum <= 1e-5 * max(1.0, full.abs().max().item())


# ------------------------------------------------------------------------------------------ 3. one rank's prototype GEMM
@functools.lru_cache(maxsize=None)
def _potentiation(n_cand, P):
    return RS.potentiation(n_cand, P, seed=n_cand + P)


# how the candidates are split: W = 2 leaves rank 0 ONE row, W = 3 none (only batches smaller than the group); W = 8 is
# balanced (mostly batches of 8 .. 31 tokens): about an eighth of the candidates each, whatever the eviction left
GEMM_SPLIT = {2: dict(big=1), 3: dict(big=0), 8: dict(big=1 << 20)}
GEMM_SEED = 0   # (under which rank 0 of 2 keeps exactly one row after the eviction: asserted)


@pytest.mark.parametrize('world', [2, 3, 8])
@pytest.mark.parametrize('P,n_cand', [(5, 77), (64, 77), (5, 1000), (64, 1000)])
def test_partial_prototype_gemm_at_a_ranks_k(P, n_cand, world):
    """`MemoryManager.partial_prototype_values` -- the code `consolidation` runs before its all-reduce -- at the ragged
    K = n_own of every rank of a group: against the fp64 product over the rank's rows, exact zeros for a rank without
    rows, and the partials summed against the unsharded GEMM"""
    from deva.inference.memory_manager import MemoryManager
    aff, vals = _potentiation(n_cand, P)
    vals_d = to_dev(vals)
    owner = RS.ownership(n_cand, world, GEMM_SEED, **GEMM_SPLIT[world])
    n_own = [int((owner == r).sum()) for r in range(world)]
    assert sum(n_own) == n_cand
    assert world != 2 or n_own[0] == 1, f'rank 0 of 2 was to own one row, owns {n_own[0]}'
    assert world != 3 or n_own[0] == 0, f'rank 0 of 3 was to own no row, owns {n_own[0]}'
    assert world != 8 or (min(n_own) >= 2 and len(set(n_own)) > 1), n_own
    gemm = ops.PackedConv(aff, None, n_cand, P, aff.shape[1], 1, 1)
    full = ops.conv2d(gemm, vals_d.reshape(1, n_cand, 1, RS.CV)).view(P, RS.CV)
    aff64, vals64 = aff.cpu().double()[:, :P], vals.double()
    assert float(aff64.max()) < 0.5 and float(aff64.min()) > 0.0, 'a (nearly) one-hot affinity: the GEMM would be a row copy'
    assert max_err(full, (aff64.t() @ vals64).float()) <= 1e-5 * max(1.0, full.abs().max().item())
    total, worst = torch.zeros_like(full), 0.0
    for r in range(world):
        rows = torch.nonzero(owner == r).flatten()
        part, = MemoryManager.partial_prototype_values(aff, P, to_dev(rows), [vals_d[to_dev(rows)]])
        torch.cuda.synchronize()
        assert tuple(part.shape) == (P, RS.CV)
        if n_own[r] == 0:
            assert bool((part == 0.0).all()), 'a rank without candidate rows must contribute exact zeros'
        ref = aff64[rows].t() @ vals64[rows]
        err, scale = (part.cpu().double() - ref).abs().max().item(), max(1.0, ref.abs().max().item())
        worst = max(worst, err / scale)
        assert err <= 1e-5 * scale, (P, n_cand, world, r, n_own[r], err)
        total += part
    err_sum = max_err(total, full)
    print(f'prototype GEMM P={P} n_cand={n_cand} W={world}: n_own {n_own}; worst partial err against fp64 / max(1, |ref|max) '
          f'{worst:.3e} (bound 1e-5); sum against the unsharded GEMM {err_sum:.3e} (bound {world * 1e-5 * max(1.0, full.abs().max().item()):.3e})')
    assert err_sum <= world * 1e-5 * max(1.0, full.abs().max().item())


# ------------------------------------------------------------------------------------------ 4. pre-filtered token shards
@kernel_property
def test_token_shards_on_the_prefilter_merge_to_the_unsharded_read():
    """what `_read_bucket_bank_sharded` hands the kernels on a long clip: three shards of 4 234 / 4 234 / 4 232 tokens, each
    large enough for the fp16 pre-filter (4 200 x 2 001 is the smallest size at which the policy engages:
    test_every_owner_of_the_tail_gives_the_same_read), on SLICED arenas (shard 0 all long-term, shard 1 across the
    long / work boundary, shard 2 all working memory; every shrinkage pointer 4-byte aligned and no more) with a non-zero
    token offset.  Every shard must stay on the pre-filter and equal the fp32 lists on the same slices; the merge of the
    three must be the unsharded read bit for bit"""
    from deva.hip import lib
    n, n_long, hw, k, world = 12700, 4500, 2001, 30, 3
    mk, ms, qk, qe = synth.affinity_inputs(n, hw, seed=n + hw + world)
    rows, shr = mk.t().contiguous(), ms.reshape(-1).contiguous()

    def one_float_in(t):
        """the arena one float into its buffer: with the even shard bounds of this case every slice [l0:l1] of it starts at
        an odd float offset, as a shard of a bank with an odd `per` does"""
        return to_dev(torch.cat([torch.full((1,), RS.NAN), t]))[1:]

    kl, sl = to_dev(rows[:n_long].contiguous()), one_float_in(shr[:n_long])
    kw, sw = to_dev(rows[n_long:].contiguous()), one_float_in(shr[n_long:])
    qk_d, qe_d = to_dev(qk), to_dev(qe)
    full_fix = torch.zeros(n, dtype=torch.int64, device=dev())
    idx, w = ops.affinity_topk(kl, sl, n_long, kw, sw, n - n_long, qk_d, qe_d, k, full_fix)
    per = -(-n // world)
    keys, counts, kinds = [], [], []
    for r in range(world):
        lo, hi = r * per, min(n, (r + 1) * per)
        l0, l1 = min(lo, n_long), min(hi, n_long)
        w0, w1 = max(lo, n_long) - n_long, max(hi, n_long) - n_long
        kinds.append((l1 > l0, w1 > w0))
        assert lib().deva_affinity_prefilter_enabled(hi - lo, hw, k) == 1, f'shard {r} ({hi - lo} tokens) is below the pre-filter policy'
        args = (kl[l0:l1] if l1 > l0 else None, sl[l0:l1] if l1 > l0 else None, l1 - l0,
                kw[w0:w1] if w1 > w0 else None, sw[w0:w1] if w1 > w0 else None, w1 - w0, qk_d, qe_d, k)
        assert all(t.data_ptr() % 8 == 4 for t in (args[1], args[4]) if t is not None), 'a shrinkage slice is 8-byte aligned'
        kk, cc = ops.affinity_candidates(*args, token_offset=lo)
        assert ops.affinity_last_read_flag(dev()) == 0, f'shard {r}: the pre-filter fell back'   # (before the scratch is reused)
        old_k, old_c = ops.affinity_candidates(*args, token_offset=lo, splits=4)
        torch.cuda.synchronize()
        assert torch.equal(cc, old_c) and int(cc.min()) == k and int(cc.max()) == k, f'shard {r}: counts'
        assert torch.equal(kk[:, :k], old_k[:, :k]), f'shard {r}: the pre-filtered keys differ from the fp32 lists'
        keys.append(kk)
        counts.append(cc)
    assert kinds == [(True, False), (True, True), (False, True)], kinds
    fix = torch.zeros(n, dtype=torch.int64, device=dev())
    idx_m, w_m = ops.affinity_merge(torch.stack(keys), torch.stack(counts), k, fix)
    torch.cuda.synchronize()
    assert torch.equal(idx_m, idx), f'{int((idx_m != idx).any(1).sum())} queries select different tokens'
    assert torch.equal(_bits(w_m), _bits(w)), 'weights differ'
    assert torch.equal(fix, full_fix), 'usage counters differ'
