"""TEST-ONLY: what rank r of an N-rank group hands to the kernels when one clip runs on several GPUs with value-sharded
storage (`KeyValueMemoryStore.shard_values`, `MemoryManager.shard_bank`), built WITHOUT a process group: ownership as the
store assigns it (of every batch of b tokens rank r owns the block [b*r//W, b*(r+1)//W), ownership survives evictions, the
survivors' local rows are renumbered in token order), the int32 row maps, the local value arenas -- inside NaN, the way an
arena that was never written looks to a kernel that reads a row it should not -- and float64 references computed from the
UNSHARDED fp32 inputs.  One process then plays every rank in turn on one device (tests/test_gpu_x_rank_shares.py)."""
import functools
import zlib

import torch

from deva.hip import ops
from gpu_util import dev, to_dev

NAN = float('nan')
SENTINEL = 12345.0
MAP_SLACK = 5     # map entries past the segment's size (the store's maps are longer than the bucket: -1 there)
PAD_ROWS = 2      # NaN rows before and after a local arena
SPARE_ROWS = 3    # NaN rows n_local .. of a local arena (capacity beyond the live rows)
OUT_PAD = 65      # sentinel floats before and after an output view (odd: the view starts 4 bytes off a 16-byte boundary)


# ------------------------------------------------------------------------------------------ ownership
def batch_sizes(m, world, g, big):
    """sizes of the batches in which m tokens arrive: `big` batches of W .. 4W-1 tokens at seeded places among batches of
    1 .. W-1 tokens (one token for W <= 2).  Of a batch smaller than the group some ranks receive nothing -- rank 0 never
    does (b*1//W == 0) -- so rank 0 ends up with the few rows the big batches give it: none at all with big == 0"""
    sizes, left = [], m
    for _ in range(big):
        if left < world:
            break
        b = min(left, int(torch.randint(world, 4 * world, (1,), generator=g)))
        sizes.append(b)
        left -= b
    while left > 0:
        b = min(left, int(torch.randint(1, max(2, world), (1,), generator=g)))
        sizes.append(b)
        left -= b
    return [sizes[i] for i in torch.randperm(len(sizes), generator=g).tolist()]


def ownership(n, world, seed, big=1):
    """-> int64 [n]: the rank that holds the value row of each of the n tokens of a segment, after n + n//2 tokens have
    arrived in `batch_sizes` and a seeded eviction has removed a third of them (the survivors keep their owner)"""
    if n == 0:
        return torch.zeros(0, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    m = n + n // 2
    owner = torch.full((m,), -1, dtype=torch.int64)
    at = 0
    for b in batch_sizes(m, world, g, big):
        for r in range(world):
            owner[at + b * r // world:at + b * (r + 1) // world] = r
        at += b
    assert at == m and bool((owner >= 0).all())
    keep = torch.sort(torch.randperm(m, generator=g)[:n])[0]
    return owner[keep]


def row_map(owner, rank):
    """int32 [n + MAP_SLACK]: local row of every token (0 .. n_local-1 in token order), -1 = another rank's; -1 past n"""
    n = owner.numel()
    mine = owner == rank
    out = torch.full((n + MAP_SLACK,), -1, dtype=torch.int32)
    out[:n][mine] = torch.arange(int(mine.sum()), dtype=torch.int32)
    return out


def local_arena(values, owner, rank):
    """values [n, cv] (host) -> this rank's token-major value arena ON THE DEVICE: the owned rows in token order, then
    SPARE_ROWS rows of NaN, as a view inside a buffer of NaN.  A rank that owns no row gets a ONE-ROW arena of NaN: what
    `_Arena.ensure(1, 0)` leaves (a torch.empty)"""
    rows = values[owner == rank]
    n_local, cv = rows.shape
    cap = n_local + SPARE_ROWS if n_local else 1
    buf = torch.full((PAD_ROWS + cap + PAD_ROWS, cv), NAN)
    buf[PAD_ROWS:PAD_ROWS + n_local] = rows
    return to_dev(buf)[PAD_ROWS:PAD_ROWS + cap]


# ------------------------------------------------------------------------------------------ part 1: the read-out
# (hw, k, cv, n_long, n_work, W): the smallest sizes at which each tiling rule of readout_sparse_kernel is crossed
# (8 queries x 256 channels per block, one term per lane, eight rows per fetch)
READ_CASES = [(1, 1, 4, 0, 5, 2), (7, 32, 252, 0, 64, 3), (8, 64, 256, 100, 100, 2), (9, 7, 260, 3, 40, 8),
              (45, 30, 512, 70, 130, 3), (257, 33, 512, 500, 700, 8)]
# seed of every case's ownership: one under which the conditions that `assert_conditions` states hold (they are asserted)
OWNER_SEED = 0


class ReadCase:
    def __init__(self, hw, k, cv, n_long, n_work, world):
        self.shape = (hw, k, cv, n_long, n_work, world)
        self.hw, self.k, self.cv, self.n_long, self.n_work, self.world = self.shape
        n = n_long + n_work
        seed = zlib.crc32(repr(self.shape).encode()) % 100000
        g = torch.Generator().manual_seed(seed)
        self.idx = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(hw)]).int()
        self.w = torch.rand(hw, k, generator=g)
        self.vl, self.vw = torch.randn(n_long, cv, generator=g), torch.randn(n_work, cv, generator=g)
        oseed = OWNER_SEED
        # the long-term segment of a group of three or more receives only batches smaller than the group: rank 0 owns
        # none of its rows
        self.own_long = ownership(n_long, world, oseed, big=0 if world >= 3 else 1)
        self.own_work = ownership(n_work, world, oseed + 1, big=1 if world == 2 else 2)
        self.owner = torch.cat([self.own_long, self.own_work])
        self.term_owner = self.owner[self.idx.long()]                                   # [hw, k]
        self._rows64 = torch.cat([self.vl, self.vw]).double()[self.idx.long()]          # [hw, k, cv]
        self.idx_d, self.w_d = to_dev(self.idx), to_dev(self.w)
        self.vl_d, self.vw_d = (to_dev(self.vl) if n_long else None), to_dev(self.vw)

    def owned(self, rank):
        """bool [hw, k]: the terms whose value row rank `rank` holds"""
        return self.term_owner == rank

    def reference(self, rank=None):
        """float64 [cv, hw]: the sum over the terms rank `rank` owns (None: over all terms), from the unsharded inputs"""
        w = self.w.double() if rank is None else torch.where(self.owned(rank), self.w, torch.zeros(())).double()
        return torch.einsum('qk,qkc->cq', w, self._rows64)

    def maps(self, rank):
        """-> (row_map_long or None, row_map_work) on the device"""
        return (to_dev(row_map(self.own_long, rank)) if self.n_long else None), to_dev(row_map(self.own_work, rank))

    def arenas(self, rank):
        """-> (val_long or None, val_work): the rank's local arenas on the device"""
        return (local_arena(self.vl, self.own_long, rank) if self.n_long else None), local_arena(self.vw, self.own_work, rank)


@functools.lru_cache(maxsize=None)
def read_case(*shape):
    """one case's inputs, ownership and references: built once, shared by the tests, never modified"""
    return ReadCase(*shape)


def assert_conditions(c):
    """what the inputs of a case must have for the test to be about what it says"""
    counts = torch.stack([(c.owner == r) for r in range(c.world)]).sum(0)
    assert bool((counts == 1).all()), 'every token is owned by exactly one rank'
    if c.world >= 3:
        assert any(int((c.own_long == r).sum()) == 0 for r in range(c.world)), 'no rank without long-term rows'
    per_query = torch.stack([c.owned(r).sum(1) for r in range(c.world)])                # [W, hw]
    assert bool((per_query == 0).any()), f'{c.shape}: every rank owns a term of every query'
    assert bool((per_query > 0).any()), f'{c.shape}: no rank owns any term'


def launch(c, val_long, val_work, weight=None, row_map_long=None, row_map_work=None):
    """ops.readout_sparse of case `c` on the given arenas / maps, written through a view inside a buffer of sentinels
    -> the [cv, hw] result on the host; asserts that nothing outside the view was written"""
    n_out = c.cv * c.hw
    buf = torch.full((OUT_PAD + n_out + OUT_PAD,), SENTINEL, device=dev())
    out = buf[OUT_PAD:OUT_PAD + n_out].view(c.cv, c.hw)
    got = ops.readout_sparse(c.idx_d, c.w_d if weight is None else weight, val_long, c.n_long, val_work, out,
                             row_map_long=row_map_long, row_map_work=row_map_work)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:OUT_PAD] == SENTINEL).all()) and bool((buf[OUT_PAD + n_out:] == SENTINEL).all()), \
        f'{c.shape}: the read-out wrote outside its output'
    return out.cpu().clone()


def partial(c, rank, maps=None):
    """rank `rank`'s partial read-out through its row maps and local arenas (maps: replace the rank's own maps)"""
    ml, mw = c.maps(rank) if maps is None else maps
    al, aw = c.arenas(rank)
    return launch(c, al, aw, row_map_long=ml, row_map_work=mw)


def check_partial(c, rank, got):
    """checks 1-3 of a rank's partial read-out `got` [cv, hw] (host) against the float64 reference; -> err / bound scale"""
    assert bool(torch.isfinite(got).all()), \
        f'{c.shape} rank {rank}: NaN / inf in the partial read-out ({int((~torch.isfinite(got)).sum())} elements)'
    empty = c.owned(rank).sum(1) == 0
    assert bool((got[:, empty] == 0.0).all()), f'{c.shape} rank {rank}: a query without an owned term is not exactly 0'
    ref = c.reference(rank)
    scale = max(1.0, ref.abs().max().item())
    err = (got.double() - ref).abs().max().item()
    print(f'read-out {c.shape} rank {rank}: {int((~empty).sum())}/{c.hw} queries with owned terms, max abs err against fp64 '
          f'{err:.3e} (bound {1e-4 * scale:.3e})')
    assert err <= 1e-4 * scale, f'{c.shape} rank {rank}: partial read-out differs from the fp64 sum over its terms by {err:.3e}'
    return err / scale


def swapped_maps(c, rank):
    """the rank's maps with two owned entries of one segment exchanged: the token of the rank's heaviest term and another
    token of the same segment that the rank owns (two rows that both exist, read for one another)"""
    w = torch.where(c.owned(rank), c.w, torch.full((), -1.0))
    q, j = divmod(int(w.argmax()), c.k)
    t1 = int(c.idx[q, j])
    in_long = t1 < c.n_long
    seg_owner, base = (c.own_long, 0) if in_long else (c.own_work, c.n_long)
    others = [t for t in torch.nonzero(seg_owner == rank).flatten().tolist() if t + base != t1]
    assert others, 'the rank owns one row of the segment only: nothing to swap'
    ml, mw = c.maps(rank)
    m = ml if in_long else mw
    a, b = t1 - base, others[len(others) // 2]
    keep = m[a].clone()
    m[a] = m[b]
    m[b] = keep
    return ml, mw


def partial_like_the_old_emulation(c, rank):
    """the partial the way tests/emu_ops.py formed it before it followed the kernel's contract: the weight of a term that
    is not live zeroed, ROW 0 of the arena STILL GATHERED for it and multiplied by that zero"""
    (ml, mw), (al, aw) = c.maps(rank), c.arenas(rank)
    t = c.idx_d.long()
    is_long = t < c.n_long
    seg = torch.where(is_long, t, t - c.n_long)
    loc = mw.long()[seg.clamp(max=mw.numel() - 1)]
    if c.n_long:
        loc = torch.where(is_long, ml.long()[seg.clamp(max=ml.numel() - 1)], loc)
    w = torch.where(loc >= 0, c.w_d, torch.zeros_like(c.w_d))
    rows_l = al if c.n_long else aw
    rows = torch.where(is_long.reshape(-1, 1), rows_l[loc.clamp(min=0).clamp(max=rows_l.shape[0] - 1).reshape(-1)],
                       aw[loc.clamp(min=0).clamp(max=aw.shape[0] - 1).reshape(-1)])
    return (rows.reshape(c.hw, c.k, c.cv) * w[:, :, None]).sum(1).t().contiguous().cpu()


# ------------------------------------------------------------------------------------------ part 2: the store
CK, CV, FRAME, SMALL_FRAME = 64, 512, 35, 5


def make_stores(world):
    """-> (the unsharded store, [rank 0's store, ..., rank W-1's store]); nothing added yet"""
    from deva.inference.kv_memory_store import KeyValueMemoryStore
    plain = KeyValueMemoryStore(save_selection=True, save_usage=True)
    shards = []
    for r in range(world):
        s = KeyValueMemoryStore(save_selection=True, save_usage=True)
        s.shard_values(r, world)
        shards.append(s)
    return plain, shards


def frame(g, n, objects, token_major=False):
    """one batch of n memory tokens on the device: key [CK, n], {obj: value [CV, n]}, shrinkage [1, n], selection [CK, n]
    (token_major: [n, CK], [n, CV], [n], [n, CK])"""
    key, sel = torch.randn(CK, n, generator=g), torch.rand(CK, n, generator=g)
    shr = torch.rand(1, n, generator=g) + 1.0
    val = {o: torch.randn(CV, n, generator=g) for o in objects}
    if token_major:
        key, sel, shr = key.t().contiguous(), sel.t().contiguous(), shr.reshape(-1)
        val = {o: v.t().contiguous() for o, v in val.items()}
    return to_dev(key), to_dev(val), to_dev(shr), to_dev(sel)


def _bits(t):
    return t.contiguous().view(torch.int32)


def check_stores(plain, shards, tag):
    """after a memory event: the replicated arenas of every rank equal the unsharded store's bit for bit; the row maps are
    a partition of the tokens with local rows 0 .. n_local-1 in token order; every value row sits, bit for bit, where its
    owner's map says; `local_rows` of a token range names the rows the map does"""
    world = len(shards)
    assert set(plain.buckets) == set(s_b for s in shards for s_b in s.buckets), tag
    for b, objs in plain.buckets.items():
        n = plain.size(b)
        assert n > 0, (tag, b)
        maps = []
        for r, s in enumerate(shards):
            assert s.buckets[b] == objs and s.size(b) == n, (tag, b, r)
            for name, pick in (('key', lambda st: st.key_arena(b)), ('shrinkage', lambda st: st.shrinkage_arena(b)),
                               ('selection', lambda st: st.selection_arena(b)), ('use', lambda st: st.usage_arenas(b)[0]),
                               ('life', lambda st: st.usage_arenas(b)[1])):
                assert torch.equal(_bits(pick(s)[:n]), _bits(pick(plain)[:n])), f'{tag}: bucket {b} rank {r}: {name} arena differs'
            lrow = s.row_map(b)
            assert lrow.dtype == torch.int32 and lrow.numel() >= n
            m = lrow[:n].cpu().long()
            n_local = s.local_size(b)
            assert int((m >= 0).sum()) == n_local and m[m >= 0].tolist() == list(range(n_local)), \
                f'{tag}: bucket {b} rank {r}: the local rows are not 0..{n_local - 1} in token order'
            maps.append(m)
        stacked = torch.stack(maps)                                                    # [W, n]
        assert bool(((stacked >= 0).sum(0) == 1).all()), f'{tag}: bucket {b}: a token without exactly one owner'
        assert sum(s.local_size(b) for s in shards) == n, (tag, b)
        owner = (stacked >= 0).long().argmax(0)
        lo, hi = n // 5 + 1, n - n // 7 - 1   # a range that begins and ends inside blocks, not at a batch boundary
        for o in objs:
            want = plain.value_arena(o)[:n].cpu()
            for r, s in enumerate(shards):
                mine = owner == r
                got = s.value_arena(o).cpu()
                assert got.shape[0] >= max(1, int(mine.sum()))
                assert torch.equal(_bits(got[maps[r][mine]]), _bits(want[mine])), \
                    f'{tag}: bucket {b} object {o} rank {r}: a value row is not where the row map says'
                if hi > lo:
                    first, last, own = s.local_rows(b, lo, hi)
                    tokens = lo + own.cpu()
                    assert tokens.tolist() == [t for t in range(lo, hi) if int(owner[t]) == r], (tag, b, r)
                    assert last - first == tokens.numel()
                    assert torch.equal(_bits(got[first:last]), _bits(want[tokens])), \
                        f'{tag}: bucket {b} object {o} rank {r}: local_rows({lo}, {hi}) names other rows than the map'


# ------------------------------------------------------------------------------------------ part 3: the partial GEMM
def potentiation(n_cand, P, seed):
    """the consolidation's affinity of n_cand candidates to P prototypes through the kernels (ops.similarity_dense +
    ops.softmax_columns) -> (aff [n_cand, ld] on the device, values [n_cand, CV] on the host).  Keys of scale 0.25: the
    scores of one prototype then lie within a few units of each other and every candidate row carries weight in every
    column -- with well separated keys each column is one-hot at the prototype itself, the GEMM degenerates to a row copy
    and a rank's product would not notice a row of its K that is dropped or read twice"""
    g = torch.Generator().manual_seed(seed)
    key, shr, sel = torch.randn(n_cand, CK, generator=g) * 0.25, torch.rand(n_cand, generator=g) + 1, torch.rand(n_cand, CK, generator=g)
    proto = torch.randperm(n_cand, generator=g)[:P].int()
    aff = ops.similarity_dense(to_dev(key), to_dev(shr), to_dev(sel), to_dev(proto), n_cand)
    ops.softmax_columns(aff, P)
    return aff, torch.randn(n_cand, CV, generator=g)
