"""harness.sharded_ids, the id-level half of the graph-sharded batch order: rank r takes a contiguous slice of every
global batch, a remainder smaller than the rank count is dropped in training and goes to rank 0 in evaluation, and the
shuffled order is the same on every rank.  CPU only: a stand-in context and a store that has nothing but a length.
And harness.expanded_batches, the generator the device-expanding baselines put behind their batches."""
import pytest
import torch

from esc_gnn_amd.harness import expanded_batches, sharded_ids

G, BATCH = 10, 4          # two full global batches and a remainder of 2, which is smaller than world 3
WORLDS = (1, 2, 3)


class _Ctx(object):
    def __init__(self, world, rank):
        self.world, self.rank = world, rank


class _Store(object):
    def __len__(self):
        return G


def _per_rank(world, shuffle, seed=None):
    """one list of (ids, global size) per rank; with a seed every rank gets its own, identically seeded generator"""
    out = []
    for rank in range(world):
        gen = None if seed is None else torch.Generator().manual_seed(seed)
        out.append([(ids.tolist(), n) for ids, n in sharded_ids(_Store(), BATCH, _Ctx(world, rank), shuffle, gen)])
    return out


def _order(shuffle, seed):
    return (torch.randperm(G, generator=torch.Generator().manual_seed(seed)) if shuffle else torch.arange(G)).tolist()


@pytest.mark.parametrize("shuffle", (False, True))
@pytest.mark.parametrize("world", WORLDS)
def test_slices_are_disjoint_contiguous_and_cover_every_global_batch(world, shuffle):
    ranks = _per_rank(world, shuffle, seed=5)
    order = _order(shuffle, 5)
    batches = [order[i:i + BATCH] for i in range(0, G, BATCH)]
    assert [len(b) for b in batches] == [4, 4, 2]
    short = len(batches[-1]) < world                          # only world 3
    assert short == (world == 3)
    kept = batches[:-1] if short else batches
    for step, want in enumerate(kept):
        pieces = [ranks[r][step] for r in range(world)]
        assert [n for _, n in pieces] == [len(want)] * world                       # the global size is reported
        assert all(len(ids) >= 1 for ids, _ in pieces)
        assert sum((ids for ids, _ in pieces), []) == want                         # rank order = contiguous, disjoint, covering
    if not short:
        assert all(len(r) == len(batches) for r in ranks)
    elif shuffle:                                             # training: dropped on every rank alike
        assert all(len(r) == len(kept) for r in ranks)
    else:                                                     # evaluation: rank 0 alone takes it, whole
        assert ranks[0][len(kept):] == [(batches[-1], len(batches[-1]))]
        assert all(len(r) == len(kept) for r in ranks[1:])


@pytest.mark.parametrize("world", WORLDS)
def test_every_graph_is_evaluated_exactly_once(world):
    seen = sorted(i for rank in _per_rank(world, False) for ids, _ in rank for i in ids)
    assert seen == list(range(G))


@pytest.mark.parametrize("world", (2, 3))
def test_shuffle_on_several_ranks_needs_a_generator(world):
    with pytest.raises(ValueError):
        next(sharded_ids(_Store(), BATCH, _Ctx(world, 0), True))
    assert len(list(sharded_ids(_Store(), BATCH, _Ctx(1, 0), True))) == 3          # one rank: the global RNG will do


@pytest.mark.parametrize("world", WORLDS)
def test_same_seed_gives_all_ranks_the_same_order(world):
    a, b = _per_rank(world, True, seed=11), _per_rank(world, True, seed=11)
    assert a == b
    steps = min(len(r) for r in a)
    merged = [i for step in range(steps) for r in range(world) for i in a[r][step][0]]
    assert merged == _order(True, 11)[:len(merged)]           # the ranks cut ONE permutation, not one each
    assert len(merged) == (8 if world == 3 else G)
    assert _per_rank(world, True, seed=12) != a


def test_only_the_length_of_the_store_is_read():
    ids, n = next(sharded_ids(_Store(), BATCH, _Ctx(2, 1), False))
    assert ids.device.type == "cpu" and ids.tolist() == [2, 3] and n == 4


class _ExpandingStore(object):
    """records every expand call and returns something that names its arguments"""

    def __init__(self):
        self.calls = []

    def expand(self, data, *extra):
        self.calls.append((data,) + extra)
        return ("expanded", data) + extra


@pytest.mark.parametrize("extra", ((), ("drnl", True)))
def test_expanded_batches_yields_every_batch_through_the_stores_expand_in_order(extra):
    store = _ExpandingStore()
    batches = [("a", 4), ("b", 4), ("c", 2)]
    it = expanded_batches(store, iter(batches), *extra)
    assert store.calls == []                                  # a generator: nothing is expanded before it is asked for
    assert next(it) == (("expanded", "a") + extra, 4) and store.calls == [("a",) + extra]      # one batch at a time
    assert list(it) == [(("expanded", "b") + extra, 4), (("expanded", "c") + extra, 2)]
    assert store.calls == [(d,) + extra for d, _ in batches]                       # the extra arguments reach every call
