"""The policy of replay.StructureGraphs without a device: a fake `make()` and plain hashable keys - what is made at which
sighting, what a failed make leaves, which entry the eviction drops, how long a sighting is remembered - and its helpers:
the two structure keys and the batch vector an entry owns, on CPU tensors."""
import types

import torch

from geossl_amd.replay import StructureGraphs, owned_batch_vector, sizes_key, tensors_key


class _Maker:
    """make() -> a new entry that names its key, counted; `fail`: None instead."""

    def __init__(self):
        self.made, self.fail = [], False

    def __call__(self, key):
        def make():
            self.made.append(key)
            return None if self.fail else {"graph": key}
        return make


def _lookup(sg, mk, key, first=False):
    return sg.lookup(key, lambda: first, mk(key))


def test_a_key_marked_for_first_sight_is_made_on_the_first_call():
    sg, mk = StructureGraphs(4), _Maker()
    got = _lookup(sg, mk, "a", first=True)
    assert got == ({"graph": "a"}, True) and mk.made == ["a"] and sg.captures == 1 and list(sg.graphs) == ["a"]
    assert _lookup(sg, mk, "a", first=True) == ({"graph": "a"}, False) and mk.made == ["a"] and sg.captures == 1
    asked = []
    assert sg.lookup("b", lambda: asked.append(1) or True, mk("b")) == ({"graph": "b"}, True)
    assert sg.lookup("b", lambda: asked.append(1) or True, mk("b"))[1] is False and asked == [1]   # asked on a miss only


def test_any_other_key_is_eager_then_made_then_a_hit():
    sg, mk = StructureGraphs(4), _Maker()
    assert _lookup(sg, mk, "a") is None and mk.made == [] and sg.captures == 0 and not sg.graphs
    assert _lookup(sg, mk, "a") == ({"graph": "a"}, True) and mk.made == ["a"] and sg.captures == 1
    assert _lookup(sg, mk, "a") == ({"graph": "a"}, False) and mk.made == ["a"] and sg.captures == 1
    assert sg.get("a") == {"graph": "a"} and sg.get("b") is None


def test_a_failed_make_stores_nothing_and_the_call_is_eager():
    sg, mk = StructureGraphs(4), _Maker()
    mk.fail = True
    assert _lookup(sg, mk, "a", first=True) is None and mk.made == ["a"]
    assert not sg.graphs and sg.captures == 0 and sg.get("a") is None


def test_a_disabled_cache_looks_nothing_up_and_makes_nothing():
    sg, mk = StructureGraphs(4), _Maker()
    assert _lookup(sg, mk, "a", first=True) is not None
    sg.enabled = False
    assert _lookup(sg, mk, "a", first=True) is None and _lookup(sg, mk, "b", first=True) is None and mk.made == ["a"]
    assert StructureGraphs(4, enabled=False).lookup("a", lambda: True, mk("a")) is None and mk.made == ["a"]


def test_eviction_drops_the_least_recently_used_key_not_the_oldest():
    sg, mk = StructureGraphs(2), _Maker()
    for key in ("a", "b"):
        assert _lookup(sg, mk, key, first=True)[1]
    assert _lookup(sg, mk, "a", first=True)[1] is False        # "a" is used: "b" is now the least recently used
    assert _lookup(sg, mk, "c", first=True)[1]
    assert sorted(sg.graphs) == ["a", "c"] and len(sg.graphs) == sg.max_graphs == 2
    sg.get("a")                                                 # (a plain get counts as a use too)
    assert _lookup(sg, mk, "d", first=True)[1] and sorted(sg.graphs) == ["a", "d"]
    assert sg.captures == 4


def test_the_sightings_memory_is_bounded():
    sg, mk = StructureGraphs(8, seen_bound=2), _Maker()
    assert sg.seen_bound == 2 and StructureGraphs(8).seen_bound == 4096
    assert _lookup(sg, mk, "a") is None
    assert _lookup(sg, mk, "b") is None and _lookup(sg, mk, "c") is None     # "a" is pushed out
    assert _lookup(sg, mk, "a") is None and mk.made == []                     # ... and eager again ("b" is pushed out)
    assert _lookup(sg, mk, "a") == ({"graph": "a"}, True)
    assert _lookup(sg, mk, "c") == ({"graph": "c"}, True) and _lookup(sg, mk, "b") is None


def test_structure_keys():
    a = types.SimpleNamespace(batch=torch.tensor([0, 0, 0, 1, 1]), sizes=[3, 2])
    b = types.SimpleNamespace(batch=torch.tensor([0, 0, 0, 1, 1]), sizes=(3, 2))
    assert sizes_key(a.batch.numel(), a.sizes) == sizes_key(b.batch.numel(), b.sizes)
    assert sizes_key(5, [3, 2])[0] == "sizes" and sizes_key(5, [3, 2]) != sizes_key(5, [2, 3])
    assert hash(sizes_key(5, [3, 2])) == hash(sizes_key(5, torch.tensor([3, 2]).numpy()))
    key = tensors_key(a.batch, None)
    assert key[0] == "tensors" and key[2] is None and key == tensors_key(a.batch, None)    # stable across calls
    assert tensors_key(b.batch, None) != key                                               # another tensor object
    assert tensors_key(a.batch) != key and tensors_key(a.batch)[1] == key[1]
    a.batch[0] = 0                                                                         # an in-place write: _version
    assert tensors_key(a.batch, None) != key


def test_owned_batch_vector():
    src = torch.tensor([0, 0, 0, 1, 1])
    src._geossl_sizes = ([3, 2], src._version)
    own = owned_batch_vector(src)
    assert own.data_ptr() != src.data_ptr() and torch.equal(own, src)
    assert own._geossl_sizes == ([3, 2], own._version)
    src[0] = 0                                             # the source's host sizes are stale now
    assert src._geossl_sizes[1] != src._version
    stale = owned_batch_vector(src)
    assert torch.equal(stale, src) and not hasattr(stale, "_geossl_sizes")
    assert not hasattr(owned_batch_vector(torch.tensor([0, 1])), "_geossl_sizes")
    given = owned_batch_vector(src, sizes=(3, 2))          # the caller's sizes stand in
    assert given.data_ptr() != src.data_ptr() and given._geossl_sizes == ([3, 2], given._version)
