"""The device batch types every step reads (``Batch``, ``TripleBatch``) and what identifies a batch's index structure
to the graph engine (``structure_fingerprint``).  A leaf module: numpy and torch only.
"""
import numpy as np
import torch


class Batch:
    """Device-resident collated batch with the attributes do_DDM / NCSN_version_03 read
    (BatchAtomTuple, dataloaders_AtomTuple.py:40-78)."""

    def __init__(self, x, positions, batch, super_edge_index, radius_edge_index=None, num_graphs=None, sizes=None,
                 canonical=None):
        self.x, self.positions, self.batch, self.super_edge_index = x, positions, batch, super_edge_index
        self.radius_edge_index = radius_edge_index
        self._num_graphs = num_graphs
        # host-side knowledge of the collation (structure_fingerprint): atoms per molecule, and the AtomTupleExtractor
        # option when super_edge_index is its full enumeration in batch order
        self._sizes = None if sizes is None else [int(n) for n in sizes]
        self._canonical = canonical
        # (option, ratio) when super_edge_index is AtomTupleExtractor(ratio < 1) output of that option, grouped by
        # molecule in batch order with int(M * ratio) tuples per molecule (`_canonical` is None then): which tuples
        # is data, how many is a function of the sizes - what a sampled capacity bucket takes (bucket.option_of)
        self._sampled = None

    @property
    def num_graphs(self):
        if self._num_graphs is None:
            self._num_graphs = self.batch[-1].item() + 1  # dataloaders_AtomTuple.py:75-78
        return self._num_graphs

    @classmethod
    def from_numpy(cls, d, device, prepare=True):
        """prepare=False: the index structures of the step are built (from the host sizes) by the first step that needs
        them - a step that replays a capacity-bucket graph never does."""
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        rei = t(d["radius_edge_index"]) if "radius_edge_index" in d else None
        ng = int(len(d["sizes"])) if "sizes" in d else None
        canonical = canonical_option(d["sizes"], d["super_edge_index"]) if "sizes" in d else None
        out = cls(t(d["x"]), t(d["positions"]), t(d["batch"]), t(d["super_edge_index"]), rei, ng, d.get("sizes"),
                  canonical)
        if "sizes" in d:  # collation knows the molecule sizes on the host: index structures without a device read-back
            from .layout import prepare_batch
            prepare_batch(out.batch, out.super_edge_index, d["sizes"], lazy=not prepare)
        return out

    def to(self, device):
        dev = torch.device(device)
        if all(a is None or (a.device == dev or (dev.index is None and a.device.type == dev.type))
               for a in (self.x, self.positions, self.batch, self.super_edge_index, self.radius_edge_index)):
            return self  # (already there: like Tensor.to, no new object - what is cached on this one stays)
        mv = lambda a: None if a is None else a.to(device)
        out = Batch(mv(self.x), mv(self.positions), mv(self.batch), mv(self.super_edge_index),
                    mv(self.radius_edge_index), self._num_graphs, self._sizes, self._canonical)
        out._sampled = self._sampled
        return out


class TripleBatch(Batch):
    """Device-resident collated batch of atom TRIPLES with the attributes the loop of
    examples/pretrain_TorsionAnglePrediction.py:64-78 reads (BatchAtomTriple, dataloaders_AtomTriple.py:34-72):
    ``super_edge_index`` is int64 [3, T] (grouped by molecule in batch order) and ``super_edge_angle`` float32 [T] its
    targets.  The list is sampled: never a function of the sizes (``_canonical`` stays None)."""

    _triples = True

    def __init__(self, x, positions, batch, super_edge_index, super_edge_angle, radius_edge_index=None, num_graphs=None,
                 sizes=None):
        super().__init__(x, positions, batch, super_edge_index, radius_edge_index, num_graphs, sizes, None)
        self.super_edge_angle = super_edge_angle

    @classmethod
    def from_numpy(cls, d, device):
        """From a dict with x, positions, batch, super_edge_index [3, T], super_edge_angle [T], sizes [, radius_edge_index]
        (collated on the host: triples grouped by molecule in batch order)."""
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        rei = t(d["radius_edge_index"]) if "radius_edge_index" in d else None
        sizes = d.get("sizes")
        out = cls(t(d["x"]), t(d["positions"]), t(d["batch"]), t(np.asarray(d["super_edge_index"]).reshape(3, -1)),
                  t(np.asarray(d["super_edge_angle"], dtype=np.float32).reshape(-1)), rei,
                  None if sizes is None else int(len(sizes)), sizes)
        if sizes is not None:
            from .layout import prepare_batch
            prepare_batch(out.batch, out.super_edge_index, sizes, lazy=True)
        return out

    def to(self, device):
        dev = torch.device(device)
        if all(a is None or (a.device == dev or (dev.index is None and a.device.type == dev.type))
               for a in (self.x, self.positions, self.batch, self.super_edge_index, self.super_edge_angle,
                         self.radius_edge_index)):
            return self
        mv = lambda a: None if a is None else a.to(device)
        return TripleBatch(mv(self.x), mv(self.positions), mv(self.batch), mv(self.super_edge_index),
                           mv(self.super_edge_angle), mv(self.radius_edge_index), self._num_graphs, self._sizes)


def sampled_count(M, ratio):
    """Tuples AtomTupleExtractor(ratio < 1) keeps of M (dataloaders_AtomTuple.py:27): Python's ``int(M * ratio)`` - the
    ONE place this number is computed (``int(100 * 0.29)`` is 28, as in the reference; no kernel computes it)."""
    return int(M * ratio)


def tuple_slots(n, option):
    """Tuples of the full enumeration of an n-atom molecule: n (n - 1) / 2 "combination", n (n - 1) "permutation"."""
    n = int(n)
    return 0 if n < 2 else (n * (n - 1) // 2 if option == "combination" else n * (n - 1))


def kept_tuples(sizes, option, ratio):
    """``sampled_count`` of every molecule's enumeration, as an int64 array (one Python evaluation per distinct size)."""
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)
    uniq, inv = np.unique(n, return_inverse=True)
    k = np.asarray([sampled_count(tuple_slots(v, option), ratio) for v in uniq.tolist()], dtype=np.int64)
    return k[inv] if n.size else np.zeros(0, dtype=np.int64)


_PAIR_CACHE = {}


def canonical_option(sizes, super_edge_index):
    """"combination" / "permutation" when the HOST array super_edge_index [2, S] is exactly AtomTupleExtractor's full
    enumeration (dataloaders_AtomTuple.py:19-24, ratio = 1) of molecules with these sizes, collated in batch order with
    node offsets (:64-65); None otherwise.  Such index tensors are a function of the sizes alone."""
    from .synthetic import combination_pairs, permutation_pairs
    sizes = np.asarray(sizes, dtype=np.int64)
    sei = np.asarray(super_edge_index)
    S = sei.shape[1] if sei.ndim == 2 else -1
    off = np.concatenate([[0], np.cumsum(sizes)])
    for option, count, pairs in (("combination", sizes * (sizes - 1) // 2, combination_pairs),
                                 ("permutation", sizes * (sizes - 1), permutation_pairs)):
        if int(count.sum()) != S or S == 0:
            continue
        parts = []
        for m, n in enumerate(sizes.tolist()):
            if (option, n) not in _PAIR_CACHE:
                _PAIR_CACHE[(option, n)] = pairs(n)
            parts.append(_PAIR_CACHE[(option, n)] + off[m])
        if np.array_equal(np.concatenate(parts, axis=1), sei):
            return option
    return None


_UID = [0]


def _tensor_uid(t_):
    """A number that identifies the tensor OBJECT for as long as it lives and is never handed out again (id() is: CPython
    reuses the address of a freed tensor, and a streaming loader would then look like a batch that came back)."""
    uid = t_.__dict__.get("_geossl_uid") if hasattr(t_, "__dict__") else None
    if uid is None:
        _UID[0] += 1
        uid = _UID[0]
        try:
            t_._geossl_uid = uid
        except AttributeError:
            return ("id", id(t_))
    return uid


def tensor_tag(t_):
    """What identifies a tensor that a graph binds as it is: the object, its version and its shape; None for None."""
    return None if t_ is None else (_tensor_uid(t_), t_._version, tuple(t_.shape))


def structure_fingerprint(batch, model_3d="schnet"):
    """Hashable identity of everything a captured step binds besides x, positions and the noise: the batch vector,
    super_edge_index and (PaiNN) radius_edge_index with the index structures derived from them.

    * A batch that carries its molecule sizes on the host AND whose super_edge_index is known to be the extractor's
      full enumeration (``_sizes`` / ``_canonical``: set by ``Batch.from_numpy``, ``BatchAtomTuple.from_sizes`` and by
      ``BatchAtomTuple.from_data_list`` over molecules that went through ``AtomTupleExtractor(ratio=1)``) has index
      tensors that are a function of the sizes: the fingerprint is the sizes, so every batch of a shuffled loader with
      the same molecule sizes in the same order shares a graph - and no other batch does.
    * Anything else (sampled tuples, PaiNN's geometry-dependent edge list, batches built by hand) is identified by
      the tensor OBJECTS and their versions: a graph is replayed only for the very tensors it was captured on (a
      device-resident, pre-collated batch that comes back every epoch)."""
    if getattr(batch, "_dataset", None) is not None and model_3d != "painn":
        return batch.fingerprint()   # a handle on a device-resident dataset: its index tensors ARE a function of the sizes
    rei = getattr(batch, "radius_edge_index", None) if model_3d == "painn" else None
    tags = (tensor_tag(batch.batch), tensor_tag(batch.super_edge_index), tensor_tag(rei))
    if getattr(batch, "_triples", False):   # (a triple batch: its targets are bound by a per-structure graph too)
        tags += (tensor_tag(batch.super_edge_angle),)
    cached = batch.__dict__.get("_geossl_fp")
    if cached is not None and cached[0] == tags:
        return cached[1]
    sizes, canon = getattr(batch, "_sizes", None), getattr(batch, "_canonical", None)
    if sizes is not None and canon is not None and rei is None and model_3d != "painn":
        fp = ("sizes", canon, int(batch.batch.numel()), int(batch.super_edge_index.size(1)),
              np.asarray(sizes, dtype=np.int32).tobytes())
    else:
        fp = ("tensors",) + tags
    batch.__dict__["_geossl_fp"] = (tags, fp)
    return fp
