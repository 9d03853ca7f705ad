"""Run-time switches (``GEOSSL_*`` environment variables) as plain dict lookups.

The switches are read where they act, every call, so that a test or a bench line can flip one in the middle of a process
(a backward does not read again what its forward decided: PaiNN's node keeps its route and switches on ctx).
``os.environ.get`` encodes the key, looks it up and decodes the value on every call; a replayed step asks for a dozen of
them.  ``env`` does the lookup in ``os.environ``'s own backing dict with keys encoded once (CPython on POSIX keeps the
process environment as ``bytes -> bytes`` in ``os.environ._data``, updated by every ``os.environ[...] = ...`` /
``monkeypatch.setenv``): same answers, a tenth of the cost.  Anything unexpected about the interpreter falls back to
``os.environ.get``."""
import os

_DATA = getattr(os.environ, "_data", None)
_ENCODE = getattr(os.environ, "encodekey", None)
_DECODE = getattr(os.environ, "decodevalue", None)
if not isinstance(_DATA, dict) or _ENCODE is None or _DECODE is None:
    _DATA = None
_KEYS = {}


def env(name, default=None):
    """``os.environ.get(name, default)``."""
    if _DATA is None:
        return os.environ.get(name, default)
    key = _KEYS.get(name)
    if key is None:
        key = _KEYS[name] = _ENCODE(name)
    value = _DATA.get(key)
    return default if value is None else _DECODE(value)


def masked_painn_buckets():
    """``GEOSSL_MASKED_PAINN_BUCKETS`` (default on): masked PaiNN handles of a ``DeviceLoader`` go through a capacity
    bucket, their surviving radius edges counted on the device.  ``0``: they are collated - a count launch and a read-back
    of the B counts - and run on their own tensors, the routing before the bucket took them (A/B timing)."""
    return env("GEOSSL_MASKED_PAINN_BUCKETS", "1") != "0"


def rbf_image(capturing):
    """``GEOSSL_RBF_IMAGE``: the Gaussian fragments of the filter weight-gradient kernel come from a per-step image
    (``ops.rbf_fragments``, one launch behind the pair list) instead of being rebuilt by every layer's blocks.  ``1``:
    always; ``0``: never - the launches before the image existed (A/B timing); unset: ``capturing`` - like the layer loop,
    the image belongs to captured steps, where its launch costs its kernel time only.  The same bits either way."""
    v = env("GEOSSL_RBF_IMAGE")
    if v == "0":
        return False
    return True if v == "1" else bool(capturing)


def sparse_buckets(handle):
    """``GEOSSL_SPARSE_BUCKETS``: the batches of a step that reads no pair tuples (Supervised, LEP) whose layout is sparse - a
    structure above 255 atoms, or ``GEOSSL_SPARSE_PAIRS=1`` - replay one capacity-bucket graph per batch size
    (``bucket.SPARSE``).  ``1``: every such batch; ``0``: none - the routing before that bucket existed: a per-structure
    graph from the second sighting on, eager launches before.  Unset: ``handle`` - the handles of a ``DeviceLoader`` do,
    collated batches do not (measured on shuffled pockets, DESIGN section 5: the handles' step is 9 - 13 % shorter through
    the bucket; a collated batch's step is bound by the device and the host's collation either way, and the bucket's
    replay did not beat the eager launches there.  LEP's pair handles, same section: 5 - 13 % below the fastest route of
    collated pairs; collated pairs through the bucket gain at 8 pairs and nothing at 32)."""
    v = env("GEOSSL_SPARSE_BUCKETS")
    if v == "0":
        return False
    return True if v == "1" else bool(handle)


# What the unset GEOSSL_SAMPLED_BUCKETS means for COLLATED sampled batches: the outcome of the measurement in
# profiles/sampled_tuples_bench.json by the rule "on only if no slower than the route before at bs = 128 and 1024"
# (the DDM step of collated sampled batches through the bucket is 14 - 33 % shorter at bs = 128; at
# bs = 1024 the host's per-molecule enumeration is the step either way, three of the four cells are 2 - 10 % shorter and
# one is 0.8 % longer, all inside the run-to-run spread - not shown to be no slower there, so: opt-in).
SAMPLED_BUCKETS_COLLATED_DEFAULT = False


def sampled_buckets(handle):
    """``GEOSSL_SAMPLED_BUCKETS``: batches of sampled atom tuples (``AtomTupleExtractor(ratio < 1)``: the handles of a
    ``DeviceLoader(tuple_ratio=)``, collated batches of the host extractor's molecules) replay one capacity-bucket graph
    per (batch size, option, ratio) - the tuples are per-step data of the bucket (``bucket.is_sampled``).  ``1``: handles and
    collated batches; ``0``: neither - eager launches, a per-structure graph for a batch object that comes back (the
    routing before that bucket existed).  Unset: handles do (no other replayed route exists for them); collated batches
    by ``SAMPLED_BUCKETS_COLLATED_DEFAULT`` (they do not: opt-in with ``1``)."""
    v = env("GEOSSL_SAMPLED_BUCKETS")
    if v == "0":
        return False
    return True if v == "1" else (bool(handle) or SAMPLED_BUCKETS_COLLATED_DEFAULT)


# What the unset GEOSSL_PAINN_SPARSE_BUCKETS means for the handles of a DeviceLoader: the outcome of the measurement in
# profiles/painn_bucket_bench.json by the rule stated there.
PAINN_SPARSE_BUCKETS_DEFAULT = True


def painn_sparse_buckets(handle):
    """``GEOSSL_PAINN_SPARSE_BUCKETS``: PaiNN batches of a step that reads no pair tuples (Supervised, LEP) with a
    structure above 255 atoms (or ``GEOSSL_SPARSE_PAIRS=1``) and radius edges on the device replay one capacity-bucket
    graph per batch size (``bucket.SPARSE`` with an edges part; the atom-tile kernels under a device-side atom count).
    ``1``: handles and collated batches; ``0``: neither - eager launches, a per-structure graph for a batch object that
    comes back.  Unset: handles do (``PAINN_SPARSE_BUCKETS_DEFAULT``: on shuffled pockets their step through the bucket is
    25 - 39 % shorter than the fastest route before it), collated batches do not (opt-in: their step
    still pays the host's collation and upload).
    ``GEOSSL_SPARSE_BUCKETS`` is SchNet's switch and does not open this bucket."""
    v = env("GEOSSL_PAINN_SPARSE_BUCKETS")
    if v == "0":
        return False
    return True if v == "1" else bool(handle) and PAINN_SPARSE_BUCKETS_DEFAULT


# What the unset GEOSSL_MD17_COMPLETE_EDGES means for a PaiNN batch the complete pair list can serve (finetune_md17.py):
# the outcome of the measurement in profiles/md17_bench.json by the rule stated there.
MD17_COMPLETE_EDGES_DEFAULT = True


def md17_complete_edges(applies):
    """``GEOSSL_MD17_COMPLETE_EDGES``: PaiNN's MD17 step and evaluation run on the interned complete pair list of
    (batch size, atoms per molecule) in place of the frame's own radius list - the cosine cutoff's ``[d < r]`` factor makes
    every pair beyond the cutoff an exact zero, and the interned index tensors let one captured graph replay for a whole
    trajectory.  ``applies``: every molecule of the batch has the same size n <= 33 and the backbone is the stock PaiNN;
    where it does not, no value of the switch substitutes anything.  ``1``: wherever it applies; ``0``: never - the
    batch's own edges, the route before; unset: ``MD17_COMPLETE_EDGES_DEFAULT``."""
    if not applies:
        return False
    v = env("GEOSSL_MD17_COMPLETE_EDGES")
    if v == "0":
        return False
    return True if v == "1" else MD17_COMPLETE_EDGES_DEFAULT


# What the unset GEOSSL_PAINN_TILE means for a layout with a structure above 255 atoms: the outcome of the measurement in
# profiles/painn_tile_bench.json by the rule stated there.
PAINN_TILE_DEFAULT = True


def painn_tile(max_n):
    """``GEOSSL_PAINN_TILE``: PaiNN's fused F = 128 interaction runs on the atom-tile kernels (``painn_tile.hip``: one
    launch per interaction block and pass, over all atoms).  ``1``: every layout those kernels serve - how tests and A/B
    runs reach them on small molecules; ``0``: never - the molecule-staged and per-atom kernels, call for call.  Unset:
    layouts whose largest structure is above 255 atoms (``bucket.MAX_N``), if the measurement supports it
    (``PAINN_TILE_DEFAULT``)."""
    v = env("GEOSSL_PAINN_TILE")
    if v == "0":
        return False
    if v == "1":
        return True
    return PAINN_TILE_DEFAULT and max_n > 255
