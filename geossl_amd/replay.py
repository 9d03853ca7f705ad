"""Capturing a step into HIP graphs and replaying it: the one capture every owner of graphs goes through (``warm_up``,
``capture``), its bounded memories (``seen_before``, ``make_room``), the copy into a graph's static inputs (``copy_static``),
the graphs per batch structure (``StructureGraphs``) and per training step (``StepGraphs``), a replayed loss's thread switch.
"""
import ctypes as C
import gc
import threading
import time
import warnings
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, bucket as bk
from ._lib import call, ptr, stream
from .batch import Batch, TripleBatch, structure_fingerprint, tensor_tag
from .layout import get_layout
from .switches import env as _env

_OWN_CAPTURE = [0]  # > 0 while StepGraphs._capture has a capture open


def own_capture_open():
    """True while a StepGraphs capture of this library is recording on the current stream: the one situation in which the
    step's passes leave clearing the gradient buffer to StepGraphs.refresh.  A caller that captures the step in a CUDA
    graph of ITS OWN gets the fill recorded into that graph like any other launch."""
    return _OWN_CAPTURE[0] > 0 and torch.cuda.is_current_stream_capturing()


# ---- the capture ---------------------------------------------------------------------------------------------------------
_WARMING = [0]  # > 0 while the passes of a warm_up run


def warming_up():
    """True inside the passes of `warm_up`: extra runs of the step that are not steps of the caller.  A step with state
    beside its gradients (the BatchNorm buffers of the RR heads) keeps that state out of them."""
    return _WARMING[0] > 0


def warm_up(passes):
    """`passes()` on a side stream, off the capture that follows: builds the cached layouts, sets kernel attributes.
    Nothing may be pending on the device when that capture starts (in a multi-rank job the collective's watchdog thread
    polls events of earlier all-reduces), and calls of other threads must not invalidate it: the device is drained."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _WARMING[0] += 1
    try:
        with torch.cuda.stream(side):
            passes()
    finally:
        _WARMING[0] -= 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


class capture:
    """``with capture(owner, "the ... step", flag) as cap: graph, out = cap.record(fn)`` - `fn` recorded into a new graph
    in `owner.pool` (adopted from the owner's first graph; a second `record` adds a graph to the same pool).  A capture is
    an optimisation: an exception inside the block becomes a warning, the device is drained, the owner's attribute `flag`
    is cleared and ``cap.ok`` is False behind the block.  own=True (StepGraphs): `own_capture_open` holds inside it.

    No garbage collection while a capture is open: a collection that happens to run there finalises whatever old
    graphs, events and streams sit in unreachable cycles (an engine of a model that is gone), and destroying a
    graph or querying an event inside a capture aborts the process.  (Not collecting up front either: a full
    collection of a process with torch loaded costs 45 ms, as much as the rest of the capture.)"""

    def __init__(self, owner, what, flag, own=False):
        self.owner, self.what, self.flag, self.own, self.ok = owner, what, flag, own, True

    def __enter__(self):
        self.gc_was_on = gc.isenabled()
        gc.disable()
        _OWN_CAPTURE[0] += self.own
        return self

    def record(self, fn, stream=None):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=self.owner.pool, stream=stream, capture_error_mode="thread_local"):
            out = fn()
        if self.owner.pool is None:
            self.owner.pool = graph.pool()
        return graph, out

    def __exit__(self, kind, e, tb):
        _OWN_CAPTURE[0] -= self.own
        if self.gc_was_on:
            gc.enable()
        if kind is None or not issubclass(kind, Exception):
            return False
        warnings.warn("HIP-graph capture of %s failed (%s: %s); running eagerly" % (self.what, kind.__name__, e))
        torch.cuda.synchronize()
        self.ok = False
        setattr(self.owner, self.flag, False)
        return True


def seen_before(memory, key, bound):
    """True from the second call on for one key.  `memory`: a bounded OrderedDict (a forgotten entry only moves the moment
    of a capture: a loader that never repeats a structure must not grow it for ever)."""
    seen = key in memory
    memory[key] = True
    memory.move_to_end(key)
    while len(memory) > bound:
        memory.popitem(last=False)
    return seen


def make_room(graphs, max_graphs):
    """Drop the least recently used entries of the OrderedDict `graphs` until one more fits."""
    while len(graphs) >= max_graphs:
        graphs.popitem(last=False)


def copy_static(pairs, zero=None):
    """This step's tensors into a graph's static inputs, `pairs` of (dst, src), and the float32 buffer `zero` cleared - in
    ONE launch when every pair is contiguous device memory of one dtype and shape (two pairs: geossl_copy2; anything else
    geossl_copy_n, the fill as an entry without a source), else copy by copy."""
    if all(s.is_cuda and s.is_contiguous() and d.is_contiguous() and s.dtype == d.dtype and s.shape == d.shape
           for d, s in pairs):
        if len(pairs) == 2 and zero is None:
            (d0, s0), (d1, s1) = pairs
            call("geossl_copy2", ptr(d0), ptr(s0), d0.numel() * d0.element_size(), ptr(d1), ptr(s1),
                 d1.numel() * d1.element_size(), stream())  # one launch instead of two copies
        else:
            jobs = [(d, s, d.numel() * d.element_size()) for d, s in pairs]
            jobs += [] if zero is None else [(zero, None, zero.numel() * 4)]
            cb = _lib.CopyBatch()
            for k, (d, s, nb) in enumerate(jobs):
                cb.dst[k], cb.src[k], cb.bytes[k] = ptr(d), ptr(s), nb
            call("geossl_copy_n", C.byref(cb), len(jobs), stream())
    else:
        for d, s in pairs:
            d.copy_(s)
        if zero is not None:
            zero.zero_()


# ---- one graph per batch structure ---------------------------------------------------------------------------------------
def sizes_key(n_atoms, sizes):
    """Key of a structure whose index tensors are a function of the host sizes: equal size sequences share a graph."""
    return ("sizes", int(n_atoms), np.asarray(sizes, dtype=np.int32).tobytes())


def tensors_key(*tensors):
    """Key of a structure only its tensor OBJECTS identify (batch.tensor_tag: object, version, shape; None stays None)."""
    return ("tensors",) + tuple(tensor_tag(t_) for t_ in tensors)


def owned_batch_vector(batch_vec, sizes=None):
    """A graph binds the ADDRESSES of the index structures (mol_ptr, pair_ptr, pair atoms, aggregation work list, the loop
    plan), which are cached on the batch vector (`_geossl_layout`).  Its entry therefore owns this private clone - with the
    host sizes (`sizes`, else the vector's own while its version matches) re-attached, so the clone builds the same layout
    - and keeps it alive as long as the graph: the caller's batch may be freed without those addresses being reused."""
    bvec = batch_vec.clone()
    hs = getattr(batch_vec, "_geossl_sizes", None)   # (host sizes, tensor version), layout.prepare_batch
    if sizes is None and hs is not None and hs[1] == batch_vec._version:
        sizes = hs[0]
    if sizes is not None:
        bvec._geossl_sizes = ([int(n) for n in sizes], bvec._version)
    return bvec


def parameter_addresses(*modules):   # (None: skipped; an owner of graphs is rebuilt when its modules' parameters moved)
    return tuple(p.data_ptr() for m in modules if m is not None for p in m.parameters())


class StructureGraphs:
    """One captured graph per batch structure: the counterpart of StepGraphs' buckets and the one place that knows the
    protocol.  ``graphs``: the entries an owner's capture builds, by key, least recently used first, at most ``max_graphs``, in
    ONE memory ``pool``; ``captures`` counts them; a failed capture clears ``enabled`` (FT's ``use_graph``).  A key is captured
    at first sight where its owner says so, else at the second within ``seen_bound`` sightings (a loader that never repeats a
    structure never pays).  Nothing is looked up or captured while the current stream is capturing: that call runs eagerly,
    into the caller's graph.  Derived: GF graphed.GraphedForward, FT graphed.ForceTrainer, P finetune_md17._Predictor.
    served (else eager): GF fingerprint kind "sizes" on CUDA; FT all while use_graph; P host sizes, PaiNN on complete edges
    key: GF its fingerprint; FT PaiNN tensors_key(bvec, edges), else sizes_key or tensors_key(bvec); P sizes_key + x.shape
    ... captured at first sight: GF, P for equal-sized molecules; FT for a sizes_key
    1-D against 2-D x on a hit: GF, FT that call runs eagerly and the graph stays; P the shape is in the key
    the call that captures: GF, P replay without a copy (the statics are clones of the batch); FT copies in, then replays
    warm-up: GF eager pass, loop_plan(); FT the body twice; P eager probe (None: no capture), eager pass, SchNet loop_plan()
    poll_status after a replay: GF, P yes; FT no, deliberately for now (host work in a step whose launches are pinned)"""

    def __init__(self, max_graphs, enabled=True, seen_bound=4096):
        self.graphs, self._seen, self.pool, self.captures = OrderedDict(), OrderedDict(), None, 0
        self.max_graphs, self.enabled, self.seen_bound = max_graphs, enabled, seen_bound

    def get(self, key):   # (for a caller that only replays: the entry, now the most recently used one, or None)
        g = self.graphs.get(key)
        if g is not None:
            self.graphs.move_to_end(key)
        return g

    def lookup(self, key, first_sight, make):
        """-> (entry, whether it was just made), or None: this call runs eagerly - cache off, stream capturing, a first
        sighting, or a failed ``make() -> entry or None``.  ``first_sight() -> bool`` is asked only on a miss."""
        if not self.enabled or (torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()):
            return None   # (is_initialized: a host without a device has no stream to ask)
        g = self.get(key)
        if g is not None:
            return g, False
        if not first_sight() and not seen_before(self._seen, key, self.seen_bound):
            return None
        g = make()
        if g is None:
            return None
        self.captures += 1
        make_room(self.graphs, self.max_graphs)
        self.graphs[key] = g
        return g, True


# ---- the graphs of a training step -------------------------------------------------------------------------------------
_NOISE_KEYS = ("pos_noise", "noise_level_1", "dist_noise_1", "noise_level_2", "dist_noise_2")


class StepGraphs:
    """HIP graphs of forward + backward of a step; all in ONE memory pool (their activations are dead between
    steps, so N graphs cost the device memory of the largest plus the static inputs and the loss of each).
    ``fwd_bwd(batch, noise) -> loss`` is the owner's eager step; it must leave the gradients in buffers that are the same
    for every call (the graph binds their addresses).  Least-recently-used graphs are dropped beyond ``max_graphs``.

    Which graph serves a batch (``mode="auto"``):

    * a batch of EQUAL-SIZED molecules, and anything a bucket cannot take (PaiNN's geometry-dependent edge list, sampled
      tuples without the ``_sampled`` mark, batches built by hand): one graph per ``structure_fingerprint`` - the size
      sequence, or the tensor objects;
      a structure that only a fingerprint identifies is captured on its SECOND sighting (a loader that never repeats one
      never pays for a capture);
    * a batch with a SPARSE layout (a structure of 256 to 1024 atoms - LBA's pockets - or GEOSSL_SPARSE_PAIRS=1) in a
      one-view SchNet step that reads no pair tuples (``pair_tuples=False``: Supervised, and LEP with its 2B structures
      [active | inactive]): one graph per number of structures in a sparse bucket (``bucket.SPARSE``) - by default the handles of a DeviceLoader, with
      ``GEOSSL_SPARSE_BUCKETS=1`` collated batches too (``=0``: neither; such a batch is served as the first entry says);
      a PaiNN step of that kind whose batch brings radius edges on the device (a dataset built with ``radius=``, or a
      collated ``radius_edge_index``) takes the same bucket with an edges part, under ``GEOSSL_PAINN_SPARSE_BUCKETS``;
    * every other SchNet batch - ragged molecules in shuffled order, the reference's loader (pretrain_GeoSSL.py:301) - one
      graph per (molecules in the batch, tuple option) at a CAPACITY (``geossl_amd/bucket.py``): the graph's kernels read
      the batch's real atom / pair-slot / super-edge counts and every index structure from device memory, so ONE graph
      replays on any size sequence; a batch that outgrows the capacity makes a larger bucket (its graph is captured
      again: a handful of times at the start of a run).  SAMPLED tuples (``AtomTupleExtractor(ratio < 1)``: the handles
      of a ``DeviceLoader(tuple_ratio=)``, collated batches of the host extractor's molecules) take a bucket whose option
      is ``(option, ratio)``: the kept counts are a function of the sizes, the tuples are drawn or checked on the device
      behind the gather - handles by default, collated batches under ``GEOSSL_SAMPLED_BUCKETS=1`` (``=0``: neither;
      such a batch is then served as the first entry says).

    ``mode="structure"``: per-structure graphs only, captured at the first sighting (pre-collated, device-resident
    batches that come back every epoch).

    An owner goes from a batch to a replay through ``plan`` and ``load``."""

    def __init__(self, fwd_bwd, model_3d, max_graphs=256, split=None, mode="auto", normalize=False, modules=None,
                 noise_keys=None, views=2, pair_tuples=True):
        # split = (fwd(batch, noise) -> loss with its autograd graph, bwd(loss)): forward and backward captured as TWO
        # graphs (same pool, same capture stream; replayed in this order) - the forward's loss is then on the device
        # before the backward runs, and the backward can run on a side stream while the host goes on (_AutogradStep)
        self.fwd_bwd, self.model_3d, self.max_graphs, self.split = fwd_bwd, model_3d, max_graphs, split
        self.mode, self.normalize = mode, normalize
        self.modules = modules  # (backbone, head, head): what bucket.modules_ok looks at (None: no capacity buckets)
        # the random draws a step takes as static inputs (the contrastive objectives: the position noise only)
        self.noise_keys = _NOISE_KEYS if noise_keys is None else tuple(noise_keys)
        # views of the molecules the backbone sees in a bucket (1: the Distance / Charge Prediction steps)
        self.views = views
        # the step reads the batch's pair tuples (step.Objective.pair_tuples); False: a one-view SchNet step whose
        # batches with a sparse layout go through a sparse bucket
        self.pair_tuples = pair_tuples
        self.graphs, self.pool = OrderedDict(), None
        self.enabled = True
        self.captures = 0
        self._warned = False
        self._seen = OrderedDict()
        self.bucket_ok = True   # cleared when a bucket capture failed: per-structure graphs from then on
        self._mod_ok = None
        # a float32 buffer the owner wants cleared before every replay (its flat gradient buffer): done by the launch that
        # refreshes the graph's inputs instead of a fill node inside the graph (one launch less per step)
        self.zero_with_refresh = None

    def __len__(self):
        return len(self.graphs)

    # ---- which graph
    def bucket_key(self, batch):
        """("bucket", molecules, option) when the batch goes through a capacity bucket (bucket.route), else None."""
        if (self.mode != "auto" or not self.bucket_ok or _env("GEOSSL_NO_BUCKETS") or self.modules is None):
            return None
        option = bk.route(batch, self.model_3d, self.views, self.pair_tuples, self.normalize)
        if option is None or not self._modules_ok():
            return None
        return ("bucket", len(batch._sizes), option)

    def _modules_ok(self):
        """bucket.modules_ok of this engine's modules, remembered per state of the switches it reads (the modules of a
        StepGraphs are fixed: a replaced parameter rebuilds the engine, _AutogradStep.unchanged / DDMTrainer)."""
        env = tuple(_env(k) for k in bk.MODULE_SWITCHES + bk.PAINN_SWITCHES)
        if self._mod_ok is None or self._mod_ok[0] != env:
            self._mod_ok = (env, bk.modules_ok(*self.modules))
        return self._mod_ok[1]

    def lookup(self, batch):
        """The graph that serves this batch (None: not captured yet, or its bucket is too small)."""
        key = self.bucket_key(batch)
        if key is not None:
            g = self.graphs.get(key)
            counts = None if g is None else g["bucket"].fits_batch(batch)
            if counts is None:
                return None
            g["counts"] = counts
            self.graphs.move_to_end(key)
            return g
        fp = structure_fingerprint(batch, self.model_3d)
        g = self.graphs.get(fp)
        if g is not None:
            self.graphs.move_to_end(fp)
        return g

    def capture_now(self, batch):
        """Should a batch without a graph be captured at this sighting?  Buckets and equal-sized molecules: yes (their
        graph serves every later batch of the kind); a structure known by fingerprint only: from its second sighting on
        (mode "structure": always)."""
        if self.mode != "auto" or self.bucket_key(batch) is not None:
            return True
        if bk.is_uniform(batch) and getattr(batch, "_canonical", None) is not None and self.model_3d == "schnet":
            return True
        # (a bounded memory of hashes: a collision or a forgotten entry only moves the moment of a capture)
        return seen_before(self._seen, hash(structure_fingerprint(batch, self.model_3d)), 8192)

    # ---- from a batch to a replay
    def plan(self, batch):
        """-> (the graph that serves this batch or None, whether one is to be captured for it now).  (None, False): this
        step runs eagerly - the first sighting of an index structure that only its own graph can serve (unmarked sampled
        tuples, PaiNN edge lists, batches built by hand): a loader that never repeats such a structure never pays for a
        capture, one that comes back is captured on its second step.  Ragged SchNet batches of a loader share ONE
        capacity-bucket graph and equal-sized molecules one per-structure graph: those are captured right away."""
        g = self.lookup(batch)
        return g, g is None and self.capture_now(batch)

    def load(self, g, batch, inputs=None, write=None):
        """What `plan` decided, carried out -> the graph with this step's inputs written, ready to replay, or None: run
        this step eagerly (a capture on `inputs`, the tensors its static inputs are cloned from, failed and has cleared
        ``enabled``; or the bucket refused the batch's tensors).  `write(g, batch, inputs)`: the owner's per-step inputs."""
        if g is None:
            g = self.capture(batch, inputs)
            if g is None:
                return None
        if not self.refresh(g, batch):
            return None
        if write is not None:
            write(g, batch, inputs)
        return g

    # ---- capture
    def _evict(self):
        if len(self.graphs) >= self.max_graphs and not self._warned:
            warnings.warn("more than %d distinct batch structures: the least recently used step graphs are dropped "
                          "and captured again when they come back (raise max_graphs, or run without graphs)"
                          % self.max_graphs)
            self._warned = True
        make_room(self.graphs, self.max_graphs)

    def capture(self, batch, noise):
        """Capture fwd_bwd on static inputs: clones of x / positions / the five noise tensors with the batch's own index
        tensors bound as they are (per-structure graph), or the buffers of a capacity bucket filled from the batch.  None
        when the capture failed: the owner runs eagerly (a failed bucket: per-structure graphs) from then on."""
        key = self.bucket_key(batch)
        if key is not None:
            g = self._capture_bucket(key, batch, noise)
            if g is not None or not self.enabled:
                return g
            key = None  # the bucket could not be captured: this batch's own structure
        fp = structure_fingerprint(batch, self.model_3d)
        self._evict()
        if getattr(batch, "_triples", False):   # (triples and targets bound as they are, like the other index tensors)
            sb = TripleBatch(batch.x.clone(), batch.positions.clone(), batch.batch, batch.super_edge_index,
                             batch.super_edge_angle, getattr(batch, "radius_edge_index", None), batch.num_graphs,
                             getattr(batch, "_sizes", None))
        else:
            sb = Batch(batch.x.clone(), batch.positions.clone(), batch.batch, batch.super_edge_index,
                       getattr(batch, "radius_edge_index", None), batch.num_graphs, getattr(batch, "_sizes", None),
                       getattr(batch, "_canonical", None))
        sn = {k: noise[k].clone() for k in self.noise_keys}
        g = self._capture(sb, sn)
        if g is not None:
            self.graphs[fp] = g
        return g

    def _capture_bucket(self, key, batch, noise):
        old = self.graphs.pop(key, None)
        prev = None if old is None else old["bucket"].sizes()
        del old  # (its graph and static buffers go before the larger ones are made)
        self._evict()
        args = bk.Bucket.sizing(batch, key[2], self.model_3d, self.views,
                                getattr(getattr(self.modules[0], "radial_basis", None), "n_rbf", 20), prev)
        try:
            bkt = bk.Bucket(**args)
            counts = bkt.fill(batch)
        except (ValueError, RuntimeError) as e:
            warnings.warn("capacity bucket not usable for this batch (%s); per-structure graphs from now on" % e)
            self.bucket_ok = False
            return None
        sn = bkt.static_noise(self.noise_keys)
        g0 = dict(bucket=bkt, noise=sn, counts=counts)
        self.copy_noise(g0, noise)
        g = self._capture(bkt.batch, sn)
        if g is None:
            self.enabled, self.bucket_ok = True, False  # (eager fallback is for a failed per-structure capture)
            return None
        g.update(bucket=bkt, counts=counts)
        self.graphs[key] = g
        return g

    def _capture(self, sb, sn):
        timing = [] if _env("GEOSSL_CAPTURE_TIMING") else None

        def lap(name):
            if timing is not None:
                torch.cuda.synchronize()
                timing.append((name, time.perf_counter()))
        lap("start")
        warm_up(lambda: [self.fwd_bwd(sb, sn) for _ in range(2 if not self.graphs else 1)])
        lap("warm-up passes")
        graph_bwd = None
        # (own: the owner's passes leave the gradient buffer to `refresh` only inside THIS capture)
        with capture(self, "the DDM step", "enabled", own=True) as cap:
            # an owner's forward may return (loss, extra): extra = static outputs beside the loss
            if self.split is None:
                graph, loss = cap.record(lambda: self.fwd_bwd(sb, sn))
                loss, extra = loss if isinstance(loss, tuple) else (loss, None)
            else:
                side = torch.cuda.Stream()  # both captures on ONE stream: autograd runs a node's backward where its forward ran
                graph, live = cap.record(lambda: self.split[0](sb, sn), stream=side)
                live, extra = live if isinstance(live, tuple) else (live, None)
                graph_bwd, _ = cap.record(lambda: self.split[1](live), stream=side)
                loss = live.detach()
                del live
        if not cap.ok:
            return None
        lap("capture + instantiate")
        if timing is not None:
            print("capture timing (ms):", ", ".join("%s %.1f" % (n, 1e3 * (t - timing[i][1])) for i, (n, t) in enumerate(timing[1:])))
        self.captures += 1
        return dict(graph=graph, graph_bwd=graph_bwd, batch=sb, noise=sn, loss=loss, zero=self.zero_with_refresh,
                    extra=extra)

    # ---- per-step refresh of a graph's static inputs
    @staticmethod
    def noise_views(g, batch=None):
        """The graph's five static noise tensors at the size of THIS batch (a bucket's are capacity-sized: the real rows
        are the leading ones) - what a caller's draws are written into."""
        bkt = g.get("bucket")
        if bkt is None:
            return g["noise"]
        N, P, S, W = g["counts"]
        # (the noise levels are per molecule: B is exact; a mask list holds k <= N entries, copy_noise writes k)
        real = {"N": N, "S": S}
        return {k: (v[:real[r]] if (r := bk.NOISE_SHAPES[k][0]) in real else v) for k, v in g["noise"].items()}

    @staticmethod
    def copy_noise(g, noise):
        into = StepGraphs.noise_views(g)
        for k in into:   # (the graph's own draws: all five of a DDM step)
            dst = into[k]
            # (the leading k entries: the mask kernel reads as many as the batch's k; a paired step - LEP - has one
            # label per PAIR, the leading half of a bucket's structure count)
            if k == "mask_idx" or (k == "target" and noise[k].numel() * 2 == dst.numel()):
                dst = dst[:noise[k].numel()]
            dst.copy_(noise[k].view_as(dst))

    @staticmethod
    def refresh(g, batch, noise=None):
        """x, positions and (if given) the five noise tensors of this step into the graph's static inputs; a bucket also
        gets the batch's index structures and real counts."""
        bkt, zero = g.get("bucket"), g.get("zero")
        if bkt is not None:
            try:
                bkt.fill(batch, g["counts"], zero=zero)
            except ValueError as e:  # (tensors the bucket cannot copy: the caller runs this step eagerly)
                warnings.warn("capacity bucket refused a batch (%s); the step runs eagerly" % e)
                return False
        elif getattr(batch, "_dataset", None) is not None:
            # molecules of a device-resident dataset: gathered straight into the graph's static x / positions
            sb = g["batch"]
            batch._dataset.gather_into(batch, sb.x, sb.positions, get_layout(sb.batch).mol_ptr, zero)
        else:
            copy_static([(g["batch"].x, batch.x), (g["batch"].positions, batch.positions)], zero)
        if noise is not None:
            StepGraphs.copy_noise(g, noise)
        return True


# ---- the autograd thread switch of a replayed loss -----------------------------------------------------------------------
_MT_PENDING = []   # tickets of this process whose autograd thread switch is still to be put back


def _single_thread_backward(ticket):
    """The loss of a replayed step has ONE node behind it (_ReplayedLoss) and its 59 AccumulateGrads; autograd would hand
    them to its per-device worker thread and wake the caller when it is done - a hand-over that costs 0.13 ms per
    backward() (measured, tools/ref_loop_profile.py), a fifth of a whole step at the reference's batch size.  With
    multithreading off the calling thread runs the backward itself.  The switch is autograd's own, thread-local
    (torch.autograd.set_multithreading_enabled); it is turned off when do_DDM hands out the loss and put back to what the
    caller had at the optimizer step that follows (a global optimizer post-step hook, optim.py) or, without one, at the
    next do_DDM - it cannot be put back from inside the backward: the engine restores the thread state it saw at
    backward()'s entry when the pass ends.  Other autograd work of the caller after the step - graphs that span several
    devices - sees its own setting.  GEOSSL_KEEP_AUTOGRAD_THREADS leaves the switch alone."""
    if _env("GEOSSL_KEEP_AUTOGRAD_THREADS"):
        return
    if torch.autograd.is_multithreading_enabled():
        torch.autograd.set_multithreading_enabled(False)
        # a small token, not the ticket: the pending list must not keep a step's gradient buffer alive, and the switch is
        # THREAD-LOCAL - it is put back only by the thread that turned it off
        token = ticket["mt_token"] = _MtToken(threading.get_ident())
        _MT_PENDING.append(token)


class _MtToken:
    __slots__ = ("thread", "live")

    def __init__(self, thread):
        self.thread, self.live = thread, True


def _restore_backward_threads(ticket=None):
    """Put autograd's multithreading switch back for `ticket` (None: for every step of THIS thread that is still
    pending).  A call from another thread (a ticket finalised by the garbage collector there) leaves the token pending:
    the owning thread's next step / optimizer hook restores it."""
    me = threading.get_ident()
    if ticket is not None:
        token = ticket.pop("mt_token", None) if isinstance(ticket, dict) else None
        todo = [] if token is None else [token]
    else:
        todo = [t for t in _MT_PENDING if t.thread == me]
    for t in todo:
        if t.live and t.thread == me:
            t.live = False
            torch.autograd.set_multithreading_enabled(True)
    _MT_PENDING[:] = [p for p in _MT_PENDING if p.live]
