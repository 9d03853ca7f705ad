"""Capacity buckets: the static inputs and index structures behind a step graph that is replayed on batches of ANY
size sequence.

The reference's loader is ``DataLoaderAtomTuple(dataset, batch_size, shuffle=True)`` over ragged molecules
(examples/pretrain_GeoSSL.py:301, Geom3D/dataloaders/dataloaders_AtomTuple.py:81-88; with BFS masking the sizes are
re-drawn every epoch, Geom3D/datasets/datasets_3D.py:24-67): no two batches share a size sequence, so a graph keyed by
the sequence (``batch.structure_fingerprint``) is never replayed there.  A ``Bucket`` fixes what a captured
graph binds - addresses, grids, by-value counts - at a CAPACITY (atoms, pair slots, super-edges, work items of the
aggregation; the number of molecules is the loader's batch size) and turns everything else into device DATA:

* every index structure of the step (``mol_ptr`` / ``pair_ptr`` of the two-view batch, the pair-slot atoms, the
  aggregation's work list, ``se_ptr``, the divisor of NCSN.py:210-212, the incidence lists) lives in static buffers that
  ``fill`` rewrites before a replay: the pointer arrays and the work list are computed on the host from the molecule
  sizes the collation knows (a few cumulative sums over B integers) and go up in ONE pinned copy, the per-slot arrays are
  produced on the device by the layout kernels launched eagerly with the batch's exact counts;
* the real counts sit in ``dims`` (int32, device); the kernels of the captured step are the ``_dyn`` entry points of
  include/geossl_hip.h, which take their grid from the capacity and their row count from ``dims``: rows past the real
  count are never read or written.

What a bucket holds is a closed list of PARTS, decided once from (kind, option) - ``BlobLayout.parts``, in this order:

======== ============================== ============================== ==========================================
part     present when                   blob sections it writes        device buffers
======== ============================== ============================== ==========================================
atoms    always                         dims, mol_ptr, src_off         x, positions, batch_vec, b2
pairs    not sparse                     pair_ptr, stats; SchNet: work  SchNet: pair_i, pair_j, agg_targets
tuples   "combination" / "permutation"  se_ptr, inc_ptr                sei, inc_idx
sampled  (option, ratio), ratio < 1      se_ptr, mol_id                 sei, inc_idx; inc_ptr is the device's too
triples  "triples" (views = 1)          dims[D_T], t_src_off, t_ptr    triples, triple_angle
edges    PaiNN, not sparse              e_src_off, e_ptr, big0, big1   the _Edges buffers, the two status words
sedges   PaiNN, sparse                  e_src_off, e_ptr               radius_edge_index, both incidence lists, status
======== ============================== ============================== ==========================================

(pairs also hands the gather the ADDRESS of se_ptr, which the gather takes in every dense bucket; the words of se_ptr
are written by tuples and stay zero without it.)

A part is made once.  It holds the slices of the blob sections it writes (``write_host``: integers and numpy arrays
only - ``host_image`` runs without a device); ``attach`` allocates its static buffers and writes every pointer that never
changes into the bucket's one ``Gather`` struct; ``bind`` (what a fill sets on that struct: sources, a handle's edges)
and ``after`` (what is launched behind the gather: the triples of a handle, PaiNN's edge layout) exist only on the
parts that need them.  ``Bucket.fill`` is one path over the parts.  The blob's
offsets are one running sum over the section table of ``BlobLayout``; a section whose part is absent keeps its offset
with length 0 (``dims`` .. ``stats`` exist in every bucket).  The pairs part is every dense bucket's: ``pair_ptr`` and the
divisor are functions of the sizes that PaiNN and triples buckets carry too; the pair SLOTS are SchNet's.

A SPARSE bucket (option ``SPARSE``; one view; structures of up to 1024 atoms) is, for SchNet, the bucket whose only part is
atoms: the backbone builds the compacted pair list from the positions inside the captured step
(geossl_sparse_pairs_build_dyn), at the capacity ``P_cap = 33 N_cap`` that every batch which fits the atoms fits too.
Its fill uploads mol_ptr and the counts and gathers the atom rows: nothing else of the batch is read.
The sparse PaiNN bucket (kind "painn") adds the sparse edges part: the batch's ``radius_edge_index`` at ``E_cap`` (a
handle's edges come with the gather launch, a collated batch's by a copy) and both incidence lists at capacity,
rewritten per fill by one launch (geossl_painn_incidence_layout_dyn); the atom-tile interaction kernels read them under
the device-side atom count.  No group arrays, no stage-cap atom lists, no size class of PAINN_MAX_N_CLASSES.

Beside the class: which bucket a batch takes (``route``), how one is sized for a batch (``Bucket.sizing``, ``for_batch``), whether
a batch still fits (``Bucket.fits_batch``), and the shapes of a step's static noise tensors (``NOISE_SHAPES``).

Layout of the fused two-view batch in a bucket: ``[view 0 atoms | view 1 atoms | unused]`` - view 1 starts right behind
the REAL atoms of view 0 (``dims[N]``), so the molecule CSR stays contiguous.
"""
import ctypes as C

import numpy as np
import torch
from .switches import env as _env, masked_painn_buckets, painn_sparse_buckets, sampled_buckets, sparse_buckets

from . import _lib
from ._lib import call, ptr, stream
from .batch import Batch, TripleBatch, _tensor_uid, kept_tuples

MAX_N = 255         # largest molecule a bucket takes (the limit of the aggregation's work list and of the heads)
SMALL_N = 33        # ... and the largest one of the register-form aggregation's size classes: buckets whose molecules
                    # all fit it keep the flat pair-geometry kernel and the ragged layer loop
MAX_N_CLASSES = (SMALL_N, 64, 128, MAX_N)   # a bucket's bound on the molecule size (LDS of the radius-graph kernel)
D_N, D_N2, D_P2, D_S, D_W, D_B, D_N6, D_E2, D_BIG0, D_BIG1, D_T = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10   # words of `dims`
DIMS_WORDS = 16
PAINN_MAX_N_CLASSES = (22, 33, 44, 64, 96, 128, MAX_N)   # PaiNN: the bound sizes the LDS of its per-molecule kernels


class DynDims:
    """Device addresses of a bucket's real counts, as the ``dyn_*`` arguments of the ``_dyn`` entry points."""

    def __init__(self, dims):
        base = dims.data_ptr()
        self.tensor = dims
        self.n_atoms = base + 4 * D_N       # atoms of one view (= the row offset of view 1)
        self.n_atoms2 = base + 4 * D_N2     # atoms of the two-view batch
        self.n_pairs2 = base + 4 * D_P2     # pair slots of the two-view batch
        self.n_super = base + 4 * D_S       # super-edges of one view
        self.n_work = base + 4 * D_W        # work items of the aggregation
        self.n_atoms2x3 = base + 4 * D_N6   # PaiNN: rows of the vector features viewed as [3 N2, F]
        self.n_edges2 = base + 4 * D_E2     # PaiNN: edges of the two-view batch
        self.n_big = (base + 4 * D_BIG0, base + 4 * D_BIG1)   # PaiNN: atoms of the molecules above the two stage caps
        self.n_triples = base + 4 * D_T     # atom triples of the batch (a "triples" bucket: angle prediction)


class _Layout:
    """Duck type of layout.MolLayout for the two-view batch of a bucket (capacity shapes, static buffers)."""

    uniform = False
    order = None
    _sizes_host = None

    big = None
    _warned_cap = False

    def loop_plan(self, *a, **k):
        return (None, 0)   # (the layer loop is a plan for uniform batches: they keep their per-structure graph)

    def big_atoms(self, cap):
        """PaiNN: (static list of the atoms of molecules above `cap` atoms, its capacity, device address of the real
        count) - rewritten per step by Bucket.fill; None for a cap the bucket was not made for."""
        if self.big is None:
            return None
        got = self.big.get(cap)
        if got is None and 0 < cap < self.max_n and not _Layout._warned_cap:
            import warnings
            _Layout._warned_cap = True
            warnings.warn("PaiNN bucket has no atom list for stage cap %d (lists: %s): the molecule-staged kernels are "
                          "skipped for the whole batch (the bucket was made for another radial basis or "
                          "GEOSSL_PAINN_MMA_CAP changed since)" % (cap, sorted(self.big)))
        return got


class _SuperEdges:
    """Duck type of layout.SuperEdgeLayout for a bucket."""


class _Edges:
    """Duck type of layout.EdgeLayout for the two-view batch of a PaiNN bucket: every array is a static buffer at the
    bucket's capacity that geossl_painn_edge_layout rewrites per step; the groups of a molecule end at mol_grp_end."""

    def groups(self, side, mol_ptr=None):
        assert side == "i"
        return (self.row_edge, self.grp_atom, None, self.mol_grp)


def max_n_class(hi, prev=None, model_3d="schnet"):
    """The bucket's bound on the molecule size for a batch whose largest molecule has `hi` atoms."""
    classes, exact = (PAINN_MAX_N_CLASSES, 44) if model_3d == "painn" else (MAX_N_CLASSES, SMALL_N)
    # above the sizes whose class selects a faster kernel form (the register aggregation / flat geometry / ragged loop of
    # SchNet, the matrix-pipe interaction of PaiNN) the class only sizes LDS arrays: a quarter of head room there, so that
    # the next batch's largest molecule does not cost another capture
    want = hi if (hi <= exact or _env("GEOSSL_BUCKET_NO_HEADROOM")) else int(np.ceil(1.25 * hi))
    for c in classes:
        if want <= c and (prev is None or c >= prev):
            return c
    return MAX_N


def sizes_array(batch):
    """The batch's molecule sizes as an int64 array, made once per batch object."""
    arr = batch.__dict__.get("_geossl_sizes_np")
    if arr is None:
        arr = batch.__dict__["_geossl_sizes_np"] = np.asarray(batch._sizes, dtype=np.int64)
    return arr


TRIPLES = "triples"   # the "tuple option" of a bucket whose step reads atom triples and no pair tuples (angle prediction)
# ... and of a one-view SchNet bucket on the sparse pair list, for a step that reads neither (Supervised): no pair slots,
# no pair tuples, no aggregation work list; molecules of up to layout.SPARSE_MAX_N atoms
SPARSE = "sparse"
SPARSE_MAX_N_CLASSES = (256, 512, 1024)   # its bound on the molecule size (LDS of the list's build: up to 139 KB)


def is_sampled(option):
    """A SAMPLED tuple option ``(base, ratio)`` - ("combination", 0.3): AtomTupleExtractor(ratio < 1) output.  How many
    tuples a molecule keeps is ``batch.sampled_count`` of its enumeration - a function of the sizes, so se_ptr, S, the
    divisor and every capacity stay host work; WHICH tuples is per-step data of the bucket (the sampled part)."""
    return isinstance(option, tuple)


def base_option(option):
    """The enumeration a tuple option draws from: "combination" / "permutation" of a sampled one, else the option."""
    return option[0] if isinstance(option, tuple) else option


def sparse_max_n_class(hi, prev=None):
    """The sparse bucket's bound on the molecule size for a batch whose largest molecule has `hi` atoms (the classes
    double: the head room is in the class itself); never below a previous bucket's."""
    for c in SPARSE_MAX_N_CLASSES:
        if hi <= c and (prev is None or c >= prev):
            return c
    return SPARSE_MAX_N_CLASSES[-1]


def sparse_capacities(N, B, prev=None, sizes=None):
    """(N_cap, P_cap, 0, 0) of a sparse bucket: the atoms with the slack of `capacities`, the pair list at
    SPARSE_EDGES_PER_ATOM rows per atom of the capacity - layout.sparse_pair_capacity(sizes) <= 33 sum(sizes), so a
    batch that fits the atoms fits the list."""
    from .layout import SPARSE_EDGES_PER_ATOM
    N_cap = capacities(N, 0, 0, 0, B, prev=prev, sizes=sizes)[0]
    return (N_cap, SPARSE_EDGES_PER_ATOM * N_cap, 0, 0)


def _atom_tensors_ok(batch, N, x_dims=(2,), batch_vec=True):
    """What every fill copies of a collated batch by byte count: float32 positions [N, 3] and int64 x with N rows (of
    `x_dims` dimensions), with `batch_vec` the int64 batch vector [N] too - on the device, contiguous."""
    x, pos, bv = batch.x, batch.positions, (batch.batch if batch_vec else None)
    return (pos.is_cuda and pos.dtype == torch.float32 and pos.dim() == 2 and pos.size(1) == 3 and pos.is_contiguous()
            and pos.size(0) == N
            and x.is_cuda and x.dtype == torch.long and x.dim() in x_dims and x.is_contiguous() and x.size(0) == N
            and (bv is None or (bv.is_cuda and bv.dtype == torch.long and bv.dim() == 1 and bv.is_contiguous()
                                and bv.numel() == N)))


def sparse_tensors_ok(batch):
    """What a sparse bucket's fill copies of a collated batch: int64 x [N] or [N, c] and float32 positions [N, 3] on the
    device, contiguous, N the sum of the sizes (the batch vector is generated, pair tuples are not read)."""
    if not (torch.is_tensor(getattr(batch, "x", None)) and torch.is_tensor(getattr(batch, "positions", None))):
        return False
    return (_atom_tensors_ok(batch, int(sizes_array(batch).sum()), (1, 2), batch_vec=False)
            and not batch.positions.requires_grad and batch.x.device == batch.positions.device)


def sparse_eligible(batch, model_3d="schnet"):
    """Can this batch go through a SPARSE bucket?  Molecule sizes known on the host, 1 .. 1024 atoms, and a layout of
    them would be sparse (layout.want_sparse: a structure above 255 atoms, or GEOSSL_SPARSE_PAIRS=1).  A collated batch:
    tensors as `sparse_tensors_ok`; a handle on a device-resident dataset: unmasked, pair-tuple dataset (its tuple option
    is not read).  PaiNN: also radius edges on the device - a handle of a dataset built with ``radius=``, or a collated
    int64 ``radius_edge_index`` [2, E]."""
    from .layout import SPARSE_MAX_N, want_sparse
    sizes = getattr(batch, "_sizes", None)
    if sizes is None or not len(sizes):
        return False
    lo, hi = size_range(batch)
    if lo < 1 or hi > SPARSE_MAX_N or not want_sparse(hi):
        return False
    painn = model_3d == "painn"
    if getattr(batch, "_dataset", None) is not None:
        return (getattr(batch, "_mask", None) is None and not getattr(batch, "_triples", False)
                and (not painn or batch.n_edges is not None))
    if painn and not _rei_ok(getattr(batch, "radius_edge_index", None)):
        return False
    return not getattr(batch, "_triples", False) and sparse_tensors_ok(batch)


def option_of(batch):
    """What a bucket for this batch enumerates: the AtomTupleExtractor option of a canonical pair enumeration, "triples"
    for a collated AtomTripleExtractor batch (or a handle of a triple dataset) - its list is per-step DATA of the bucket,
    not a function of the sizes -, the sampled option ``(base, ratio)`` of a batch marked as AtomTupleExtractor(ratio < 1)
    output (``_sampled``: a DeviceLoader(tuple_ratio=) handle, a collated batch of the host extractor's molecules), or
    None."""
    if getattr(batch, "_triples", False):
        return TRIPLES
    canon = getattr(batch, "_canonical", None)
    return canon if canon is not None else getattr(batch, "_sampled", None)


def n_triples(batch):
    """Triples of a triple batch (a handle knows them on the host; a collated batch by its tensor's shape)."""
    if getattr(batch, "_dataset", None) is not None:
        return int(batch.n_triples)
    return int(batch.super_edge_index.size(1))


def batch_counts(sizes, option, views=2):
    """(atoms N, pair slots P, super-edges S, aggregation work items W of the `views`-view batch) of molecules `sizes`.
    option "triples": no pair tuples (S = 0); "sparse": atoms only (N, 0, 0, 0)."""
    n = sizes if isinstance(sizes, np.ndarray) else np.asarray(sizes, dtype=np.int64)
    if option == SPARSE:
        return int(n.sum()), 0, 0, 0
    from .layout import aggregate_by_targets, work_items_bound
    P = int((n * (n - 1) // 2).sum())
    if is_sampled(option):
        S = int(kept_tuples(n, *option).sum())
    else:
        S = P if option == "combination" else (0 if option == TRIPLES else 2 * P)
    W = work_items_bound(np.concatenate([n] * views), aggregate_by_targets(views * len(n)))   # (a bound: 8 padded queues)
    return int(n.sum()), P, S, W


def eligible(batch, model_3d, normalize=False):
    """Can this batch go through a bucket graph?  Molecule sizes known on the host (1 .. 255 atoms, at least one molecule
    with a pair), super_edge_index the extractor's full enumeration - every index tensor of the SchNet step is then a
    function of the sizes; PaiNN: also a collated radius_edge_index on the device (its structures are rebuilt on the
    device per step, geossl_painn_edge_layout)."""
    sizes, canon = getattr(batch, "_sizes", None), option_of(batch)
    if (model_3d not in ("schnet", "painn") or normalize or sizes is None
            or (canon not in ("combination", "permutation", TRIPLES) and not is_sampled(canon)) or not len(sizes)):
        return False
    # sampled tuples (GEOSSL_SAMPLED_BUCKETS): a loader's handles by default - no other replayed route exists for them
    if is_sampled(canon) and not sampled_buckets(getattr(batch, "_dataset", None) is not None):
        return False
    lo, hi = size_range(batch)
    if lo < 1 or hi > MAX_N or hi < 2:
        return False
    if getattr(batch, "_dataset", None) is not None:   # a handle on a device-resident dataset: gathered by the fill itself
        if model_3d != "painn":
            return True
        if getattr(batch, "_mask", None) is None:
            return batch.n_edges is not None
        # a masked PaiNN handle: its edge count is drawn - the fill counts the survivors on the device and the bucket is
        # sized by the handle's host-side bound (GEOSSL_MASKED_PAINN_BUCKETS=0: it runs on its collated tensors)
        return masked_painn_buckets() and getattr(batch, "n_edges_bound", None) is not None
    if model_3d == "painn" and not _rei_ok(getattr(batch, "radius_edge_index", None)):
        return False
    return tensors_ok(batch)


def _rei_ok(rei):
    """A collated int64 radius_edge_index [2, E] on the device, contiguous along the edges."""
    return (rei is not None and rei.is_cuda and rei.dtype == torch.long and rei.dim() == 2 and rei.size(0) == 2
            and rei.stride(1) == 1)


def route(batch, model_3d, views, pair_tuples, normalize):
    """The option of the bucket this batch goes through in a step of `views` views of a `model_3d` backbone, or None.
    A sparse layout (a structure above 255 atoms, or GEOSSL_SPARSE_PAIRS=1) in a one-view SchNet step that reads no pair
    tuples: the sparse bucket - no other bucket takes such a layout, and every other step keeps its routing.  Everything
    else: `eligible`, except equal-sized SchNet molecules (their per-structure graph serves every batch of the kind;
    PaiNN's edge list differs batch by batch anyway)."""
    if (not pair_tuples and views == 1 and model_3d == "schnet"
            and sparse_buckets(getattr(batch, "_dataset", None) is not None) and sparse_eligible(batch)):
        return SPARSE
    # PaiNN in such a step: the sparse bucket with an edges part, on the atom-tile kernels (a switch of its own:
    # GEOSSL_PAINN_SPARSE_BUCKETS; GEOSSL_PAINN_TILE=0 / GEOSSL_PAINN_VECTOR leave no kernel that takes its layout)
    if (not pair_tuples and views == 1 and model_3d == "painn" and not normalize
            and painn_sparse_buckets(getattr(batch, "_dataset", None) is not None)
            and _env("GEOSSL_PAINN_TILE") != "0" and not _env("GEOSSL_PAINN_VECTOR")
            and sparse_eligible(batch, "painn")):
        return SPARSE
    option = option_of(batch)
    # (equal-sized molecules share their tuples only when those are the full enumeration)
    if not eligible(batch, model_3d, normalize) or (model_3d != "painn" and is_uniform(batch) and not is_sampled(option)):
        return None
    return option


def handle_edges(batch):
    """Edges of a dataset handle as far as the host knows them: the count, or - a masked handle - an upper bound."""
    return batch.n_edges_bound if getattr(batch, "_mask", None) is not None else batch.n_edges


def batch_edges(batch, model_3d="painn"):
    """Edges of a PaiNN batch's radius_edge_index (a tensor shape or a handle's host-side count / bound: no read-back),
    else None."""
    if model_3d != "painn":
        return None
    if getattr(batch, "_dataset", None) is not None:
        return handle_edges(batch)
    return int(batch.radius_edge_index.size(1))


def triple_tensors_ok(batch):
    """`tensors_ok` for a collated triple batch: int64 super_edge_index [3, T] and float32 super_edge_angle [T] without
    a gradient, contiguous along what `Bucket.fill` copies; x / positions / batch as the molecule sizes give them."""
    sei, ang = batch.super_edge_index, getattr(batch, "super_edge_angle", None)
    if ang is None or not torch.is_tensor(sei):
        return False
    return (_atom_tensors_ok(batch, int(sizes_array(batch).sum()))
            and sei.is_cuda and sei.dtype == torch.long and sei.dim() == 2 and sei.size(0) == 3
            and (sei.size(1) == 0 or sei.stride(1) == 1)
            and ang.is_cuda and ang.dtype == torch.float32 and ang.dim() == 1 and ang.numel() == sei.size(1)
            and ang.is_contiguous() and not ang.requires_grad)


def tensors_ok(batch):
    """The batch's tensors are what `Bucket.fill` copies by byte count: int64 x [N, c] / batch [N] / super_edge_index
    [2, S], float32 positions [N, 3], all contiguous along what is copied, with N and S the counts the molecule sizes
    give (an int32 x, or a super_edge_index altered after the extractor marked it canonical, would make the copy read past
    the source).  Checked once per (batch object, tensor versions)."""
    if option_of(batch) == TRIPLES:
        return triple_tensors_ok(batch)
    sei = batch.super_edge_index
    # (lifetime-unique stamps: id() of a freed tensor is handed out again)
    tag = tuple((_tensor_uid(t_), t_._version) for t_ in (batch.x, batch.positions, batch.batch, sei))
    got = batch.__dict__.get("_geossl_tensors_ok")
    if got is not None and got[0] == tag:
        return got[1]
    n = sizes_array(batch)
    option = option_of(batch)
    if is_sampled(option):
        S = int(kept_tuples(n, *option).sum())
    else:
        P = int((n * (n - 1) // 2).sum())
        S = P if option == "combination" else 2 * P
    ok = (_atom_tensors_ok(batch, int(n.sum()))
          and sei.is_cuda and sei.dtype == torch.long and sei.dim() == 2 and sei.size(0) == 2 and sei.size(1) == S
          and sei.stride(1) == 1)
    batch.__dict__["_geossl_tensors_ok"] = (tag, ok)
    return ok


MODULE_SWITCHES = ("GEOSSL_NO_CHAIN", "GEOSSL_NCSN_SPLIT_BWD", "GEOSSL_NCSN_SEPARATE_HEADS", "GEOSSL_ARITH_24BIT")  # read by modules_ok
PAINN_SWITCHES = ("GEOSSL_PAINN_NO_CHAIN", "GEOSSL_PAINN_SILU_KERNELS")   # ... for a PaiNN backbone as well


def modules_ok(model, n1=None, n2=None):
    """The step of these modules can run on a bucket: the F = 128 chain path of SchNet / PaiNN (the chained row kernel is
    the one that takes a device-side row count) and the paired NCSN heads (two different modules of width 128).  No heads
    (n1 = n2 = None): the contrastive steps, whose loss reads the readout of the 2B molecules - exact counts, no capacity.
    One DistancePredictor of width 2 * 128 / ChargePredictor of width 128 / Discriminator of width 128 / property head of
    width 128 (n2 = None): the Distance / Charge Prediction, 3D InfoGraph and Supervised steps on a one-view bucket
    (InfoGraph's and the property head's readouts read view 0's B real molecule offsets: exact counts); one
    TorsionAnglePredictor of width 3 * 128: the angle-prediction step on a one-view "triples" bucket; Linear(2 * 128, 1):
    LEP's pair head, whose 2B structures [active | inactive] are the B_bucket molecules of a sparse bucket."""
    from .Geom3D.models.painn import PaiNN
    from .Geom3D.models.schnet import SchNet
    from .NCSN import NCSN_version_03, _head_params
    if any(_env(k) for k in MODULE_SWITCHES):
        return False
    if isinstance(model, SchNet):
        if (model.hidden_channels != 128 or model.num_filters != 128 or model.num_interactions < 1 or model.dipole
                or model.atomref is not None or model.mean is not None):
            return False
    elif isinstance(model, PaiNN):
        import torch.nn.functional as F_
        if (model.n_atom_basis != 128 or model.radial_basis.n_rbf not in (8, 16, 20) or model.share_filters
                or model.n_interactions < 1 or model.activation is not F_.silu
                or (model.n_interactions > 1 and model.interactions[0] is model.interactions[1])
                or any(_env(k) for k in PAINN_SWITCHES)):
            return False
    else:
        return False
    if n1 is None and n2 is None:
        return True
    from .pretrain_DistancePrediction import DistancePredictor, fused_head_ok
    if isinstance(n1, DistancePredictor) and n2 is None:
        return fused_head_ok(n1) and n1.predictor.in_features == 2 * 128
    from .pretrain_TorsionAnglePrediction import TorsionAnglePredictor, fused_head_ok as torsion_head_ok
    if isinstance(n1, TorsionAnglePredictor) and n2 is None:
        return torsion_head_ok(n1) and n1.predictor.in_features == 3 * 128
    from .pretrain_ChargePrediction import ChargePredictor, fused_head_ok as charge_head_ok
    if isinstance(n1, ChargePredictor) and n2 is None:
        return charge_head_ok(n1) and n1.predictor.in_features == 128
    from .pretrain_3DInfoGraph import Discriminator, fused_head_ok as infograph_head_ok, readout_of
    if isinstance(n1, Discriminator) and n2 is None:
        return infograph_head_ok(n1) and n1.weight.size(0) == 128 and readout_of(model) is not None
    from .pretrain_Supervised import head_width, readout_of as property_readout_of
    if isinstance(n1, (torch.nn.Linear, torch.nn.Sequential)) and n2 is None:
        if type(n1) is torch.nn.Linear and n1.in_features == 2 * 128:   # LEP's pair head on a width-128 backbone
            from .finetune_lep import head_params as pair_head_params
            return pair_head_params(n1) is not None and property_readout_of(model) is not None
        return head_width(n1) == 128 and property_readout_of(model) is not None
    from .Geom3D.models.autoencoder import AutoEncoder
    if isinstance(n1, AutoEncoder) or isinstance(n2, AutoEncoder):
        # the RR step: two distinct AutoEncoders of width 128 the fused heads serve (their rows are the 2B readouts: exact)
        from .pretrain_GeoSSL import fused_heads_ok as rr_heads_ok
        return rr_heads_ok(n1, n2) and n1.emb_dim == 128
    if not (isinstance(n1, NCSN_version_03) and isinstance(n2, NCSN_version_03)) or n1 is n2 \
            or n1.emb_dim != 128 or n2.emb_dim != 128:
        return False
    return not ({id(p) for p in _head_params(n1)} & {id(p) for p in _head_params(n2)})


def size_range(batch):
    r = batch.__dict__.get("_geossl_size_range")
    if r is None:
        n = sizes_array(batch)
        r = batch.__dict__["_geossl_size_range"] = (int(n.min()), int(n.max()))
    return r


def is_uniform(batch):
    sizes = getattr(batch, "_sizes", None)
    if sizes is None or not len(sizes):
        return False
    lo, hi = size_range(batch)
    return lo == hi


def _round_up(v, g):
    return int(-(-int(v) // g) * g)


def _slacks(B, sizes=None):
    """Relative head room of a capacity over the first batch's count, for (atoms, pair-slot-like counts): it has to cover
    the spread of a shuffled loader's batch sums, ~ cv / sqrt(B) with cv the relative spread of the per-molecule count -
    three of those standard deviations, from the sizes of the batch at hand when they are given (molecules with hydrogens
    spread twice as much in their pair-slot counts as the 18 +- 4 atoms of set B), never below 1.5 / sqrt(B)."""
    base = min(0.25, max(0.03, 1.5 / np.sqrt(max(B, 1))))
    if sizes is None or len(sizes) < 2:
        return base, base
    n = np.asarray(sizes, dtype=np.float64)
    p = n * (n - 1) / 2
    cv = lambda v: float(v.std() / max(v.mean(), 1e-9))
    f = 3.0 / np.sqrt(max(B, 1))
    return max(base, min(0.4, f * cv(n))), max(base, min(0.4, f * cv(p)))


def capacities(N, P, S, W, B, prev=None, sizes=None):
    """Capacities for a batch with these counts: a slack that covers the spread of a shuffled loader's batch sums
    (`_slacks`), rounded to the kernels' tile sizes; never below a previous bucket's."""
    sn, sp = _slacks(B, sizes)
    if prev is not None:   # a bucket that was outgrown once: the first batch underestimated the spread
        sn, sp = 1.5 * sn, 1.5 * sp
    cap = lambda v, g, sl: _round_up(v * (1.0 + sl) + g, g)
    out = [cap(N, 32, sn), cap(P, 64, sp), cap(S, 64, sp), cap(W, 64, sp)]
    if prev is not None:
        out = [max(a, b) for a, b in zip(out, prev)]
    return tuple(out)


def triple_capacity(T, B, prev=None):
    """Capacity for the sampled triples of a batch with T of them: the per-molecule count goes with n^3, so its batch sums
    spread far more than the atoms' - half as much again (twice after a bucket was outgrown), never below a block's 1024."""
    cap = _round_up(max(T, 1) * (2.0 if prev is not None else 1.5) + 1024, 1024)
    return cap if prev is None else max(cap, int(prev))


def edge_capacity(E, B, prev=None, sizes=None):
    """Capacity for the edges of a PaiNN batch (one view) with E edges, with the slack of `capacities` for pair-slot-like
    counts (the edges of a molecule lie between its atoms and its pair slots)."""
    slack = _slacks(B, sizes)[1] * (1.5 if prev is not None else 1.0)
    cap = _round_up(E * (1.0 + slack) + 64, 64)
    return cap if prev is None else max(cap, int(prev))


def host_plan(sizes, option, views=2):
    """Everything of a batch's index structures that is a function of the molecule sizes alone, as numpy arrays - the part
    of a bucket fill that runs on the host (and is tested without a GPU): counts (N, P, S, W); mol_ptr / pair_ptr of the
    TWO-VIEW batch ([2B + 1], view 1 behind view 0); se_ptr [B + 1]; the aggregation's work list over the 2B molecules
    (largest first, stable; 27 .. 33-atom molecules as 2 or 4 items, larger ones one item per atom: molecule | part << 24;
    over the B molecules of view 0 only when views = 1); the divisor of NCSN.py:210-212
    (last molecule with a super-edge, + 1); inc_ptr [N + 1] (an atom of an n-atom molecule lies on n - 1 tuples of the
    "combination" enumeration, 2 (n - 1) of "permutation").  A sampled option ``(base, ratio)``: S = sum k_m, se_ptr from
    the k_m = int(M_m * ratio), the divisor "last molecule with k_m > 0, + 1", ``kept`` = the k_m and NO inc_ptr (it depends
    on the draw: geossl_sampled_tuples writes it).  option "sparse": counts (N, 0, 0, 0) and ``mol_ptr``
    [B + 1] of the one view - no pair, tuple or work entry exists."""
    n = sizes if isinstance(sizes, np.ndarray) else np.asarray(sizes, dtype=np.int64)
    B = n.shape[0]
    if option == SPARSE:
        mp = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(n, out=mp[1:])
        return dict(counts=(int(mp[-1]), 0, 0, 0), mol_ptr=mp)
    N, P, S, W = batch_counts(n, option, views)
    mult = 1 if option == "combination" else (0 if option == TRIPLES or is_sampled(option) else 2)
    mp = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(n, out=mp[1:])
    npair = n * (n - 1) // 2
    pp = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(npair, out=pp[1:])
    from .layout import aggregate_by_targets, aggregate_work_list
    work = aggregate_work_list(np.concatenate([n] * views), aggregate_by_targets(views * B))
    if work.size > W:
        raise ValueError("aggregation work list longer than its bound")   # (work_items_bound: cannot happen)
    out = dict(counts=(N, P, S, W), mol_ptr2=np.concatenate([mp, mp[1:] + N]), pair_ptr2=np.concatenate([pp, pp[1:] + P]),
               work=work)
    if is_sampled(option):
        # a sampled option: k_m = int(M_m * ratio) tuples per molecule (batch.kept_tuples); the divisor is the last
        # molecule that KEEPS a tuple, + 1; the incidence pointers depend on the draw and are the device's to write
        k = kept_tuples(n, *option)
        sp = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(k, out=sp[1:])
        has = np.nonzero(k > 0)[0]
        out.update(se_ptr=sp, divisor=int(has[-1]) + 1 if has.size else 0, kept=k)
        return out
    has = np.nonzero(npair > 0)[0]
    ip = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.repeat((n - 1) * mult, n), out=ip[1:])
    out.update(se_ptr=pp * mult, divisor=int(has[-1]) + 1 if has.size else 0, inc_ptr=ip)
    return out


# ------------------------------------------------------------------------------------------------ the parts of a bucket
class _Part:
    """One part of a bucket.  Made by `BlobLayout` from integers alone, it holds the slices of the blob sections it owns
    and `write_host` writes them (numpy only: `host_image` runs without a device).  `attach`, called once by the
    bucket's constructor, allocates the part's static buffers and writes every pointer that never changes into the
    bucket's one `Gather` struct.  A part that has something to set per fill has `bind`; one that launches behind the
    gather has `after`; `fill` calls only the hooks that exist."""

    bind = after = None


class _Atoms(_Part):
    """Every bucket: the counts, mol_ptr and the molecules' offsets in a dataset; x / positions / batch vector."""

    def __init__(self, lay):
        o, B, sparse = lay.off, lay.B, lay.option == SPARSE
        self.V, self.B, self.option = lay.views, B, lay.option
        self.plan_key = "mol_ptr" if sparse else "mol_ptr2"   # (a sparse bucket: the B real offsets of its one view)
        self.mol = slice(o["mol_ptr"], o["mol_ptr"] + (B + 1 if sparse else 2 * B + 1))
        self.src = slice(o["src_off"], o["src_off"] + B)

    def write_host(self, h, hp, n, N, P, S, E, T, masked_edges, src):
        V, work = self.V, hp.get("work")
        # (masked PaiNN: dims[D_E2] and e_ptr are written by geossl_masked_edge_offsets, behind the upload on the stream;
        # D_W: the work list's real length - 8 queues - which is <= the bound W the capacity was checked with)
        h[0:8] = (N, V * N, V * P, S, 0 if work is None else work.size, self.B, 3 * V * N, 0 if masked_edges else V * E)
        h[self.mol] = hp[self.plan_key]
        if src is not None:
            h[self.src] = src[0]

    def attach(self, b):
        i64, g, x_cols = dict(dtype=torch.int64, device=b.device), b._g, b.x_cols
        b.x, b.batch_vec = torch.zeros(b.N_cap, x_cols, **i64), torch.zeros(b.N_cap, **i64)
        b.positions = torch.zeros(b.N_cap, 3, dtype=torch.float32, device=b.device)
        b.b2 = torch.zeros(b.views * b.N_cap, **i64)   # placeholder for the backbone's `batch` argument
        g.option, g.x_cols = (0 if base_option(self.option) in ("combination", SPARSE) else 1), x_cols
        g.mol_ptr, self.src_ptr = b._base + 4 * self.mol.start, b._base + 4 * self.src.start
        g.x_dst, g.pos_dst, g.batch_dst = ptr(b.x), ptr(b.positions), ptr(b.batch_vec)

    def bind(self, g, batch, ds, E, masked_edges):
        src = ds if ds is not None else batch
        # (a collated batch: its molecules start where the bucket's do; the extractor's enumeration is generated)
        g.x_src, g.pos_src, g.src_off = ptr(src.x), ptr(src.positions), (self.src_ptr if ds is not None else g.mol_ptr)


class _Pairs(_Part):
    """Every bucket but a sparse one: pair_ptr of the two-view batch and the divisor of NCSN.py:210-212 (the last
    molecule with a pair, + 1), which are functions of the sizes that every dense step carries; SchNet: the pair slots
    themselves (pair_i / pair_j, written by the gather) and the aggregation's work list."""

    def __init__(self, lay):
        o = lay.off
        self.slots = lay.kind == "schnet"
        self.pair = slice(o["pair_ptr"], o["pair_ptr"] + 2 * lay.B + 1)
        self.work, self.stats, self.se = o["work"], slice(o["stats"], o["stats"] + 4), o["se_ptr"]

    def write_host(self, h, hp, n, N, P, S, E, T, masked_edges, src):
        h[self.pair] = hp["pair_ptr2"]
        if self.slots:
            work = hp["work"]
            h[self.work:self.work + work.size] = work
        st = h[self.stats].view(np.int64)
        st[0], st[1] = hp["divisor"], 0

    def attach(self, b):
        lay, g = b.lay2, b._g
        g.se_ptr = b._base + 4 * self.se
        if self.slots:
            from .layout import aggregate_by_targets
            lay.pair_i, lay.pair_j = (torch.zeros(2 * b.P_cap, dtype=torch.int32, device=b.device) for _ in "ij")
            lay.agg_work = b.blob[self.work:self.work + b.W_cap]
            lay.agg_targets = aggregate_by_targets(b.views * b.B)
            g.pair_ptr2, g.pair_i, g.pair_j = b._base + 4 * self.pair.start, ptr(lay.pair_i), ptr(lay.pair_j)


class _Tuples(_Part):
    """"combination" / "permutation": se_ptr and inc_ptr from the host; the enumerated tuples `sei` and their incidence
    lists by the gather.  (The buffers and the `sel` object exist in every bucket - the heads' duck type - at S_cap.)"""

    def __init__(self, lay):
        o = lay.off
        self.se, self.inc = slice(o["se_ptr"], o["se_ptr"] + lay.B + 1), o["inc_ptr"]

    def write_host(self, h, hp, n, N, P, S, E, T, masked_edges, src):
        h[self.se] = hp["se_ptr"]
        h[self.inc:self.inc + 2 * (N + 1)].view(np.int64)[:] = hp["inc_ptr"]

    def attach(self, b):
        g = b._g
        g.sei0, g.sei1 = ptr(b.sei[0]), ptr(b.sei[1])
        g.inc_ptr, g.inc_idx = ptr(b.sel.inc_ptr), ptr(b.sel.inc_idx)


class _SampledTuples(_Part):
    """A sampled option ``(base, ratio)``: se_ptr from the host (the kept counts are a function of the sizes), the tuples
    and both incidence arrays by ONE launch behind the gather (geossl_sampled_tuples; the gather's sei / inc pointers
    stay NULL) - drawn there from the handle's seed, or checked there after a collated batch's tensor / a handle's
    host-drawn list was copied in.  A tuple that leaves its molecule sets the status word, polled a few fills late."""

    def __init__(self, lay):
        o, B = lay.off, lay.B
        self.B, self.base = B, _TUPLE_OPTIONS[lay.option[0]]
        self.se, self.ids = slice(o["se_ptr"], o["se_ptr"] + B + 1), slice(o["mol_id"], o["mol_id"] + B)

    def write_host(self, h, hp, n, N, P, S, E, T, masked_edges, src):
        h[self.se] = hp["se_ptr"]
        if src is not None:   # (the low word of the molecules' dataset ids: the draw's counter)
            h[self.ids] = (np.asarray(src[5], dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)

    def attach(self, b):
        self.b = b
        b.tuple_status = _lib.StatusWord(b.device, "super_edge_index must be grouped by molecule in batch order with both "
                                         "ends of a tuple in the same molecule and different (collated "
                                         "AtomTupleExtractor output is)")
        # (geossl_sampled_tuples: mol_ptr, se_ptr, B, option, mol_id | capacities, outputs, status)
        self.head = (b._g.mol_ptr, b._base + 4 * self.se.start, self.B, self.base, b._base + 4 * self.ids.start)
        self.tail = (b.N_cap, b.S_cap, ptr(b.sei[0]), ptr(b.sei[1]), ptr(b.sel.inc_ptr), ptr(b.sel.inc_idx),
                     ptr(b.tuple_status.word))

    def after(self, batch, ds, N, E, T, masked_edges):
        b = self.b
        draw = getattr(batch, "_tuple_draw", None) if ds is not None else None
        seed = None if draw is None else draw.seed
        if seed is None:   # the batch's own tuples: a collated tensor, or a handle's host-drawn list (batch atom ids)
            sei = batch.super_edge_index if ds is None else torch.from_numpy(draw.tuples)
            if sei.size(1):
                b.sei[:, :sei.size(1)].copy_(sei)
        _poll(b.tuple_status)
        call("geossl_sampled_tuples", *self.head, 0 if seed is None else 1, 0 if seed is None else int(seed), *self.tail,
             stream())
        b.tuple_status.arm(every=8)


_TUPLE_OPTIONS = {"combination": 0, "permutation": 1}


class _Triples(_Part):
    """"triples" (one view; angle prediction): a sampled list of atom triples with a float payload, static inputs at
    T_cap - a handle's by geossl_gather_triples from the offsets uploaded here, a collated batch's by one copy each."""

    def __init__(self, lay):
        o, B = lay.off, lay.B
        self.src, self.ptr = slice(o["t_src_off"], o["t_src_off"] + B), slice(o["t_ptr"], o["t_ptr"] + B + 1)

    def write_host(self, h, hp, n, N, P, S, E, T, masked_edges, src):
        h[D_T] = T
        if src is not None:
            h[self.src] = src[3]
            tp = h[self.ptr]
            tp[0] = 0
            np.cumsum(src[4], out=tp[1:])

    def attach(self, b):
        self.b = b
        b.triples = torch.zeros(3, max(b.T_cap, 1), dtype=torch.int64, device=b.device)
        b.triple_angle = torch.zeros(max(b.T_cap, 1), dtype=torch.float32, device=b.device)
        # (geossl_gather_triples: where the molecules' triples start in the dataset and in the batch, mol_ptr, B, outputs)
        self.args = (b._base + 4 * self.src.start, b._base + 4 * self.ptr.start, b._g.mol_ptr, b.B, ptr(b.triples[0]),
                     ptr(b.triples[1]), ptr(b.triples[2]), ptr(b.triple_angle))

    def after(self, batch, ds, N, E, T, masked_edges):
        if T and ds is None:
            self.b.triples[:, :T].copy_(batch.super_edge_index)
            self.b.triple_angle[:T].copy_(batch.super_edge_angle)
        elif T:   # the molecules' sampled triples (node offset added) and their angles: one launch
            call("geossl_gather_triples", ptr(ds.triples), ds.triples.size(1), ptr(ds.triple_angle), *self.args, stream())


class _EdgesPart(_Part):
    """PaiNN: the structures of the batch's radius_edge_index for the two-view batch (geossl_painn_edge_layout: one
    launch on the batch's own edge tensor or on a handle's gathered edges, outputs at E_cap; a masked handle's edge
    count stays on the device: geossl_painn_edge_layout_dyn), and the atoms of the molecules above the stage caps of
    the molecule-staged interaction kernels (`big_caps`: up to two lists, from the host)."""

    def __init__(self, lay):
        o, B = lay.off, lay.B
        self.B, self.V = B, lay.views
        self.big = tuple((c, D_BIG0 + k, o["big%d" % k]) for k, c in enumerate(lay.big_caps))
        self.src, self.ptr = slice(o["e_src_off"], o["e_src_off"] + B), slice(o["e_ptr"], o["e_ptr"] + B + 1)

    def write_host(self, h, hp, n, N, P, S, E, T, masked_edges, src):
        if self.big:
            from .layout import big_atom_list
            n2 = np.concatenate([n] * self.V)
            for cap, word, start in self.big:
                idx = big_atom_list(n2, cap)
                h[word] = idx.size
                h[start:start + idx.size] = idx
        if src is not None:
            h[self.src] = src[1]
            ep = h[self.ptr]
            ep[:] = 0
            if not masked_edges:
                np.cumsum(src[2], out=ep[1:])

    def attach(self, b):
        self.b, dev, lay = b, b.device, b.lay2
        B, Nc, Ec, V = b.B, b.N_cap, b.E_cap, b.views
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        if self.big:
            lay.big = {c: (b.blob[start:start + 2 * Nc], 2 * Nc, b.dyn.n_big[k]) for k, (c, _, start) in enumerate(self.big)}
        el = _Edges()
        el.E, el.N, el.B = V * Ec, V * Nc, V * B
        el.idx_i, el.idx_j = torch.zeros(2 * Ec, **i64), torch.zeros(2 * Ec, **i64)
        el.inc = {"i": (torch.zeros(2 * Nc + 1, **i64), torch.zeros(max(2 * Ec, 1), **i32)),
                  "j": (torch.zeros(2 * Nc + 1, **i64), torch.zeros(max(2 * Ec, 1), **i32))}
        G = int(_lib.load().geossl_painn_group_capacity(2 * Ec, 2 * Nc))
        el.row_edge = torch.full((4 * G,), -1, **i32)
        el.grp_atom = torch.full((G,), -1, **i32)
        el.mol_grp = torch.zeros(2 * B + 1, **i32)
        el.mol_grp_end = torch.zeros(2 * B, **i32)
        # set by geossl_painn_edge_layout on an edge that leaves its molecule (the reference's collated
        # radius_edge_index never has one); read without draining the stream, a few steps late (_lib.StatusWord)
        b.el_status = _lib.StatusWord(dev, "radius_edge_index must be grouped by molecule in batch order with both "
                                      "ends in the same molecule (collated MoleculeDataset3DRadius output is)")
        el.status = b.el_status.word
        # set by geossl_masked_edge_offsets when a masked batch's surviving edges exceed E_cap (the capacity comes
        # from a host-side upper bound: it cannot happen)
        b.ecap_status = _lib.StatusWord(dev, "a masked batch kept more radius edges than its bucket's edge "
                                        "capacity (the handle's n_edges_bound is not an upper bound)")
        b._keep, b._e_cnt = None, None   # the count launch's kept lists / survivor counts (first masked fill)
        el.dyn = b.dyn
        b.el = el
        b.e2 = torch.zeros(2, 1, **i64)   # placeholder for PaiNN.forward's radius_edge_index argument
        b.rei = None                      # the collated edges of a batch drawn from a dataset (made on first use)
        self.src_ptr, self.e_ptr = b._base + 4 * self.src.start, b._base + 4 * self.ptr.start
        # (the layout launch: ... mol_ptr, N, B, rows of the incidence pointers | its outputs)
        self.mol_ptr, self.outs = ptr(lay.mol_ptr), (
            ptr(el.idx_i), ptr(el.idx_j), ptr(el.inc["i"][0]), ptr(el.inc["i"][1]), ptr(el.inc["j"][0]),
            ptr(el.inc["j"][1]), ptr(el.row_edge), ptr(el.grp_atom), ptr(el.mol_grp), ptr(el.mol_grp_end), ptr(el.status))

    def bind(self, g, batch, ds, E, masked_edges):
        b = self.b
        if ds is not None and b.rei is None:
            b.rei = torch.zeros(2, max(b.E_cap, 1), dtype=torch.int64, device=b.device)
            self.rei = (ptr(b.rei[0]), ptr(b.rei[1]))
        # (a handle's edges are gathered; masked: whether any edge survives is the device's to know)
        if ds is not None and (ds.edges.size(1) if masked_edges else E):
            g.e0_src, g.e1_src, g.e_src_off, g.e_ptr = ptr(ds.edges[0]), ptr(ds.edges[1]), self.src_ptr, self.e_ptr
            g.e0_dst, g.e1_dst = self.rei
        else:
            g.e0_src = g.e1_src = g.e_src_off = g.e_ptr = g.e0_dst = g.e1_dst = None

    def after(self, batch, ds, N, E, T, masked_edges):
        b = self.b
        rei = batch.radius_edge_index if ds is None else None   # (a handle's were gathered into b.rei)
        r0, r1 = self.rei if ds is not None else (ptr(rei[0]), ptr(rei[1]))
        _poll(b.el_status)
        if masked_edges:   # (E = e_ptr[B], in device memory)
            call("geossl_painn_edge_layout_dyn", r0, r1, b.E_cap, self.e_ptr + 4 * self.B, self.mol_ptr, N, self.B,
                 2 * b.N_cap, *self.outs, stream())
        else:
            call("geossl_painn_edge_layout", r0, r1, E, self.mol_ptr, N, self.B, 2 * b.N_cap, *self.outs, stream())
        b.el_status.arm(every=8)


class _SparseEdgesPart(_Part):
    """PaiNN on a sparse bucket (one view, structures of up to 1024 atoms): the batch's radius_edge_index in a static
    [2, E_cap] buffer - a handle's edges gathered with their atom offsets by the gather launch, a collated batch's by
    one copy - and both incidence lists at capacity, rewritten by ONE launch behind it
    (geossl_painn_incidence_layout_dyn: the counts come from `dims`).  What the atom-tile interaction kernels read; no
    group layout, no stage-cap lists."""

    def __init__(self, lay):
        o, B = lay.off, lay.B
        self.B = B
        self.src, self.ptr = slice(o["e_src_off"], o["e_src_off"] + B), slice(o["e_ptr"], o["e_ptr"] + B + 1)

    def write_host(self, h, hp, n, N, P, S, E, T, masked_edges, src):
        if src is not None:
            h[self.src] = src[1]
            ep = h[self.ptr]
            ep[0] = 0
            np.cumsum(src[2], out=ep[1:])

    def attach(self, b):
        self.b, dev = b, b.device
        Nc, Ec = b.N_cap, max(b.E_cap, 1)
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        b.rei = torch.zeros(2, Ec, **i64)
        el = _Edges()
        el.E, el.N, el.B = b.E_cap, Nc, b.B
        el.idx_i, el.idx_j = b.rei[0], b.rei[1]   # (one view: the incidence lists index the edge list itself)
        el.inc = {"i": (torch.zeros(Nc + 1, **i64), torch.zeros(Ec, **i32)),
                  "j": (torch.zeros(Nc + 1, **i64), torch.zeros(Ec, **i32))}
        b.el_status = _lib.StatusWord(dev, "radius_edge_index must be grouped by molecule in batch order with both "
                                      "ends in the same molecule (collated MoleculeDataset3DRadius output is)")
        el.status, el.dyn = b.el_status.word, b.dyn
        b.el = el
        b.e2 = torch.zeros(2, 1, **i64)   # placeholder for PaiNN.forward's radius_edge_index argument
        self.src_ptr, self.e_ptr = b._base + 4 * self.src.start, b._base + 4 * self.ptr.start
        self.rei = (ptr(b.rei[0]), ptr(b.rei[1]))
        self.outs = (ptr(el.inc["i"][0]), ptr(el.inc["i"][1]), ptr(el.inc["j"][0]), ptr(el.inc["j"][1]), ptr(el.status))

    def bind(self, g, batch, ds, E, masked_edges):
        if ds is not None and E:
            g.e0_src, g.e1_src, g.e_src_off, g.e_ptr = ptr(ds.edges[0]), ptr(ds.edges[1]), self.src_ptr, self.e_ptr
            g.e0_dst, g.e1_dst = self.rei
        else:
            g.e0_src = g.e1_src = g.e_src_off = g.e_ptr = g.e0_dst = g.e1_dst = None

    def after(self, batch, ds, N, E, T, masked_edges):
        b = self.b
        if ds is None and E:
            b.rei[:, :E].copy_(batch.radius_edge_index)
        _poll(b.el_status)
        call("geossl_painn_incidence_layout_dyn", *self.rei, b.E_cap, b.dyn.n_edges2, b._g.mol_ptr, b.N_cap, self.B,
             b.max_n, *self.outs, b.dyn.n_atoms, None, stream())
        b.el_status.arm(every=8)


def _poll(status):
    """A status word's late error as the ValueError a refused fill raises."""
    try:
        status.poll()
    except IndexError as e:
        raise ValueError(str(e)) from None


class BlobLayout:
    """What a bucket holds, decided once from (kind, option, views, max_n, n_rbf) and the capacities: the blob's
    sections `off` (name -> first int32 word) with its length `words`, and the parts in order, each holding the slices
    of the sections it writes."""

    def __init__(self, B, caps, option, kind="schnet", views=2, max_n=SMALL_N, n_rbf=20):
        self.B, self.option, self.kind, self.views = int(B), option, kind, int(views)
        Nc, Wc = int(caps[0]), int(caps[3])
        sparse, painn, triples = option == SPARSE, kind == "painn", option == TRIPLES
        self.big_caps = ()
        if painn and max_n > 0 and not sparse:
            from .layout import painn_stage_caps
            # (the stage caps depend on the radial basis: 73 / 74 / 75 atoms for the backward at 20 / 16 / 8 functions -
            # lists made for another basis would never be found and the whole batch would fall back to the per-atom kernels)
            self.big_caps = tuple(c for c in painn_stage_caps(128, int(n_rbf)) if 0 < c < max_n)
        nb = len(self.big_caps)
        # the sections in blob order, (name, int32 words): one running sum.  dims .. stats exist in every bucket (a kind
        # without the part leaves them unwritten); the int64 sections `stats` and `inc_ptr` start on an even word
        sections = (("dims", DIMS_WORDS), ("mol_ptr", 2 * B + 1), ("pair_ptr", 2 * B + 1), ("se_ptr", B + 1),
                    ("work", Wc), ("stats", 4), ("inc_ptr", 0 if sparse else 2 * (Nc + 1)),
                    ("big0", 2 * Nc if nb > 0 else 0), ("big1", 2 * Nc if nb > 1 else 0), ("src_off", B),
                    ("e_src_off", B if painn else 0), ("e_ptr", B + 1 if painn else 0),
                    ("t_src_off", B if triples else 0), ("t_ptr", B + 1 if triples else 0))
        if is_sampled(option):   # (the molecules' dataset ids, the counter of a device draw: a sampled bucket's alone)
            sections += (("mol_id", B),)
        self.off, at = {}, 0
        for name, words in sections:
            at = _round_up(at, 2) if name == "stats" else at
            self.off[name] = at
            at += words
        self.words = at
        kinds = ((_Atoms,) + (() if sparse else (_Pairs,))
                 + ((_Tuples,) if option in ("combination", "permutation") else ())
                 + ((_SampledTuples,) if is_sampled(option) else ())
                 + ((_Triples,) if triples else ())
                 + (((_SparseEdgesPart if sparse else _EdgesPart),) if painn else ()))
        self.parts = tuple(kind_(self) for kind_ in kinds)
        self.writers = tuple(p.write_host for p in self.parts)


def host_image(h, lay, n, counts=None, src=None, E=0, T=None, masked_edges=False):
    """The host half of a fill: everything of the blob that is a function of the molecule sizes `n` - and, for a handle
    on a dataset, of where the chosen molecules (their edges, their triples) start there: src = (src_off, edge_off,
    edge_cnt, triple_off, triple_cnt[, ids - read by a sampled bucket]) of the chosen ids, None for a collated batch -
    into `h`, an int32 numpy view of `lay.words` words (the bucket's pinned staging slot; in a test a plain array).
    E: the batch's edges (PaiNN), T: its triples; masked_edges: the edge count and e_ptr are the device's to write.
    Words the batch does not define are left as they are (a reused slot keeps what an earlier fill wrote past this
    batch's counts)."""
    hp = host_plan(n, lay.option, lay.views)
    N, P, S, W = counts if counts is not None else hp["counts"]
    for write in lay.writers:
        write(h, hp, n, N, P, S, E, T, masked_edges, src)


# which static noise tensor of a step has how many rows - "N": atoms, "S": super-edges (both at capacity in a bucket, the
# real rows leading), "B": molecules (exact), or a number - with its trailing shape and dtype
NOISE_SHAPES = {"pos_noise": ("N", (3,), torch.float32), "dist_noise_1": ("S", (1,), torch.float32),
                "dist_noise_2": ("S", (1,), torch.float32), "noise_level_1": ("B", (), torch.long),
                "noise_level_2": ("B", (), torch.long),
                # Charge Prediction's mask input: the device draw's seed, or the host-drawn list (k <= N entries)
                "mask_seed": (1, (), torch.long), "mask_idx": ("N", (), torch.long),
                # the Supervised step's target column; LEP's labels - one per pair, the leading half of the 2B rows
                "target": ("B", (), torch.float32)}


class Bucket:
    """The static inputs and index structures of one step graph at a CAPACITY, as a list of parts decided once in the
    constructor (`BlobLayout.parts`; the table of the parts is in the module's docstring).

    `fill` is one path: check the batch, take a staging slot, `host_image` (every part's `write_host`), one upload, the
    parts' `bind` on the bucket's `Gather` struct, the gather launch, the parts' `after`.  A sparse bucket (views = 1;
    kind "painn" adds the sparse edges part) is, for SchNet, the bucket whose only part is atoms: `lay2` is a SPARSE layout at capacity - N = N_cap, P = P_cap (rows
    of the pair list the backbone builds per step), max_n a class of SPARSE_MAX_N_CLASSES, mol_ptr the B real offsets.

    views = 1 (a step with no second view: Distance Prediction): the backbone's layout `lay2` and the counts in `dims`
    describe view 0 alone - B molecules, its aggregation work list, its pair slots and edges.  The gather and the PaiNN
    edge layout still write the two-view structures (view 1 lands in buffer space this step never reads); view 0 comes
    first in every one of them, so its slices are the one-view structures."""

    def __init__(self, device, B, caps, option, x_cols=2, max_n=SMALL_N, kind="schnet", E_cap=0, n_rbf=20, views=2,
                 T_cap=0):
        if views not in (1, 2):
            raise ValueError("a bucket holds one or two views")
        if option == TRIPLES and views != 1:
            raise ValueError("a triples bucket holds one view")
        if option == SPARSE and (views != 1 or kind not in ("schnet", "painn")):
            raise ValueError("a sparse bucket holds one view of a SchNet or PaiNN batch")
        self.views = V = int(views)
        self.device, self.B, self.option, self.max_n = device, int(B), option, int(max_n)
        self.kind, self.E_cap, self.x_cols = kind, int(E_cap), int(x_cols)
        self.T_cap = int(T_cap) if option == TRIPLES else 0
        self.N_cap, self.P_cap, self.S_cap, self.W_cap = (int(c) for c in caps[:4])
        B, Nc, Sc = self.B, self.N_cap, self.S_cap
        self.layout = L = BlobLayout(B, self.caps(), option, kind, V, self.max_n, n_rbf)
        o = self.off = L.off
        self.words, self.big_caps = L.words, L.big_caps
        # ---- the blob: everything the host computes, uploaded in one copy (int32 words; int64 parts 8-byte aligned)
        self.blob = torch.zeros(self.words, dtype=torch.int32, device=device)
        self._base = self.blob.data_ptr()
        self.dims = self.blob[0:DIMS_WORDS]
        self.dyn = DynDims(self.dims)
        self._host = [[torch.zeros(self.words, dtype=torch.int32).pin_memory(), None] for _ in range(3)]
        self._slot = 0
        # ---- molecule layout of the views the backbone sees (the blob's pointer arrays always hold both views)
        lay = self.lay2 = _Layout()
        lay.N, lay.B, lay.P, lay.max_n = V * Nc, V * B, V * self.P_cap, self.max_n
        lay.mol_ptr = self.blob[o["mol_ptr"]:o["mol_ptr"] + V * B + 1]
        lay.pair_ptr = self.blob[o["pair_ptr"]:o["pair_ptr"] + V * B + 1]
        lay.device, lay.dyn, lay.agg_work = device, self.dyn, None
        lay.sparse = option == SPARSE
        if lay.sparse:
            lay.pair_i, lay.pair_j, lay.pair_capacity = None, None, self.P_cap
        self.el = None
        # ---- super-edge bookkeeping of the heads (every bucket: the heads' duck type; filled by the tuples part)
        self.sei = torch.zeros(2, Sc, dtype=torch.int64, device=device)
        self.sel = sel = _SuperEdges()
        sel.S, sel.N, sel.B = Sc, Nc, B
        sel.se_ptr = self.blob[o["se_ptr"]:o["se_ptr"] + B + 1]
        sel.stats = self.blob[o["stats"]:o["stats"] + 4].view(torch.int64)
        sel.inc_ptr = self.blob[o["inc_ptr"]:o["inc_ptr"] + (0 if lay.sparse else 2 * (Nc + 1))].view(torch.int64)
        sel.inc_idx = torch.zeros(2 * Sc, dtype=torch.int32, device=device)
        sel.dyn = self.dyn
        # ---- the parts' static buffers, and the gather's argument struct with every pointer that never changes
        self._g = _lib.Gather()
        for part in L.parts:
            part.attach(self)
        self._binds = tuple(p.bind for p in L.parts if p.bind is not None)
        self._afters = tuple(p.after for p in L.parts if p.after is not None)
        lay._batch_version = self.b2._version
        sel.sei0, sel.sei1, sel.batch = self.sei[0], self.sei[1], self.batch_vec
        sel._versions = (self.batch_vec._version, self.sei._version)
        # ---- the batch object the captured step sees
        if option == TRIPLES:
            self.batch = TripleBatch(self.x, self.positions, self.batch_vec, self.triples, self.triple_angle, None, B, None)
        else:
            self.batch = Batch(self.x, self.positions, self.batch_vec, self.sei, None, B, None,
                               None if is_sampled(option) else option)
        self.batch._bucket = self
        self.real = None  # (N, P, S, W) of the batch last filled in

    @staticmethod
    def sizing(batch, option, model_3d, views, n_rbf=20, prev=None):
        """The constructor's arguments of the bucket for this batch: capacities with the slack of `capacities` /
        `edge_capacity` / `triple_capacity` over its counts, the size class of its largest molecule; prev: `sizes()` of
        the bucket it outgrew (nothing shrinks)."""
        n, B, hi = sizes_array(batch), len(batch._sizes), size_range(batch)[1]
        caps0, n0, E0, T0 = prev if prev is not None else (None,) * 4
        counts = batch_counts(n, option, views)
        if option == SPARSE:
            caps, max_n = sparse_capacities(counts[0], B, caps0, sizes=n), sparse_max_n_class(hi, n0)
        else:
            caps, max_n = capacities(*counts, B=B, prev=caps0, sizes=n), max_n_class(hi, n0, model_3d)
        if getattr(batch, "_dataset", None) is not None:
            dev, x_cols = batch.device, batch.x_cols
        else:
            dev, x_cols = batch.positions.device, (batch.x.size(1) if batch.x.dim() == 2 else 1)
        return dict(device=dev, B=B, caps=caps, option=option, x_cols=x_cols, max_n=max_n, n_rbf=n_rbf, kind=model_3d,
                    views=views, E_cap=edge_capacity(batch_edges(batch), B, E0, sizes=n) if model_3d == "painn" else 0,
                    T_cap=triple_capacity(n_triples(batch), B, T0) if option == TRIPLES else 0)

    @classmethod
    def for_batch(cls, batch, option, model_3d, views, n_rbf=20, prev=None):
        """The bucket for this batch (`sizing`); prev: the bucket it outgrew.  (StepGraphs calls `sizing` and the
        constructor itself, so that the outgrown bucket is gone before the larger one is allocated.)"""
        return cls(**cls.sizing(batch, option, model_3d, views, n_rbf, None if prev is None else prev.sizes()))

    def sizes(self):
        """What a larger successor is sized from: (caps, max_n, E_cap, T_cap)."""
        return (self.caps(), self.max_n, self.E_cap, self.T_cap)

    def caps(self):
        return (self.N_cap, self.P_cap, self.S_cap, self.W_cap)

    def fits(self, counts, hi=None, E=None, T=None):
        """counts = (N, P, S, W) of a batch; hi: its largest molecule; E: its edges (PaiNN); T: its triples."""
        return (all(c <= cap for c, cap in zip(counts, self.caps())) and (hi is None or hi <= self.max_n)
                and (E is None or self.kind != "painn" or E <= self.E_cap)
                and (T is None or self.option != TRIPLES or T <= self.T_cap))

    def fits_batch(self, batch):
        """The batch's counts (N, P, S, W) if it fits - counts, largest molecule, edges (or a masked handle's bound on
        them) and triples, all from the host - else None."""
        counts = batch_counts(sizes_array(batch), self.option, self.views)
        return counts if self.fits(counts, size_range(batch)[1], batch_edges(batch, self.kind),
                                   n_triples(batch) if self.option == TRIPLES else None) else None

    def static_noise(self, keys):
        """Static noise tensors of a step on this bucket (NOISE_SHAPES): atom and super-edge rows at capacity."""
        rows = {"N": self.N_cap, "S": self.S_cap, "B": self.B}
        return {k: torch.zeros((rows.get(r, r),) + tail, dtype=dt, device=self.device)
                for k, (r, tail, dt) in ((k, NOISE_SHAPES[k]) for k in keys)}

    def _check(self, batch, ds, n, counts):
        """Step 1 of `fill`: the batch is one this bucket can take.  -> (E, T, masked_edges)"""
        opt, mask = self.option, getattr(batch, "_mask", None)
        painn, x_cols = self.kind == "painn", self.x.size(1)
        if opt == SPARSE:
            if mask is not None or getattr(batch, "_triples", False):
                raise ValueError("a sparse bucket takes unmasked batches of whole molecules (a masked PaiNN batch is "
                                 "served up to %d atoms per molecule, by the dense bucket)" % MAX_N if painn else
                                 "a sparse bucket takes unmasked batches of whole molecules")
        elif option_of(batch) != opt:
            raise ValueError("batch and bucket disagree on the tuple option")
        if ds is not None:   # (a triples or sparse bucket does not read the dataset's tuple option)
            if ((base_option(opt) in ("combination", "permutation") and ds.option != base_option(opt))
                    or ds.x_cols != x_cols
                    or ds.device != self.x.device):
                raise ValueError("dataset and bucket disagree (tuple option, x columns or device)")
            if painn and ds.edges is None:
                raise ValueError("PaiNN bucket fill expects a dataset built with radius=...")
        elif painn and not _rei_ok(batch.radius_edge_index):
            raise ValueError("PaiNN bucket fill expects a collated int64 radius_edge_index [2, E] on the device")
        E = batch_edges(batch) if painn else 0   # (a masked handle: an upper bound - the count is the device's)
        T = n_triples(batch) if opt == TRIPLES else None
        # (a dense bucket needs a pair somewhere - the divisor; a sparse one whole molecules)
        if not self.fits(counts, int(n.max()), E, T) or (int(n.min()) < 1 if opt == SPARSE else counts[1] < 1):
            raise ValueError("batch exceeds the bucket's capacity")
        if ds is None:
            if opt == SPARSE:   # (a 1-D x - DatasetLBA's atomic numbers - is its one column)
                ok = (sparse_tensors_ok(batch) and batch.x.numel() == counts[0] * x_cols
                      and batch.x.device == self.x.device)
            else:
                ok = tensors_ok(batch) and batch.x.size(1) == x_cols
            if not ok:
                raise ValueError("bucket fill expects contiguous collated int64 / float32 tensors of the sizes' shapes")
        return E, T, painn and ds is not None and mask is not None

    def fill(self, batch, counts=None, zero=None):
        """The batch's atom types, positions, index tensors and derived structures into the static buffers; `zero`: a
        float32 buffer cleared by the same launch (the owner's flat gradient buffer).  `batch`: a collated batch on the
        device, or a handle on a device-resident dataset (Geom3D.dataloaders.DatasetBatch) whose molecules are gathered
        from there.  One pinned upload (`host_image`: everything that is a function of the molecule sizes) + one launch
        (geossl_gather_molecules: atom rows, batch vector and the cleared buffer; per part super-edges and incidence
        lists, pair-slot atoms, radius edges) + what the parts launch behind it (triples of a handle:
        geossl_gather_triples, of a collated batch two copies; sampled tuples: geossl_sampled_tuples, behind one copy
        of the batch's own list where it has one; PaiNN: geossl_painn_edge_layout).  A masked handle adds
        the small upload of its mask and launches geossl_gather_masked_molecules instead: the BFS and the gather are that
        one launch.  A masked PaiNN handle is four launches - count (BFS + survivors per molecule),
        geossl_masked_edge_offsets (e_ptr and dims[D_E2] on the device), gather, geossl_painn_edge_layout_dyn - and
        nothing is read back: the host only checks the handle's upper bound on the edges against E_cap."""
        B, o = self.B, self.off
        n = sizes_array(batch)
        if n.shape[0] != B:
            raise ValueError("bucket of %d molecules got a batch of %d" % (B, n.shape[0]))
        if counts is None or self.option == SPARSE:
            counts = batch_counts(n, self.option, self.views)
        ds = getattr(batch, "_dataset", None)
        E, T, masked_edges = self._check(batch, ds, n, counts)
        slot = self._host[self._slot]
        self._slot = (self._slot + 1) % len(self._host)
        if slot[1] is not None:
            slot[1].synchronize()   # the upload that last read this staging buffer (three steps ago)
        src = None
        if ds is not None:   # a handle: where its molecules (their edges, their triples) start in the dataset
            ids, painn, triples = batch.ids, self.kind == "painn", self.option == TRIPLES
            src = (ds.off[ids], ds.edge_off[ids] if painn else None, ds.edge_cnt[ids] if painn else None,
                   ds.triple_off[ids] if triples else None, ds.triple_cnt[ids] if triples else None, ids)
        host_image(slot[0].numpy(), self.layout, n, counts, src, E, T, masked_edges)
        self.blob.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        # ---- device side: one launch
        g = self._g
        for bind in self._binds:
            bind(g, batch, ds, E, masked_edges)
        g.zero, g.zero_count = (ptr(zero), zero.numel()) if zero is not None else (None, 0)
        st_ = stream()
        if ds is not None and getattr(batch, "_mask", None) is not None:
            # a masked handle (DeviceLoader(mask_ratio=...)): the kept atoms are drawn (or read) by the same launch
            m, mblob = ds.mask_plan(batch, with_edges=masked_edges)
            if masked_edges:
                # count launch (kept lists + survivors per molecule), then their offsets and the batch's edge count made
                # on the device: the gather below reads e_ptr, the layout and the captured step the counts, from there
                if self._keep is None:
                    self._keep = torch.zeros(max(self.N_cap, 1), dtype=torch.int32, device=self.device)
                    self._e_cnt = torch.zeros(B, dtype=torch.int32, device=self.device)
                _poll(self.ecap_status)
                m.keep_out, m.e_count = ptr(self._keep), ptr(self._e_cnt)
                call("geossl_gather_masked_molecules", C.byref(g), C.byref(m), B, st_)
                call("geossl_masked_edge_offsets", ptr(self._e_cnt), B, self.E_cap, self.views,
                     self._base + 4 * o["e_ptr"], self.dyn.n_edges2, ptr(self.ecap_status.word), st_)
                self.ecap_status.arm(every=8)
                m.keep_out, m.e_count, m.keep_in = None, None, ptr(self._keep)
            call("geossl_gather_masked_molecules", C.byref(g), C.byref(m), B, st_)
            del mblob
        else:
            call("geossl_gather_molecules", C.byref(g), B, st_)
        for after in self._afters:
            after(batch, ds, counts[0], E, T, masked_edges)
        self.real = tuple(counts)
        # (a masked PaiNN fill: only the device knows the edges, blob[e_ptr + B]; a sparse bucket has none)
        self.real_E = None if masked_edges or self.option == SPARSE else E
        return self.real
