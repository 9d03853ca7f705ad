"""A dataset of molecules resident in HBM and the loader that draws shuffled batches from it without host collation.

The reference trains from ``DataLoaderAtomTuple(dataset, batch_size, shuffle=True)`` (examples/pretrain_GeoSSL.py:
295-301): every step the host fetches ``batch_size`` molecules (Geom3D/datasets/datasets_3D.py:69-80), concatenates them
(``BatchAtomTuple.from_data_list``, Geom3D/dataloaders/dataloaders_AtomTuple.py:46-73) and copies the result to the
device (:248).  At MI355X step rates that collation IS the step (0.5-0.7 ms of host work beside a 1.3-1.6 ms
step at the reference's batch size).  Here the molecules are uploaded once:

* ``DeviceDataset`` keeps the concatenated ``x [Ntot, C] int64`` / ``positions [Ntot, 3] float32`` of all molecules in
  device memory, the atom offsets and sizes on the HOST (a size table: every index structure of a batch is a function
  of the sizes), and - for PaiNN - the concatenated per-molecule ``radius_edge_index`` built once on the device by the
  radius-graph kernel on the unperturbed geometry (datasets_3D_Radius.py:105-131) with per-molecule
  edge offsets on the host (ONE read-back, at construction).
* ``DeviceLoader`` yields ``DatasetBatch`` handles in the order ``torch.utils.data.DataLoader(shuffle=True)`` would
  visit the molecules (the same ``torch.randperm`` under the same seed).  A handle carries molecule ids and host sizes
  only.  A step that replays a captured graph hands it to ``geossl_gather_molecules`` (csrc/gather.hip), which writes
  the chosen molecules - atom rows, batch vector, super-edges, pair slots, incidence lists, radius edges - straight into
  the graph's static inputs: one small pinned upload of offsets + one launch per step, no read-back, no host tensors.
  Anything else that touches ``handle.x`` / ``.positions`` / ``.batch`` / ``.super_edge_index`` /
  ``.radius_edge_index`` gets the collated tensors (built by the same kernel into fresh memory, then cached), so a
  handle is accepted wherever a collated batch is (``do_DDM``, the modules themselves, eager steps).
* ``DeviceDataset(..., triples=, triple_counts=[, triple_angle=])`` (or ``dataset.sample_triples(ratio)``): a dataset for
  angle prediction on atom triples (examples/pretrain_TorsionAnglePrediction.py).  The sampled triples of every molecule
  (local atom indices) and their angles live in device memory, the per-molecule offsets on the host; a handle of such a
  dataset shows ``super_edge_index [3, T]`` / ``super_edge_angle [T]`` - the triples, not the pair tuples - written by
  ``geossl_gather_triples`` (csrc/torsion_head.hip), bit for bit what ``BatchAtomTriple.from_data_list`` gives.
* ``DeviceLoader(mask_ratio=r)`` yields MASKED handles: the reference's BFS atom masking (datasets_3D.py:24-67; see
  ``masking``) over the dataset's bond graph, kept lists drawn on the device (``mask_rng="device"``) or by the
  reference's own np.random draws on the host (``"numpy"``).  A masked handle carries the kept sizes; its gather is
  ``geossl_gather_masked_molecules``.  With radius edges the survivor count depends on the draw: collating such a
  handle takes a count launch and a read-back of B counts before the gather; a PaiNN capacity bucket (``bucket.Bucket.
  fill``) keeps the counts on the device instead (``geossl_masked_edge_offsets``) and is sized by the handle's host-side
  bound ``n_edges_bound``.
* ``DeviceLoader(tuple_ratio=r)`` yields SAMPLED handles: the reference's ``AtomTupleExtractor(ratio < 1)``
  (``--distance_sample_ratio``) - every molecule keeps ``int(M * r)`` of its M tuples (``batch.sampled_count``: known on
  the host before the draw, like a masked batch's sizes), chosen on the device by ``geossl_sampled_tuples``
  (csrc/sampled_tuples.hip, ``tuple_rng="device"``) or by the reference's own ``np.random.choice`` calls on the host
  (``"numpy"``).  Such a handle carries the kept counts and the mark ``_sampled = (option, ratio)`` (``_canonical`` is
  None: nothing about it is the full enumeration); a sampled capacity bucket draws its tuples behind the gather, and
  ``handle.super_edge_index`` is the same launch into fresh memory.
* ``PairedDeviceDataset``: LEP's protein-ligand pairs (Geom3D/dataloaders/dataloaders_LEP.py) - ONE ``DeviceDataset``
  over the 2M structures, active m at id m and inactive m at id M + m, with the labels ``y [M]`` beside it.  The loader
  yields ``PairedBatch`` handles; the batch of 2B structures ``[active | inactive]`` that the one-pass step runs on
  (finetune_lep.fused_batch) is a plain ``DatasetBatch`` of that dataset, so every gather above serves it.
"""
import ctypes as C

import numpy as np
import torch

from ... import _lib
from ..._lib import call, ptr, stream
from ...batch import Batch, TripleBatch, kept_tuples
from . import masking

_OPTIONS = {"combination": 0, "permutation": 1}


class _Staging:
    """A ring of pinned int32 staging buffers (grow-only) for the small per-step uploads; a slot is reused only after the
    copy that last read it has completed."""

    def __init__(self, slots=3):
        self.slots = [[None, None] for _ in range(slots)]
        self.i = 0

    def take(self, words):
        slot = self.slots[self.i]
        self.i = (self.i + 1) % len(self.slots)
        if slot[1] is not None:
            slot[1].synchronize()
            slot[1] = None
        if slot[0] is None or slot[0].numel() < words:
            slot[0] = torch.empty(max(words + words // 2, 1024), dtype=torch.int32).pin_memory()
        return slot

    @staticmethod
    def sent(slot):
        slot[1] = torch.cuda.Event()
        slot[1].record()


def check_force(force, n_atoms):
    """The per-atom targets of a DeviceDataset as a float32 [n_atoms, 3] tensor (where they are); ValueError for any
    other shape or row count."""
    f = force if torch.is_tensor(force) else torch.from_numpy(np.ascontiguousarray(force))
    if f.dim() != 2 or f.size(1) != 3:
        raise ValueError("force is [Ntot, 3]: one row per atom, got %s" % (tuple(f.shape),))
    if f.size(0) != int(n_atoms):
        raise ValueError("sizes sum to %d atoms, force has %d rows" % (int(n_atoms), f.size(0)))
    return f.to(torch.float32)


class DeviceDataset:
    def __init__(self, x, positions, sizes, device, option="combination", radius=None, max_num_neighbors=32,
                 bond_index=None, bond_counts=None, y=None, triples=None, triple_counts=None, triple_angle=None,
                 force=None):
        """x [Ntot, C] int64 (or [Ntot]: one column), positions [Ntot, 3] float32 (numpy or tensors; molecule after
        molecule), sizes [M] atoms per molecule.  option: the AtomTupleExtractor enumeration of the batches drawn from it.  radius: also build the
        per-molecule radius_edge_index (PaiNN) on this geometry.  bond_index [2, Etot] (local atom indices, molecule
        after molecule) with bond_counts [M]: the bond graph (``data.edge_index``) that atom masking walks.  y [M, T]
        (or [M]): per-molecule targets, kept in device memory as float32 (the Supervised / fine-tuning steps).
        triples [3, Ttot] int (local atom indices, molecule after molecule) with triple_counts [M]: the atom triples of
        angle prediction (AtomTripleExtractor output per molecule); triple_angle [Ttot] float32 their targets, or None:
        computed once on the device by ops.triple_angles (this library's definition: the angle at the middle atom).
        force [Ntot, 3] float32: a per-atom target (MD17's forces, datasets_MD17.py), one row per atom, kept in device
        memory; a handle shows its molecules' rows as ``.force``."""
        if option not in _OPTIONS:
            raise ValueError("option is 'combination' or 'permutation'")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.GeosslHipError("a DeviceDataset lives on an MI355X (no CPU fallback)")
        if dev.index is None:   # ("cuda": the current device, by number - buckets and graphs compare devices)
            dev = torch.device("cuda", torch.cuda.current_device())
        as_t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, dt).contiguous()
        self.device, self.option = dev, option
        self.sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64))
        M = self.sizes.shape[0]
        self.off = np.zeros(M + 1, dtype=np.int64)
        np.cumsum(self.sizes, out=self.off[1:])
        self.x, self.positions = as_t(x, torch.int64), as_t(positions, torch.float32)
        if self.x.dim() == 1:   # (DatasetLBA's records: the atomic numbers alone - one column)
            self.x = self.x.reshape(-1, 1)
        if self.x.dim() != 2 or self.positions.dim() != 2 or self.positions.size(1) != 3:
            raise ValueError("x is [Ntot, C], positions [Ntot, 3]")
        Nt = int(self.off[-1])
        if self.x.size(0) != Nt or self.positions.size(0) != Nt:
            raise ValueError("sizes sum to %d atoms, x has %d rows, positions %d" % (Nt, self.x.size(0), self.positions.size(0)))
        if M and (self.sizes.min() < 1 or Nt >= 2 ** 31):
            raise ValueError("molecules have at least one atom; at most 2^31 - 1 atoms in all")
        self.x_cols = int(self.x.size(1))
        self.pairs = self.sizes * (self.sizes - 1) // 2
        self.radius, self.edges, self.edge_cnt, self.edge_off = None, None, None, None
        self._staging = _Staging()
        self.bonds, self.bond_off, self.bond_ptr, self.bond_dst = None, None, None, None
        if (bond_index is None) != (bond_counts is None):
            raise ValueError("bond_index and bond_counts come together")
        if bond_index is not None:
            self._set_bonds(bond_index, bond_counts)
        if radius is not None:
            self._build_edges(float(radius), int(max_num_neighbors))
        self.triples, self.triple_angle, self.triple_cnt, self.triple_off = None, None, None, None
        if (triples is None) != (triple_counts is None) or (triple_angle is not None and triples is None):
            raise ValueError("triples and triple_counts come together (triple_angle only with them)")
        if triples is not None:
            self._set_triples(triples, triple_counts, triple_angle)
        self.y, self._mol_off = None, None
        if y is not None:
            self.y = as_t(y, torch.float32)
            if self.y.dim() == 1:
                self.y = self.y.reshape(-1, 1)
            if self.y.dim() != 2 or self.y.size(0) != M:
                raise ValueError("y holds one row of targets per molecule: [%d, T], got %s" % (M, tuple(self.y.shape)))
        self.force = None
        if force is not None:
            self.force = check_force(force, Nt).to(dev).contiguous()

    def mol_off(self):
        """The atom offsets of the molecules [M + 1] as an int64 device tensor (uploaded once, on first use)."""
        if self._mol_off is None:
            self._mol_off = torch.from_numpy(self.off).to(self.device)
        return self._mol_off

    # ---- construction
    @classmethod
    def from_numpy(cls, d, device, **kw):
        """From a dict with x, positions, sizes (geossl_amd.synthetic.make_molecules / make_batch) and, when present,
        bond_index / bond_counts (synthetic.add_bonds)."""
        for k in ("bond_index", "bond_counts"):
            if k not in kw and d.get(k) is not None:
                kw[k] = d[k]
        return cls(d["x"], d["positions"], d["sizes"], device, **kw)

    @classmethod
    def from_data_list(cls, data_list, device, **kw):
        """From the reference's per-molecule records (``Data`` objects with ``x`` and ``positions``,
        datasets_3D.py:69-80, ``edge_index`` when every record has one, and ``y`` - a row of targets per molecule, the
        Molecule3D ``data.y`` - and ``force``, a row per atom, the MD17 records' - when every record has one):
        concatenated once, uploaded once."""
        x = torch.cat([torch.as_tensor(d.x) for d in data_list], dim=0)
        fs = [getattr(d, "force", None) for d in data_list]
        if "force" not in kw and data_list and all(f_ is not None for f_ in fs):
            kw["force"] = torch.cat([torch.as_tensor(f_, dtype=torch.float32).reshape(-1, 3) for f_ in fs], dim=0)
        ys = [getattr(d, "y", None) for d in data_list]
        if "y" not in kw and data_list and all(y_ is not None for y_ in ys):
            kw["y"] = torch.stack([torch.as_tensor(y_, dtype=torch.float32).reshape(-1) for y_ in ys], dim=0)
        pos = torch.cat([torch.as_tensor(d.positions) for d in data_list], dim=0)
        ei = [getattr(d, "edge_index", None) for d in data_list]
        if "bond_index" not in kw and data_list and all(e is not None for e in ei):
            kw["bond_index"] = torch.cat([torch.as_tensor(e).reshape(2, -1) for e in ei], dim=1).numpy()
            kw["bond_counts"] = [int(torch.as_tensor(e).reshape(2, -1).size(1)) for e in ei]
        return cls(x, pos, [int(d.x.size(0)) for d in data_list], device, **kw)

    def _set_bonds(self, bond_index, bond_counts):
        """The bond graph: a host copy (the numpy-mode BFS) and a CSR over dataset atoms on the device (successors in
        edge order, local indices)."""
        bi = bond_index.cpu().numpy() if torch.is_tensor(bond_index) else np.asarray(bond_index)
        bi = np.ascontiguousarray(bi.reshape(2, -1).astype(np.int64))
        cnt = np.asarray(bond_counts, dtype=np.int64)
        M = len(self)
        if cnt.shape != (M,) or (M and cnt.min() < 0) or int(cnt.sum()) != bi.shape[1]:
            raise ValueError("bond_counts has one entry per molecule and sums to the columns of bond_index")
        if bi.shape[1] >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 bonds in all")
        boff = np.zeros(M + 1, dtype=np.int64)
        np.cumsum(cnt, out=boff[1:])
        n_of = np.repeat(self.sizes, cnt)
        if bi.size and (bi.min() < 0 or (bi >= n_of[None, :]).any()):
            raise ValueError("bond_index holds local atom indices (0 .. n-1 of its molecule)")
        if (bi[0] == bi[1]).any():
            raise ValueError("the bond graph has a self-loop")
        src = np.repeat(self.off[:-1], cnt) + bi[0]          # dataset atom of each bond's source
        order = np.argsort(src, kind="stable")
        deg = np.bincount(src, minlength=int(self.off[-1]))
        rp = np.zeros(int(self.off[-1]) + 1, dtype=np.int32)
        np.cumsum(deg, out=rp[1:])
        self.bonds, self.bond_off = bi, boff
        self.bond_ptr = torch.from_numpy(rp).to(self.device)
        self.bond_dst = torch.from_numpy(np.ascontiguousarray(bi[1][order].astype(np.int32))).to(self.device)
        if self.bond_dst.numel() == 0:
            self.bond_dst = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._succ = {}

    def _set_triples(self, triples, triple_counts, triple_angle):
        """The triple lists: int32 [3, Ttot] local atom indices and float32 [Ttot] angles on the device, per-molecule
        offsets on the host (like the edge offsets)."""
        tr = triples.cpu().numpy() if torch.is_tensor(triples) else np.asarray(triples)
        tr = np.ascontiguousarray(tr.reshape(3, -1).astype(np.int64))
        cnt = np.asarray(triple_counts, dtype=np.int64)
        M = len(self)
        if cnt.shape != (M,) or (M and cnt.min() < 0) or int(cnt.sum()) != tr.shape[1]:
            raise ValueError("triple_counts has one entry per molecule and sums to the columns of triples")
        if tr.shape[1] >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 triples in all")
        if tr.size and (tr.min() < 0 or (tr >= np.repeat(self.sizes, cnt)[None, :]).any()):
            raise ValueError("triples holds local atom indices (0 .. n-1 of its molecule)")
        self.triple_cnt = cnt
        self.triple_off = np.zeros(M + 1, dtype=np.int64)
        np.cumsum(cnt, out=self.triple_off[1:])
        Tt = tr.shape[1]
        dev = self.device
        self.triples = torch.zeros(3, max(Tt, 1), dtype=torch.int32, device=dev)
        self.triples[:, :Tt] = torch.from_numpy(tr.astype(np.int32)).to(dev)
        if triple_angle is not None:
            ang = (triple_angle if torch.is_tensor(triple_angle)
                   else torch.from_numpy(np.ascontiguousarray(np.asarray(triple_angle, dtype=np.float32))))
            ang = ang.to(dev, torch.float32).reshape(-1)
            if ang.numel() != Tt:
                raise ValueError("triple_angle holds one angle per triple")
        else:   # the angle at the middle atom, on the dataset's own geometry (dataset atom ids = local + atom offset)
            from ...ops import triple_angles
            glob = torch.from_numpy(tr + np.repeat(self.off[:-1], cnt)[None, :]).to(dev)
            ang = triple_angles(self.positions, glob)
        self.triple_angle = torch.zeros(max(Tt, 1), dtype=torch.float32, device=dev)
        self.triple_angle[:Tt] = ang

    def sample_triples(self, ratio):
        """Draw the dataset's triples with AtomTripleExtractor(ratio), molecule after molecule on the global np.random
        stream (what the reference's per-molecule transform does over the same molecules), angles by ops.triple_angles.
        Host work, once.  -> self"""
        from .dataloaders_AtomTriple import AtomTripleExtractor
        ext = AtomTripleExtractor(ratio)
        parts = [ext.triples(int(n)) for n in self.sizes]
        tr = np.concatenate(parts, axis=1) if parts else np.empty((3, 0), dtype=np.int64)
        self._set_triples(tr, [p_.shape[1] for p_ in parts], None)
        return self

    def successors(self, i):
        """to_networkx successor lists of molecule i (cached)."""
        s = self._succ.get(i)
        if s is None:
            s = self._succ[i] = masking.successors(int(self.sizes[i]), self.bonds[:, self.bond_off[i]:self.bond_off[i + 1]])
        return s

    def check_masking(self, ratio):
        """Can this dataset be masked at `ratio`?  Raises ValueError when not."""
        if self.bonds is None:
            raise ValueError("atom masking walks the bond graph: build the DeviceDataset with bond_index / bond_counts "
                             "(or records with edge_index)")
        if len(self) and int(self.sizes.max()) > masking.MASK_MAX_N:
            raise ValueError("atom masking takes molecules of at most %d atoms" % masking.MASK_MAX_N)
        if len(self) and (masking.kept_count(self.sizes, ratio) > self.sizes).any():
            raise ValueError("mask_ratio %r keeps more atoms than a molecule has" % (ratio,))

    def _build_edges(self, radius, max_num_neighbors):
        """radius_graph(positions, r) of every molecule (datasets_3D_Radius.py:120) in two launches over the whole
        dataset: [source ; target] with DATASET atom ids, target-major - a molecule's edges are one contiguous run."""
        from ...layout import SPARSE_MAX_N
        from ...ops import radius_cap
        M, Nt, dev = len(self), int(self.off[-1]), self.device
        mol_ptr = torch.from_numpy(self.off.astype(np.int32)).to(dev)
        max_n = int(self.sizes.max()) if M else 0
        if max_n > SPARSE_MAX_N:   # (the graph kernels keep a structure's positions and bit matrix in LDS)
            raise ValueError("radius edges are built for structures of at most %d atoms (the largest here has %d)"
                             % (SPARSE_MAX_N, max_n))
        r2 = float(torch.tensor(radius * radius, dtype=torch.float32))
        cap = radius_cap(max_num_neighbors)
        deg = torch.zeros(Nt, dtype=torch.int32, device=dev)
        call("geossl_radius_graph_count", ptr(self.positions), ptr(mol_ptr), M, max_n, r2, cap, ptr(deg), stream())
        edge_ptr = torch.zeros(Nt + 1, dtype=torch.int64, device=dev)
        edge_ptr[1:] = torch.cumsum(deg, 0, dtype=torch.int64)
        self.edge_off = edge_ptr[torch.from_numpy(self.off).to(dev)].cpu().numpy().astype(np.int64)   # the one read-back
        E = int(self.edge_off[-1])
        if E >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 radius edges in all")
        e = torch.empty(2, max(E, 1), dtype=torch.int64, device=dev)
        w = torch.empty(max(E, 1), dtype=torch.float32, device=dev)
        if E:
            call("geossl_radius_graph_fill", ptr(self.positions), ptr(mol_ptr), M, max_n, r2, cap, ptr(edge_ptr), ptr(e[0]),
                 ptr(e[1]), ptr(w), stream())
        self.edges, self.radius = e[:, :E], radius
        self.edge_cnt = np.diff(self.edge_off)

    def __len__(self):
        return int(self.sizes.shape[0])

    # ---- batches
    def batch(self, ids):
        """The handle of these molecules (what an unmasked DeviceLoader yields)."""
        return DatasetBatch(self, ids)

    def __getitem__(self, ids):
        if isinstance(ids, (int, np.integer)):
            ids = [int(ids)]
        return DatasetBatch(self, ids)

    def upload_plan(self, hb, with_edges):
        """int32 words [src_off (B) | mol_ptr (B+1) | se_ptr (B+1) | e_src_off (B) | e_ptr (B+1) | mol_id (B, a sampled
        handle)] of a handle on the device (fresh memory) -> (tensor, offsets)."""
        B = hb.num_graphs
        o = {"src_off": 0, "mol_ptr": B, "se_ptr": 2 * B + 1}
        words = 3 * B + 2
        if with_edges:
            o["e_src_off"], o["e_ptr"] = words, words + B
            words += 2 * B + 1
        if hb._sampled is not None:
            o["mol_id"], words = words, words + B
        slot = self._staging.take(words)
        h = slot[0].numpy()
        h[0:B] = self.off[hb.ids]
        mp = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(hb._sizes, out=mp[1:])
        h[B:2 * B + 1] = mp
        sp = np.zeros(B + 1, dtype=np.int64)
        if hb._sampled is not None:   # (the kept counts; the draw's counter: the low word of the dataset ids)
            np.cumsum(hb.tuple_counts, out=sp[1:])
            h[o["mol_id"]:o["mol_id"] + B] = (hb.ids & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        else:
            pairs = self.pairs[hb.ids] if hb._mask is None else hb._sizes * (hb._sizes - 1) // 2
            np.cumsum(pairs * (1 if self.option == "combination" else 2), out=sp[1:])
        h[2 * B + 1:3 * B + 2] = sp
        if with_edges and hb._mask is not None:   # (masked: the batch's edge offsets follow the count launch)
            h[o["e_src_off"]:o["e_src_off"] + B] = self.edge_off[hb.ids]
            h[o["e_ptr"]:o["e_ptr"] + B + 1] = 0
        elif with_edges:
            h[o["e_src_off"]:o["e_src_off"] + B] = self.edge_off[hb.ids]
            ep = np.zeros(B + 1, dtype=np.int64)
            np.cumsum(self.edge_cnt[hb.ids], out=ep[1:])
            h[o["e_ptr"]:o["e_ptr"] + B + 1] = ep
        blob = torch.empty(words, dtype=torch.int32, device=self.device)
        blob.copy_(slot[0][:words], non_blocking=True)
        self._staging.sent(slot)
        return blob, o

    def mask_plan(self, hb, with_edges=False):
        """A masked handle's side of geossl_gather_masked_molecules on the device (fresh memory): int32 words
        [mol_id (B int64) | src_n (B) | e_src_cnt (B, with_edges) | keep (N, numpy mode)] -> a filled _lib.Mask whose
        buffers stay alive with the returned tensor."""
        B, mk = hb.num_graphs, hb._mask
        o = {"mol_id": 0, "src_n": 2 * B}
        words = 3 * B
        if with_edges:
            o["e_src_cnt"], words = words, words + B
        if mk.keep is not None:
            o["keep"], words = words, words + hb.n_atoms
        slot = self._staging.take(words)
        h = slot[0].numpy()
        h[0:2 * B].view(np.int64)[:] = hb.ids
        h[o["src_n"]:o["src_n"] + B] = hb._src_n
        if with_edges:
            h[o["e_src_cnt"]:o["e_src_cnt"] + B] = self.edge_cnt[hb.ids]
        if mk.keep is not None:
            h[o["keep"]:o["keep"] + hb.n_atoms] = mk.keep
        blob = torch.empty(words, dtype=torch.int32, device=self.device)
        blob.copy_(slot[0][:words], non_blocking=True)
        self._staging.sent(slot)
        base = blob.data_ptr()
        m = _lib.Mask()
        m.bond_ptr, m.bond_dst = ptr(self.bond_ptr), ptr(self.bond_dst)
        m.mol_id, m.src_n = base + 4 * o["mol_id"], base + 4 * o["src_n"]
        if with_edges:
            m.e_src_cnt = base + 4 * o["e_src_cnt"]
        if mk.keep is not None:
            m.keep_in = base + 4 * o["keep"]
        m.seed = 0 if mk.seed is None else int(mk.seed)
        m.max_n = int(hb._src_n.max())
        return m, blob

    def collate(self, hb):
        """The collated batch of a handle as fresh device tensors - what ``BatchAtomTuple.from_data_list`` over these
        molecules followed by ``.to(device)`` holds (bit for bit) - with the host-side sizes attached."""
        from ...layout import prepare_batch
        B, dev = hb.num_graphs, self.device
        N, S = hb.n_atoms, (0 if self.triples is not None else hb.n_super)   # (a triple dataset enumerates no pair tuples)
        with_edges = self.edges is not None
        blob, o = self.upload_plan(hb, with_edges)
        hb.__dict__["_plan"] = (blob, o)   # (the uploaded offsets: a per-atom target is gathered from them, `.force`)
        x = torch.empty(N, self.x_cols, dtype=torch.int64, device=dev)
        pos = torch.empty(N, 3, dtype=torch.float32, device=dev)
        bvec = torch.empty(N, dtype=torch.int64, device=dev)
        sei = torch.empty(2, S, dtype=torch.int64, device=dev)
        g = _lib.Gather()
        g.x_src, g.pos_src, g.x_cols, g.option = ptr(self.x), ptr(self.positions), self.x_cols, _OPTIONS[self.option]
        base = blob.data_ptr()
        g.src_off, g.mol_ptr, g.se_ptr = base + 4 * o["src_off"], base + 4 * o["mol_ptr"], base + 4 * o["se_ptr"]
        g.x_dst, g.pos_dst, g.batch_dst = ptr(x), ptr(pos), ptr(bvec)
        sampled = hb._sampled is not None   # (its tuples come from geossl_sampled_tuples behind the gather)
        if S and not sampled:
            g.sei0, g.sei1 = ptr(sei[0]), ptr(sei[1])
        rei = None
        if hb._mask is not None:
            m, mblob = self.mask_plan(hb, with_edges)
            keep = None
            if with_edges:
                rei, keep = self._masked_edges(hb, g, m, blob, o)
            call("geossl_gather_masked_molecules", C.byref(g), C.byref(m), B, stream())
            del mblob, keep   # (stream order: a later owner of this memory writes after the launch read it)
        else:
            if with_edges:
                E = hb.n_edges
                rei = torch.empty(2, E, dtype=torch.int64, device=dev)
                if E:
                    g.e0_src, g.e1_src = ptr(self.edges[0]), ptr(self.edges[1])
                    g.e_src_off, g.e_ptr = base + 4 * o["e_src_off"], base + 4 * o["e_ptr"]
                    g.e0_dst, g.e1_dst = ptr(rei[0]), ptr(rei[1])
            call("geossl_gather_molecules", C.byref(g), B, stream())
        if self.triples is not None:   # a triple dataset: the handle shows its triples and their angles
            return self._collate_triples(hb, x, pos, bvec, rei, blob, o)
        if sampled:
            self._sampled_tuples(hb, blob, o, sei)
        out = Batch(x, pos, bvec, sei, rei, B, hb._sizes, None if sampled else self.option)
        out._sampled = hb._sampled
        prepare_batch(bvec, sei, hb._sizes, lazy=True)
        return out

    def _sampled_tuples(self, hb, blob, o, sei):
        """The tuples of a sampled handle into `sei` [2, S]: drawn by geossl_sampled_tuples from the handle's seed, or -
        a host-drawn list - copied in and checked by it; the same launch a bucket fill makes for the handle."""
        draw, B, base = hb._tuple_draw, hb.num_graphs, blob.data_ptr()
        if not sei.size(1):
            return
        if draw.seed is None:
            sei.copy_(torch.from_numpy(draw.tuples))
        st = self.__dict__.get("_tuple_status")
        if st is None:
            st = self.__dict__["_tuple_status"] = _lib.StatusWord(self.device, "a sampled handle's tuples leave their "
                                                                  "molecules")
        st.poll()
        call("geossl_sampled_tuples", base + 4 * o["mol_ptr"], base + 4 * o["se_ptr"], B, _OPTIONS[self.option],
             base + 4 * o["mol_id"], 0 if draw.seed is None else 1, 0 if draw.seed is None else int(draw.seed),
             hb.n_atoms, sei.size(1), ptr(sei[0]), ptr(sei[1]), None, None, ptr(st.word), stream())
        st.arm(every=8)

    def _collate_triples(self, hb, x, pos, bvec, rei, blob, o):
        from ...layout import prepare_batch
        B, T, dev = hb.num_graphs, hb.n_triples, self.device
        tri = torch.empty(3, T, dtype=torch.int64, device=dev)
        ang = torch.empty(T, dtype=torch.float32, device=dev)
        if T:
            slot = self._staging.take(2 * B + 1)
            h = slot[0].numpy()
            h[0:B] = self.triple_off[hb.ids]
            h[B] = 0
            np.cumsum(self.triple_cnt[hb.ids], out=h[B + 1:2 * B + 1])
            tb = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
            tb.copy_(slot[0][:2 * B + 1], non_blocking=True)
            self._staging.sent(slot)
            base = tb.data_ptr()
            call("geossl_gather_triples", ptr(self.triples), self.triples.size(1), ptr(self.triple_angle), base,
                 base + 4 * B, blob.data_ptr() + 4 * o["mol_ptr"], B, ptr(tri[0]), ptr(tri[1]), ptr(tri[2]), ptr(ang),
                 stream())
        out = TripleBatch(x, pos, bvec, tri, ang, rei, B, hb._sizes)
        prepare_batch(bvec, tri, hb._sizes, lazy=True)
        return out

    def _masked_edges(self, hb, g, m, blob, o):
        """Radius edges of a masked handle: the count launch (kept lists + survivors per molecule), ONE read-back of
        the B counts, the batch's edge offsets into `blob`; `g` / `m` are then set up for the gather launch (keep_in =
        the count launch's kept lists) and the [2, E] edge tensor is returned with the kept lists' buffer."""
        B, dev, base = hb.num_graphs, self.device, blob.data_ptr()
        keep = torch.empty(max(hb.n_atoms, 1), dtype=torch.int32, device=dev)
        cnt = torch.empty(B, dtype=torch.int32, device=dev)
        g.e0_src, g.e1_src = ptr(self.edges[0]), ptr(self.edges[1])
        g.e_src_off = base + 4 * o["e_src_off"]
        m.keep_out, m.e_count = ptr(keep), ptr(cnt)
        call("geossl_gather_masked_molecules", C.byref(g), C.byref(m), B, stream())
        counts = cnt.cpu().numpy().astype(np.int64)     # the read-back
        ep = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(counts, out=ep[1:])
        E = int(ep[-1])
        hb.n_edges = E
        blob[o["e_ptr"]:o["e_ptr"] + B + 1].copy_(torch.from_numpy(ep.astype(np.int32)))
        rei = torch.empty(2, E, dtype=torch.int64, device=dev)
        m.keep_out, m.e_count, m.keep_in = None, None, ptr(keep)
        if E:
            g.e_ptr, g.e0_dst, g.e1_dst = base + 4 * o["e_ptr"], ptr(rei[0]), ptr(rei[1])
        else:
            g.e0_src = g.e1_src = g.e_src_off = None
        return rei, keep

    def gather_into(self, hb, x_dst, pos_dst, mol_ptr, zero=None):
        """x / positions of the handle's molecules into the static inputs of a per-structure graph (whose index tensors
        are bound): `mol_ptr` is the int32 [B+1] device array of that structure."""
        B = hb.num_graphs
        if x_dst.size(1) != self.x_cols or x_dst.size(0) != hb.n_atoms or pos_dst.size(0) != hb.n_atoms:
            raise ValueError("static inputs do not have the batch's shape")
        slot = self._staging.take(B)
        slot[0].numpy()[0:B] = self.off[hb.ids]
        dst = self.__dict__.get("_src_off_dev")   # (one buffer: upload and launch are ordered on the stream)
        if dst is None or dst.numel() < B:
            dst = self.__dict__["_src_off_dev"] = torch.empty(max(B, 1024), dtype=torch.int32, device=self.device)
        dst[:B].copy_(slot[0][:B], non_blocking=True)
        self._staging.sent(slot)
        g = _lib.Gather()
        g.x_src, g.pos_src, g.x_cols, g.option = ptr(self.x), ptr(self.positions), self.x_cols, _OPTIONS[self.option]
        g.src_off, g.mol_ptr = ptr(dst), ptr(mol_ptr)
        g.x_dst, g.pos_dst = ptr(x_dst), ptr(pos_dst)
        if zero is not None:
            g.zero, g.zero_count = ptr(zero), zero.numel()
        if hb._mask is not None:
            m, mblob = self.mask_plan(hb)
            call("geossl_gather_masked_molecules", C.byref(g), C.byref(m), B, stream())
            del mblob
        else:
            call("geossl_gather_molecules", C.byref(g), B, stream())


_SAMPLED_STAMP = [0]   # the last stamp handed to a sampled handle's fingerprint (never handed out again)


class DatasetBatch:
    """``batch_size`` molecules of a ``DeviceDataset`` by id: what the loader hands to a step.  Host side only - ids,
    sizes, counts; the collated tensors exist once somebody asks for them.  `mask` (masking.MaskDraw): a masked batch
    - its sizes are the kept counts, the original ones are ``_src_n``; the radius edges of a masked batch are counted
    when it is collated (``n_edges`` is None until then; ``n_edges_bound`` is an upper bound known on the host, which is
    what a PaiNN capacity bucket is sized by - its fill counts the survivors on the device and reads nothing back)."""

    def __init__(self, dataset, ids, mask=None, tuples=None):
        self._dataset = dataset
        self.ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64))
        if self.ids.ndim != 1 or not self.ids.size:
            raise ValueError("a batch is a non-empty list of molecule ids")
        if self.ids.min() < 0 or self.ids.max() >= len(dataset):
            raise IndexError("molecule id out of range")
        self._sizes = dataset.sizes[self.ids]            # (numpy: bucket.sizes_array takes it as it is)
        self._mask = mask
        if mask is not None:
            self._src_n = self._sizes
            self._sizes = masking.kept_count(self._src_n, mask.ratio)
            if mask.keep is not None and mask.keep.shape != (int(self._sizes.sum()),):
                raise ValueError("kept lists of a masked batch hold k(n) atoms per molecule")
        # a triple dataset: the handle's super_edge_index are its sampled triples - nothing the sizes determine
        self._triples = getattr(dataset, "triples", None) is not None
        self._canonical = None if self._triples else dataset.option
        # `tuples` (TupleDraw): a SAMPLED batch - AtomTupleExtractor(ratio < 1) over its molecules.  The kept counts are a
        # function of the sizes (``tuple_counts``); which tuples is the draw's.  ``_sampled`` = (option, ratio) is the mark
        # a sampled capacity bucket reads (bucket.option_of); ``_canonical`` stays None: nothing here is the enumeration
        self._sampled, self._tuple_draw, self.tuple_counts = None, tuples, None
        if tuples is not None:
            if self._triples:
                raise ValueError("sampled pair tuples of a triple dataset are not supported: its batches show triples")
            self._canonical, self._sampled = None, (dataset.option, float(tuples.ratio))
            self.tuple_counts = kept_tuples(self._sizes, dataset.option, tuples.ratio)
            if tuples.tuples is not None and tuples.tuples.shape != (2, int(self.tuple_counts.sum())):
                raise ValueError("the tuples of a sampled batch hold int(M * ratio) columns per molecule")
        if self._triples and mask is not None:
            raise ValueError("atom masking of a triple dataset is not supported (its triples name atoms by index)")
        self.n_triples = int(dataset.triple_cnt[self.ids].sum()) if self._triples else 0
        self.device = dataset.device
        self.x_cols = dataset.x_cols
        self.num_graphs = int(self.ids.size)
        self.n_atoms = int(self._sizes.sum())
        P = int(dataset.pairs[self.ids].sum()) if mask is None else int((self._sizes * (self._sizes - 1) // 2).sum())
        self.n_super = P if dataset.option == "combination" else 2 * P
        if tuples is not None:
            self.n_super = int(self.tuple_counts.sum())
        self.n_edges = int(dataset.edge_cnt[self.ids].sum()) if dataset.edges is not None and mask is None else None
        # what a capacity is sized by: the edge count, or - masked - a host-side upper bound on the survivors (a molecule
        # keeps at most the edges it has and at most the k (k - 1) ordered pairs of its k kept atoms); None without edges
        self.n_edges_bound = self.n_edges
        if dataset.edges is not None and mask is not None:
            k = self._sizes
            self.n_edges_bound = int(np.minimum(dataset.edge_cnt[self.ids], k * (k - 1)).sum())
        self._batch = None

    def materialize(self):
        if self._batch is None:
            self._batch = self._dataset.collate(self)
        return self._batch

    x = property(lambda self: self.materialize().x)
    positions = property(lambda self: self.materialize().positions)
    batch = property(lambda self: self.materialize().batch)
    super_edge_index = property(lambda self: self.materialize().super_edge_index)
    radius_edge_index = property(lambda self: self.materialize().radius_edge_index)
    super_edge_angle = property(lambda self: self.materialize().super_edge_angle if self._triples else None)

    @property
    def y(self):
        """The targets as the reference's collation holds them: the molecules' rows concatenated along dim 0 ([B * T];
        ``batch.y.view(B, -1)[:, task_id]`` is a column).  None for a dataset without targets."""
        ds = self._dataset
        if ds.y is None:
            return None
        got = self.__dict__.get("_y")
        if got is None:
            ids = torch.from_numpy(self.ids).to(ds.device, non_blocking=False)
            got = self.__dict__["_y"] = ds.y.index_select(0, ids).reshape(-1)
        return got

    @property
    def force(self):
        """The per-atom targets of the batch's atoms [N, 3] (finetune_md17.py:49 ``batch_data.force``): gathered on the
        device on first access, in one launch (geossl_gather_atom_rows) from the source offsets the position gather
        uploaded.  None for a dataset without them."""
        ds = self._dataset
        if getattr(ds, "force", None) is None:
            return None
        if self._mask is not None:
            raise ValueError("a masked handle has no forces: the forces of a masked subgraph are not the frame's")
        got = self.__dict__.get("_force")
        if got is None:
            from ...ops import gather_atom_rows
            self.materialize()
            blob, o = self.__dict__["_plan"]
            base = blob.data_ptr()
            got = self.__dict__["_force"] = gather_atom_rows(ds.force, base + 4 * o["src_off"], base + 4 * o["mol_ptr"],
                                                             self.num_graphs, self.n_atoms)
        return got

    def to(self, device, **kw):
        """``batch.to(device)`` of the reference's loop (pretrain_GeoSSL.py:248): the molecules are there already."""
        dev = torch.device(device)
        if dev.type != self.device.type or (dev.index is not None and dev.index != self.device.index):
            raise _lib.GeosslHipError("a DatasetBatch lives on %s (its molecules are gathered there; there is no copy to "
                                      "another device)" % self.device)
        return self

    def fingerprint(self):
        """batch.structure_fingerprint of the collated batch, from the host sizes alone."""
        fp = self.__dict__.get("_fp")
        if fp is None and self._triples:   # (sampled triples: only the same molecules share index tensors)
            fp = self.__dict__["_fp"] = ("triples", id(self._dataset), self.ids.tobytes())
        if fp is None and self._sampled is not None:
            # sampled tuples: only the same draw shares index tensors - this handle alone.  A lifetime-unique stamp, not
            # id(): a shuffled loader's handles are freed step by step and CPython hands their addresses out again
            _SAMPLED_STAMP[0] += 1
            fp = self.__dict__["_fp"] = ("sampled", _SAMPLED_STAMP[0])
        if fp is None:
            fp = self.__dict__["_fp"] = ("sizes", self._canonical, self.n_atoms, self.n_super,
                                         np.asarray(self._sizes, dtype=np.int32).tobytes())
        return fp


class TupleDraw:
    """How the tuples of one sampled batch are chosen: `seed` (device draw, geossl_sampled_tuples) or `tuples` (the
    host's list: int64 [2, S] batch atom ids, molecule after molecule, each molecule's in the order np.random.choice
    drew them - what the host extractor's collated batch holds)."""

    def __init__(self, ratio, seed=None, tuples=None):
        self.ratio, self.seed, self.tuples = ratio, seed, tuples


TUPLE_RNGS = ("device", "numpy")


def check_tuple_ratio(ratio):
    r = float(ratio)
    if not (0.0 < r <= 1.0):
        raise ValueError("tuple_ratio is in (0, 1], got %r" % (ratio,))
    return r


class PairedDeviceDataset:
    """M protein-ligand pairs - each in its ACTIVE and its INACTIVE conformation, with a label - resident in HBM: what
    ``DataLoaderLEP`` collates per step (dataloaders_LEP.py), uploaded once.  The 2M structures are one ``DeviceDataset``
    (``structures``): active m at id m, inactive m at id M + m; ``y [M]`` float32 on the device beside it."""

    def __init__(self, x_active, positions_active, sizes_active, x_inactive, positions_inactive, sizes_inactive, y,
                 device, radius=None, max_num_neighbors=32):
        """x_* [Ntot_*] int64 (or [Ntot_*, C]), positions_* [Ntot_*, 3] float32, sizes_* [M] atoms per structure (numpy
        or tensors; structure after structure); y [M], integer or float: stored as float32 (finetune_lep.py:43).
        radius: also build every structure's radius_edge_index (PaiNN) once on the device, as ``DeviceDataset`` does."""
        as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        xa, xi = as_t(x_active).cpu(), as_t(x_inactive).cpu()
        pa, pi = as_t(positions_active).cpu().float(), as_t(positions_inactive).cpu().float()
        if xa.dim() != xi.dim() or xa.shape[1:] != xi.shape[1:]:
            raise ValueError("x_active and x_inactive have the same columns")
        # the reference's two asserts (dataloaders_LEP.py:49-52): a position row that sums to 0 marks a padded / missing atom
        assert (pa.sum(1) == 0).sum() == 0
        assert (pi.sum(1) == 0).sum() == 0
        sa, si = (np.asarray(as_t(n_).cpu().numpy() if torch.is_tensor(n_) else n_, dtype=np.int64).reshape(-1)
                  for n_ in (sizes_active, sizes_inactive))
        if sa.shape != si.shape:
            raise ValueError("one active and one inactive structure per pair: got %d and %d" % (sa.size, si.size))
        M = int(sa.size)
        self.x_1d = xa.dim() == 1   # (DatasetLEP's records: the atom types alone - the backbone gets them as they are)
        self.structures = DeviceDataset(torch.cat([xa, xi]), torch.cat([pa, pi]), np.concatenate([sa, si]), device,
                                        radius=radius, max_num_neighbors=max_num_neighbors)
        self.device, self.x_cols = self.structures.device, self.structures.x_cols
        self.sizes = self.structures.sizes            # [2M]: active | inactive
        self.sizes_active, self.sizes_inactive = self.sizes[:M], self.sizes[M:]
        yt = as_t(y).reshape(-1)
        if yt.numel() != M:
            raise ValueError("y holds one label per pair: [%d], got %s" % (M, tuple(as_t(y).shape)))
        self.y = yt.to(self.device, torch.float32).contiguous()
        self._M = M

    @classmethod
    def from_data_list(cls, items, device, radius=None, max_num_neighbors=32):
        """From the reference's LEP records (``x_active``, ``positions_active``, ``x_inactive``, ``positions_inactive``,
        ``y``: what ``DataLoaderLEP`` consumes): concatenated once, uploaded once.  radius: the structures' radius edges
        are built on the device from these positions (the records' own ``radius_edge_index_*`` are not read)."""
        cat = lambda k: torch.cat([torch.as_tensor(getattr(d, k)) for d in items], dim=0)
        n = lambda k: [int(torch.as_tensor(getattr(d, k)).size(0)) for d in items]
        y = torch.cat([torch.as_tensor(d.y).reshape(-1) for d in items])
        return cls(cat("x_active"), cat("positions_active"), n("x_active"), cat("x_inactive"),
                   cat("positions_inactive"), n("x_inactive"), y, device, radius=radius,
                   max_num_neighbors=max_num_neighbors)

    def __len__(self):
        return self._M

    def batch(self, ids):
        return PairedBatch(self, ids)

    def __getitem__(self, ids):
        return PairedBatch(self, [int(ids)] if isinstance(ids, (int, np.integer)) else ids)


class PairedBatch:
    """``batch_size`` pairs of a ``PairedDeviceDataset`` by id.  Host side only: the pair ids, the ids and sizes of the 2B
    fused structures ``[active 0 .. B-1 | inactive 0 .. B-1]`` (the batch the one-pass LEP step runs on:
    ``fused()``, a ``DatasetBatch`` of the dataset's ``structures``), and ``y [B]`` on the device.  Whoever asks for the
    attributes of a collated ``BatchLEP`` (``x_active``, ``positions_active``, ``batch_active``, the three inactive ones)
    gets them from ONE gather launch on the device - bit for bit ``BatchLEP.from_data_list`` of the same records - so the
    reference's lines, the eager step and ``eval_LEP`` take a handle unchanged."""

    _mask, _triples, _canonical = None, False, None   # (whole structures; the LEP step reads no tuples)

    def __init__(self, dataset, ids):
        self._dataset = dataset
        self.ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64))
        M = len(dataset)
        if self.ids.ndim != 1 or not self.ids.size:
            raise ValueError("a batch is a non-empty list of pair ids")
        if self.ids.min() < 0 or self.ids.max() >= M:
            raise IndexError("pair id out of range")
        B = int(self.ids.size)
        self.fused_ids = np.concatenate([self.ids, self.ids + M])
        self._sizes = dataset.sizes[self.fused_ids]
        self._sizes_active, self._sizes_inactive = self._sizes[:B], self._sizes[B:]
        self.num_graphs = B
        self.n_atoms = int(self._sizes.sum())
        self.device, self.x_cols = dataset.device, dataset.x_cols
        self._fused, self._batch = None, None

    def fused(self):
        """The 2B structures as a handle on the dataset's ``structures`` (made once)."""
        if self._fused is None:
            self._fused = _FusedPairs(self)
        return self._fused

    @property
    def y(self):
        got = self.__dict__.get("_y")
        if got is None:
            ds = self._dataset
            got = self.__dict__["_y"] = ds.y.index_select(0, torch.from_numpy(self.ids).to(ds.device))
        return got

    def materialize(self):
        """The collated tensors of both sides: views of the fused handle's gathered x / positions / batch vector."""
        if self._batch is None:
            fb, B, na = self.fused().materialize(), self.num_graphs, int(self._sizes_active.sum())
            x = fb.x[:, 0] if self._dataset.x_1d else fb.x
            self._batch = dict(x_active=x[:na], x_inactive=x[na:], positions_active=fb.positions[:na],
                               positions_inactive=fb.positions[na:], batch_active=fb.batch[:na],
                               batch_inactive=fb.batch[na:] - B)
            rei = fb.radius_edge_index
            if rei is not None:   # (a dataset built with radius=: each side's edges with its own running atom counts)
                ea = int(self._dataset.structures.edge_cnt[self.ids].sum())
                self._batch.update(radius_edge_index_active=rei[:, :ea], radius_edge_index_inactive=rei[:, ea:] - na)
        return self._batch

    x_active = property(lambda self: self.materialize()["x_active"])
    x_inactive = property(lambda self: self.materialize()["x_inactive"])
    positions_active = property(lambda self: self.materialize()["positions_active"])
    positions_inactive = property(lambda self: self.materialize()["positions_inactive"])
    batch_active = property(lambda self: self.materialize()["batch_active"])
    batch_inactive = property(lambda self: self.materialize()["batch_inactive"])
    # (None for a dataset built without radius=: the attribute a collated BatchLEP without edges does not have either)
    radius_edge_index_active = property(lambda self: self.materialize().get("radius_edge_index_active"))
    radius_edge_index_inactive = property(lambda self: self.materialize().get("radius_edge_index_inactive"))

    def to(self, device, **kw):
        """``batch.to(device)`` of the reference's loop: the structures are there already."""
        dev = torch.device(device)
        if dev.type != self.device.type or (dev.index is not None and dev.index != self.device.index):
            raise _lib.GeosslHipError("a PairedBatch lives on %s (its structures are gathered there; there is no copy to "
                                      "another device)" % self.device)
        return self


class _FusedPairs(DatasetBatch):
    """The 2B structures of a ``PairedBatch`` as a handle on the paired dataset's ``structures``: what a bucket fill, a
    per-structure graph's refresh and the eager step gather from.  No pair tuples are enumerated (``n_super`` = 0:
    the LEP step reads none, and 2B pockets would have millions), and no tuple option routes it to a dense bucket."""

    def __init__(self, pairs):
        super().__init__(pairs._dataset.structures, pairs.fused_ids)
        self._canonical, self.n_super = None, 0
        self.pairs = pairs

    y = property(lambda self: self.pairs.y)


class DeviceLoader:
    """``DataLoaderAtomTuple(dataset, batch_size, shuffle)`` (dataloaders_AtomTuple.py:81-88) over a ``DeviceDataset``:
    iterating yields the dataset's handles (``dataset.batch(ids)``: ``DatasetBatch``, or ``PairedBatch`` over a
    ``PairedDeviceDataset``).  With ``shuffle=True`` the molecules are visited in the order
    ``torch.utils.data.RandomSampler`` produces under the same global torch seed (one ``torch.randperm`` per epoch from
    a generator seeded by one draw of the default generator), so a run is reproducible against the reference's loader."""

    def __init__(self, dataset, batch_size=1, shuffle=True, drop_last=False, generator=None, mask_ratio=0.0,
                 mask_rng="device", tuple_ratio=1.0, tuple_rng="device"):
        """mask_ratio > 0: yield masked handles (the reference's ``--GeoSSL_atom_masking_ratio``, datasets_3D.py:77-78).
        mask_rng "device": the kept atoms are drawn on the GPU from Philox-4x32-10, keyed by one np.random.randint
        draw per epoch (so np.random.seed(seed) repeats a run) with counter (molecule id, draw index); the rule is in
        include/geossl_hip.h (geossl_gather_masked_molecules) and DESIGN 2.  "numpy": the reference's own BFS and
        np.random draws on the host, molecule after molecule in batch order when the handle is yielded (bit-for-bit
        the masks of a reference run; about as slow as it).

        tuple_ratio < 1: yield SAMPLED handles - the reference's ``--distance_sample_ratio``, AtomTupleExtractor(ratio)
        (pretrain_GeoSSL.py:295, pretrain_DistancePrediction.py:111): every molecule keeps int(M * ratio) of its M
        tuples.  tuple_rng "device": the kept tuples are drawn on the GPU (geossl_sampled_tuples: the smallest Philox
        keys of the enumeration's slots, counter (slot, molecule id); the rule is in include/geossl_hip.h), keyed by one
        more np.random.randint draw per epoch, made after the mask seed and only when tuple_ratio < 1.  "numpy": the
        reference's own np.random.choice call per molecule in batch order when the handle is yielded; with
        mask_rng="numpy" the two interleave per molecule, mask draws first (Molecule3DDataset.__getitem__, then the
        transform).  Not for triple datasets, paired datasets or molecules above 255 atoms (the sparse bucket)."""
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), shuffle, drop_last
        self.generator = generator
        self.mask_ratio = masking.check_ratio(mask_ratio)
        if mask_rng not in masking.MASK_RNGS:
            raise ValueError("mask_rng is 'device' or 'numpy'")
        self.mask_rng = mask_rng
        if self.mask_ratio > 0:
            if isinstance(dataset, PairedDeviceDataset):
                raise ValueError("mask_ratio > 0 with a paired dataset is not supported: the reference's LEP loader "
                                 "masks nothing")
            if getattr(dataset, "triples", None) is not None:
                raise ValueError("mask_ratio > 0 with a triple dataset is not supported: the sampled triples name atoms "
                                 "by index, and masking renumbers them")
            if getattr(dataset, "force", None) is not None:
                raise ValueError("mask_ratio > 0 with a dataset that holds per-atom forces is not supported: the forces "
                                 "of a masked subgraph are not the frame's")
            dataset.check_masking(self.mask_ratio)
        self.tuple_ratio = check_tuple_ratio(tuple_ratio)
        if tuple_rng not in TUPLE_RNGS:
            raise ValueError("tuple_rng is 'device' or 'numpy'")
        self.tuple_rng = tuple_rng
        if self.tuple_ratio < 1:
            if isinstance(dataset, PairedDeviceDataset):
                raise ValueError("tuple_ratio < 1 with a paired dataset is not supported: the LEP step reads no tuples "
                                 "and its loader samples none")
            if getattr(dataset, "triples", None) is not None:
                raise ValueError("tuple_ratio < 1 with a triple dataset is not supported: its batches show the sampled "
                                 "triples, not pair tuples (sample those with sample_triples(ratio))")
            if len(dataset) and int(dataset.sizes.max()) > 255:
                raise ValueError("tuple_ratio < 1 takes molecules of at most 255 atoms: larger structures go through the "
                                 "sparse bucket, which enumerates no tuples")

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def order(self):
        n = len(self.dataset)
        if not self.shuffle:
            return np.arange(n, dtype=np.int64)
        gen = self.generator
        # torch.utils.data.DataLoader.__iter__ draws the workers' base seed first (_BaseDataLoaderIter.__init__), from the
        # loader's generator or the default one ...
        torch.empty((), dtype=torch.int64).random_(generator=gen)
        if gen is None:   # ... then RandomSampler.__iter__ seeds a generator of its own with one more draw
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            gen = torch.Generator()
            gen.manual_seed(seed)
        return torch.randperm(n, generator=gen).numpy()

    def __iter__(self):
        order, bs = self.order(), self.batch_size
        r, tr = self.mask_ratio, self.tuple_ratio
        if r == 0 and tr >= 1:
            for k in range(len(self)):
                yield self.dataset.batch(order[k * bs:(k + 1) * bs])
            return
        ds = self.dataset
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if r > 0 and self.mask_rng == "device" else None
        tseed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if tr < 1 and self.tuple_rng == "device" else None
        host_mask, host_tuples = r > 0 and seed is None, tr < 1 and tseed is None
        ext = None
        if host_tuples:
            from .dataloaders_AtomTuple import AtomTupleExtractor
            ext = AtomTupleExtractor(tr, ds.option)
        for k in range(len(self)):
            ids = order[k * bs:(k + 1) * bs]
            keep, tuples = None, None
            if host_mask or host_tuples:
                # the reference's own draws, molecule after molecule: the BFS of __getitem__, then the transform's
                # np.random.choice over the tuples of the atoms that are left
                keeps, tups, at = [], [], 0
                for i in ids:
                    n = int(ds.sizes[i])
                    if host_mask:
                        keeps.append(masking.reference_bfs(n, ds.successors(int(i)), r))
                    if r > 0:
                        n = int(masking.kept_count(n, r))
                    if host_tuples:
                        tups.append(ext._one(n).numpy() + at)
                    at += n
                if host_mask:
                    keep = np.concatenate(keeps).astype(np.int32)
                if host_tuples:
                    tuples = np.ascontiguousarray(np.concatenate(tups, axis=1).astype(np.int64))
            yield DatasetBatch(ds, ids, masking.MaskDraw(r, seed=seed, keep=keep) if r > 0 else None,
                               TupleDraw(tr, seed=tseed, tuples=tuples) if tr < 1 else None)
