"""Thin functional wrappers over the C ABI (one call = one or a few kernel launches on the current
stream).  Every function takes/returns CUDA tensors; nothing here computes on the host."""
import ctypes as C
import math
import os
import types

import numpy as np
import torch
from .switches import env as _env

from . import _lib
from ._lib import call, ptr, stream
from .layout import MolLayout, SPARSE_MAX_N, get_layout

PI_F32 = float(torch.tensor(math.pi, dtype=torch.float32))
# molecules of the (two-view) batch up to which ragged batches take the layer loop.  Same-box A/B on set B (trainer, one
# bucket graph), loop against separate launches: 128 molecules per view 0.865 -> 0.820 ms (+5.5 %), 256 1.18 -> 1.23 ms,
# 512 1.75 -> 2.06 ms: with one block per molecule an operation of the loop is a 9 us chain of dependent round trips
# (weights from L2, rows through L2 between operations) whatever the batch, and from 256 molecules per view on the
# separate launches fill the chip better.  (First form, every wave the unrolled walk of its molecule's size class: 0.839
# ms at 128 with 31 spilled registers; the block form above has none.)
RAGGED_LOOP_MAX_MOLS = int(_env("GEOSSL_RAGGED_LOOP_MAX", 256))


def _f32(t):
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    return t.contiguous()


def radius_cap(max_num_neighbors, loop=False):
    # torch_cluster.radius_graph searches max_num_neighbors (+1 when loop=False: the self hit) candidates
    return max_num_neighbors if loop else max_num_neighbors + 1


def _check_graph_size(layout):
    """The graph kernels keep a molecule's positions and bit matrix in LDS: 1024 atoms at most."""
    if layout.max_n > SPARSE_MAX_N:
        raise ValueError("the radius graph takes structures of at most %d atoms (the largest here has %d)"
                         % (SPARSE_MAX_N, layout.max_n))


def radius_graph(pos, r, batch=None, loop=False, max_num_neighbors=32, layout=None, return_weight=False):
    """torch_geometric.nn.radius_graph(pos, r, batch) as called at schnet.py:91 and
    datasets_3D_Radius.py:120 -> int64 [2, E] = [source j; target i], target-major, sources ascending."""
    _lib.require_cuda(pos)
    if loop:
        raise NotImplementedError("loop=True is not on the GeoSSL path")
    pos = _f32(pos)
    N = pos.size(0)
    if batch is None:
        batch = torch.zeros(N, dtype=torch.long, device=pos.device)
    lay = layout or get_layout(batch)
    _check_graph_size(lay)
    r2 = float(torch.tensor(float(r) * float(r), dtype=torch.float32))
    cap = radius_cap(max_num_neighbors)
    deg = torch.zeros(N, dtype=torch.int32, device=pos.device)
    call("geossl_radius_graph_count", ptr(pos), ptr(lay.mol_ptr), lay.B, lay.max_n, r2, cap, ptr(deg), stream())
    edge_ptr = torch.zeros(N + 1, dtype=torch.int64, device=pos.device)
    edge_ptr[1:] = torch.cumsum(deg, 0, dtype=torch.int64)
    E = int(edge_ptr[-1].item())
    edge_index = torch.empty(2, E, dtype=torch.int64, device=pos.device)
    weight = torch.empty(E, dtype=torch.float32, device=pos.device)
    if E > 0:
        call("geossl_radius_graph_fill", ptr(pos), ptr(lay.mol_ptr), lay.B, lay.max_n, r2, cap, ptr(edge_ptr),
             ptr(edge_index[0]), ptr(edge_index[1]), ptr(weight), stream())
    return (edge_index, weight) if return_weight else edge_index


def painn_incidence_layout(edge_index, mol_ptr, N, B, max_n, out=None, status=None, dyn_E=None, dyn_N=None):
    """Both incidence lists of a collated one-view ``radius_edge_index`` (what layout.EdgeLayout.inc holds) in one launch
    (geossl_painn_incidence_layout), structures of up to SPARSE_MAX_N atoms -> (iptr_i int64 [N + 1], ilist_i int32 [E],
    iptr_j, ilist_j, status int32 [1]).  `max_n`: the largest structure, a host integer.  `out` / `status`: buffers to
    write into (a bucket's, at capacity: `edge_index` then has E_cap columns and N is the atom capacity) with the real
    counts in device memory (`dyn_E`, `dyn_N`: int32 tensors).  No allocation with `out` and `status` given, no read-back:
    the status word (an edge that leaves its structure, a list not grouped by structure) is the caller's to read."""
    _lib.require_cuda(edge_index, mol_ptr)
    if edge_index.dtype != torch.long or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("radius_edge_index must be int64 [2, E]")
    if mol_ptr.dtype != torch.int32 or mol_ptr.numel() != B + 1:
        raise ValueError("mol_ptr must be int32 [B + 1]")
    if max_n > SPARSE_MAX_N:
        raise ValueError("the incidence lists take structures of at most %d atoms (the largest here has %d)"
                         % (SPARSE_MAX_N, max_n))
    if (dyn_E is None) != (dyn_N is None):
        raise ValueError("dyn_E and dyn_N come together")
    E, dev = int(edge_index.size(1)), edge_index.device
    r0, r1 = edge_index[0], edge_index[1]
    if not (r0.is_contiguous() and r1.is_contiguous()):
        raise ValueError("radius_edge_index must have contiguous rows")
    if out is None:
        out = (torch.empty(N + 1, dtype=torch.int64, device=dev), torch.empty(max(E, 1), dtype=torch.int32, device=dev),
               torch.empty(N + 1, dtype=torch.int64, device=dev), torch.empty(max(E, 1), dtype=torch.int32, device=dev))
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    iptr_i, ilist_i, iptr_j, ilist_j = out
    if iptr_i.numel() < N + 1 or iptr_j.numel() < N + 1 or ilist_i.numel() < E or ilist_j.numel() < E:
        raise ValueError("incidence buffers are smaller than (N + 1, E)")
    tail = (ptr(iptr_i), ptr(ilist_i), ptr(iptr_j), ptr(ilist_j), ptr(status))
    if dyn_E is not None:
        call("geossl_painn_incidence_layout_dyn", ptr(r0), ptr(r1), E, ptr(dyn_E), ptr(mol_ptr), N, B, max(int(max_n), 1),
             *tail, ptr(dyn_N), None, stream())
    else:
        call("geossl_painn_incidence_layout", ptr(r0), ptr(r1), E, ptr(mol_ptr), N, B, max(int(max_n), 1), *tail, None,
             stream())
    return iptr_i, ilist_i, iptr_j, ilist_j, status


def pair_geometry(pos, layout, cutoff, max_num_neighbors=32, mol_live=None):
    """Radius graph in pair-slot form: (pair_d [P], pair_c [P], pair_flag [P] u8).  mol_live (int32 [B], optional)
    receives the number of slots with an edge per molecule (what `live_pairs` starts from)."""
    if getattr(layout, "sparse", False):
        raise _lib.GeosslHipError("a sparse layout (a structure above 255 atoms, or GEOSSL_SPARSE_PAIRS=1) has no dense "
                                  "pair slots: ops.sparse_pair_geometry builds its pair list")
    _check_graph_size(layout)
    pos = _f32(pos)
    dev = pos.device
    P = layout.P
    pair_d = torch.empty(P, dtype=torch.float32, device=dev)
    pair_c = torch.empty(P, dtype=torch.float32, device=dev)
    pair_flag = torch.empty(P, dtype=torch.uint8, device=dev)
    r2 = float(torch.tensor(float(cutoff) * float(cutoff), dtype=torch.float32))
    if P > 0:
        if mol_live is not None:
            call("geossl_pair_geometry_live", ptr(pos), ptr(layout.mol_ptr), ptr(layout.pair_ptr), layout.B, layout.max_n,
                 r2, radius_cap(max_num_neighbors), float(cutoff), ptr(pair_d), ptr(pair_c), ptr(pair_flag),
                 ptr(mol_live), stream())
        else:
            call("geossl_pair_geometry", ptr(pos), ptr(layout.mol_ptr), ptr(layout.pair_ptr), layout.B, layout.max_n, r2,
                 radius_cap(max_num_neighbors), float(cutoff), ptr(pair_d), ptr(pair_c), ptr(pair_flag), stream())
    return pair_d, pair_c, pair_flag


def live_pairs_enabled():
    """GEOSSL_LIVE_PAIRS=0: the filter network runs on every pair slot of a dense layout, as before the live-pair list."""
    return _env("GEOSSL_LIVE_PAIRS", "1") != "0"


class LivePairs:
    """The pair slots of a dense layout that carry an edge, in slot order, packed back to back (csrc/sparse_pairs.hip:
    k_live_pairs): pair_d, pair_c, pair_flag, pair_i, pair_j of those rows, ``row_slot`` (the dense slot of each row) and
    ``n_live`` (int32 [1], device), the number of rows - never read back: the filter kernels take its address as their
    dyn_P.  Every array has the layout's P rows (a capacity); rows past n_live hold flag 0, pair_i = pair_j = 0,
    pair_c = 0, pair_d = cutoff, row_slot = 0."""

    __slots__ = ("P", "pair_d", "pair_c", "pair_flag", "pair_i", "pair_j", "row_slot", "n_live")

    @property
    def dyn_P(self):
        return self.n_live.data_ptr()


def live_pairs(pair_d, pair_c, pair_flag, layout, mol_live, cutoff, out=None):
    """(pair_d, pair_c, pair_flag) of `pair_geometry` called with mol_live -> LivePairs.  One launch, no read-back.  `out`:
    a LivePairs of an earlier call on the same layout whose buffers are written again."""
    P = layout.P
    dev = pair_d.device
    lp = out
    if lp is None:
        lp = LivePairs()
        lp.P = P
        i32 = dict(dtype=torch.int32, device=dev)
        lp.pair_d = torch.empty(max(P, 1), dtype=torch.float32, device=dev)
        lp.pair_c = torch.empty(max(P, 1), dtype=torch.float32, device=dev)
        lp.pair_flag = torch.empty(max(P, 1), dtype=torch.uint8, device=dev)
        lp.pair_i, lp.pair_j = torch.empty(max(P, 1), **i32), torch.empty(max(P, 1), **i32)
        lp.row_slot = torch.empty(max(P, 1), **i32)
        lp.n_live = torch.empty(1, **i32)
    elif lp.P != P:
        raise ValueError("the LivePairs given as `out` was made for another capacity")
    dyn = getattr(layout, "dyn", None)
    call("geossl_live_pairs_build", ptr(pair_d), ptr(pair_c), ptr(pair_flag), ptr(layout.pair_i), ptr(layout.pair_j),
         ptr(layout.mol_ptr), ptr(layout.pair_ptr), ptr(mol_live), layout.B, P, float(cutoff),
         dyn.n_pairs2 if dyn is not None else None, ptr(lp.pair_d), ptr(lp.pair_c), ptr(lp.pair_flag), ptr(lp.pair_i),
         ptr(lp.pair_j), ptr(lp.row_slot), ptr(lp.n_live), stream())
    return lp


class SparsePairs:
    """The radius graph of one forward as a compacted pair list (csrc/sparse_pairs.hip): pair_i, pair_j (int32 global
    atom ids, a < b, lexicographic per molecule in batch order), pair_d, pair_c, pair_flag as in the dense form, and the
    per-atom incidence lists inc_ptr [N + 1], inc_pair / inc_src [2 P] (atom t's pairs in ascending partner order: row,
    partner | edge partner -> t << 30 | edge t -> partner << 31).  ``P`` is the CAPACITY every array is sized by (from
    host sizes, layout.sparse_pair_capacity); ``n_pairs`` (int32 [1], device) the real number of rows, which nothing
    here reads back - the filter kernels take its address as their dyn_P.  Rows past it hold flag 0, pair_i = pair_j = 0,
    pair_c = 0, pair_d = cutoff.  ``dyn_N``: None, or - the list of a capacity bucket's layout, where ``N`` is a
    capacity too - the device address of the real atom count, which the aggregation's capacity launch reads."""

    __slots__ = ("P", "N", "pair_i", "pair_j", "pair_d", "pair_c", "pair_flag", "inc_ptr", "inc_pair", "inc_src",
                 "n_pairs", "dyn_N")

    @property
    def dyn_P(self):
        return self.n_pairs.data_ptr()


def sparse_pair_geometry(pos, layout, cutoff, max_num_neighbors=32):
    """Radius graph as a sparse pair list -> SparsePairs.  No device-to-host read.  A capacity bucket's layout (it
    carries ``dyn``): N, P and max_n are capacities, mol_ptr holds the real offsets and the real atom count is read on
    the device (geossl_sparse_pairs_build_dyn)."""
    if not getattr(layout, "sparse", False):
        raise _lib.GeosslHipError("sparse_pair_geometry needs a sparse layout (GEOSSL_SPARSE_PAIRS=1 makes any layout one)")
    _check_graph_size(layout)
    if radius_cap(max_num_neighbors) > 33:
        raise ValueError("the capacity of the sparse pair list is sized for max_num_neighbors <= 32")
    pos = _f32(pos)
    dev, N, P = pos.device, layout.N, layout.P
    i32 = dict(dtype=torch.int32, device=dev)
    sp = SparsePairs()
    sp.P, sp.N = P, N
    sp.pair_i, sp.pair_j = torch.empty(max(P, 1), **i32), torch.empty(max(P, 1), **i32)
    sp.pair_d = torch.empty(max(P, 1), dtype=torch.float32, device=dev)
    sp.pair_c = torch.empty(max(P, 1), dtype=torch.float32, device=dev)
    sp.pair_flag = torch.empty(max(P, 1), dtype=torch.uint8, device=dev)
    sp.inc_ptr = torch.empty(N + 1, **i32)
    sp.inc_pair, sp.inc_src = torch.empty(max(2 * P, 1), **i32), torch.empty(max(2 * P, 1), **i32)
    sp.n_pairs = torch.empty(1, **i32)
    work = torch.empty(layout.B + 2 * N, **i32)
    r2 = float(torch.tensor(float(cutoff) * float(cutoff), dtype=torch.float32))
    sp.dyn_N = _dyn(getattr(layout, "dyn", None), "n_atoms2")
    args = (ptr(pos), ptr(layout.mol_ptr), layout.B, N, layout.max_n, r2,
            radius_cap(max_num_neighbors), float(cutoff), P, ptr(work), ptr(work[layout.B:]), ptr(work[layout.B + N:]),
            ptr(sp.pair_i), ptr(sp.pair_j), ptr(sp.pair_d), ptr(sp.pair_c), ptr(sp.pair_flag), ptr(sp.inc_ptr),
            ptr(sp.inc_pair), ptr(sp.inc_src), ptr(sp.n_pairs))
    if sp.dyn_N is None:
        call("geossl_sparse_pairs_build", *args, stream())
    else:
        call("geossl_sparse_pairs_build_dyn", *args, sp.dyn_N, stream())
    return sp


def aggregate_sparse(x, Wf_l, pairs, swap=False, out=None):
    """Neighbour aggregation over a sparse pair list: x, out [N, F]; Wf_l [P, F] rows of the list.  swap: the transposed
    graph (the backward).  Bit-identical to `aggregate` on the same filter rows.  The list of a capacity bucket
    (``pairs.dyn_N``): rows at and past the real atom count are neither read nor written."""
    N, F = x.shape
    if out is None:
        out = torch.empty_like(x)
    args = (ptr(x), ptr(Wf_l), ptr(pairs.inc_ptr), ptr(pairs.inc_pair), ptr(pairs.inc_src), N, F, 1 if swap else 0,
            ptr(out))
    if pairs.dyn_N is None:
        call("geossl_cfconv_aggregate_sparse", *args, stream())
    else:
        call("geossl_cfconv_aggregate_sparse_dyn", *args, pairs.dyn_N, stream())
    return out


def pair_position_grad_sparse(pos, pairs, dd, out=None):
    """dd [L, P] (dL/d length per block and row, geossl_cfconv_filter_dpos) -> dpos [N, 3] through the incidence lists."""
    N = pos.size(0)
    if out is None:
        out = torch.empty(N, 3, dtype=torch.float32, device=pos.device)
    call("geossl_pair_position_grad_sparse", ptr(pos), ptr(pairs.pair_d), ptr(dd), ptr(pairs.inc_ptr), ptr(pairs.inc_pair),
         ptr(pairs.inc_src), N, pairs.P, dd.size(0), ptr(out), stream())
    return out


class PairGraph:
    """The radius graph of one SchNet forward, whichever of its three forms it has (`pair_graph` decides):
    ``slots``: the arrays addressed like Wf (pair_d, pair_c, pair_flag, pair_i, pair_j, dyn_P = device address of the
    real row count or None) - the dense pair slots, or the SparsePairs of a sparse layout.  The filter forward runs on
    them when it writes every row, filter_dpos always;
    ``rows``: the arrays the filter weight-gradient launch walks - the LivePairs (with ``row_slot`` and dyn_P = n_live)
    where a live-pair list was built, else ``slots`` itself;
    ``fwd_on_rows``: the filter forward runs on ``rows`` through the row map (T compact, Wf per slot), not on ``slots``;
    ``loop_flag``: the pair_flag the layer loop walks, None where it may not be used (dense layouts with pairs only);
    ``rbf_image``: the Gaussian fragments of the filter weight-gradient launch over ``rows`` (`rbf_fragments`), or None."""

    __slots__ = ("layout", "sparse", "slots", "rows", "fwd_on_rows", "loop_flag", "rbf_image")

    def T_for_rows(self, T):
        """T [L, P, F] as the forward stored it -> T at the rows of ``rows`` (regrouped if it was stored per slot)."""
        if T is None or self.rows is self.slots or self.fwd_on_rows:
            return T
        out = torch.empty_like(T)
        call("geossl_gather_live_rows", ptr(T), ptr(self.rows.row_slot), ptr(self.rows.n_live), T.size(1), T.size(0),
             T.size(2), ptr(out), stream())
        return out

    def aggregate(self, x, Wf_l, swap=False, out=None):
        if self.sparse:
            return aggregate_sparse(x, Wf_l, self.slots, swap=swap, out=out)
        return aggregate(x, Wf_l, self.slots.pair_flag, self.layout, swap=swap, out=out)

    def position_grad(self, pos, dd, out):
        """dd [L, P] (geossl_cfconv_filter_dpos on ``slots``) -> out [N, 3] (zeroed by the caller)."""
        if self.sparse:   # (rows past the list's real count are never looked at: no incidence entry names one)
            return pair_position_grad_sparse(pos, self.slots, dd, out=out)
        lay = self.layout
        call("geossl_pair_position_grad", ptr(pos), ptr(self.slots.pair_d), ptr(dd), ptr(lay.mol_ptr), ptr(lay.pair_ptr),
             lay.B, lay.P, dd.size(0), ptr(out), stream())
        return out


def rbf_fragments(rows, P, offset, coeff, out=None):
    """The Gaussian fragments of every 32-row tile of ``rows`` (a LivePairs, a SparsePairs or the dense slots; P = its
    capacity) as the filter weight-gradient kernel multiplies them (csrc/rbf_frag.h) -> uint8 [8 KB per tile].  One
    launch, sized by the capacity, every tile written; geossl_cfconv_filter_bwd_frag(_dyn) reads it."""
    nbytes = _lib.load().geossl_rbf_fragments_bytes(P)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=rows.pair_d.device)
    elif out.numel() != nbytes:
        raise ValueError("the image given as `out` was made for another capacity")
    call("geossl_rbf_fragments_dyn", ptr(rows.pair_d), P, offset.numel(), ptr(offset), float(coeff), ptr(out), rows.dyn_P,
         stream())
    return out


def pair_graph(pos, layout, cutoff, want_rows, want_pos, rbf=None):
    """-> PairGraph.  A SPARSE layout (a structure above 255 atoms, layout.want_sparse) gets the compacted list of the
    pairs that carry an edge: P is then the list's capacity and its real row count stays on the device (the sparse
    layout of a capacity bucket, bucket.SPARSE: the atom count is a capacity as well, read on the device).  A dense layout
    gets its pair slots, and - unless GEOSSL_LIVE_PAIRS=0 - the list of the slots that carry an edge (93 % of them in
    QM9-sized molecules at 5 A, fewer in extended ones; `live_pairs`, one launch) for the filter network to run on: with
    parameter gradients (want_rows) or without a position gradient (want_pos).  The position gradient reads T and Wf by
    one index, so with it the forward keeps the dense rows and the backward regroups T (`T_for_rows`): the filter
    weight gradients are then those of the path without it, bit for bit.
    ``rbf`` = (offset, coeff) of the model's Gaussian smearing: with want_rows the graph also gets the image of the
    Gaussian fragments over ``rows`` (`rbf_fragments`), built right behind the list it is made from - once per forward,
    for all layers of the weight-gradient launch."""
    g = PairGraph()
    g.layout, g.sparse = layout, bool(getattr(layout, "sparse", False))
    g.rbf_image = None
    dyn = getattr(layout, "dyn", None)
    want_image = rbf is not None and want_rows and layout.P > 0
    if g.sparse:
        g.slots = g.rows = sparse_pair_geometry(pos, layout, cutoff)
        g.fwd_on_rows, g.loop_flag = False, None
        if want_image:
            g.rbf_image = rbf_fragments(g.rows, layout.P, *rbf)
        return g
    use_live = layout.P > 0 and live_pairs_enabled() and (want_rows or not want_pos)
    mol_live = torch.empty(layout.B, dtype=torch.int32, device=pos.device) if use_live else None
    pair_d, pair_c, pair_flag = pair_geometry(pos, layout, cutoff, mol_live=mol_live)
    g.slots = g.rows = types.SimpleNamespace(pair_d=pair_d, pair_c=pair_c, pair_flag=pair_flag, pair_i=layout.pair_i,
                                             pair_j=layout.pair_j, dyn_P=_dyn(dyn, "n_pairs2"))
    if use_live:
        g.rows = live_pairs(pair_d, pair_c, pair_flag, layout, mol_live, cutoff)
    g.fwd_on_rows = use_live and not want_pos
    g.loop_flag = pair_flag if layout.P > 0 else None
    if want_image:
        g.rbf_image = rbf_fragments(g.rows, layout.P, *rbf)
    return g


class PaiNNRoute:
    """The interaction kernels of one PaiNN forward and of its backward (`painn_route` decides, once, in the forward):
    ``form``: "tile" - the atom-tile kernels (painn_tile.hip): ALL atoms in one launch per block and pass, no staged launch
    and no lists; "mma" - the matrix-pipe forward (painn_mma.hip), which stages the rows of a molecule of up to
    ``stage_f`` atoms in LDS, with the per-atom kernel over ``big_f`` (the atoms of the larger molecules: list, entries,
    device address of the real count) where there is such a list; "vector" - the molecule-staged vector forward;
    ``big_b``: the atoms of the molecules above the LDS rows of the molecule-staged backward - skipped there
    (``bwd_entry`` = ..._bwd_mol_skip) and covered by the per-atom kernel - or None (..._bwd_mol takes every molecule;
    always with "tile");
    ``mu_is_zero``: the first block's mu is NULL, not 3 N F zeros (and so is its gradient);
    ``keep_mu``: GEOSSL_PAINN_NO_MU_ZERO as the forward read it (the last block forms its mu', d mu' starts as zeros);
    ``call``: the node's `call` - its launches go the way of the node's other launches (whoever wraps painn.call sees them)."""

    __slots__ = ("form", "lay", "el", "N", "F", "R", "dN", "stage_f", "big_f", "big_b", "bwd_entry", "mu_is_zero", "keep_mu",
                 "call")

    def forward(self, q, mu, xc, geom, fw, fb, q2, mu2):
        """Block l, painn.py:54-64: (q, mu, xc) -> (q2, mu2) over geom = (dirv, fcut, phi); fw / fb: the block's 3F filter
        rows.  One block per molecule (the rows its edges read are staged in LDS once), or per atom tile (rows from L2; a
        sparse bucket: N is the atom capacity, the grid's, and atoms 0 .. *dN - 1 are real)."""
        el, lay, N, F, R, st, call = self.el, self.lay, self.N, self.F, self.R, stream(), self.call
        inc_ptr, inc_idx = el.inc["i"]
        dirv, fcut, phi = geom
        edge = (ptr(phi), ptr(fcut), ptr(dirv), ptr(fw), ptr(fb))
        head = (ptr(q), ptr(mu), ptr(xc), ptr(el.idx_j))
        if self.form == "tile":
            call("geossl_painn_interaction_fwd_tile", *head, ptr(inc_ptr), ptr(inc_idx), *edge, None, N, self.dN, F, R,
                 ptr(q2), ptr(mu2), st)
        elif self.form == "mma":   # LDS: 3.5 KB per atom + 3 KB
            row_edge, grp_atom, _, mol_grp = el.groups("i", lay.mol_ptr)
            call("geossl_painn_interaction_fwd_mma_dyn", *head, ptr(row_edge), ptr(grp_atom), ptr(mol_grp), *edge,
                 ptr(lay.mol_ptr), lay.B, self.stage_f, N, F, R, ptr(q2), ptr(mu2), ptr(getattr(el, "mol_grp_end", None)), st)
            big = self.big_f
            if big is not None and big[1] > 0:
                call("geossl_painn_interaction_fwd_atoms", *head, ptr(inc_ptr), ptr(inc_idx), *edge, ptr(big[0]), big[1],
                     big[2], F, R, ptr(q2), ptr(mu2), st)
        else:
            call("geossl_painn_interaction_fwd_mol", *head, ptr(inc_ptr), ptr(inc_idx), *edge, ptr(lay.mol_ptr), lay.B,
                 lay.max_n, N, F, R, ptr(q2), ptr(mu2), st)

    def workspace(self, device):
        """The scratch of the backward launches of this form."""
        lib = _lib.load()
        n = lib.geossl_painn_interaction_bwd_tile_workspace_floats(self.N, self.F, self.R) if self.form == "tile" else \
            lib.geossl_painn_interaction_bwd_mol_workspace_floats(self.N, self.lay.B, self.F, self.R)
        return torch.empty(max(int(n), 1), dtype=torch.float32, device=device)

    def backward(self, dq2, dmu2, mu, xc, geom, fw, fb, dxc, dmu_in, g_fw, g_fb, ws, acc):
        """Block l backwards: (dq2, dmu2) -> (dxc, dmu_in; NULL with mu) and the block's filter gradients (acc: added)."""
        el, lay, N, F, R, st, call = self.el, self.lay, self.N, self.F, self.R, stream(), self.call
        inc_ptr, inc_idx = el.inc["j"]
        dirv, fcut, phi = geom
        args = (ptr(dq2), ptr(dmu2), ptr(mu), ptr(xc), ptr(el.idx_i), ptr(inc_ptr), ptr(inc_idx), ptr(phi), ptr(fcut),
                ptr(dirv), ptr(fw), ptr(fb))
        outs = (ptr(dxc), ptr(dmu_in), ptr(g_fw), ptr(g_fb), ptr(ws))
        if self.form == "tile":   # (atom_list NULL: all atoms)
            call("geossl_painn_interaction_bwd_tile", *args, None, N, self.dN, F, R, *outs, acc, st)
            return
        call(self.bwd_entry, *args, ptr(lay.mol_ptr), lay.B, lay.max_n, N, F, R, *outs, acc, st)
        big = self.big_b
        if big is not None and big[1] > 0:
            call("geossl_painn_interaction_bwd_atoms", *args, ptr(big[0]), big[1], big[2], F, R, *outs, 1, st)


def painn_route(lay, el, N, F, R, mma, training, want_pos, call=call):
    """-> PaiNNRoute, from the layout, the library's limits and the switches (GEOSSL_PAINN_TILE, _MMA_CAP, _NO_SPLIT,
    _NO_MU_ZERO), all read here.  `mma`: the configuration has matrix-pipe kernels and GEOSSL_PAINN_VECTOR is not set.
    Tile: the switch decides (switches.painn_tile: by default only layouts with a structure above 255 atoms, which no staged
    kernel holds), the library says which shapes it serves; of the capacity buckets (``el.dyn``) the SPARSE one takes them
    (up to 1024 atoms, no group arrays or atom lists: no other kernel serves it), the dense ones keep their kernels.
    Otherwise the matrix-pipe forward where every molecule fits its LDS rows; with larger ones (Molecule3D with hydrogens)
    it keeps those that fit if layout.painn_stage_caps gives a forward cap and the layout an atom list (host-side sizes),
    else the vector forward serves the whole batch.  The backward splits likewise at its own cap.  mu is NULL where one
    forward kernel covers every atom, unless forces (the edge gradients read mu), a split backward or the switch keep it."""
    from .layout import painn_stage_caps
    from .switches import painn_tile
    lib = _lib.load()
    r = PaiNNRoute()
    dyn = getattr(el, "dyn", None)
    r.lay, r.el, r.N, r.F, r.R, r.dN, r.call = lay, el, N, F, R, _dyn(dyn, "n_atoms2"), call
    r.form, r.stage_f, r.big_f, r.big_b = "vector", lay.max_n, None, None
    bucket, sparse = dyn is not None, bool(getattr(lay, "sparse", False))
    if mma and (sparse if bucket else (el.E > 0 and painn_tile(lay.max_n))) and lib.geossl_painn_tile_ok(int(F), int(R)):
        r.form = "tile"
    elif bucket and sparse:
        raise _lib.GeosslHipError("a sparse capacity-bucket layout serves the atom-tile kernels only (F = 128, 8 / 16 / "
                                  "20 radial functions, without GEOSSL_PAINN_VECTOR)")
    else:
        cap_f, cap_b = painn_stage_caps(F, R)
        if mma and el.E > 0:
            if 0 < cap_f < lay.max_n:
                r.big_f = lay.big_atoms(cap_f)
            if r.big_f is not None:
                r.form, r.stage_f = "mma", cap_f
            elif lay.max_n <= int(lib.geossl_painn_stage_cap(0, F, R)):
                r.form = "mma"
        if training and 0 < cap_b < lay.max_n and F in (64, 128):
            r.big_b = lay.big_atoms(cap_b)
    r.bwd_entry = "geossl_painn_interaction_bwd_mol" if r.big_b is None else "geossl_painn_interaction_bwd_mol_skip"
    r.keep_mu = bool(_env("GEOSSL_PAINN_NO_MU_ZERO"))
    covered = r.form == "tile" or (r.form == "mma" and r.big_f is None and R in (8, 16, 20) and r.big_b is None)
    r.mu_is_zero = covered and not want_pos and not r.keep_mu
    return r


def gaussian_smearing(dist, offset, coeff):
    """GaussianSmearing.forward, schnet.py:205-207."""
    _lib.require_cuda(dist)
    d = _f32(dist).view(-1)
    out = torch.empty(d.numel(), offset.numel(), dtype=torch.float32, device=d.device)
    call("geossl_rbf_fwd", ptr(d), d.numel(), ptr(offset), offset.numel(), float(coeff), ptr(out), stream())
    return out


class PreparedWeight:
    """MFMA operand image of a Linear weight (geossl_linear_prepare): `image` is an int32 tensor; K / NO are the
    contraction and output widths of the product it was built for."""
    __slots__ = ("image", "K", "NO")

    def __init__(self, image, K, NO):
        self.image, self.K, self.NO = image, K, NO


def prepare_linear(weights, transB=True):
    """Convert Linear weights (all the same shape) to their operand images in one launch per GEOSSL_TN_MAX weights.
    transB as in `linear`.  Returns a list of PreparedWeight, or None when the shape has no prepared path."""
    w0 = weights[0]
    NO, K = (w0.size(0), w0.size(1)) if transB else (w0.size(1), w0.size(0))
    words = int(_lib.load().geossl_linear_image_words(K, NO))
    if words == 0:
        return None
    out = []
    for lo in range(0, len(weights), _lib.TN_MAX):
        chunk = weights[lo:lo + _lib.TN_MAX]
        images = torch.empty(len(chunk), words, dtype=torch.int32, device=w0.device)
        pb = _lib.PrepareBatch()
        for i, w in enumerate(chunk):
            assert w.shape == w0.shape and w.stride(1) == 1
            pb.W[i], pb.image[i] = ptr(w), ptr(images[i])
            pb.ldw[i] = 0 if w.is_contiguous() else w.stride(0)
        call("geossl_linear_prepare", C.byref(pb), len(chunk), K, NO, 1 if transB else 0, stream())
        out += [PreparedWeight(images[i], K, NO) for i in range(len(chunk))]
    return out


def linear(x, w, bias=None, res=None, tprev=None, transB=True, flags=0, out=None, K=None, NO=None):
    """Y = epi(X @ Bm); transB: w is torch layout [NO][K] (forward) else [K][NO] (dX = dY @ W).
    x / out may be column slices of wider row-major tensors (row stride = x.stride(0) / out.stride(0));
    K / NO default to the slice widths.  `w` may be a PreparedWeight (transB is then fixed by its image)."""
    R = x.size(0)
    prepared = isinstance(w, PreparedWeight)
    if prepared:
        K, NO = w.K, w.NO
    K = x.size(1) if K is None else K
    NO = (w.size(0) if transB else w.size(1)) if NO is None else NO
    if out is None:
        out = torch.empty(R, NO, dtype=torch.float32, device=x.device)
    if bias is not None:
        flags |= _lib.EPI_BIAS
    if res is not None:
        flags |= _lib.EPI_RESIDUAL
    if tprev is not None:
        flags |= _lib.EPI_MUL_DSSP
    assert x.stride(1) == 1 and out.stride(1) == 1
    for aux in (res, tprev):
        assert aux is None or (aux.stride(0) == out.stride(0) and aux.stride(1) == 1)
    if prepared:
        call("geossl_linear_prepared", ptr(x), x.stride(0), ptr(w.image), ptr(bias), ptr(res), ptr(tprev), ptr(out),
             out.stride(0), R, K, NO, flags, stream())
    else:
        call("geossl_linear", ptr(x), x.stride(0), ptr(w), ptr(bias), ptr(res), ptr(tprev), ptr(out), out.stride(0), R,
             K, NO, 1 if transB else 0, flags, stream())
    return out


def prepare_chain(weights, transB=True, both=False):
    """Operand images (geossl_chain_prepare) of square F x F Linear weights for `linear_chain`, one launch per
    GEOSSL_PREPARE_MAX images.  transB as in `linear`.  A weight may be a column block of a wider matrix (unit column
    stride, row stride a multiple of 4, 16-byte aligned): it is converted where it lies.  Returns a list of int32
    tensors, or None if F has no chain path; `both`: (forward images (transB=True), backward images (transB=False)) of
    every weight from the same launch."""
    w0 = weights[0]
    F = w0.size(0)
    words = int(_lib.load().geossl_chain_image_words(F)) if w0.size(1) == F else 0
    if words == 0:
        return (None, None) if both else None
    jobs = [(w, 1) for w in weights] + [(w, 2) for w in weights] if both else [(w, 0) for w in weights]
    out = []
    for lo in range(0, len(jobs), _lib.PREPARE_MAX):
        chunk = jobs[lo:lo + _lib.PREPARE_MAX]
        images = torch.empty(len(chunk), words, dtype=torch.int32, device=w0.device)
        pb = _lib.PrepareBatch()
        for i, (w, tb) in enumerate(chunk):
            assert w.shape == w0.shape and w.stride(1) == 1
            pb.W[i], pb.image[i] = ptr(w), ptr(images[i])
            pb.ldw[i] = 0 if w.is_contiguous() else w.stride(0)
            pb.tb[i] = tb
        call("geossl_chain_prepare", C.byref(pb), len(chunk), F, 1 if transB else 0, stream())
        out += [images[i] for i in range(len(chunk))]
    return (out[:len(weights)], out[len(weights):]) if both else out


def _dyn(layout_or_dyn, field):
    """Device address of a bucket's real count (bucket.DynDims), or None."""
    d = getattr(layout_or_dyn, "dyn", layout_or_dyn)
    return None if d is None else getattr(d, field)


def linear_chain(x, stages, dyn_rows=None):
    """Several F -> F Linear layers applied to the rows of x back to back in one launch (geossl_linear_chain).
    stages: list of dicts with `image` (from prepare_chain) and optional `bias`, `res`, `tprev`, `flags`, `store`,
    `same_input` (F = 128 only: the stage reads the input of the stage before it, not its result), `x` (F = 128 only:
    the stage reads its own input rows) with `add_prev` (and adds the result of the stage before it)
    (default True: the stage's result is written to a new [R, F] tensor).  F = 128 only: flags EPI_SILU (the stage
    stores its result as it is, hands silu of it to the next stage and writes that to `out_act` if given) and
    EPI_MUL_DSILU (tprev is a saved pre-activation: * silu'(tprev)); up to five stages.  Returns the list of stored
    results (None where store is False)."""
    R, F = x.shape  # (x may be a column slice: its row stride is passed)
    assert x.stride(1) == 1 and 1 <= len(stages) <= _lib.CHAIN_MAX
    ch = _lib.Chain()
    ch.nstage = len(stages)
    outs = []
    for s, sd in enumerate(stages):
        st = ch.st[s]
        o = sd.get("out")  # a preallocated [R, F] destination (e.g. a row slice of a larger tensor) ...
        if o is None and sd.get("store", True):  # ... or a new tensor, unless the stage is not stored at all
            o = torch.empty(R, F, dtype=torch.float32, device=x.device)
        # out / res / tprev of a stage share one row stride (they may be column slices of wider row-major tensors)
        rows_ = [a for a in (o, sd.get("res"), sd.get("tprev"), sd.get("out_act")) if a is not None]
        ld = rows_[0].stride(0) if rows_ else F
        for a in rows_:
            assert a.stride(0) == ld and a.stride(1) == 1 and a.size(0) == R and a.size(1) == F
        st.image, st.bias, st.res, st.tprev, st.out = (ptr(sd["image"]), ptr(sd.get("bias")), ptr(sd.get("res")),
                                                       ptr(sd.get("tprev")), ptr(o))
        st.out_act = ptr(sd.get("out_act"))
        st.ld, st.flags = ld, int(sd.get("flags", 0)) | (_lib.CHAIN_SAME_INPUT if sd.get("same_input") else 0)
        xin = sd.get("x")  # the stage's own input rows (F = 128): one of several F-wide passes over a wide input
        if xin is not None:
            assert s > 0 and xin.stride(1) == 1 and xin.size(0) == R and xin.size(1) == F
            st.xin, st.ldxin = ptr(xin), xin.stride(0)
            st.flags |= _lib.CHAIN_NEW_INPUT | (_lib.CHAIN_ADD_PREV if sd.get("add_prev") else 0)
        else:
            st.xin, st.ldxin = None, 0
        outs.append(o)
    # dyn_rows: device address of the real row count when R is a capacity (bucket.DynDims; F = 128 only)
    call("geossl_linear_chain_dyn", ptr(x), x.stride(0), C.byref(ch), R, F, dyn_rows, stream())
    return outs


# GeosslLoopOp as 64-bit words (include/geossl_hip.h; checked against the ctypes layout when the module is imported):
# word 0 = kind | swap << 32, 1 = X, 2 = Wf, 3 = out, 4 = chain.nstage, then 9 words per stage: image, bias, res, tprev,
# out, ld | flags << 32, xin, ldxin, out_act
_LOOP_WORDS, _LOOP_STAGE0, _LOOP_STAGE_WORDS = 50, 5, 9
assert C.sizeof(_lib.LoopOp) == 8 * _LOOP_WORDS and _lib.LoopOp.chain.offset == 32 and _lib.Chain.st.offset == 8 \
    and C.sizeof(_lib.ChainStage) == 8 * _LOOP_STAGE_WORDS and _lib.ChainStage.ld.offset == 40 \
    and _lib.ChainStage.out_act.offset == 64


def layer_loop(ops_list, layout, pair_flag, N, F, stagger=0):
    """The operations of `ops_list` - ("chain", x, stages) / ("agg", x, Wf_l, out, swap) - as ONE launch in which every
    block carries its own molecules through all of them (geossl_schnet_layer_loop).  Returns False when the shape has no
    such path (the caller then launches them one by one).  The operation list is written as plain 64-bit words (a
    field-by-field ctypes fill of 14 operations cost more host time than the 14 calls it replaces)."""
    plan, nblk = layout.loop_plan()
    # RAGGED molecules of a SMALL batch (the reference's batch sizes): every launch of the pass is then a 5 .. 9 us
    # latency and the loop removes 13 of the 14; blocks of one or two molecules found from mol_ptr on the device (a
    # capacity bucket's index structures are device data).  Beyond RAGGED_LOOP_MAX_MOLS the ragged loop loses to the
    # separate launches (a block owns its molecules for the whole pass: 650-670 us per pass against 470 us at 2 x 1024
    # molecules) and is not used.
    ragged = (plan is None and F == 128 and 1 < layout.max_n <= 33 and layout.B <= RAGGED_LOOP_MAX_MOLS
              and not _env("GEOSSL_NO_RAGGED_LOOP") and len(ops_list) <= _lib.LOOP_MAX_OPS)
    if not ragged and (plan is None or F != 128 or not layout.uniform or layout.max_n > 20
                       or len(ops_list) > _lib.LOOP_MAX_OPS):
        return False
    words = [0] * (_LOOP_WORDS * len(ops_list))
    dp = lambda t_: 0 if t_ is None else t_.data_ptr()
    for i, op in enumerate(ops_list):
        b = _LOOP_WORDS * i
        if op[0] == "chain":
            _, x, stages = op
            assert x.shape == (N, F) and x.is_contiguous() and len(stages) <= 3
            words[b + 1], words[b + 4] = x.data_ptr(), len(stages)
            for s, sd in enumerate(stages):
                w = b + _LOOP_STAGE0 + _LOOP_STAGE_WORDS * s
                o, r, tp = sd.get("out"), sd.get("res"), sd.get("tprev")
                for a in (o, r, tp):
                    assert a is None or (a.shape == (N, F) and a.is_contiguous())
                words[w], words[w + 1], words[w + 2], words[w + 3], words[w + 4] = (
                    sd["image"].data_ptr(), dp(sd.get("bias")), dp(r), dp(tp), dp(o))
                words[w + 5] = F | (int(sd.get("flags", 0)) << 32)
        else:
            _, x, Wf_l, out, swap = op
            words[b], words[b + 1], words[b + 2], words[b + 3] = 1 | ((1 if swap else 0) << 32), x.data_ptr(), \
                Wf_l.data_ptr(), out.data_ptr()
    arr = np.array(words, dtype=np.uint64)
    if ragged:
        call("geossl_schnet_layer_loop_ragged", arr.ctypes.data, len(ops_list), ptr(layout.mol_ptr), ptr(layout.pair_ptr),
             ptr(pair_flag), layout.B, 1 if layout.B <= 512 else 2, N, F, stream())
        return True
    call("geossl_schnet_layer_loop", arr.ctypes.data, len(ops_list), ptr(plan), nblk, ptr(layout.mol_ptr),
         ptr(layout.pair_ptr), ptr(pair_flag), layout.max_n, 1 if layout.uniform else 0, N, F, int(stagger), stream())
    return True


def launch_ops(ops_list, graph, dyn_rows=None):
    """The operations of `ops_list` (see layer_loop) as one launch each; the aggregations over `graph` (a PairGraph)."""
    for op in ops_list:
        if op[0] == "chain":
            linear_chain(op[1], op[2], dyn_rows=dyn_rows)
        else:
            graph.aggregate(op[1], op[2], swap=op[4], out=op[3])


def linear_wgrad(problems, R, M, N, accumulate=False, lda=None, ldb=None, ldw=None, dyn_rows=None):
    """Batched weight gradients.  problems: list of (A [R,M], B [R,N], dW [M,N], db [M] or None); lda/ldb/ldw are
    the row strides when A / B / dW are column slices of wider tensors."""
    dev = problems[0][0].device
    lda, ldb, ldw = lda or M, ldb or N, ldw or N
    for lo in range(0, len(problems), _lib.TN_MAX):
        chunk = problems[lo:lo + _lib.TN_MAX]
        tb = _lib.TnBatch()
        for i, (A, Bm, dW, db) in enumerate(chunk):
            tb.A[i], tb.B[i], tb.dW[i], tb.db[i] = ptr(A), ptr(Bm), ptr(dW), ptr(db)
        nfl = _lib.load().geossl_tn_workspace_floats(R, M, N, len(chunk))
        ws = torch.empty(nfl, dtype=torch.float32, device=dev)
        call("geossl_linear_wgrad_dyn", C.byref(tb), len(chunk), R, M, N, lda, ldb, ldw, ptr(ws), 1 if accumulate else 0,
             dyn_rows, stream())


def aggregate(x, Wf_l, pair_flag, layout, swap=False, out=None):
    """x, out: full [N, F] tensors (rows are addressed by global atom index)."""
    N, F = x.shape
    if out is None:
        out = torch.empty_like(x)
    work = getattr(layout, "agg_work", None)
    if work is not None and 32 < F <= 128:
        call("geossl_cfconv_aggregate_targets_dyn" if getattr(layout, "agg_targets", False)
             else "geossl_cfconv_aggregate_work_dyn", ptr(x), ptr(Wf_l), ptr(pair_flag), ptr(layout.mol_ptr),
             ptr(layout.pair_ptr), ptr(work), work.numel(), layout.max_n, F, 1 if swap else 0, ptr(out),
             _dyn(layout, "n_work"), stream())
        return out
    if getattr(layout, "dyn", None) is not None:
        raise _lib.GeosslHipError("a capacity-bucket layout needs the work-list aggregation (64 or 128 features)")
    call("geossl_cfconv_aggregate", ptr(x), ptr(Wf_l), ptr(pair_flag), ptr(layout.mol_ptr), ptr(layout.pair_ptr),
         ptr(layout.order), layout.B, layout.max_n, F, 1 if swap else 0, ptr(out), stream())
    return out


def pair_product(a, b, layout, pair_flag, swap=False):
    """d aggregate / d filter rows as a tensor [P, F]: f0 a[i] b[j] + f1 a[j] b[i] per pair slot."""
    N, F = a.shape
    out = torch.empty(layout.P, F, dtype=torch.float32, device=a.device)
    call("geossl_pair_product", ptr(a), ptr(b), ptr(layout.pair_i), ptr(layout.pair_j), ptr(pair_flag), layout.P, F,
         1 if swap else 0, ptr(out), stream())
    return out


def segment_reduce(h, layout, reduce):
    """torch_scatter.scatter(h, batch, dim=0, reduce) for a sorted batch (schnet.py:115)."""
    out = torch.empty(layout.B, h.size(1), dtype=torch.float32, device=h.device)
    call("geossl_segment_reduce_fwd", ptr(h), ptr(layout.mol_ptr), layout.B, h.size(1), 1 if reduce == "mean" else 0,
         ptr(out), stream())
    return out


def pair_distance(pos, sei0, sei1):
    """pretrain_GeoSSL.py:199-205 -> [S, 1]."""
    pos = _f32(pos)
    S = sei0.numel()
    out = torch.empty(S, 1, dtype=torch.float32, device=pos.device)
    call("geossl_pair_distance", ptr(pos), ptr(sei0), ptr(sei1), S, ptr(out), stream())
    return out


def ddm_views(pos, noise, sei0, sei1, z=None, dyn=None):
    """Both views of a DDM step in one launch (pretrain_GeoSSL.py:68-74,199-205): ([pos ; pos + noise] as one [2N, 3]
    tensor, super-edge lengths of the clean view [S, 1], of the perturbed view [S, 1]); with the atom types `z` [N]
    (any stride) also [z ; z]."""
    pos, noise = _f32(pos), _f32(noise)
    N, S = pos.size(0), sei0.numel()
    pos2 = torch.empty(2 * N, 3, dtype=torch.float32, device=pos.device)
    d01 = torch.empty(S, 1, dtype=torch.float32, device=pos.device)
    d02 = torch.empty(S, 1, dtype=torch.float32, device=pos.device)
    z2 = None
    if z is not None:
        assert z.dim() == 1 and z.dtype == torch.long and z.numel() == N
        z2 = torch.empty(2 * N, dtype=torch.long, device=pos.device)
    # dyn (bucket.DynDims): N and S are capacities, the real counts are read on the device; view 1 starts at row dims[N]
    call("geossl_ddm_views_dyn", ptr(pos), ptr(noise), ptr(sei0), ptr(sei1), N, S, ptr(pos2), ptr(d01), ptr(d02), ptr(z),
         z.stride(0) if z is not None and N > 0 else 1, ptr(z2), _dyn(dyn, "n_atoms"), _dyn(dyn, "n_super"), stream())
    return (pos2, d01, d02) if z is None else (pos2, d01, d02, z2)


def add_scaled(a, b, alpha=1.0):
    a, b = _f32(a), _f32(b)
    out = torch.empty_like(a)
    call("geossl_axpy", ptr(a), ptr(b), float(alpha), a.numel(), ptr(out), stream())
    return out


class _RowNormalize(torch.autograd.Function):
    """F.normalize(h, dim=-1) (pretrain_GeoSSL.py:193-195) on the HIP path."""

    @staticmethod
    def forward(ctx, h, eps):
        h = _f32(h)
        N, F = h.shape
        y = torch.empty_like(h)
        norm = torch.empty(N, dtype=torch.float32, device=h.device) if ctx.needs_input_grad[0] else None
        call("geossl_row_normalize_fwd", ptr(h), N, F, float(eps), ptr(y), ptr(norm), stream())
        ctx.save_for_backward(y, norm)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, g):
        y, norm = ctx.saved_tensors
        N, F = y.shape
        dh = torch.empty_like(y)
        call("geossl_row_normalize_bwd", ptr(g.contiguous()), ptr(y), ptr(norm), N, F, ctx.eps, ptr(dh), stream())
        return dh, None


def row_normalize(h, eps=1e-12):
    _lib.require_cuda(h)
    return _RowNormalize.apply(h, eps)


class _EnergyForceLoss(torch.autograd.Function):
    """finetune_md17.py:46-51 after the position gradient: pred_force = -dE/dpos and
    loss = c_E * criterion(pred_energy, actual_energy) + c_F * criterion(pred_force, actual_force), criterion = L1Loss
    (:236) or MSELoss, as one node on the element-wise / reduction kernels of csrc/tape.hip (fixed summation order)."""

    @staticmethod
    def forward(ctx, pred_energy, actual_energy, dE_dpos, actual_force, c_e, c_f, kind):
        from . import tape as tp
        pe, ae = _f32(pred_energy).reshape(1, -1), _f32(actual_energy).reshape(1, -1)
        gp, af = _f32(dE_dpos).reshape(1, -1), _f32(actual_force).reshape(1, -1)
        ne, nf = pe.size(1), gp.size(1)
        de = tp._raw_binary(tp.SUB, pe, tp.FULL, ae, tp.FULL, 1, ne)
        df = tp._raw_binary(tp.ADD, gp, tp.FULL, af, tp.FULL, 1, nf, -1.0)       # (-dE/dpos) - actual_force
        if kind == "l1":
            te, tf = tp._raw_unary(tp.ABS, de), tp._raw_unary(tp.ABS, df)
        else:
            te, tf = tp._raw_binary(tp.MUL, de, tp.FULL, de, tp.FULL, 1, ne), tp._raw_binary(tp.MUL, df, tp.FULL, df, tp.FULL, 1, nf)
        se = tp._raw_unary(tp.AFFINE, tp._raw_reduce(tp.ROW, te), c_e / max(ne, 1))
        sf = tp._raw_unary(tp.AFFINE, tp._raw_reduce(tp.ROW, tf), c_f / max(nf, 1))
        ctx.save_for_backward(de, df)
        ctx.meta = (c_e / max(ne, 1), c_f / max(nf, 1), kind, pred_energy.shape, dE_dpos.shape)
        return tp._raw_binary(tp.ADD, se, tp.FULL, sf, tp.FULL, 1, 1).view(())

    @staticmethod
    def backward(ctx, g):
        from . import tape as tp
        de, df = ctx.saved_tensors
        we, wf, kind, shape_e, shape_f = ctx.meta
        g = g.contiguous().view(1, 1)
        if kind == "l1":
            de, df, fe, ff = tp._raw_unary(tp.SIGN, de), tp._raw_unary(tp.SIGN, df), we, -wf
        else:
            fe, ff = 2.0 * we, -2.0 * wf
        d_pe = tp._raw_binary(tp.MUL, de, tp.FULL, g, tp.ROW, 1, de.size(1), fe) if ctx.needs_input_grad[0] else None
        d_gp = tp._raw_binary(tp.MUL, df, tp.FULL, g, tp.ROW, 1, df.size(1), ff) if ctx.needs_input_grad[2] else None
        return (None if d_pe is None else d_pe.view(shape_e), None, None if d_gp is None else d_gp.view(shape_f), None,
                None, None, None)


def energy_force_loss(pred_energy, actual_energy, dE_dpos, actual_force, energy_coeff=0.05, force_coeff=0.95, loss="l1"):
    """The training loss of finetune_md17.py:46-51 from the energies and the position gradient of their sum
    (``dE_dpos = grad(pred_energy, positions, ones, create_graph=True)[0]``; the force is its negative) - on the
    library's kernels, so that a train-on-forces step launches no ATen arithmetic (config.py:59-60 for the defaults)."""
    if loss not in ("l1", "mse"):
        raise ValueError("loss is 'l1' (finetune_md17.py:236) or 'mse'")
    _lib.require_cuda(pred_energy, actual_energy, dE_dpos, actual_force)
    # the kernels walk flat buffers of pred_energy.numel() / dE_dpos.numel() elements: a target of another size would be
    # read past its end (torch's L1Loss / MSELoss raise or broadcast here; broadcasting targets is not supported)
    if actual_energy.numel() != pred_energy.numel():
        raise ValueError("actual_energy has %d elements, pred_energy %d" % (actual_energy.numel(), pred_energy.numel()))
    if tuple(actual_force.shape) != tuple(dE_dpos.shape):
        raise ValueError("actual_force has shape %s, dE_dpos %s" % (tuple(actual_force.shape), tuple(dE_dpos.shape)))
    return _EnergyForceLoss.apply(pred_energy, actual_energy, dE_dpos, actual_force, float(energy_coeff),
                                  float(force_coeff), loss)


def two_views(pos, noise, z, dyn=None):
    """The positions and atom types of the two views of a contrastive step as one 2N-atom batch (pretrain_GeoSSL.py:68-74:
    [pos ; pos + noise], [z ; z]) in one launch - ddm_views without the super-edge lengths, which these objectives never
    read.  dyn (bucket.DynDims): N is a capacity, the real count is read on the device; view 1 starts at row dims[N]."""
    pos, noise = _f32(pos), _f32(noise)
    N = pos.size(0)
    assert z.dim() == 1 and z.dtype == torch.long and z.numel() == N
    pos2 = torch.empty(2 * N, 3, dtype=torch.float32, device=pos.device)
    z2 = torch.empty(2 * N, dtype=torch.long, device=pos.device)
    call("geossl_ddm_views_dyn", ptr(pos), ptr(noise), None, None, N, 0, ptr(pos2), None, None, ptr(z),
         z.stride(0) if N > 0 else 1, ptr(z2), _dyn(dyn, "n_atoms"), None, stream())
    return pos2, z2


def _pair_grads(X, Y, B, F):
    """dX / dY of a contrastive loss as the two halves of ONE [2B, F] buffer: when X and Y are the halves of a fused
    two-view readout (pretrain_GeoSSL.split_views) their split's backward joins them without a copy."""
    d = torch.empty(2 * B, F, dtype=torch.float32, device=X.device)
    return d[:B], d[B:]


class _InfoNCELoss(torch.autograd.Function):
    """(CE(X Y^T / T, arange B) + CE(Y X^T / T, arange B)) / 2 (pretrain_GeoSSL.py:141-176) on csrc/contrastive.hip:
    -> (loss fp32 scalar, counts int32 [2] = rows / columns whose first argmax is the diagonal)."""

    @staticmethod
    def forward(ctx, X, Y, inv_t):
        X, Y = _f32(X), _f32(Y)
        B, F = X.shape
        dev = X.device
        stats = torch.empty(5 * B, dtype=torch.float32, device=dev)
        amax = torch.empty(2 * B, dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        call("geossl_infonce_fwd", ptr(X), ptr(Y), B, F, float(inv_t), ptr(stats), ptr(amax), ptr(loss), ptr(counts),
             stream())
        ctx.save_for_backward(X, Y, stats, amax)
        ctx.inv_t = float(inv_t)
        ctx.mark_non_differentiable(counts)
        return loss, counts

    @staticmethod
    def backward(ctx, gout, _gcounts):
        X, Y, stats, amax = ctx.saved_tensors
        B, F = X.shape
        dX, dY = _pair_grads(X, Y, B, F)
        g = gout.to(torch.float32).contiguous()
        call("geossl_infonce_bwd", ptr(X), ptr(Y), ptr(stats), ptr(amax), B, F, ctx.inv_t, ptr(g), ptr(dX), ptr(dY),
             stream())
        return dX, dY, None


class _EBMNCELoss(torch.autograd.Function):
    """EBM-NCE (pretrain_GeoSSL.py:103-138) on csrc/contrastive.hip: the positive pair <x_i, y_i> and num_neg negatives
    <x_i, y_{(i+k) mod B}> through BCEWithLogitsLoss in fp64 -> (loss fp64 scalar, counts int32 [2] = {pos > 0, neg < 0})."""

    @staticmethod
    def forward(ctx, X, Y, num_neg):
        X, Y = _f32(X), _f32(Y)
        B, F = X.shape
        dev = X.device
        pred = torch.empty(B, num_neg + 1, dtype=torch.float32, device=dev)
        terms = torch.empty(B, dtype=torch.float64, device=dev)
        hits = torch.empty(2 * B, dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float64, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        call("geossl_ebm_nce_fwd", ptr(X), ptr(Y), B, F, int(num_neg), ptr(pred), ptr(terms), ptr(hits), ptr(loss),
             ptr(counts), stream())
        ctx.save_for_backward(X, Y, pred)
        ctx.num_neg = int(num_neg)
        ctx.mark_non_differentiable(counts)
        return loss, counts

    @staticmethod
    def backward(ctx, gout, _gcounts):
        X, Y, pred = ctx.saved_tensors
        B, F = X.shape
        dX, dY = _pair_grads(X, Y, B, F)
        g = gout.to(torch.float64).contiguous()
        call("geossl_ebm_nce_bwd", ptr(X), ptr(Y), ptr(pred), B, F, ctx.num_neg, ptr(g), ptr(dX), ptr(dY), stream())
        return dX, dY, None


def _check_pair(X, Y):
    _lib.require_cuda(X, Y)
    if X.dim() != 2 or X.shape != Y.shape or X.size(0) < 1:
        raise ValueError("X and Y are [B, F] readouts of the two views with B >= 1, got %s and %s"
                         % (tuple(X.shape), tuple(Y.shape)))


def infonce_loss(X, Y, T):
    """InfoNCE of two views' readouts (pretrain_GeoSSL.py:141-176, CE_criterion = nn.CrossEntropyLoss()) ->
    (loss, counts): counts [2] int32 on the device, the reference's acc = (counts[0] / B + counts[1] / B) / 2."""
    _check_pair(X, Y)
    return _InfoNCELoss.apply(X, Y, 1.0 / float(T))


def ebm_nce_loss(X, Y, num_neg=1):
    """EBM-NCE of two views' readouts (pretrain_GeoSSL.py:103-138, criterion = nn.BCEWithLogitsLoss()) ->
    (loss float64, counts): counts [2] int32 on the device, acc = (counts[0] + counts[1]) / (B (1 + num_neg))."""
    _check_pair(X, Y)
    num_neg = int(num_neg)
    if not 1 <= num_neg <= X.size(0):
        # (cycle_index(B, k) of examples/util.py:19-22 fails for k > B: the reference cannot run such a step either)
        raise ValueError("num_neg must lie in [1, B] (B = %d), got %d" % (X.size(0), num_neg))
    return _EBMNCELoss.apply(X, Y, num_neg)


def _param_grads(params, needs=None):
    """Where a head's backward writes its parameter gradients -> (direct, buffers), one buffer (or None) per parameter.
    direct: inside _lib.direct_grads() with dense fp32 .grad tensors the kernels ADD into .grad (accumulate = 1) and
    autograd gets None for the parameters; else the buffers are fresh and autograd gets them.
    needs None (distance, torsion, charge: one launch writes every gradient): direct when all parameters own such a
    .grad, and every parameter has a buffer.  needs = the parameters' slice of ctx.needs_input_grad (InfoGraph, property,
    pair): only the parameters that require a gradient decide, and only they get a buffer."""
    if needs is None:
        direct = _lib.direct_grads_enabled(params)
        return direct, [p.grad if direct else torch.empty_like(p) for p in params]
    live = [p for p in params if p.requires_grad]
    direct = bool(live) and _lib.direct_grads_enabled(live)
    if direct:
        return True, [p.grad if p.requires_grad else None for p in params]
    return False, [torch.empty_like(p, dtype=torch.float32) if n else None for p, n in zip(params, needs)]


def _cat_head_forward(ctx, name, dyn_field, h, W, b, sides, inputs, rows, dyn):
    """Forward of a head that is Linear(sides F, 1) on a concatenation of atom rows (csrc/head_common.h: distance,
    sides = 2; torsion, sides = 3): geossl_<name>_head_fwd_dyn on h, W, b, the head's own `inputs` and `rows` index rows
    -> (Wd, residual, loss, pred).  residual [rows] is what the backward needs of the loss (sgn, or pred - target)."""
    N, F = h.shape
    f32 = dict(dtype=torch.float32, device=h.device)
    Wd, bd = W.detach().contiguous().view(-1), b.detach().contiguous().view(-1)
    proj = torch.empty(max(N, 1), sides, **f32)
    pred, residual = torch.empty(rows, **f32), torch.empty(rows, **f32)
    ws = torch.empty(int(getattr(_lib.load(), "geossl_%s_head_fwd_workspace_floats" % name)(rows)), **f32)
    loss = torch.empty((), **f32)
    call("geossl_%s_head_fwd_dyn" % name, ptr(h), N, F, ptr(Wd), ptr(bd), *[ptr(t) for t in inputs], rows, ptr(proj),
         ptr(pred), ptr(residual), ptr(ws), ptr(loss), _dyn(dyn, "n_atoms"), _dyn(dyn, dyn_field), stream())
    ctx.params, ctx.dyn = (W, b), dyn
    ctx.mark_non_differentiable(pred)
    return Wd, residual, loss, pred


def _cat_head_backward(ctx, name, dyn_field, h, Wd, index_args, gout):
    """Backward of the same heads: geossl_<name>_head_bwd_dyn with the head's own `index_args` between W and gout ->
    the gradients of (h, W, b) followed by the six Nones of the other forward arguments."""
    N, F = h.shape
    direct, (dW, db) = _param_grads(ctx.params)
    dh = torch.empty_like(h)
    ws = torch.empty(int(getattr(_lib.load(), "geossl_%s_head_bwd_workspace_floats" % name)(N, F)), dtype=torch.float32,
                     device=h.device)
    g = gout.to(torch.float32).contiguous()
    call("geossl_%s_head_bwd_dyn" % name, ptr(h), N, F, ptr(Wd), *index_args, ptr(g), ptr(dh), ptr(dW), ptr(db), ptr(ws),
         1 if direct else 0, _dyn(ctx.dyn, "n_atoms"), _dyn(ctx.dyn, dyn_field), stream())
    return (dh,) + ((None, None) if direct else (dW, db)) + (None,) * 6


class _DistanceHead(torch.autograd.Function):
    """L1Loss(Linear(2F, 1)(cat(h_u, h_v)).squeeze(), |pos_u - pos_v|) (examples/pretrain_DistancePrediction.py:15-25,
    71-77) on csrc/distance_head.hip -> (loss fp32 scalar, pred [S]).  The backward returns dh through autograd; dW / db
    go through autograd too, or, inside _lib.direct_grads() with dense fp32 .grad buffers, are added into them."""

    @staticmethod
    def forward(ctx, h, W, b, positions, sei0, sei1, inc_ptr, inc_idx, dyn):
        h = _f32(h)
        Wd, sgn, loss, pred = _cat_head_forward(ctx, "distance", "n_super", h, W, b, 2, (_f32(positions), sei0, sei1),
                                                sei0.numel(), dyn)
        ctx.save_for_backward(h, Wd, sei0, sgn, inc_ptr, inc_idx)
        return loss, pred

    @staticmethod
    def backward(ctx, gout, _gpred):
        h, Wd, sei0, sgn, inc_ptr, inc_idx = ctx.saved_tensors
        return _cat_head_backward(ctx, "distance", "n_super", h, Wd,
                                  (ptr(sei0), sgn.numel(), ptr(sgn), ptr(inc_ptr), ptr(inc_idx)), gout)


def distance_head_width_ok(F):
    """The node-feature widths the fused distance head serves (a wave holds one row: F = 64 V, V = 1, 2, 4, 8)."""
    return bool(_lib.load().geossl_distance_head_width_ok(int(F)))


def distance_head(h, W, b, positions, super_edge_index, incidence, dyn=None):
    """The distance-prediction loss of pretrain_DistancePrediction.py:71-77 -> (loss, pred): h [N, F] node features,
    W [1, 2F] / b [1] the predictor's weight and bias, positions [N, 3] (no gradient), super_edge_index int64 [2, S],
    incidence = (inc_ptr int64 [N + 1], inc_idx int32 [2S]): every atom's super-edges (as u or v) in ascending order
    (layout.SuperEdgeLayout).  dyn (bucket.DynDims): N and S are capacities, the real counts are read on the device."""
    _lib.require_cuda(h, W, b, positions, super_edge_index)
    F = h.size(1)
    if h.dim() != 2 or W.numel() != 2 * F or b.numel() != 1 or not distance_head_width_ok(F):
        raise ValueError("distance_head: h [N, F] with F in (64, 128, 256, 512), W [1, 2F], b [1]; got %s, %s, %s"
                         % (tuple(h.shape), tuple(W.shape), tuple(b.shape)))
    if positions.requires_grad:
        raise ValueError("distance_head: the target distances carry no gradient (positions.requires_grad)")
    sei = super_edge_index
    inc_ptr, inc_idx = incidence
    return _DistanceHead.apply(h, W, b, positions, sei[0].contiguous(), sei[1].contiguous(), inc_ptr, inc_idx, dyn)


class _TorsionHead(torch.autograd.Function):
    """MSELoss(Linear(3F, 1)(cat(h_u, h_v, h_w)).squeeze(), super_edge_angle) (examples/pretrain_TorsionAnglePrediction.py:
    16-27, 73-78) on csrc/torsion_head.hip -> (loss fp32 scalar, pred [T]).  The backward returns dh through autograd;
    dW / db go through autograd too, or, inside _lib.direct_grads() with dense fp32 .grad buffers, are added into them."""

    @staticmethod
    def forward(ctx, h, W, b, tri0, tri1, tri2, angle, mol_ptr, dyn):
        h = _f32(h)
        Wd, res, loss, pred = _cat_head_forward(ctx, "torsion", "n_triples", h, W, b, 3, (tri0, tri1, tri2, angle),
                                                tri0.numel(), dyn)
        ctx.save_for_backward(h, Wd, tri0, tri1, tri2, res, mol_ptr)
        return loss, pred

    @staticmethod
    def backward(ctx, gout, _gpred):
        h, Wd, tri0, tri1, tri2, res, mol_ptr = ctx.saved_tensors
        return _cat_head_backward(ctx, "torsion", "n_triples", h, Wd,
                                  (ptr(tri0), ptr(tri1), ptr(tri2), res.numel(), ptr(res), ptr(mol_ptr),
                                   mol_ptr.numel() - 1), gout)


def torsion_head_width_ok(F):
    """The node-feature widths the fused angle head serves (a wave holds one row: F = 64 V, V = 1, 2, 4, 8)."""
    return bool(_lib.load().geossl_torsion_head_width_ok(int(F)))


def torsion_head(h, W, b, triples, angle, mol_ptr, dyn=None):
    """The angle-prediction loss of pretrain_TorsionAnglePrediction.py:73-78 -> (loss, pred): h [N, F] node features,
    W [1, 3F] / b [1] the predictor's weight and bias, triples int64 [3, T] (batch atom ids, grouped by molecule in batch
    order: collated AtomTripleExtractor output), angle float32 [T] the targets (no gradient), mol_ptr int32 [B + 1] the
    atom offsets of the molecules (layout.MolLayout.mol_ptr): the backward scans a molecule's run of triples per atom.
    dyn (bucket.DynDims): N and T are capacities, the real counts are read on the device."""
    _lib.require_cuda(h, W, b, triples, angle, mol_ptr)
    F = h.size(1)
    if h.dim() != 2 or W.numel() != 3 * F or b.numel() != 1 or not torsion_head_width_ok(F):
        raise ValueError("torsion_head: h [N, F] with F in (64, 128, 256, 512), W [1, 3F], b [1]; got %s, %s, %s"
                         % (tuple(h.shape), tuple(W.shape), tuple(b.shape)))
    if triples.dtype != torch.long or triples.dim() != 2 or triples.size(0) != 3:
        raise ValueError("torsion_head: triples must be int64 [3, T]")
    T = triples.size(1)
    if angle.dtype != torch.float32 or angle.numel() != T or angle.requires_grad:
        raise ValueError("torsion_head: angle is a float32 [T] target without a gradient")
    if mol_ptr.dtype != torch.int32 or mol_ptr.dim() != 1 or (h.size(0) > 0 and mol_ptr.numel() < 2):
        raise ValueError("torsion_head: mol_ptr is int32 [B + 1]")
    return _TorsionHead.apply(h, W, b, triples[0].contiguous(), triples[1].contiguous(), triples[2].contiguous(),
                              angle.contiguous().view(-1), mol_ptr.contiguous(), dyn)


def triple_angles(positions, super_edge_index):
    """The angle (radians, [0, pi]) at the MIDDLE atom of every triple (u, v, w) of super_edge_index int64 [3, T]:
    atan2(|a x b|, a . b) with a = pos_u - pos_v, b = pos_w - pos_v; 0 when a or b is zero -> float32 [T]
    (geossl_triple_angles).  This is THIS LIBRARY'S definition of ``super_edge_angle``, not the reference's: the reference
    tree does not contain the code that fills that attribute (MoleculeDataset3DTorsionAngle is missing), so nothing pins
    it; the training step takes the target from the batch and never computes it."""
    _lib.require_cuda(positions, super_edge_index)
    pos = _f32(positions)
    sei = super_edge_index
    if pos.dim() != 2 or pos.size(1) != 3 or sei.dtype != torch.long or sei.dim() != 2 or sei.size(0) != 3:
        raise ValueError("triple_angles: positions float32 [N, 3], super_edge_index int64 [3, T]")
    T = sei.size(1)
    out = torch.empty(T, dtype=torch.float32, device=pos.device)
    if T:
        call("geossl_triple_angles", ptr(pos), pos.size(0), ptr(sei[0].contiguous()), ptr(sei[1].contiguous()),
             ptr(sei[2].contiguous()), T, ptr(out), stream())
    return out


def charge_mask_count(N, ratio):
    """k of the Charge Prediction mask: Python's int(N * ratio), computed by the library (the device uses the same rule)."""
    return int(_lib.load().geossl_charge_mask_count(int(N), float(ratio)))


def charge_mask(x, ratio, C, seed=None, given=None, dyn=None):
    """The masked-atom draw of pretrain_ChargePrediction.py:62-66 on the device -> (idx int64 [K], labels int64 [K],
    k int32 [1]).  x: int64 [N, cols] atom features, column 0 overwritten in place with the token C - 1 on the masked
    rows.  seed (int64 [1] on the device, advanced by the launch): a device draw (Philox, ascending list); given (int64
    [>= k]): a host-drawn list used as it is.  dyn (bucket.DynDims): N is a capacity, the real count is read on the device
    (K = N then; the real k is k[0]); else K = int(N * ratio)."""
    _lib.require_cuda(x, seed, given)
    if x.dtype != torch.long or x.dim() != 2 or not x.is_contiguous():
        raise ValueError("charge_mask: x must be a contiguous int64 [N, cols] tensor")
    if (seed is None) == (given is None):
        raise ValueError("charge_mask: exactly one of seed / given")
    if not 0.0 <= float(ratio) <= 1.0:
        raise ValueError("charge_mask: ratio must lie in [0, 1]")
    N = x.size(0)
    K = N if dyn is not None else charge_mask_count(N, ratio)
    if given is not None and (given.dtype != torch.long or not given.is_contiguous() or given.numel() < K
                              and dyn is None):
        raise ValueError("charge_mask: given must be a contiguous int64 list of at least k entries")
    dev = x.device
    if given is not None and given.numel() == 0:   # (k = 0: a list with no entries still selects the host-list form)
        given = torch.zeros(1, dtype=torch.long, device=dev)
    idx = torch.empty(max(K, 1), dtype=torch.long, device=dev)
    labels = torch.empty(max(K, 1), dtype=torch.long, device=dev)
    k = torch.empty(1, dtype=torch.int32, device=dev)
    call("geossl_charge_mask_dyn", ptr(x), x.size(1), N, float(ratio), int(C), ptr(seed), ptr(given), ptr(idx),
         ptr(labels), ptr(k), _dyn(dyn, "n_atoms"), stream())
    return idx[:K], labels[:K], k


class _ChargeHead(torch.autograd.Function):
    """CrossEntropyLoss(Linear(F, C)(h[idx]), labels) (examples/pretrain_ChargePrediction.py:15-25,81) on
    csrc/charge_head.hip -> loss (fp32 scalar).  The backward returns dh [N, F] (zero off the masked rows) through
    autograd; dW / db go through autograd too, or, inside _lib.direct_grads() with dense fp32 .grad buffers, are added
    into them."""

    @staticmethod
    def forward(ctx, h, W, b, idx, labels, k, status, dyn):
        h = _f32(h)
        N, F = h.shape
        C = W.size(0)
        K = idx.numel()
        dev = h.device
        Wd, bd = W.detach().contiguous(), b.detach().contiguous()
        lib = _lib.load()
        prob = torch.empty(max(K, 1), C, dtype=torch.float32, device=dev)
        ws = torch.empty(int(lib.geossl_charge_head_fwd_workspace_floats(K)), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        call("geossl_charge_head_fwd_dyn", ptr(h), N, F, ptr(Wd), ptr(bd), C, ptr(idx), ptr(labels), K, ptr(k),
             ptr(prob), ptr(ws), ptr(loss), ptr(status), _dyn(dyn, "n_atoms"), stream())
        ctx.save_for_backward(h, Wd, idx, labels, k, prob)
        ctx.params, ctx.dyn = (W, b), dyn
        return loss

    @staticmethod
    def backward(ctx, gout):
        h, Wd, idx, labels, k, prob = ctx.saved_tensors
        N, F = h.shape
        C, K = Wd.size(0), idx.numel()
        direct, (dW, db) = _param_grads(ctx.params)
        dh = torch.empty_like(h)
        ws = torch.empty(max(int(_lib.load().geossl_charge_head_bwd_workspace_floats(K, F, C)), 1), dtype=torch.float32,
                         device=h.device)
        g = gout.to(torch.float32).contiguous()
        call("geossl_charge_head_bwd_dyn", ptr(h), N, F, ptr(Wd), C, ptr(idx), ptr(labels), K, ptr(k), ptr(prob),
             ptr(g), ptr(dh), ptr(dW), ptr(db), ptr(ws), 1 if direct else 0, _dyn(ctx.dyn, "n_atoms"), stream())
        if direct:
            dW = db = None
        return dh, dW, db, None, None, None, None, None


def charge_head_width_ok(F, C):
    """The widths the fused charge head serves: F = 64, 128, 256 or 512 (a wave holds one row) and 2 <= C <= 16."""
    return bool(_lib.load().geossl_charge_head_width_ok(int(F), int(C)))


def charge_head(h, W, b, idx, labels, k, status, dyn=None):
    """The Charge Prediction loss of pretrain_ChargePrediction.py:81 -> loss: h [N, F] node features, W [C, F] / b [C]
    the predictor's Linear, idx / labels int64 [K] the masked atoms and their original types with k (int32 [1] on the
    device) real rows (charge_mask), status: an int32 word that a row out of range flags (the backbone's
    _lib.StatusWord).  dyn (bucket.DynDims): N is a capacity, the real atom count is read on the device."""
    _lib.require_cuda(h, W, b, idx, labels, k, status)
    if (h.dim() != 2 or W.dim() != 2 or W.size(1) != h.size(1) or b.numel() != W.size(0)
            or not charge_head_width_ok(h.size(1), W.size(0))):
        raise ValueError("charge_head: h [N, F] with F in (64, 128, 256, 512), W [C, F] with 2 <= C <= 16, b [C]; "
                         "got %s, %s, %s" % (tuple(h.shape), tuple(W.shape), tuple(b.shape)))
    if idx.numel() != labels.numel() or idx.numel() > h.size(0):
        raise ValueError("charge_head: idx and labels hold the same K <= N rows")
    return _ChargeHead.apply(h, W, b, idx, labels, k, status, dyn)


INFOGRAPH_READOUTS = {"add": 0, "sum": 0, "mean": 1}


def _infograph_wgrad(s, dh, dW, accumulate):
    """dW = s^T dh (linear_wgrad: A = s [B, F], B = dh [B, F]); F = 256 as four 128-column blocks of one launch."""
    B, F = s.shape
    if F <= 128:
        linear_wgrad([(s, dh, dW, None)], B, F, F, accumulate=accumulate)
        return
    c = 128
    probs = [(s[:, i:i + c], dh[:, j:j + c], dW[i:i + c, j:j + c], None) for i in range(0, F, c) for j in range(0, F, c)]
    linear_wgrad(probs, B, c, c, accumulate=accumulate, lda=F, ldb=F, ldw=F)


class _InfoGraphHead(torch.autograd.Function):
    """The 3D InfoGraph loss (examples/pretrain_3DInfoGraph.py:56-76) on csrc/infograph_head.hip -> (loss fp32 scalar,
    counts int32 [2] = #(pos > 0), #(neg < 0)).  m None: the readout of x over `layout` is part of the head (readout "add" /
    "mean"); else m [B, F] is the caller's readout and gets its own gradient.  The backward returns dx (with the readout's
    backward in it) and dm through autograd; dW goes through autograd too, or, inside _lib.direct_grads() with a dense
    fp32 .grad, is added into it."""

    @staticmethod
    def forward(ctx, x, W, m, layout, readout, dyn):
        x = _f32(x)
        N, F = x.shape
        B = int(layout.B)
        dev = x.device
        Wd = W.detach().contiguous()
        mode = 2 if m is not None else INFOGRAPH_READOUTS[readout]
        md = _f32(m) if m is not None else None
        f32 = dict(dtype=torch.float32, device=dev)
        s, h = torch.empty(B, F, **f32), torch.empty(B, F, **f32)
        scores = torch.empty(2, N, **f32)
        ws = torch.empty(int(_lib.load().geossl_infograph_fwd_workspace_floats(B)), **f32)
        loss = torch.empty((), **f32)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        call("geossl_infograph_fwd_dyn", ptr(x), N, F, ptr(Wd), ptr(layout.mol_ptr), B, mode, ptr(md), ptr(s), ptr(h),
             ptr(scores), ptr(ws), ptr(loss), ptr(counts), _dyn(dyn, "n_atoms"), stream())
        ctx.save_for_backward(x, Wd, s, h, scores)
        ctx.lay, ctx.mode, ctx.dyn, ctx.W = layout, mode, dyn, W
        ctx.mark_non_differentiable(counts)
        ctx.set_materialize_grads(False)   # (no zero-filled gradient of the counts: the backward is kernels only)
        return loss, counts

    @staticmethod
    def backward(ctx, gout, _gcounts):
        if gout is None:
            return None, None, None, None, None, None
        x, Wd, s, h, scores = ctx.saved_tensors
        N, F = x.shape
        B = s.size(0)
        W = ctx.W
        dx = torch.empty_like(x)
        dm = torch.empty(B, F, dtype=torch.float32, device=x.device) if ctx.mode == 2 else None
        dh = torch.empty(B, F, dtype=torch.float32, device=x.device)
        g = gout.to(torch.float32).contiguous()
        call("geossl_infograph_bwd_dyn", ptr(x), N, F, ptr(Wd), ptr(ctx.lay.mol_ptr), B, ctx.mode, ptr(s), ptr(h),
             ptr(scores), ptr(g), ptr(dx), ptr(dm), ptr(dh), _dyn(ctx.dyn, "n_atoms"), stream())
        direct, (dW,) = _param_grads((W,), ctx.needs_input_grad[1:2])
        if dW is not None:
            _infograph_wgrad(s, dh, dW, direct)
        return dx, None if direct else dW, dm, None, None, None


def infograph_width_ok(F):
    """The widths the fused InfoGraph head serves: F = 64, 128 or 256."""
    return bool(_lib.load().geossl_infograph_width_ok(int(F)))


def _check_infograph(x, W, layout):
    _lib.require_cuda(x, W, layout.mol_ptr)
    if x.dim() != 2 or W.dim() != 2 or tuple(W.shape) != (x.size(1), x.size(1)) or not infograph_width_ok(x.size(1)):
        raise ValueError("infograph: node_repr [N, F] with F in (64, 128, 256) and W [F, F]; got %s, %s"
                         % (tuple(x.shape), tuple(W.shape)))
    if int(layout.B) < 1:
        raise ValueError("infograph: at least one molecule")


def infograph_head(h, W, layout, readout, dyn=None):
    """3D InfoGraph with the readout inside the head (pretrain_3DInfoGraph.py:56-76 after the backbone's
    return_latent=True call) -> (loss, counts): h [N, F] node features of atoms sorted by molecule, W [F, F] the
    Discriminator's weight, layout: the batch's MolLayout (mol_ptr, B), readout "mean" / "add" ("sum"), the backbone's.
    counts [2] int32 on the device: acc = (counts[0] + counts[1]) / (2 N).  dyn (bucket.DynDims): N is a capacity, the
    real atom count is read on the device."""
    _check_infograph(h, W, layout)
    if readout not in INFOGRAPH_READOUTS:
        raise ValueError("infograph_head: readout is 'mean', 'add' or 'sum', got %r" % (readout,))
    return _InfoGraphHead.apply(h, W, None, layout, readout, dyn)


def infograph_loss(node_repr, molecule_repr, W, layout):
    """3D InfoGraph on a readout the caller brings (do_InfoGraph's arguments) -> (loss, counts); the gradient reaches
    node_repr and molecule_repr [B, F] both."""
    _check_infograph(node_repr, W, layout)
    _lib.require_cuda(molecule_repr)
    if molecule_repr.dim() != 2 or tuple(molecule_repr.shape) != (int(layout.B), node_repr.size(1)):
        raise ValueError("infograph_loss: molecule_repr [B, F] with B = %d, got %s"
                         % (int(layout.B), tuple(molecule_repr.shape)))
    return _InfoGraphHead.apply(node_repr, W, molecule_repr, layout, None, None)


PROPERTY_READOUTS = {"add": 0, "sum": 0, "mean": 1}
PROPERTY_LOSSES = {"mae": 0, "mse": 1}


def _property_w1_grad(dz, m, dW1, db1, accumulate):
    """dW1 = dz^T m, db1 = column sums of dz (linear_wgrad: A = dz [B, F/2], B = m [B, F]); F = 256 as two 128-column
    problems of one launch."""
    B, K = dz.shape
    F = m.size(1)
    if F <= 128:
        linear_wgrad([(dz, m, dW1, db1)], B, K, F, accumulate=accumulate)
        return
    c = 128
    probs = [(dz, m[:, j:j + c], dW1[:, j:j + c], db1 if j == 0 else None) for j in range(0, F, c)]
    linear_wgrad(probs, B, K, c, accumulate=accumulate, lda=K, ldb=F, ldw=F)


class _PropertyHead(torch.autograd.Function):
    """The Supervised step after the backbone (pretrain_Supervised.py:89-101) on csrc/property_head.hip -> (loss fp32
    scalar, pred [B] fp32, non-differentiable).  params: (w, b) of Linear(F, 1), or (W1, b1, w2, b2) of the default
    create_output_layers().  The backward returns dh (the readout's backward in it) and the head's gradients through
    autograd, or, inside _lib.direct_grads() with dense fp32 .grad tensors, adds the head's gradients into them."""

    @staticmethod
    def forward(ctx, h, y, stats, layout, readout, loss_kind, dyn, *params):
        h = _f32(h)
        N, F = h.shape
        B = int(layout.B)
        dev = h.device
        mlp = len(params) == 4
        ps = [p.detach().contiguous() for p in params]
        W1, b1 = ps[0], ps[1]
        W2, b2 = (ps[2], ps[3]) if mlp else (None, None)
        f32 = dict(dtype=torch.float32, device=dev)
        m = torch.empty(B, F, **f32)
        z = torch.empty(B, F // 2, **f32) if mlp else None
        pred = torch.empty(B, **f32)
        ws = torch.empty(int(_lib.load().geossl_property_workspace_floats(B)), **f32)
        loss = torch.empty((), **f32)
        call("geossl_property_fwd_dyn", ptr(h), N, F, ptr(layout.mol_ptr), B, PROPERTY_READOUTS[readout],
             1 if mlp else 0, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(y), y.stride(0), ptr(stats),
             PROPERTY_LOSSES[loss_kind], ptr(m), ptr(z), ptr(pred), ptr(ws), ptr(loss), _dyn(dyn, "n_atoms"), stream())
        ctx.save_for_backward(m, z, pred, y, stats, W1, W2)
        ctx.lay, ctx.readout, ctx.loss_kind, ctx.dyn, ctx.params, ctx.N = layout, readout, loss_kind, dyn, params, N
        ctx.mark_non_differentiable(pred)
        ctx.set_materialize_grads(False)
        return loss, pred

    @staticmethod
    def backward(ctx, gout, _gpred):
        params = ctx.params
        none = (None,) * (7 + len(params))
        if gout is None:
            return none
        m, z, pred, y, stats, W1, W2 = ctx.saved_tensors
        B, F = m.shape
        mlp = len(params) == 4
        dev = m.device
        dh = torch.empty(ctx.N, F, dtype=torch.float32, device=dev)
        dz = torch.empty(B, F // 2, dtype=torch.float32, device=dev) if mlp else None
        ws = torch.empty(int(_lib.load().geossl_property_workspace_floats(B)), dtype=torch.float32, device=dev)
        g = gout.to(torch.float32).contiguous()
        direct, grads = _param_grads(params, ctx.needs_input_grad[7:])
        # the vector gradients of the launch: (w, b) of head 0, (w2, b2) of head 1
        vw, vb = (grads[2], grads[3]) if mlp else (grads[0], grads[1])
        call("geossl_property_bwd_dyn", ctx.N, F, ptr(ctx.lay.mol_ptr), B, PROPERTY_READOUTS[ctx.readout],
             1 if mlp else 0, ptr(W1), ptr(W2), ptr(m), ptr(z), ptr(pred), ptr(y), y.stride(0), ptr(stats),
             PROPERTY_LOSSES[ctx.loss_kind], ptr(g), ptr(dh), ptr(dz), ptr(vw), ptr(vb), ptr(ws), 1 if direct else 0,
             _dyn(ctx.dyn, "n_atoms"), stream())
        if mlp and (grads[0] is not None or grads[1] is not None):
            dW1 = grads[0] if grads[0] is not None else torch.empty_like(W1)
            _property_w1_grad(dz, m, dW1, grads[1], direct)
        if direct:
            grads = [None] * len(params)
        return (dh, None, None, None, None, None, None) + tuple(grads)


def property_width_ok(F):
    """The widths the fused property head serves: F = 64, 128 or 256."""
    return bool(_lib.load().geossl_property_width_ok(int(F)))


def _check_property(h, layout, readout, params):
    _lib.require_cuda(h, layout.mol_ptr, *params)
    F = h.size(1) if h.dim() == 2 else -1
    if h.dim() != 2 or not property_width_ok(F):
        raise ValueError("property head: h [N, F] with F in (64, 128, 256), got %s" % (tuple(h.shape),))
    shapes = [tuple(p.shape) for p in params]
    if shapes not in ([(1, F), (1,)], [(F // 2, F), (F // 2,), (1, F // 2), (1,)]):
        raise ValueError("property head: Linear(F, 1) or Dense(F, F/2) + Dense(F/2, 1) parameters, got %s" % (shapes,))
    if readout not in PROPERTY_READOUTS:
        raise ValueError("property head: readout is 'mean', 'add' or 'sum', got %r" % (readout,))
    if int(layout.B) < 1:
        raise ValueError("property head: at least one molecule")


def _property_stats(stats, device):
    if not torch.is_tensor(stats):
        stats = torch.tensor([float(stats[0]), float(stats[1])], dtype=torch.float32).to(device)
    if stats.dtype != torch.float32 or stats.numel() != 2 or not stats.is_cuda or not stats.is_contiguous():
        raise ValueError("property head: stats is (mean, std), or a float32 [2] device tensor")
    return stats


def property_head(h, params, layout, readout, y, stats, loss="mae", dyn=None):
    """The Supervised loss with the readout inside the head -> (loss, pred): h [N, F] per-atom latent of atoms sorted by
    molecule (the backbone's latent_only output), params (w, b) of Linear(F, 1) or (W1, b1, w2, b2) of PaiNN's default
    create_output_layers(), layout: the batch's MolLayout, readout "mean" / "add" ("sum"), y [B] the target column (any
    stride), stats (mean, std) - a float32 [2] device tensor is read at launch time, so a replayed graph sees new values;
    loss "mae" (L1) or "mse".  pred [B] is the normalised prediction.  dyn (bucket.DynDims): N is a capacity, the real
    atom count is read on the device."""
    _check_property(h, layout, readout, params)
    if loss not in PROPERTY_LOSSES:
        raise ValueError("property head: loss is 'mae' or 'mse', got %r" % (loss,))
    B = int(layout.B)
    _lib.require_cuda(y)
    if y.dim() != 1 or y.numel() != B or y.dtype != torch.float32 or y.stride(0) < 1:
        raise ValueError("property head: y is a float32 [B] column, B = %d, got %s" % (B, tuple(y.shape)))
    stats = _property_stats(stats, h.device)
    return _PropertyHead.apply(h, y, stats, layout, readout, loss, dyn, *params)


def property_predict(h, params, layout, readout, stats, dyn=None):
    """eval() of finetune_qm9.py:290-374 after the backbone: pred * std + mean [B] (no autograd)."""
    _check_property(h, layout, readout, params)
    stats = _property_stats(stats, h.device)
    h = _f32(h.detach())
    N, F = h.shape
    B = int(layout.B)
    ps = [p.detach().contiguous() for p in params]
    mlp = len(ps) == 4
    pred = torch.empty(B, dtype=torch.float32, device=h.device)
    call("geossl_property_predict_dyn", ptr(h), N, F, ptr(layout.mol_ptr), B, PROPERTY_READOUTS[readout], 1 if mlp else 0,
         ptr(ps[0]), ptr(ps[1]), ptr(ps[2] if mlp else None), ptr(ps[3] if mlp else None), ptr(stats), ptr(pred),
         _dyn(dyn, "n_atoms"), stream())
    return pred


def property_targets(y, task_id, mol_off, src_off, B, out):
    """out [B] = y[m, task_id] of the dataset molecules whose first atoms are src_off [B] (int32, device): y [M, T]
    float32, mol_off [M + 1] int64 on the device."""
    call("geossl_property_targets", ptr(y), y.size(0), y.size(1), int(task_id), ptr(mol_off), src_off, int(B), ptr(out),
         stream())
    return out


# ---- MD17 evaluation (csrc/force_head.hip) ------------------------------------------------------------------------------
def energy_head(h, params, layout, readout):
    """finetune_md17.py:94-97 after the backbone with the seed of :99's position gradient -> (energy [B], seed [N, F] =
    d(sum of the energies) / dh), no autograd: h [N, F] the per-atom latent, params (w, b) of Linear(F, 1) or (W1, b1, w2,
    b2) of PaiNN's default create_output_layers(), layout the batch's MolLayout, readout "mean" / "add" ("sum")."""
    _check_property(h, layout, readout, params)
    h = _f32(h.detach())
    N, F = h.shape
    B = int(layout.B)
    if int(layout.N) != N:
        raise ValueError("energy head: the layout has %d atoms, h %d rows" % (int(layout.N), N))
    ps = [p.detach().contiguous() for p in params]
    mlp = len(ps) == 4
    energy = torch.empty(B, dtype=torch.float32, device=h.device)
    seed = torch.empty(N, F, dtype=torch.float32, device=h.device)
    call("geossl_energy_head_fwd", ptr(h), N, F, ptr(layout.mol_ptr), B, PROPERTY_READOUTS[readout], 1 if mlp else 0,
         ptr(ps[0]), ptr(ps[1]), ptr(ps[2] if mlp else None), ptr(ps[3] if mlp else None), ptr(energy), ptr(seed),
         stream())
    return energy, seed


def force_metrics_buffer(device):
    """The zeroed accumulator of force_metrics_accumulate: int64 [4] holding (two fp64 sums, two int64 counts)."""
    return torch.zeros(4, dtype=torch.int64, device=device)


def force_metrics_accumulate(pred_energy, y, dE_dpos, force_target, acc):
    """Adds one batch of finetune_md17.py:116-117's absolute errors onto `acc` (force_metrics_buffer): pred_energy, y [B];
    dE_dpos (the predicted force is its negative), force_target [N, 3].  Elements whose dE_dpos is NaN are skipped on
    both sides (:104-107).  No sync; read `acc` once with force_metrics_read."""
    _lib.require_cuda(pred_energy, y, dE_dpos, force_target, acc)
    pe, yy = _f32(pred_energy.detach()).reshape(-1), _f32(y.detach()).reshape(-1)
    g, ft = _f32(dE_dpos.detach()), _f32(force_target.detach())
    if yy.numel() != pe.numel():
        raise ValueError("y has %d elements, pred_energy %d" % (yy.numel(), pe.numel()))
    if g.dim() != 2 or g.size(1) != 3 or tuple(ft.shape) != tuple(g.shape):
        raise ValueError("dE_dpos and force_target are [N, 3], got %s and %s" % (tuple(g.shape), tuple(ft.shape)))
    if acc.dtype != torch.int64 or acc.numel() != 4 or not acc.is_contiguous():
        raise ValueError("acc is the int64 [4] buffer of force_metrics_buffer")
    call("geossl_force_metrics_accumulate", ptr(pe), ptr(yy), pe.numel(), ptr(g), ptr(ft), g.size(0), ptr(acc), stream())
    return acc


def force_metrics_read(acc):
    """The one device read of an evaluation -> (sum |dE|, sum |dF|, energies counted, force elements counted)."""
    host = acc.cpu()
    sums = host[:2].view(torch.float64)
    return float(sums[0]), float(sums[1]), int(host[2]), int(host[3])


def gather_atom_rows(src, src_off, mol_ptr, B, N, out=None):
    """Rows of the per-atom array src [Ntot, C] float32 of B molecules into batch order -> [N, C]: src_off (int32 [B],
    a device address or tensor) the molecules' first rows in src, mol_ptr (int32 [B + 1]) their offsets in the batch.
    out: a contiguous float32 [N, C] tensor to write (a graph's static input)."""
    _lib.require_cuda(src, out)
    if src.dtype != torch.float32 or src.dim() != 2 or not src.is_contiguous():
        raise ValueError("src is a contiguous float32 [Ntot, C] tensor")
    if out is None:
        out = torch.empty(int(N), src.size(1), dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (int(N), src.size(1)) or not out.is_contiguous():
        raise ValueError("out is a contiguous float32 [%d, %d] tensor" % (int(N), src.size(1)))
    a = lambda v: ptr(v) if torch.is_tensor(v) else v
    call("geossl_gather_atom_rows", ptr(src), src.size(0), src.size(1), a(src_off), a(mol_ptr), int(B), int(N), ptr(out),
         stream())
    return out


# ---- evaluation passes (csrc/eval_collect.hip) --------------------------------------------------------------------------
EVAL_KINDS = {"regression": 0, "bce": 1}


def eval_buffer(device):
    """The zeroed accumulator of eval_collect: int64 [4] holding (fp64 sum a, fp64 sum s, int64 rows, one unused word)."""
    return torch.zeros(4, dtype=torch.int64, device=device)


def eval_collect(pred, target, kind, offset, out_pred, out_true, acc):
    """One batch of an evaluation pass onto `acc` (eval_buffer) and into the result arrays: pred, target float32 [B];
    kind "regression" / 0 (a = |pred - target|, s = (pred - target)^2) or "bce" / 1 (a = the BCE-with-logits term of the
    logit pred and the label target, s = 0); out_pred / out_true: float32 [M] arrays whose rows [offset, offset + B)
    are written, or None (the sums alone).  No sync; read `acc` once with eval_read."""
    kind = EVAL_KINDS.get(kind, kind)
    if kind not in (0, 1):
        raise ValueError("eval_collect: kind is 'regression' (0) or 'bce' (1), got %r" % (kind,))
    _lib.require_cuda(pred, target, out_pred, out_true, acc)
    p, t = _f32(pred.detach()).reshape(-1), _f32(target.detach()).reshape(-1)
    B, offset = p.numel(), int(offset)
    if t.numel() != B:
        raise ValueError("eval_collect: target has %d elements, pred %d" % (t.numel(), B))
    if acc.dtype != torch.int64 or acc.numel() != 4 or not acc.is_contiguous():
        raise ValueError("eval_collect: acc is the int64 [4] buffer of eval_buffer")
    for o in (out_pred, out_true):
        if o is not None and (o.dtype != torch.float32 or o.dim() != 1 or not o.is_contiguous() or offset < 0
                              or offset + B > o.numel()):
            raise ValueError("eval_collect: a result array is a contiguous float32 [M] with offset + B <= M "
                             "(offset %d, B %d)" % (offset, B))
    call("geossl_eval_collect", ptr(p), ptr(t), B, kind, offset, ptr(out_pred), ptr(out_true), ptr(acc), stream())
    return acc


def eval_read(acc):
    """The one small device read of an evaluation pass -> (sum a, sum s, rows)."""
    host = acc.cpu()
    sums = host[:2].view(torch.float64)
    return float(sums[0]), float(sums[1]), int(host[2])


# ---- LEP pair head (csrc/pair_head.hip) ---------------------------------------------------------------------------------
class _PairHead(torch.autograd.Function):
    """The LEP step after the backbone (finetune_lep.py:40-45) on csrc/pair_head.hip -> (loss fp32 scalar, z [B] fp32
    logits, non-differentiable).  h is the latent of the 2B-structure batch [active | inactive], (w, b) the parameters
    of Linear(2F, 1).  The backward returns dh (the readout's backward in it) and the head's gradients through autograd,
    or, inside _lib.direct_grads() with dense fp32 .grad tensors, adds the head's gradients into them.  dyn
    (bucket.DynDims, or None): the rows of h are a capacity - the `_dyn` entry points, which are the exact ones with the
    real atom count read on the device."""

    @staticmethod
    def forward(ctx, h, y, layout, readout, dyn, w, b):
        h = _f32(h)
        N, F = h.shape
        B = int(layout.B) // 2
        f32 = dict(dtype=torch.float32, device=h.device)
        wd, bd = w.detach().contiguous(), b.detach().contiguous()
        m = torch.empty(2 * B, F, **f32)
        z = torch.empty(B, **f32)
        ws = torch.empty(int(_lib.load().geossl_pair_head_workspace_floats(B)), **f32)
        loss = torch.empty((), **f32)
        call("geossl_pair_head_fwd_dyn", ptr(h), N, F, ptr(layout.mol_ptr), B, PROPERTY_READOUTS[readout], ptr(wd),
             ptr(bd), ptr(y), ptr(m), ptr(z), ptr(ws), ptr(loss), _dyn(dyn, "n_atoms"), stream())
        ctx.save_for_backward(m, z, y, wd)
        ctx.lay, ctx.readout, ctx.params, ctx.N, ctx.dyn = layout, readout, (w, b), N, dyn
        ctx.mark_non_differentiable(z)
        ctx.set_materialize_grads(False)
        return loss, z

    @staticmethod
    def backward(ctx, gout, _gz):
        if gout is None:
            return (None,) * 7
        m, z, y, wd = ctx.saved_tensors
        F = m.size(1)
        B = z.numel()
        dev = m.device
        dh = torch.empty(ctx.N, F, dtype=torch.float32, device=dev)
        ws = torch.empty(int(_lib.load().geossl_pair_head_workspace_floats(B)), dtype=torch.float32, device=dev)
        g = gout.to(torch.float32).contiguous()
        direct, grads = _param_grads(ctx.params, ctx.needs_input_grad[5:])
        call("geossl_pair_head_bwd_dyn", ctx.N, F, ptr(ctx.lay.mol_ptr), B, PROPERTY_READOUTS[ctx.readout], ptr(wd),
             ptr(m), ptr(z), ptr(y), ptr(g), ptr(dh), ptr(grads[0]), ptr(grads[1]), ptr(ws), 1 if direct else 0,
             _dyn(ctx.dyn, "n_atoms"), stream())
        if direct:
            grads = [None, None]
        return (dh, None, None, None, None) + tuple(grads)


def pair_head_width_ok(F):
    """The backbone widths the fused pair head serves: F = 32, 64 or 128 (a head of 64 / 128 / 256 inputs)."""
    return bool(_lib.load().geossl_pair_head_width_ok(int(F)))


def _check_pair_head(h, layout, readout, w, b):
    _lib.require_cuda(h, layout.mol_ptr, w, b)
    F = h.size(1) if h.dim() == 2 else -1
    if h.dim() != 2 or not pair_head_width_ok(F):
        raise ValueError("pair head: h [N, F] with F in (32, 64, 128), got %s" % (tuple(h.shape),))
    if (tuple(w.shape), tuple(b.shape)) != ((1, 2 * F), (1,)) or w.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("pair head: float32 Linear(2F, 1) parameters, got %s, %s" % (tuple(w.shape), tuple(b.shape)))
    if readout not in PROPERTY_READOUTS:
        raise ValueError("pair head: readout is 'mean', 'add' or 'sum', got %r" % (readout,))
    if int(layout.B) < 2 or int(layout.B) % 2 or int(layout.N) != h.size(0):
        raise ValueError("pair head: the layout of 2B structures [active | inactive] over the rows of h, got B = %d, "
                         "N = %d for %d rows" % (layout.B, layout.N, h.size(0)))


def pair_head(h, w, b, layout, readout, y, dyn=None):
    """The LEP loss with the readout inside the head -> (loss, z): h [N, F] per-atom latent of the 2B structures
    [active 0 .. B-1 | inactive 0 .. B-1] (atoms sorted by structure), (w [1, 2F], b [1]) of Linear(2F, 1), layout: the
    MolLayout of the 2B structures, readout "mean" / "add" ("sum"), y [B] float32 labels.  loss is the mean
    BCE-with-logits of z_b = b + <w[0:F], m_b> + <w[F:2F], m_{B+b}>; z [B] the logits.  dyn (bucket.DynDims): the rows of
    h are a capacity and the real atom count is read on the device (layout.mol_ptr holds the real offsets)."""
    _check_pair_head(h, layout, readout, w, b)
    B = int(layout.B) // 2
    _lib.require_cuda(y)
    if y.dim() != 1 or y.numel() != B or y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("pair head: y is a contiguous float32 [B], B = %d, got %s %s" % (B, y.dtype, tuple(y.shape)))
    return _PairHead.apply(h, y, layout, readout, dyn, w, b)


def pair_predict(h, w, b, layout, readout, dyn=None):
    """eval() of finetune_lep.py:77-85 after the backbone: the logits [B] (no autograd); dyn as in `pair_head`."""
    _check_pair_head(h, layout, readout, w, b)
    h = _f32(h.detach())
    N, F = h.shape
    B = int(layout.B) // 2
    z = torch.empty(B, dtype=torch.float32, device=h.device)
    call("geossl_pair_head_predict_dyn", ptr(h), N, F, ptr(layout.mol_ptr), B, PROPERTY_READOUTS[readout],
         ptr(w.detach().contiguous()), ptr(b.detach().contiguous()), ptr(z), _dyn(dyn, "n_atoms"), stream())
    return z


# ---- GeoSSL-RR: the two AutoEncoder heads of a step (csrc/rr_head.hip) ---------------------------------------------------
RR_LOSSES = {"l1": 0, "l2": 1, "cosine": 2}
RR_STATS = {"fwd": 0, "bwd": 0}   # calls of the fused head (tests: a step took the kernels)


def rr_head_width_ok(F):
    """The width the fused AutoEncoder heads serve: F = 128."""
    return bool(_lib.load().geossl_rr_head_width_ok(int(F)))


def _ptr_array(tensors):
    """A host array of device pointers (kept alive by the caller for the duration of the call)."""
    return np.array([0 if t is None else t.data_ptr() for t in tensors], dtype=np.uint64)


def rr_head_forward(X, Y, params, buffers, bn, kind):
    """geossl_rr_head_fwd -> (loss, saved): X, Y [B, 128] contiguous fp32; params: the 12 detached parameters (per head
    W1, b1, gamma, beta, W2, b2); buffers: per head running_mean, running_var, num_batches_tracked - updated IN PLACE;
    bn: ((eps, momentum), (eps, momentum)).  saved = (zhat [2, B, F], istd [2, F], act [2, B, F], p [2, B, F])."""
    B, F = X.shape
    f32 = dict(dtype=torch.float32, device=X.device)
    zhat, act, p = torch.empty(2, B, F, **f32), torch.empty(2, B, F, **f32), torch.empty(2, B, F, **f32)
    istd = torch.empty(2, F, **f32)
    ws = torch.empty(int(_lib.load().geossl_rr_head_workspace_floats(B)), **f32)
    loss = torch.empty((), **f32)
    pa, ba = _ptr_array(params), _ptr_array(buffers)
    call("geossl_rr_head_fwd", ptr(X), ptr(Y), B, F, RR_LOSSES[kind], pa.ctypes.data, ba.ctypes.data, float(bn[0][0]),
         float(bn[0][1]), float(bn[1][0]), float(bn[1][1]), ptr(zhat), ptr(istd), ptr(act), ptr(p), ptr(ws), ptr(loss),
         stream())
    RR_STATS["fwd"] += 1
    return loss, (zhat, istd, act, p)


def rr_head_backward(X, Y, params, saved, kind, detach_target, gout, grads, accumulate):
    """geossl_rr_head_bwd -> dxy [2B, 128]: rows [0, B) the gradient of X, rows [B, 2B) that of Y; grads: 12 buffers,
    written or (accumulate) added to."""
    B, F = X.shape
    f32 = dict(dtype=torch.float32, device=X.device)
    zhat, istd, act, p = saved
    dp, dz = torch.empty(2, B, F, **f32), torch.empty(2, B, F, **f32)
    dt = None if detach_target else torch.empty(2, B, F, **f32)
    dxy = torch.empty(2 * B, F, **f32)
    tn = torch.empty(int(_lib.load().geossl_tn_workspace_floats(B, F, F, 4)), **f32)
    pa, ga = _ptr_array(params), _ptr_array(grads)
    call("geossl_rr_head_bwd", ptr(X), ptr(Y), B, F, RR_LOSSES[kind], 1 if detach_target else 0, pa.ctypes.data,
         ptr(zhat), ptr(istd), ptr(act), ptr(p), ptr(gout), ptr(dp), ptr(dz), ptr(dt), ga.ctypes.data,
         1 if accumulate else 0, ptr(dxy), ptr(tn), stream())
    RR_STATS["bwd"] += 1
    return dxy


class _RRHeads(torch.autograd.Function):
    """(AE_1(X, Y) + AE_2(Y, X)) / 2 (examples/pretrain_GeoSSL.py:96-98) on csrc/rr_head.hip -> loss fp32 scalar.  The
    backward returns dX, dY (two halves of one buffer: split_views' backward joins them without a copy) and the heads'
    gradients through autograd, or, inside _lib.direct_grads() with dense fp32 .grad tensors, adds them into those."""

    @staticmethod
    def forward(ctx, X, Y, kind, detach_target, bn, buffers, *params):
        X, Y = _f32(X.detach()), _f32(Y.detach())
        ps = [p.detach().contiguous() for p in params]
        loss, saved = rr_head_forward(X, Y, ps, buffers, bn, kind)
        ctx.save_for_backward(X, Y, *saved, *ps)
        ctx.kind, ctx.detach_target, ctx.params = kind, detach_target, params
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, gout):
        params = ctx.params
        if gout is None:
            return (None,) * (6 + len(params))
        X, Y, zhat, istd, act, p = ctx.saved_tensors[:6]
        ps = ctx.saved_tensors[6:]
        direct, grads = _param_grads(params)
        g = gout.to(torch.float32).contiguous()
        dxy = rr_head_backward(X, Y, ps, (zhat, istd, act, p), ctx.kind, ctx.detach_target, g, grads, direct)
        B = X.size(0)
        return (dxy[:B], dxy[B:], None, None, None, None) + ((None,) * len(params) if direct else tuple(grads))


def rr_heads(X, Y, kind, detach_target, bn, buffers, params):
    """The fused loss of both AutoEncoder heads -> fp32 scalar: X, Y [B, 128] (B >= 2) the two views' readouts, kind
    "l1" / "l2" / "cosine", bn ((eps, momentum) per head), buffers (running_mean, running_var, num_batches_tracked per
    head; updated in place), params (W1, b1, gamma, beta, W2, b2 per head)."""
    _lib.require_cuda(X, Y, *buffers, *params)
    if (X.dim() != 2 or X.shape != Y.shape or not rr_head_width_ok(X.size(1)) or X.size(0) < 2 or len(params) != 12
            or len(buffers) != 6 or kind not in RR_LOSSES):
        raise ValueError("rr_heads: X, Y [B, 128] with B >= 2, 12 parameters, 6 buffers and a loss of %s; got %s, %s, %r"
                         % (tuple(RR_LOSSES), tuple(X.shape), tuple(Y.shape), kind))
    return _RRHeads.apply(X, Y, kind, bool(detach_target), bn, buffers, *params)


# ---- molecular dynamics: the integrator around the force pass (csrc/md_integrate.hip) --------------------------------
MD_STATE_WORDS = 8      # int64: steps completed, step in flight + 1, seed, record_every, first step, thermostat, 2 unused
MD_PARAM_WORDS = 4      # fp32: dt, c1, sigma_T, unused
MD_STEP_DONE, MD_STEP_NEXT, MD_SEED, MD_RECORD_EVERY, MD_FIRST, MD_THERMOSTAT = range(6)


def _md_dense(t, dtype, shape, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
        raise ValueError("md: %s is a contiguous CUDA %s tensor of shape %s" % (what, str(dtype)[6:], shape))
    return t


def md_normals(seed, step, N, device=None, out=None):
    """The thermostat's draws of step `step` under `seed` -> fp32 [N, 3]: what md_advance uses for its Langevin update."""
    N = int(N)
    if out is None:
        out = torch.empty(N, 3, dtype=torch.float32, device=device if device is not None else "cuda")
    _md_dense(out, torch.float32, (N, 3), "out")
    call("geossl_md_normals", int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), N, ptr(out), stream())
    return out


def md_advance(pos, vel, grad, cinv_mass, rsqrt_mass, params, state):
    """First half of an MD step, in place on pos and vel (include/geossl_hip.h): half kick with grad, drift (Langevin:
    half drift, thermostat, half drift).  params fp32 [4], state int64 [8]: device data, read by the launch."""
    N = pos.size(0) if torch.is_tensor(pos) and pos.dim() == 2 else -1
    for t, what in ((pos, "pos"), (vel, "vel"), (grad, "grad")):
        _md_dense(t, torch.float32, (N, 3), what)
    _md_dense(cinv_mass, torch.float32, (N,), "cinv_mass")
    _md_dense(rsqrt_mass, torch.float32, (N,), "rsqrt_mass")
    _md_dense(params, torch.float32, (MD_PARAM_WORDS,), "params")
    _md_dense(state, torch.int64, (MD_STATE_WORDS,), "state")
    call("geossl_md_advance", ptr(pos), ptr(vel), ptr(grad), ptr(cinv_mass), ptr(rsqrt_mass), ptr(params), ptr(state), N,
         stream())


def md_finish(pos, vel, grad_new, energy_new, grad, energy, cinv_mass, ke_coef, mol_ptr, params, state, frames=None,
              record_only=False):
    """Second half of an MD step: the kick with grad_new (kept in grad, energy_new in energy), the molecules' kinetic
    energies in fp64 and, when the step is one to record, its frame into `frames` = (traj_pos [R, N, 3], traj_vel
    [R, N, 3], traj_pot [R, B] fp32, traj_kin [R, B] fp64).  record_only: no kick, slot 0 written."""
    N = pos.size(0) if torch.is_tensor(pos) and pos.dim() == 2 else -1
    B = energy.numel() if torch.is_tensor(energy) else -1
    for t, what in ((pos, "pos"), (vel, "vel"), (grad_new, "grad_new"), (grad, "grad")):
        _md_dense(t, torch.float32, (N, 3), what)
    _md_dense(energy_new, torch.float32, (B,), "energy_new")
    _md_dense(energy, torch.float32, (B,), "energy")
    _md_dense(cinv_mass, torch.float32, (N,), "cinv_mass")
    _md_dense(ke_coef, torch.float64, (N,), "ke_coef")
    _md_dense(mol_ptr, torch.int32, (B + 1,), "mol_ptr")
    _md_dense(params, torch.float32, (MD_PARAM_WORDS,), "params")
    _md_dense(state, torch.int64, (MD_STATE_WORDS,), "state")
    R, tp = 0, (None, None, None, None)
    if frames is not None:
        tp = frames
        R = tp[0].size(0) if torch.is_tensor(tp[0]) and tp[0].dim() == 3 else -1
        _md_dense(tp[0], torch.float32, (R, N, 3), "traj_pos")
        _md_dense(tp[1], torch.float32, (R, N, 3), "traj_vel")
        _md_dense(tp[2], torch.float32, (R, B), "traj_pot")
        _md_dense(tp[3], torch.float64, (R, B), "traj_kin")
    if record_only and R < 1:
        raise ValueError("md: record_only writes slot 0 of `frames`")
    call("geossl_md_finish", ptr(pos), ptr(vel), ptr(grad_new), ptr(energy_new), ptr(grad), ptr(energy), ptr(cinv_mass),
         ptr(ke_coef), ptr(mol_ptr), B, N, ptr(params), ptr(state), 1 if record_only else 0, R, ptr(tp[0]), ptr(tp[1]),
         ptr(tp[2]), ptr(tp[3]), stream())


# ---- structure relaxation: FIRE around the force pass (csrc/relax.hip) -----------------------------------------------
FIRE_PARAM_WORDS = 8    # fp32: ftol, dt_max, dt_min, max_step, f_inc, f_dec, alpha_start, f_alpha
FIRE_IPARAM_WORDS = 4   # int64: n_min, record_every, call counter of trajectory slot 0, unused
FIRE_MOL_WORDS = 4      # int32 per molecule: npos, done, nsteps, calls
FIRE_FTOL, FIRE_DT_MAX, FIRE_DT_MIN, FIRE_MAX_STEP, FIRE_F_INC, FIRE_F_DEC, FIRE_ALPHA_START, FIRE_F_ALPHA = range(8)
FIRE_N_MIN, FIRE_RECORD_EVERY, FIRE_FIRST = range(3)
FIRE_NPOS, FIRE_DONE, FIRE_NSTEPS, FIRE_CALLS = range(4)


def fire_frames(R, N, B, device, fill=None):
    """The eight trajectory buffers of fire_step for R frames: positions, velocities [R, N, 3], energy, fmax, dt, alpha
    [R, B] fp32, npos, done [R, B] int32."""
    make = (lambda *s, **k: torch.zeros(*s, **k)) if fill is None else (lambda *s, **k: torch.full(s, fill, **k))
    f32, i32 = dict(dtype=torch.float32, device=device), dict(dtype=torch.int32, device=device)
    return (make(R, N, 3, **f32), make(R, N, 3, **f32), make(R, B, **f32), make(R, B, **f32), make(R, B, **f32),
            make(R, B, **f32), make(R, B, **i32), make(R, B, **i32))


def fire_step(pos, vel, grad_new, energy_new, grad, energy, cinv_mass, mol_ptr, params, iparams, mol_dt, mol_alpha,
              mol_state, frames=None, evaluate_only=False):
    """One FIRE step of every molecule, in place (include/geossl_hip.h): the convergence test at pos with grad_new, the
    frame when the molecule's call counter hits a slot of `frames` (the eight buffers of `fire_frames`), the update of
    vel, pos and the molecule's words.  evaluate_only: the test and slot 0 of `frames`, nothing else written."""
    N = pos.size(0) if torch.is_tensor(pos) and pos.dim() == 2 else -1
    B = energy.numel() if torch.is_tensor(energy) else -1
    for t, what in ((pos, "pos"), (vel, "vel"), (grad_new, "grad_new"), (grad, "grad")):
        _md_dense(t, torch.float32, (N, 3), what)
    _md_dense(energy_new, torch.float32, (B,), "energy_new")
    _md_dense(energy, torch.float32, (B,), "energy")
    _md_dense(cinv_mass, torch.float32, (N,), "cinv_mass")
    _md_dense(mol_ptr, torch.int32, (B + 1,), "mol_ptr")
    _md_dense(params, torch.float32, (FIRE_PARAM_WORDS,), "params")
    _md_dense(iparams, torch.int64, (FIRE_IPARAM_WORDS,), "iparams")
    _md_dense(mol_dt, torch.float32, (B,), "mol_dt")
    _md_dense(mol_alpha, torch.float32, (B,), "mol_alpha")
    _md_dense(mol_state, torch.int32, (B, FIRE_MOL_WORDS), "mol_state")
    R, tp = 0, (None,) * 8
    if frames is not None:
        tp = tuple(frames)
        R = tp[0].size(0) if len(tp) == 8 and torch.is_tensor(tp[0]) and tp[0].dim() == 3 else -1
        _md_dense(tp[0], torch.float32, (R, N, 3), "traj_pos")
        _md_dense(tp[1], torch.float32, (R, N, 3), "traj_vel")
        for t, what in zip(tp[2:6], ("traj_energy", "traj_fmax", "traj_dt", "traj_alpha")):
            _md_dense(t, torch.float32, (R, B), what)
        for t, what in zip(tp[6:], ("traj_npos", "traj_done")):
            _md_dense(t, torch.int32, (R, B), what)
    if evaluate_only and R < 1:
        raise ValueError("md: evaluate_only writes slot 0 of `frames`")
    call("geossl_fire_step", ptr(pos), ptr(vel), ptr(grad_new), ptr(energy_new), ptr(grad), ptr(energy), ptr(cinv_mass),
         ptr(mol_ptr), B, N, ptr(params), ptr(iparams), ptr(mol_dt), ptr(mol_alpha), ptr(mol_state),
         1 if evaluate_only else 0, R, *[ptr(t) for t in tp], stream())


def fire_active(mol_state, active):
    """active[0] (int32) = the number of molecules whose `done` word is 0: the one word a relaxation's host loop reads."""
    B = mol_state.size(0) if torch.is_tensor(mol_state) and mol_state.dim() == 2 else -1
    _md_dense(mol_state, torch.int32, (B, FIRE_MOL_WORDS), "mol_state")
    _md_dense(active, torch.int32, (1,), "active")
    call("geossl_fire_active", ptr(mol_state), B, ptr(active), stream())


# ---- normal-mode analysis: Hessian rounds, finishing pass, batched Jacobi (csrc/vibrations.hip) ------------------------
HESSIAN_STATE_WORDS = 4   # int64: round, round in flight, 2 unused
HESSIAN_ROUND, HESSIAN_IN_FLIGHT = range(2)
HESSIAN_PROJECT = {None: 0, "t": 1, "tr": 2}
JACOBI_MAX_DIM = 99       # A and V of one matrix in the LDS of a CU
HESSIAN_MAX_DIM = 3 * 255


def _hessian_shapes(x0, mol_ptr, C):
    N = x0.size(0) if torch.is_tensor(x0) and x0.dim() == 2 else -1
    B = mol_ptr.numel() - 1 if torch.is_tensor(mol_ptr) else -1
    C = int(C)
    if C < 1 or B < 1:
        raise ValueError("md: coords_per_pass and the number of molecules are at least 1")
    _md_dense(x0, torch.float32, (N, 3), "x0")
    _md_dense(mol_ptr, torch.int32, (B + 1,), "mol_ptr")
    return N, B, C


def hessian_displace(x0, mol_ptr, delta, state, C, img):
    """The image positions of round state[0] (include/geossl_hip.h): img [2 C, N, 3] = x0 with local coordinate k =
    round C + c of every molecule moved by +delta (image 2 c) and -delta (image 2 c + 1); delta fp32 [1] and state int64
    [4] are device data."""
    N, B, C = _hessian_shapes(x0, mol_ptr, C)
    _md_dense(delta, torch.float32, (1,), "delta")
    _md_dense(state, torch.int64, (HESSIAN_STATE_WORDS,), "state")
    _md_dense(img, torch.float32, (2 * C, N, 3), "img")
    call("geossl_hessian_displace", ptr(x0), ptr(mol_ptr), ptr(delta), ptr(state), B, N, C, ptr(img), stream())


def hessian_collect(x0, img, grad, energy_img, mol_ptr, state, C, R, hessian, energy, fmax):
    """The rows of round state[1] into hessian [B, M, M] fp64 from the image batch's gradients; at round R, energy and
    fmax [B] fp64 of image 0 instead.  Advances state[0]."""
    N, B, C = _hessian_shapes(x0, mol_ptr, C)
    M = hessian.size(1) if torch.is_tensor(hessian) and hessian.dim() == 3 else -1
    if not 1 <= M <= HESSIAN_MAX_DIM or int(R) < 0:
        raise ValueError("md: hessian is [B, M, M] with 1 <= M <= %d and R >= 0" % HESSIAN_MAX_DIM)
    _md_dense(img, torch.float32, (2 * C, N, 3), "img")
    _md_dense(grad, torch.float32, (2 * C * N, 3), "grad")
    _md_dense(energy_img, torch.float32, (2 * C * B,), "energy_img")
    _md_dense(state, torch.int64, (HESSIAN_STATE_WORDS,), "state")
    _md_dense(hessian, torch.float64, (B, M, M), "hessian")
    _md_dense(energy, torch.float64, (B,), "energy")
    _md_dense(fmax, torch.float64, (B,), "fmax")
    call("geossl_hessian_collect", ptr(img), ptr(grad), ptr(energy_img), ptr(mol_ptr), ptr(state), B, N, C, int(R), M,
         ptr(hessian), ptr(energy), ptr(fmax), stream())


def hessian_finish(hessian, x0, masses, mol_ptr, project, D, asymmetry, n_projected, workspace=None):
    """The finishing pass, in place on hessian [B, M, M] fp64 (symmetrised, zero outside each 3 n_b block): D [B, M, M] =
    the mass-weighted, projected Hessian, asymmetry [B] fp64, n_projected [B] int32.  project: None, "t" or "tr"."""
    N, B, _ = _hessian_shapes(x0, mol_ptr, 1)
    M = hessian.size(1) if torch.is_tensor(hessian) and hessian.dim() == 3 else -1
    if not 1 <= M <= HESSIAN_MAX_DIM or project not in HESSIAN_PROJECT:
        raise ValueError("md: hessian is [B, M, M] with 1 <= M <= %d, project None, 't' or 'tr'" % HESSIAN_MAX_DIM)
    _md_dense(hessian, torch.float64, (B, M, M), "hessian")
    _md_dense(D, torch.float64, (B, M, M), "D")
    _md_dense(masses, torch.float64, (N,), "masses")
    _md_dense(asymmetry, torch.float64, (B,), "asymmetry")
    _md_dense(n_projected, torch.int32, (B,), "n_projected")
    words = int(_lib.load().geossl_hessian_finish_workspace(B, M))
    if workspace is None:
        workspace = torch.empty(words, dtype=torch.float64, device=hessian.device)
    _md_dense(workspace, torch.float64, (words,), "workspace")
    call("geossl_hessian_finish", ptr(hessian), ptr(x0), ptr(masses), ptr(mol_ptr), B, N, M, HESSIAN_PROJECT[project],
         ptr(D), ptr(asymmetry), ptr(n_projected), ptr(workspace), stream())


def sym_eig_jacobi(A, dims, max_sweeps, eigenvalues=None, modes=None, sweeps=None, converged=None):
    """Batched symmetric eigendecomposition on the device -> (eigenvalues [B, M] ascending, NaN past dims; modes [B, M, M],
    eigenvectors in columns; sweeps [B]; converged [B] int32).  A [B, M, M] fp64 with M <= 99, dims [B] int32."""
    B = A.size(0) if torch.is_tensor(A) and A.dim() == 3 else -1
    M = A.size(1) if B > 0 else -1
    if not 1 <= M <= JACOBI_MAX_DIM or not 0 <= int(max_sweeps) <= 4096:
        raise ValueError("md: the device eigensolver takes [B, M, M] with 1 <= M <= %d and 0 <= max_sweeps <= 4096"
                         % JACOBI_MAX_DIM)
    _md_dense(A, torch.float64, (B, M, M), "A")
    _md_dense(dims, torch.int32, (B,), "dims")
    dev = A.device
    eigenvalues = torch.empty(B, M, dtype=torch.float64, device=dev) if eigenvalues is None else eigenvalues
    modes = torch.empty(B, M, M, dtype=torch.float64, device=dev) if modes is None else modes
    sweeps = torch.empty(B, dtype=torch.int32, device=dev) if sweeps is None else sweeps
    converged = torch.empty(B, dtype=torch.int32, device=dev) if converged is None else converged
    _md_dense(eigenvalues, torch.float64, (B, M), "eigenvalues")
    _md_dense(modes, torch.float64, (B, M, M), "modes")
    _md_dense(sweeps, torch.int32, (B,), "sweeps")
    _md_dense(converged, torch.int32, (B,), "converged")
    call("geossl_sym_eig_jacobi", ptr(A), ptr(dims), B, M, int(max_sweeps), ptr(eigenvalues), ptr(modes), ptr(sweeps),
         ptr(converged), stream())
    return eigenvalues, modes, sweeps, converged
