"""Host twins of the incidence-list entry (csrc/painn_inc.hip) for the tests, in two independent forms.

``layout_twin``: numpy, a stable sort by key within each structure - how the kernel is built.
``edge_layout_definition``: plain Python, the definition of layout.EdgeLayout restated - atom a's list on side "i" is
every edge e of a's structure with row 0 == a, in ascending e (side "j": row 1), and iptr is the running total.

Both leave out an edge with an end outside its structure and report it (status 1).  The kernel keeps a structure's
lists inside the structure's span of the edge list [e0, e1): the slots that left-out edges leave free at the end of the
span belong to the structure's last atom and hold e0.  ``lists_of`` cuts them off again, so both forms compare atom by
atom."""
import numpy as np


def _mol_ptr(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def layout_twin(edge_index, sizes, E=None, N_cap=None):
    """-> (iptr_i int64 [N_cap + 1], ilist_i int32 [E], iptr_j, ilist_j, status), or (None, None, None, None, 1) for a
    list that is not grouped by structure in batch order (nothing is promised about its lists).  E: the real edge count
    (the first E columns count), N_cap: atoms [N, N_cap] get empty lists at E."""
    ptr = _mol_ptr(sizes)
    N = int(ptr[-1])
    E = edge_index.shape[1] if E is None else int(E)
    N_cap = N if N_cap is None else int(N_cap)
    si, sj = np.asarray(edge_index[0][:E], dtype=np.int64), np.asarray(edge_index[1][:E], dtype=np.int64)
    if E and (si.min() < 0 or si.max() >= N):
        return None, None, None, None, 1
    mol = np.searchsorted(ptr, si, side="right") - 1
    if np.any(np.diff(mol) < 0):
        return None, None, None, None, 1
    status = 0
    out = []
    span = np.searchsorted(mol, np.arange(len(sizes) + 1))         # first edge of every structure
    keep = (sj >= ptr[mol]) & (sj < ptr[mol + 1])
    if not keep.all():
        status = 1
    for key in (si, sj):
        iptr = np.full(N_cap + 1, E, dtype=np.int64)
        ilist = np.full(E, -1, dtype=np.int32)
        for m in range(len(sizes)):
            e0, e1 = int(span[m]), int(span[m + 1])
            e = np.arange(e0, e1)[keep[e0:e1]]
            k = key[e] - ptr[m]
            order = np.argsort(k, kind="stable")
            ilist[e0:e0 + e.size] = e[order]
            ilist[e0 + e.size:e1] = e0
            iptr[ptr[m]:ptr[m + 1]] = e0 + np.concatenate([[0], np.cumsum(np.bincount(k, minlength=int(sizes[m])))[:-1]])
        out += [iptr, ilist]
    return out[0], out[1], out[2], out[3], status


def edge_layout_definition(edge_index, sizes):
    """-> ({"i": lists, "j": lists}, status): lists[a] = the edges of atom a in ascending order, by the definition."""
    batch = [m for m, n in enumerate(sizes) for _ in range(int(n))]
    N, E = len(batch), edge_index.shape[1]
    lists = {"i": [[] for _ in range(N)], "j": [[] for _ in range(N)]}
    status = 0
    for e in range(E):
        i, j = int(edge_index[0][e]), int(edge_index[1][e])
        if not (0 <= i < N and 0 <= j < N) or batch[i] != batch[j]:
            status = 1
            continue
        lists["i"][i].append(e)
        lists["j"][j].append(e)
    return lists, status


def lists_of(iptr, ilist, sizes, kept):
    """The per-atom lists that (iptr, ilist) hold; kept[a] = entries of atom a that are edges (the rest of a structure's
    last list must be the filler: the span's first edge)."""
    ptr = _mol_ptr(sizes)
    out = []
    for m in range(len(sizes)):
        for a in range(int(ptr[m]), int(ptr[m + 1])):
            row = [int(v) for v in ilist[int(iptr[a]):int(iptr[a + 1])]]
            if a + 1 < ptr[m + 1]:
                assert len(row) == kept[a], (a, len(row), kept[a])
            else:
                assert all(v == int(iptr[ptr[m]]) for v in row[kept[a]:]), (a, row[kept[a]:])
                row = row[:kept[a]]
            out.append(row)
    return out
