"""Record what ``bucket.Bucket.fill`` leaves behind, case by case: the fixture tests/golden/bucket_fill_images.npz.

For every case of ``CASES`` a fresh bucket takes FOUR fills (the fourth lands in staging slot 0 again, so the stale
words of a reused slot are covered).  After each fill the whole blob is kept as int32 words, every other tensor the
bucket owns as a SHA-256 of its bytes, together with the host inputs of the fill (sizes, counts, the handle's offsets,
E, T) and the constructor's arguments.  Only the public surface of the bucket is used, so the same file runs on any
revision:

    python tools/record_bucket_images.py OUT.npz            # record (needs the GPU)
    python tools/record_bucket_images.py --diff A.npz B.npz  # compare two recordings
    python tools/record_bucket_images.py --check             # the cases against their capacities (host only)

tests/test_bucket_image_cpu.py replays the host image of every fill from the fixture without a device;
tests/test_gpu_bucket_images.py records the cases again on the tree under test and compares.
"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S7 = [5, 18, 2, 9, 33, 1, 12]
# name, kind, option, views, source ("collated" | "handle"), max_n, four size sequences of one B; optional: n_rbf,
# masked (DeviceLoader(mask_ratio=0.3): the sizes are those of the dataset's molecules, the batch holds the kept atoms),
# x1d (a dataset / batch whose x has one dimension).  Fills 2 .. 4 fit the bucket sized for the first (`--check`), one
# of them within a few rows of a capacity.  The small PaiNN cases cannot come that near: their tight capacity is the
# edge capacity (sized from the first batch's edges, which follow the pair slots), the edges are a property of the drawn
# geometry that only the device's radius graph counts exactly, and a sequence that overshoots it aborts the recording.
# Recorded (`--check` prints them from the fixture): 1736 / 1856 edges (small), 754 / 832 (triples), a bound of 1056 /
# 1280 (masked); the big case takes 4792 / 4800 pair slots at 3485 / 3968 edges.
# Cases that share their sequences share their molecules.
_S7_SEQS = [S7, [33, 1, 2, 3, 4, 5, 6], [17, 21, 2, 9, 33, 1, 25], [2, 2, 1, 30, 1, 8, 20]]          # pair slots 1211 / 1216
_S7_PERM_SEQS = [S7, [33, 1, 2, 3, 4, 5, 6], [17, 21, 5, 9, 33, 1, 22], [2, 2, 1, 30, 1, 8, 20]]     # tuples 2302 / 2304
_S7_MASK_SEQS = [S7, [33, 1, 2, 3, 4, 5, 6], [17, 21, 9, 11, 33, 8, 28], [2, 2, 1, 30, 1, 8, 20]]    # kept pair slots 701 / 704
_S4_SEQS = [[34, 3, 60, 1], [1, 64, 10, 52], [60, 35, 19, 2], [12, 3, 33, 50]]                      # pair slots 3387 / 3392
_T5_SEQS = [[5, 18, 3, 9, 12], [4, 4, 20, 6, 3], [7, 3, 11, 2, 5], [19, 9, 7, 8, 20]]               # pair slots 446 / 448
_T5_PAINN_SEQS = [[5, 18, 3, 9, 12], [4, 4, 20, 6, 3], [7, 3, 11, 2, 5], [17, 9, 7, 9, 18]]         # edges 754 / 832
_P3_SEQS = [[80, 5, 20], [20, 74, 3], [96, 2, 22], [30, 40, 50]]                                    # pair slots 4792 / 4800
_P4_SEQS = [[9, 18, 2, 33], [33, 1, 4, 8], [21, 19, 10, 33], [2, 2, 30, 12]]                        # edges 1736 / 1856
_P5_SEQS = [[9, 18, 2, 33, 12], [33, 3, 4, 8, 30], [12, 20, 4, 33, 18], [2, 2, 30, 12, 1]]             # bound on the kept edges 1056 / 1280
_SP_SEQS = [[300, 2, 64, 1], [1, 2, 60, 510], [310, 20, 90, 3], [256, 100, 7, 64]]                  # atoms 573 / 576


def _case(name, kind, option, views, source, max_n, seqs, **kw):
    return dict(dict(name=name, kind=kind, option=option, views=views, source=source, max_n=max_n, seqs=seqs, n_rbf=20,
                     masked=False, x1d=False), **kw)


CASES = [
    _case("schnet_comb_collated", "schnet", "combination", 2, "collated", 33, _S7_SEQS),
    _case("schnet_comb_handle", "schnet", "combination", 2, "handle", 33, _S7_SEQS),
    _case("schnet_perm_v1_collated", "schnet", "permutation", 1, "collated", 33, _S7_PERM_SEQS),
    _case("schnet_perm_v1_handle", "schnet", "permutation", 1, "handle", 33, _S7_PERM_SEQS),
    _case("schnet_comb_class64_collated", "schnet", "combination", 2, "collated", 64, _S4_SEQS),
    _case("schnet_triples_collated", "schnet", "triples", 1, "collated", 33, _T5_SEQS),
    _case("schnet_triples_handle", "schnet", "triples", 1, "handle", 33, _T5_SEQS),
    _case("schnet_masked_handle", "schnet", "combination", 2, "handle", 33, _S7_MASK_SEQS, masked=True),
    _case("painn_big_collated", "painn", "combination", 2, "collated", 128, _P3_SEQS),
    _case("painn_big_handle", "painn", "combination", 2, "handle", 128, _P3_SEQS),
    _case("painn_small_collated", "painn", "combination", 2, "collated", 33, _P4_SEQS),
    _case("painn_small_handle", "painn", "combination", 2, "handle", 33, _P4_SEQS),
    _case("painn_masked_handle", "painn", "combination", 2, "handle", 33, _P5_SEQS, masked=True),
    _case("painn_triples_handle", "painn", "triples", 1, "handle", 33, _T5_PAINN_SEQS),
    _case("sparse_collated_x1d", "schnet", "sparse", 1, "collated", 512, _SP_SEQS, x1d=True),
    _case("sparse_handle", "schnet", "sparse", 1, "handle", 512, _SP_SEQS, x1d=True),
]
MASK_RATIO = 0.3
FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                       "bucket_fill_images.npz")
ZERO_FLOATS = 4099


def batch_sizes(case, k):
    """The molecule sizes the k-th fill sees (a masked handle: the kept atoms)."""
    n = np.asarray(case["seqs"][k], dtype=np.int64)
    if case["masked"]:
        from geossl_amd.Geom3D.dataloaders import masking
        n = masking.kept_count(n, MASK_RATIO)
    return n


def molecules(case):
    """The dataset of a case as numpy arrays: the molecules of its four sequences one after the other (fill k takes the
    ids k B .. k B + B - 1), with bonds for a masked case and sampled triples - none for the molecules of the third
    sequence - for a triples case."""
    from geossl_amd.synthetic import add_bonds, make_molecules
    sizes = np.concatenate([np.asarray(s, dtype=np.int64) for s in case["seqs"]])
    seed = 1000 + len(case["seqs"][0])
    mols = make_molecules(0, seed=seed, sizes=sizes)
    if case["masked"]:
        add_bonds(mols, seed=seed, cut=0.3)
    if case["x1d"]:
        mols["x"] = np.ascontiguousarray(mols["x"][:, 0])
    if case["option"] == "triples":
        rng = np.random.default_rng(seed)
        B = len(case["seqs"][0])
        cnt = np.where(sizes >= 3, 2 * sizes, 0)
        cnt[2 * B:3 * B] = 0
        mols["triple_counts"] = cnt
        mols["triples"] = np.concatenate([rng.integers(0, n, size=(3, c)) for n, c in zip(sizes, cnt)], axis=1)
        mols["triple_angle"] = rng.random(int(cnt.sum())).astype(np.float32)
    return mols


def ctor_args(case, E=0, T=0):
    """The constructor's arguments of the case's bucket: sized for the first sequence by the library's own rules."""
    from geossl_amd import bucket as bk
    n = batch_sizes(case, 0)
    B = len(n)
    counts = bk.batch_counts(n, case["option"], case["views"])
    if case["option"] == "sparse":
        caps = bk.sparse_capacities(counts[0], B, sizes=n)
    else:
        caps = bk.capacities(*counts, B=B, sizes=n)
    return dict(B=B, caps=[int(c) for c in caps], option=case["option"], x_cols=1 if case["x1d"] else 2,
                max_n=case["max_n"], kind=case["kind"], n_rbf=case["n_rbf"], views=case["views"],
                E_cap=int(bk.edge_capacity(E, B, sizes=n)) if case["kind"] == "painn" else 0,
                T_cap=int(bk.triple_capacity(T, B)) if case["option"] == "triples" else 0)


def check():
    """Every fill of every case against the capacities of the bucket made for the first (atoms, pair slots,
    super-edges, work items, largest molecule; edges and triples as the fixture recorded them, when it is there); host
    only."""
    from geossl_amd import bucket as bk
    meta = load(FIXTURE)[1] if os.path.exists(FIXTURE) else {}
    ok = True
    for case in CASES:
        a, m = ctor_args(case), meta.get(case["name"])
        for k in range(4):
            n = batch_sizes(case, k)
            c = bk.batch_counts(n, case["option"], case["views"])
            fit = all(x <= cap for x, cap in zip(c, a["caps"])) and int(n.max()) <= a["max_n"] and len(n) == a["B"]
            more = ""
            if m is not None and case["kind"] == "painn":
                more = " edges %d / %d" % (m["fills"][k]["E"], m["ctor"]["E_cap"])
                fit = fit and m["fills"][k]["E"] <= m["ctor"]["E_cap"]
            if m is not None and case["option"] == "triples":
                more += " triples %d / %d" % (m["fills"][k]["T"], m["ctor"]["T_cap"])
                fit = fit and m["fills"][k]["T"] <= m["ctor"]["T_cap"]
            ok &= fit
            print("%-30s fill %d counts %s caps %s%s %s" % (case["name"], k, c, tuple(a["caps"]), more,
                                                            "" if fit else "DOES NOT FIT"))
    return ok


def owned_tensors(bkt):
    """(name, tensor) of every tensor a bucket owns besides the blob; absent ones are left out."""
    out = [("x", bkt.x), ("positions", bkt.positions), ("batch_vec", bkt.batch_vec), ("sei", bkt.sei),
           ("pair_i", getattr(bkt.lay2, "pair_i", None)), ("pair_j", getattr(bkt.lay2, "pair_j", None)),
           ("inc_idx", bkt.sel.inc_idx), ("triples", getattr(bkt, "triples", None)),
           ("triple_angle", getattr(bkt, "triple_angle", None)), ("rei", getattr(bkt, "rei", None))]
    el = bkt.el
    if el is not None:
        out += [("el.idx_i", el.idx_i), ("el.idx_j", el.idx_j), ("el.inc_i_ptr", el.inc["i"][0]),
                ("el.inc_i_idx", el.inc["i"][1]), ("el.inc_j_ptr", el.inc["j"][0]), ("el.inc_j_idx", el.inc["j"][1]),
                ("el.row_edge", el.row_edge), ("el.grp_atom", el.grp_atom), ("el.mol_grp", el.mol_grp),
                ("el.mol_grp_end", el.mol_grp_end), ("el_status", bkt.el_status.word), ("ecap_status", bkt.ecap_status.word)]
    return [(k, v) for k, v in out if v is not None]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def batches(case, device):
    """(dataset, the four batches) of a case on the device: DeviceLoader handles in dataset order, or their collated
    twins."""
    import torch
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    mols = molecules(case)
    kw = {}
    if case["kind"] == "painn":
        kw["radius"] = 5.0
    if case["option"] == "triples":
        kw.update(triples=mols["triples"], triple_counts=mols["triple_counts"], triple_angle=mols["triple_angle"])
    if case["option"] in ("combination", "permutation"):
        kw["option"] = case["option"]
    ds = DeviceDataset.from_numpy(mols, device, **kw)
    np.random.seed(77)   # (the masked loader's Philox key is one np.random draw per epoch)
    hbs = list(DeviceLoader(ds, batch_size=len(case["seqs"][0]), shuffle=False,
                            mask_ratio=MASK_RATIO if case["masked"] else 0.0))
    assert len(hbs) == 4
    if case["source"] == "handle":
        return ds, hbs
    out = []
    for hb in hbs:
        co = ds.collate(hb)
        if case["option"] == "sparse":   # (DatasetLBA's collation: x is the atomic numbers alone)
            co = pg.Batch(co.x[:, 0].contiguous(), co.positions, co.batch, None, num_graphs=hb.num_graphs,
                          sizes=hb._sizes)
        out.append(co)
    torch.cuda.synchronize()
    return ds, out


def record_case(case, device):
    """-> (arrays {key: ndarray}, meta dict) of one case."""
    import torch
    from geossl_amd import bucket as bk
    ds, bs = batches(case, device)
    hbs = [ds.batch(np.arange(k * len(case["seqs"][0]), (k + 1) * len(case["seqs"][0]))) for k in range(4)]
    painn, triples = case["kind"] == "painn", case["option"] == "triples"

    def edges(b):
        if not painn:
            return 0
        return int(bk.handle_edges(b)) if case["source"] == "handle" else int(b.radius_edge_index.size(1))
    a = ctor_args(case, edges(bs[0]), bk.n_triples(bs[0]) if triples else 0)
    bkt = bk.Bucket(torch.device(device), a["B"], tuple(a["caps"]), a["option"], x_cols=a["x_cols"], max_n=a["max_n"],
                    kind=a["kind"], E_cap=a["E_cap"], n_rbf=a["n_rbf"], views=a["views"], T_cap=a["T_cap"])
    arrays, fills = {}, []
    for k, b in enumerate(bs):
        n = batch_sizes(case, k)
        counts = bk.batch_counts(n, case["option"], case["views"])
        zero = torch.ones(ZERO_FLOATS, dtype=torch.float32, device=device)
        real = bkt.fill(b, counts if k % 2 == 0 else None, zero=zero)
        torch.cuda.synchronize()
        ids = hbs[k].ids
        pre = "%s/%d/" % (case["name"], k)
        arrays[pre + "blob"] = bkt.blob.cpu().numpy().astype(np.int32)
        arrays[pre + "sizes"] = n
        if case["source"] == "handle":
            arrays[pre + "src_off"] = ds.off[ids]
            if painn:
                arrays[pre + "edge_off"], arrays[pre + "edge_cnt"] = ds.edge_off[ids], ds.edge_cnt[ids]
            if triples:
                arrays[pre + "triple_off"], arrays[pre + "triple_cnt"] = ds.triple_off[ids], ds.triple_cnt[ids]
        fills.append(dict(counts=[int(c) for c in counts], real=[int(c) for c in real],
                          real_E=None if bkt.real_E is None else int(bkt.real_E), E=edges(b),
                          T=bk.n_triples(b) if triples else None,
                          masked_edges=bool(painn and case["masked"]), zero=_sha(zero),
                          digests={name: _sha(t_) for name, t_ in owned_tensors(bkt)}))
    meta = dict(ctor=a, off={k: int(v) for k, v in bkt.off.items()}, words=int(bkt.blob.numel()),
                big_caps=[int(c) for c in bkt.big_caps], handle=case["source"] == "handle", fills=fills)
    return arrays, meta


def record(device="cuda:0", names=None):
    """Every case (or those named) -> {key: ndarray} with the cases' metadata as one JSON string under "meta"."""
    arrays, meta = {}, {}
    for case in CASES:
        if names is None or case["name"] in names:
            a, m = record_case(case, device)
            arrays.update(a)
            meta[case["name"]] = m
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return arrays


def load(path):
    with np.load(path, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    return arrays, json.loads(str(arrays.pop("meta")))


def diff(got, want):
    """The differences between two recordings ((arrays, meta) each) as a list of strings; empty: identical."""
    out = []
    (ga, gm), (wa, wm) = got, want
    for name in sorted(set(gm) | set(wm)):
        if name not in gm or name not in wm:
            out.append("%s: only in one recording" % name)
            continue
        g, w = gm[name], wm[name]
        for key in ("ctor", "off", "words", "big_caps", "handle"):
            if g[key] != w[key]:
                out.append("%s: %s %r != %r" % (name, key, g[key], w[key]))
        for k, (gf, wf) in enumerate(zip(g["fills"], w["fills"])):
            for key in sorted(set(gf) | set(wf)):
                if key == "digests":
                    bad = sorted(t_ for t_ in set(gf[key]) | set(wf[key]) if gf[key].get(t_) != wf[key].get(t_))
                    if bad:
                        out.append("%s fill %d: tensors differ: %s" % (name, k, ", ".join(bad)))
                elif gf.get(key) != wf.get(key):
                    out.append("%s fill %d: %s %r != %r" % (name, k, key, gf.get(key), wf.get(key)))
    for key in sorted(set(ga) | set(wa)):
        if key not in ga or key not in wa:
            out.append("%s: only in one recording" % key)
        elif ga[key].shape != wa[key].shape or not np.array_equal(ga[key], wa[key]):
            bad = np.nonzero(ga[key] != wa[key])[0][:8].tolist() if ga[key].shape == wa[key].shape else "shape"
            out.append("%s differs (words %s)" % (key, bad))
    return out


def main(argv):
    if argv[:1] == ["--check"]:
        return 0 if check() else 1
    if argv[:1] == ["--diff"]:
        d = diff(load(argv[1]), load(argv[2]))
        print("\n".join(d) if d else "identical: every case, every fill")
        return 1 if d else 0
    arrays = record()
    np.savez_compressed(argv[0], **arrays)
    print("recorded %d cases into %s" % (len(CASES), argv[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
