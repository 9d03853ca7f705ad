"""The step-graph engine makes the same C-ABI calls, in the same order, on every route from a batch to a replay.

Per case a few consecutive steps at the smallest shapes that take the route, with `call` of `_lib` and of every loaded
`geossl_amd` module that imported it wrapped by a recorder: the entry points each step calls must be those below, and
beside them the owner's `captures`, its number of graphs and the keys of a graph's entry.  A step of at most a dozen
calls - a replay - is written out; a longer one - an eager step, or a capture with its warm-up passes - is held as
(number of calls, sha1 of the names joined by blanks).  The lists were RECORDED ON THE PARENT of the commit that moved the
engine out of pretrain_GeoSSL.py into geossl_amd/replay.py and geossl_amd/autograd_step.py - by `run_case` below, run
from a job script on the code before the move, not on the code under test - so the test states that the move (and
whatever touches the capture, the sightings memory, the static-input copy or the replay protocol next) changes no launch.
Cases k to q - the trainers and reference-style loops of the other objectives - were recorded likewise on the parent of
the commit that gave both owners of the step graphs one `step.Objective` per objective and the do_* functions one routing
helper.
What the launches compute is the subject of the bit-for-bit tests of the routes (test_gpu_round4.py, test_gpu_round5.py,
test_gpu_round6.py, test_gpu_force_training.py, test_gpu_sparse_bucket.py)."""
import hashlib
import importlib
import pkgutil
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHNET = dict(hidden_channels=128, num_filters=128, num_interactions=2, num_gaussians=51, cutoff=5.0, node_class=9,
              readout="mean")
PAINN = dict(n_atom_basis=128, n_interactions=2, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")
RAGGED = ((6, 5, 6, 4), (3, 4, 5, 6), (5, 3, 3, 6))   # (the largest first: the bucket of the first step takes all three)
STEP_KEYS = ["batch", "extra", "graph", "graph_bwd", "loss", "noise", "zero"]
CASES = ("a: DDMTrainer, ragged SchNet", "b: DDMTrainer, equal sizes", "c: DDMTrainer, PaiNN by hand",
         "d: reference loop", "e: DistancePredictionTrainer", "f: SupervisedTrainer, sparse bucket",
         "g: GraphedForward", "h: ForceTrainer, SchNet", "h: ForceTrainer, PaiNN",
         "i: predict_MD17, SchNet", "i: predict_MD17, PaiNN",
         "j: MD17Trainer, handles, SchNet", "j: MD17Trainer, handles, PaiNN",
         "k: ContrastiveTrainer, InfoNCE", "k: ContrastiveTrainer, EBM_NCE", "l: RRTrainer", "l: RRTrainer, ae_lr",
         "m: ChargePredictionTrainer, device masks", "m: ChargePredictionTrainer, numpy masks",
         "n: TorsionAnglePredictionTrainer", "o: InfoGraphTrainer", "p: LEPTrainer, sparse bucket",
         "p: LEPTrainer, per structure", "q: reference loop, do_InfoNCE", "q: reference loop, do_RR",
         "q: reference loop, do_DistancePrediction", "q: reference loop, do_ChargePrediction",
         "q: reference loop, do_Supervised")


def _raw(sizes, seed):
    from geossl_amd.synthetic import make_batch
    raw = make_batch(0, seed=seed, sizes=np.asarray(sizes, dtype=np.int64))
    raw["x"][:, 0] = np.clip(raw["x"][:, 0], 1, 8)
    return raw


def _batch(sizes, seed):
    from geossl_amd import pretrain_GeoSSL as pg
    return pg.Batch.from_numpy(_raw(sizes, seed), DEV)


def _by_hand(sizes, seed):
    """A batch as a caller builds it from its own tensors: no host sizes, the radius graph of its positions."""
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    from helpers import t
    raw = _raw(sizes, seed)
    bt = pg.Batch(t(raw["x"], DEV), t(raw["positions"], DEV), t(raw["batch"], DEV), t(raw["super_edge_index"], DEV),
                  num_graphs=len(sizes))
    bt.radius_edge_index = ops.radius_graph(bt.positions, 5.0, bt.batch)
    return bt


def _schnet(**kw):
    from filler import fill_module_
    from geossl_amd.Geom3D.models import SchNet
    return fill_module_(SchNet(**dict(SCHNET, **kw))).to(DEV)


def _painn():
    from filler import fill_module_
    from geossl_amd.Geom3D.models import PaiNN
    return fill_module_(PaiNN(**PAINN)).to(DEV)


def _heads():
    from helpers import product_ncsn
    return product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9)


def _ae_heads():
    """Two AutoEncoder heads of RR in training mode, as built (torch's CPU generator where `run_case` seeded it)."""
    from geossl_amd.Geom3D.models import AutoEncoder
    return [AutoEncoder(128, "l2", True).to(DEV) for _ in range(2)]


def _triple_batch(sizes, seed):
    """A collated batch of atom triples: every triple of every molecule, with the fp64 twin's angles."""
    import torsion_twin as tw
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import AtomTripleExtractor
    raw, ext = _raw(sizes, seed), AtomTripleExtractor(1)
    off = np.concatenate([[0], np.cumsum(sizes)])
    tri = np.ascontiguousarray(np.concatenate([ext.triples(int(n)) + off[m] for m, n in enumerate(sizes)], axis=1))
    ang = tw.triple_angles(torch.from_numpy(raw["positions"]), torch.from_numpy(tri)).float()
    return pg.TripleBatch.from_numpy(dict(x=raw["x"], positions=raw["positions"], batch=raw["batch"], sizes=raw["sizes"],
                                          super_edge_index=tri, super_edge_angle=ang.numpy()), DEV)


def _lep_items(pair_sizes, seed):
    """The LEP records of these pairs: 1-D atom types, float32 positions, an integer label each."""
    import lba_structures as ls
    from geossl_amd.Geom3D.dataloaders import Data
    active, inactive = pair_sizes
    sa, si = ls.structures(active, seed), ls.structures(inactive, seed + 17)
    oa, oi = np.concatenate([[0], np.cumsum(active)]), np.concatenate([[0], np.cumsum(inactive)])
    f = torch.from_numpy
    return [Data(x_active=f(sa["x"][oa[b]:oa[b + 1]].copy()), positions_active=f(sa["positions"][oa[b]:oa[b + 1]].copy()),
                 x_inactive=f(si["x"][oi[b]:oi[b + 1]].copy()), positions_inactive=f(si["positions"][oi[b]:oi[b + 1]].copy()),
                 y=torch.tensor([(b + seed) % 2], dtype=torch.long)) for b in range(len(active))]


def _force_modules(kind):
    """Backbone and energy head of the force-training and MD17 cases."""
    from filler import fill_module_
    from geossl_amd.Geom3D.models.painn import Dense
    if kind == "painn":
        model = _painn()
        return model, fill_module_(model.create_output_layers()).to(DEV)
    return _schnet(readout="add"), fill_module_(Dense(128, 1)).to(DEV)


def _fresh_complete_edges(patch):
    """No interned complete pair list from an earlier case: the list and the layouts cached on its tensors are built once
    per process, so their launches would otherwise fall to whichever case runs first."""
    from geossl_amd import finetune_md17
    patch(finetune_md17, "_COMPLETE", {})


class _Recorder:
    """`call` of _lib and of every loaded geossl_amd module that holds it, wrapped; one list of names per step."""

    def __init__(self, patch):
        import geossl_amd
        from geossl_amd import _lib
        # every module of the package is loaded first: one that a step imported while `call` is wrapped would keep the
        # wrapper for good (`from ._lib import call`) and hand a later case's calls to this one
        for m in pkgutil.walk_packages(geossl_amd.__path__, "geossl_amd."):
            importlib.import_module(m.name)
        self.patch, self.real, self.steps, self.on = patch, _lib.call, [], False

    def _record(self, name, *a):
        if self.on:   # (between steps a case builds its next batch: not the engine's calls)
            self.steps[-1].append(name[len("geossl_"):])
        return self.real(name, *a)

    def step(self, fn):
        for name, mod in list(sys.modules.items()):
            if name.startswith("geossl_amd") and mod is not None and mod.__dict__.get("call") is self.real:
                self.patch(mod, "call", self._record)
        self.steps.append([])
        self.on = True
        try:
            out = fn()
            torch.cuda.synchronize()
        finally:
            self.on = False
        return out


def _flat(*modules):
    return torch.cat([p.detach().reshape(-1) for m in modules for p in m.parameters()]).clone()


def run_case(case, patch, setenv):
    """-> (the names each step called, {"captures", "graphs", "keys"}, {"loss": [per step], "params": one vector}).
    patch / setenv: monkeypatch's setattr and setenv (or a job script's own)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd import _lib
    _lib.load()
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    rec = _Recorder(patch)
    letter = case[0]
    losses = []
    if letter in "abc":
        kind = "painn" if letter == "c" else "schnet"
        model, (n1, n2) = (_painn() if letter == "c" else _schnet()), _heads()
        tr = pg.DDMTrainer(model, n1, n2, lr=5e-4, model_3d=kind, use_graph=True)
        if letter == "a":
            batches = [_batch(s, 20 + i) for i, s in enumerate(RAGGED)]
        elif letter == "b":
            batches = [_batch((5, 5, 5, 5), 30 + i) for i in range(3)]
        else:
            batches = [_by_hand(RAGGED[0], 40)] * 3
        for bt in batches:
            losses.append(rec.step(lambda: tr.step(bt)).clone())
        sg, modules = tr.step_graphs, (model, n1, n2)
        stats = dict(captures=sg.captures, graphs=len(sg.graphs), keys=sorted(next(iter(sg.graphs.values()))))
        route = next(iter(sg.graphs))[0]
        assert route == {"a": "bucket", "b": "sizes", "c": "tensors"}[letter], route
    elif letter == "d":
        model, (n1, n2) = _schnet(), _heads()
        opt = torch.optim.Adam([{"params": model.parameters()}, {"params": n1.parameters()}, {"params": n2.parameters()}],
                               lr=5e-4)
        args = pg.Args("schnet")

        def ref_step(bt):
            loss, _ = pg.do_DDM(args, bt, model, NCSN_models=(n1, n2), mu=0.0, sigma=0.3, graph=True)
            value = loss.detach().item()
            opt.zero_grad()
            loss.backward()
            opt.step()
            return value
        for i, s in enumerate(RAGGED):
            bt = _batch(s, 20 + i)
            losses.append(torch.tensor(rec.step(lambda: ref_step(bt))))
        (sg,) = model.__dict__["_geossl_autograd_step"].graphs.values()
        modules = (model, n1, n2)
        stats = dict(captures=sg.captures, graphs=len(sg.graphs), keys=sorted(next(iter(sg.graphs.values()))))
        assert next(iter(sg.graphs))[0] == "bucket" and next(iter(sg.graphs.values()))["graph_bwd"] is not None
    elif letter == "e":
        from filler import fill_module_
        from geossl_amd.pretrain_DistancePrediction import DistancePredictionTrainer, DistancePredictor
        model, head = _schnet(), fill_module_(DistancePredictor(128)).to(DEV)
        tr = DistancePredictionTrainer(model, head, lr=5e-4, use_graph=True)
        for i, s in enumerate(RAGGED):
            bt = _batch(s, 20 + i)
            losses.append(rec.step(lambda: tr.step(bt)).clone())
        sg, modules = tr.step_graphs, (model, head)
        stats = dict(captures=sg.captures, graphs=len(sg.graphs), keys=sorted(next(iter(sg.graphs.values()))))
        assert next(iter(sg.graphs))[0] == "bucket"
    elif letter == "f":
        import lba_structures as ls
        from filler import fill_module_
        from geossl_amd.pretrain_Supervised import SupervisedTrainer
        from helpers import t
        setenv("GEOSSL_SPARSE_BUCKETS", "1")   # (collated batches take the sparse bucket with the switch on)
        model, head = _schnet(cutoff=10.0), fill_module_(torch.nn.Linear(128, 1)).to(DEV)
        tr = SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", lr=5e-4, use_graph=True)
        for i, sizes in enumerate(((260, 256), (256, 260), (260, 256))):
            s = ls.structures(sizes, i)
            bt = pg.Batch(t(s["x"], DEV), t(s["positions"], DEV), t(s["batch"], DEV), None, num_graphs=2, sizes=sizes)
            bt.y = torch.tensor([0.5, -1.25], device=DEV)
            losses.append(rec.step(lambda: tr.step(bt)).clone())
        sg, modules = tr.step_graphs, (model, head)
        stats = dict(captures=sg.captures, graphs=len(sg.graphs), keys=sorted(next(iter(sg.graphs.values()))))
        assert next(iter(sg.graphs)) == ("bucket", 2, "sparse"), list(sg.graphs)
    elif letter == "g":
        from geossl_amd.graphed import GraphedForward
        model = _schnet()
        gf = GraphedForward(model)
        uni = [_batch((5, 5, 5, 5), 30 + i) for i in range(2)]
        rag = _batch(RAGGED[0], 20)
        flat_x = _batch((5, 5, 5, 5), 32)
        flat_x.x = flat_x.x[:, 0].contiguous()   # (a 1-D x against the 2-D x the graph of this size sequence was made on)
        for bt in uni + [rag, rag, rag, flat_x]:   # capture, replay; eager, capture, replay; eager
            losses.append(rec.step(lambda: gf(bt)).clone())
        modules = (model,)
        stats = dict(captures=gf.captures, graphs=len(gf.graphs), keys=sorted(next(iter(gf.graphs.values()))))
        assert gf.enabled
    elif letter == "i":
        import types
        from geossl_amd.finetune_md17 import _predictor, predict_MD17
        kind = "painn" if case.endswith("PaiNN") else "schnet"
        model, head = _force_modules(kind)
        args = types.SimpleNamespace(model_3d=kind)

        def frame(sizes, seed, flat=True):   # (MD17 batches: 1-D x, host sizes, PaiNN with the frame's own radius list)
            from geossl_amd import ops
            bt = _batch(sizes, seed)
            if flat:
                bt.x = bt.x[:, 0].contiguous()
            if kind == "painn":
                bt.radius_edge_index = ops.radius_graph(bt.positions, 5.0, bt.batch)
            return bt
        if kind == "schnet":   # capture, replay; eager, capture, replay; a 2-D x behind the 1-D ones: another key
            batches = ([frame((4, 4), 60 + i) for i in range(2)] + [frame((4, 3), 62 + i) for i in range(3)]
                       + [frame((4, 4), 65, flat=False)])
        else:                  # capture, replay on the complete pair list; the frame's own edges: eager
            batches = [frame((4, 4), 60 + i) for i in range(3)]
            _fresh_complete_edges(patch)
        for i, bt in enumerate(batches):
            if kind == "painn" and i == 2:
                setenv("GEOSSL_MD17_COMPLETE_EDGES", "0")
            e, f = rec.step(lambda: predict_MD17(args, bt, model, head))
            losses.append(torch.cat([e.reshape(-1), f.reshape(-1)]))
        modules, pr = (model, head), _predictor(model, head, kind)
        stats = dict(captures=pr.captures, graphs=len(pr.graphs), keys=sorted(next(iter(pr.graphs.values()))))
        assert pr.enabled
    elif letter == "j":
        from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset, DeviceLoader
        from geossl_amd.finetune_md17 import MD17Trainer
        kind = "painn" if case.endswith("PaiNN") else "schnet"
        model, head = _force_modules(kind)
        raws = [_raw((4, 4), 70 + i) for i in range(4)]
        gen = torch.Generator().manual_seed(3)
        ds = DeviceDataset(np.concatenate([r["x"][:, 0] for r in raws]), np.concatenate([r["positions"] for r in raws]),
                           [4] * 8, DEV, y=torch.randn(8, generator=gen), force=torch.randn(32, 3, generator=gen),
                           radius=5.0 if kind == "painn" else None)
        tr = MD17Trainer(model, head, model_3d=kind, lr=5e-4)
        if kind == "painn":
            _fresh_complete_edges(patch)
        # SchNet (a sizes key): collated and captured, then replays from the handle; PaiNN (the interned tensors' key): the
        # collated step eagerly, then captured, then replays from the handle
        for hb in DeviceLoader(ds, batch_size=2, shuffle=False):
            losses.append(rec.step(lambda: tr.step(hb)).clone())
        modules = (model, head)
        stats = dict(captures=tr.captures, graphs=len(tr.graphs), keys=sorted(next(iter(tr.graphs.values()))))
        assert tr.use_graph and len(losses) == 4
    elif letter in "klmno":
        from filler import fill_module_
        np.random.seed(7)   # (the numpy masks of case m)
        model = _schnet()
        if letter == "k":     # device noise: the step's own draw, straight into the graph's static input
            tr = pg.ContrastiveTrainer(model, option=case.split(", ")[1], lr=5e-4, use_graph=True)
            modules = (model,)
        elif letter == "l":   # ae_lr: a second Adam launch over the heads' range of the flat buffer
            heads = _ae_heads()
            tr = pg.RRTrainer(model, heads[0], heads[1], lr=5e-4, use_graph=True,
                              ae_lr=1e-3 if case.endswith("ae_lr") else None)
            modules = (model,) + tuple(heads)
        elif letter == "m":
            from geossl_amd.pretrain_ChargePrediction import ChargePredictionTrainer, ChargePredictor
            head = fill_module_(ChargePredictor(128)).to(DEV)
            tr = ChargePredictionTrainer(model, head, lr=5e-4, use_graph=True, seed=11,
                                         mask_rng="device" if "device" in case else "numpy")
            modules = (model, head)
        elif letter == "n":
            from geossl_amd.pretrain_TorsionAnglePrediction import (TorsionAnglePredictionTrainer,
                                                                    TorsionAnglePredictor)
            head = fill_module_(TorsionAnglePredictor(128)).to(DEV)
            tr = TorsionAnglePredictionTrainer(model, head, lr=5e-4, use_graph=True)
            modules = (model, head)
        else:
            from geossl_amd.pretrain_3DInfoGraph import Discriminator, InfoGraphTrainer
            head = fill_module_(Discriminator(128)).to(DEV)
            tr = InfoGraphTrainer(model, head, lr=5e-4, use_graph=True)
            modules = (model, head)
        for i, s in enumerate(RAGGED):
            bt = _triple_batch(s, 20 + i) if letter == "n" else _batch(s, 20 + i)
            out = rec.step(lambda: tr.step(bt))
            losses.append(torch.cat([o.double().reshape(-1) for o in out]) if isinstance(out, tuple) else out.clone())
        sg = tr.step_graphs
        stats = dict(captures=sg.captures, graphs=len(sg.graphs), keys=sorted(next(iter(sg.graphs.values()))))
        assert next(iter(sg.graphs))[0] == "bucket"
    elif letter == "p":
        from filler import fill_module_
        from geossl_amd.Geom3D.dataloaders import BatchLEP
        from geossl_amd.finetune_lep import LEPTrainer
        sparse = case.endswith("sparse bucket")
        if sparse:
            setenv("GEOSSL_SPARSE_BUCKETS", "1")   # (collated pairs take the sparse bucket with the switch on)
        model, head = _schnet(cutoff=10.0), fill_module_(torch.nn.Linear(256, 1)).to(DEV)
        with torch.no_grad():
            head.weight.mul_(0.05)   # (logits of order one with the filler's weights: no sigmoid saturates)
        tr = LEPTrainer(model, head, lr=5e-4, use_graph=True)
        # sparse bucket: capture, replay, replay; small pairs with the same two size sequences: eager, capture, replay
        pairs = ((((260, 256), (256, 258)), ((256, 260), (258, 256)), ((260, 256), (256, 258))) if sparse
                 else (((5, 4), (3, 6)),) * 3)
        for i, ps in enumerate(pairs):
            bt = BatchLEP.from_data_list(_lep_items(ps, i)).to(DEV)
            losses.append(rec.step(lambda: tr.step(bt)).clone())
        sg, modules = tr.step_graphs, (model, head)
        stats = dict(captures=sg.captures, graphs=len(sg.graphs), keys=sorted(next(iter(sg.graphs.values()))))
        key = next(iter(sg.graphs))
        assert (key[0], key[-1]) == ("bucket", "sparse") if sparse else key[0] == "tensors", list(sg.graphs)
    elif letter == "q":
        import types
        from filler import fill_module_
        np.random.seed(7)   # (do_ChargePrediction's numpy masks)
        name = case.split(", ")[1]
        model = _schnet()
        args = types.SimpleNamespace(model_3d="schnet", normalize=False, T=0.1, charge_masking_ratio=0.3,
                                     mask_rng="numpy", loss="mae")
        first = lambda out: out[0] if isinstance(out, tuple) else out
        if name == "do_InfoNCE":
            heads, slot = (), "_geossl_contrastive_step_InfoNCE"
            do = lambda bt: pg.do_InfoNCE(args, bt, model, graph=True)
        elif name == "do_RR":
            heads, slot = tuple(_ae_heads()), "_geossl_rr_step"
            do = lambda bt: pg.do_RR(args, bt, model, AE_models=heads, graph=True)
        elif name == "do_DistancePrediction":
            from geossl_amd.pretrain_DistancePrediction import DistancePredictor, do_DistancePrediction
            heads, slot = (fill_module_(DistancePredictor(128)).to(DEV),), "_geossl_distance_step"
            do = lambda bt: do_DistancePrediction(args, bt, model, heads[0], graph=True)
        elif name == "do_ChargePrediction":
            from geossl_amd.pretrain_ChargePrediction import ChargePredictor, do_ChargePrediction
            heads, slot = (fill_module_(ChargePredictor(128)).to(DEV),), "_geossl_charge_step"
            do = lambda bt: do_ChargePrediction(args, bt, model, heads[0], graph=True)
        else:
            from geossl_amd.pretrain_Supervised import do_Supervised
            heads, slot = (fill_module_(torch.nn.Linear(128, 1)).to(DEV),), "_geossl_supervised_step"
            do = lambda bt: do_Supervised(args, bt, model, heads[0], 0.25, 1.5, task_id=0, graph=True)
        modules = (model,) + heads
        opt = torch.optim.Adam([{"params": m.parameters()} for m in modules], lr=5e-4)

        def ref_step(bt):
            loss = first(do(bt))
            value = loss.detach().item()
            opt.zero_grad()
            loss.backward()
            opt.step()
            return value
        for i, s in enumerate(RAGGED):
            bt = _batch(s, 20 + i)
            bt.y = torch.linspace(-1.0, 1.0, len(s), device=DEV)
            losses.append(torch.tensor(rec.step(lambda: ref_step(bt))))
        (sg,) = model.__dict__[slot].graphs.values()
        stats = dict(captures=sg.captures, graphs=len(sg.graphs), keys=sorted(next(iter(sg.graphs.values()))))
        assert next(iter(sg.graphs))[0] == "bucket" and next(iter(sg.graphs.values()))["graph_bwd"] is not None
    else:
        from geossl_amd.graphed import ForceTrainer
        kind = "painn" if case.endswith("PaiNN") else "schnet"
        model, head = _force_modules(kind)
        tr = ForceTrainer(model, head, model_3d=kind, lr=5e-4)
        gen = torch.Generator().manual_seed(3)
        kept = _by_hand((4, 4), 50)   # (PaiNN: the very same edge tensor every step)
        for i in range(3):
            bt = kept if kind == "painn" else _batch((4, 4), 50 + i)
            y_e, y_f = torch.randn(2, generator=gen).to(DEV), torch.randn(8, 3, generator=gen).to(DEV)
            losses.append(rec.step(lambda: tr.step(bt, y_e, y_f)).clone())
        modules = (model, head)
        stats = dict(captures=tr.captures, graphs=len(tr.graphs), keys=sorted(next(iter(tr.graphs.values()))))
        assert tr.use_graph
    values = {"loss": [v.detach().double().reshape(-1).cpu() for v in losses], "params": _flat(*modules).cpu()}
    return rec.steps, stats, values


def short(step, ordered=True):
    """A step's names as EXPECTED holds them: written out up to a dozen, else (how many, their digest).  ordered=False:
    the digest of the sorted names - what the force-training cases (h, j) hold, whose eager and capture steps called the
    second-order tape's entry points in an order that differed between two runs of the parent itself (the same calls
    as often; their replay steps are written out like all others)."""
    if len(step) <= 12:
        return " ".join(step)
    return (len(step), hashlib.sha1(" ".join(step if ordered else sorted(step)).encode()).hexdigest()[:16])


@pytest.mark.parametrize("case", CASES)
def test_step_engine_launch_sequence(case, monkeypatch):
    steps, stats, values = run_case(case, monkeypatch.setattr, monkeypatch.setenv)
    assert all(torch.isfinite(v).all() for v in values["loss"]) and torch.isfinite(values["params"]).all()
    want_steps, want_stats = EXPECTED[case]
    assert stats == want_stats, stats
    assert len(steps) == len(want_steps)
    for k, (got, want) in enumerate(zip(steps, want_steps)):
        assert short(got, ordered=case[0] not in "hj") == want, "step %d: %s" % (k, " ".join(got))


# per case: (one entry per step in `short` form, the owner's counts and the keys of a graph's entry); written by the job
# script that ran `run_case` on the parent commit (twice, in two processes and two orders of the cases: the same lists)
_BUCKET_KEYS = ["batch", "bucket", "counts", "extra", "graph", "graph_bwd", "loss", "noise", "zero"]
_PREDICT_KEYS = ["bvec", "graph", "layout", "out", "pos", "rei", "x"]
_FORCE_KEYS = ["bvec", "graph", "loss", "ones", "pos", "rei", "x", "y_e", "y_f"]
_GATHER_ADAM = "gather_molecules adam_step"
_BUCKET_STATS = {"captures": 1, "graphs": 1, "keys": _BUCKET_KEYS}
EXPECTED = {
    "a: DDMTrainer, ragged SchNet": ([
        (67, "f1b1ce4918d00058"),
        "gather_molecules ddm_noise_seeded adam_step",
        "gather_molecules ddm_noise_seeded adam_step",
    ], {"captures": 1, "graphs": 1, "keys": _BUCKET_KEYS}),
    "b: DDMTrainer, equal sizes": ([
        (66, "0f45ac0f6f596b2b"),
        "copy_n ddm_noise_seeded adam_step",
        "copy_n ddm_noise_seeded adam_step",
    ], {"captures": 1, "graphs": 1, "keys": STEP_KEYS}),
    "c: DDMTrainer, PaiNN by hand": ([
        (50, "0a1a75f926780d60"),
        (117, "e8ad290282ac8445"),
        "copy_n ddm_noise_seeded adam_step",
    ], {"captures": 1, "graphs": 1, "keys": STEP_KEYS}),
    "d: reference loop": ([
        (66, "c1a76ded1212d253"),
        "gather_molecules adam_step",
        "gather_molecules adam_step",
    ], {"captures": 1, "graphs": 1, "keys": _BUCKET_KEYS}),
    "e: DistancePredictionTrainer": ([
        (60, "4d7f8152fc7d501f"),
        "gather_molecules adam_step",
        "gather_molecules adam_step",
    ], {"captures": 1, "graphs": 1, "keys": _BUCKET_KEYS}),
    "f: SupervisedTrainer, sparse bucket": ([
        (67, "9de0e24d10b5d478"),
        "gather_molecules adam_step",
        "gather_molecules adam_step",
    ], {"captures": 1, "graphs": 1, "keys": _BUCKET_KEYS}),
    "g: GraphedForward": ([
        (22, "c1eb25a53f402d28"),
        "copy2",
        (14, "4a54030f4f042e39"),
        (22, "7f2d159afd8d2f3c"),
        "copy2",
        (14, "4a54030f4f042e39"),
    ], {"captures": 2, "graphs": 2, "keys": ["batch_vec", "graph", "layout", "out", "pos", "x"]}),
    "h: ForceTrainer, SchNet": ([
        (1037, "297144397fcef8f0"),
        "copy_n adam_step",
        "copy_n adam_step",
    ], {"captures": 1, "graphs": 1, "keys": _FORCE_KEYS}),
    "h: ForceTrainer, PaiNN": ([
        (779, "3740ceed3b937739"),
        (2321, "1249d6c5da60340b"),
        "copy_n adam_step",
    ], {"captures": 1, "graphs": 1, "keys": _FORCE_KEYS}),
    "i: predict_MD17, SchNet": ([
        (53, "594796d420592639"),
        "copy2",
        (22, "b77776ec2932984b"),
        (53, "3eddd29ae86e0e26"),
        "copy2",
        (53, "594796d420592639"),
    ], {"captures": 3, "graphs": 3, "keys": _PREDICT_KEYS}),
    "i: predict_MD17, PaiNN": ([
        (108, "96819637f0d12e94"),
        "copy2",
        (38, "d952c1b4e6859739"),
    ], {"captures": 1, "graphs": 1, "keys": _PREDICT_KEYS}),
    "j: MD17Trainer, handles, SchNet": ([
        (1039, "7cba23c2145edcab"),
        "gather_molecules property_targets gather_atom_rows adam_step",
        "gather_molecules property_targets gather_atom_rows adam_step",
        "gather_molecules property_targets gather_atom_rows adam_step",
    ], {"captures": 1, "graphs": 1, "keys": _FORCE_KEYS}),
    "j: MD17Trainer, handles, PaiNN": ([
        (785, "d488987973e625c9"),
        (2323, "7a5627b0c4bec9a4"),
        "gather_molecules property_targets gather_atom_rows adam_step",
        "gather_molecules property_targets gather_atom_rows adam_step",
    ], {"captures": 1, "graphs": 1, "keys": _FORCE_KEYS}),
    # cases k to q: recorded the same way on the parent of the commit that put the trainers on step.Objective and the
    # do_* functions on step.run_graphed (two processes, two orders: the same lists in order, every step)
    "k: ContrastiveTrainer, InfoNCE": ([(69, "d7fe70cc969a59fa")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "k: ContrastiveTrainer, EBM_NCE": ([(69, "185e0aec4346a516")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "l: RRTrainer": ([(69, "08f9adab9f60e898")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "l: RRTrainer, ae_lr": ([(70, "92564d94a0c4c008")] + ["gather_molecules adam_step adam_step"] * 2, _BUCKET_STATS),
    "m: ChargePredictionTrainer, device masks": ([(63, "502e5351997d595e")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "m: ChargePredictionTrainer, numpy masks": ([(63, "502e5351997d595e")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "n: TorsionAnglePredictionTrainer": ([(60, "e9de7ee6eea163e6")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "o: InfoGraphTrainer": ([(63, "6d96f818e60bc278")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "p: LEPTrainer, sparse bucket": ([(67, "e02826ead4e0180f")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "p: LEPTrainer, per structure": ([
        (25, "5a26a038b3b1bf51"),
        (59, "7f5707a8199974dc"),
        "copy_n adam_step",
    ], {"captures": 1, "graphs": 1, "keys": STEP_KEYS}),
    "q: reference loop, do_InfoNCE": ([(69, "d7fe70cc969a59fa")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "q: reference loop, do_RR": ([(69, "08f9adab9f60e898")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "q: reference loop, do_DistancePrediction": ([(60, "4d7f8152fc7d501f")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
    "q: reference loop, do_ChargePrediction": ([(64, "a60ccbea4928091d")]
                                               + ["gather_molecules charge_mask_dyn adam_step"] * 2, _BUCKET_STATS),
    "q: reference loop, do_Supervised": ([(60, "6a243c08e880c2f7")] + [_GATHER_ADAM] * 2, _BUCKET_STATS),
}
