"""Evaluation passes (``eval()`` of examples/finetune_qm9.py :278-384, finetune_lba.py :68-101, finetune_lep.py :66-101)
replayed from forward-only HIP graphs, with the metrics' sums kept on the device.

``Evaluator(model, head, model_3d, kind)`` owns a ``replay.StepGraphs`` whose owner function is the forward alone, under
``torch.no_grad()``: the backbone's latent and ``ops.property_predict`` (kind "property": Supervised / QM9 / LBA) or
``ops.pair_predict`` on the one-pass batch of 2B structures (kind "pair": LEP).  The routing is the training step's own
(``bucket.route``): one dense one-view bucket graph per batch size for ragged structures of at most 255 atoms, the sparse
bucket for pockets and LEP's 2B structures under GEOSSL_SPARSE_BUCKETS / GEOSSL_PAINN_SPARSE_BUCKETS, per-structure graphs
from the second sighting otherwise, eager launches for the rest.  The graph's static output is the prediction vector
(what StepGraphs calls ``loss``); its static input ``target`` is written per batch by the training step's own
``write_targets`` / ``write_labels``.  A graph reads the parameters' live values and the (mean, std) tensor: training
between two evaluations, or new statistics, need no recapture.

``run(loader)`` makes, per served batch, the gather / fill, the target launch, the replay and ONE ``ops.eval_collect``
launch (csrc/eval_collect.hip), which adds the batch's error sums onto an accumulator and writes its rows into the
loader-long result arrays; nothing is read back inside the loop.  A batch the fused head refuses (CPU tensors, an unserved
width or head, B = 1, a collated batch without host sizes) gets whatever ``predict_Supervised`` / ``predict_LBA`` /
``predict_LEP`` does for it today - the ``eager`` callable of the caller - and its result is collected in loader order by
the same launch.
"""
import torch

from . import _lib, ops
from . import finetune_lep as lep
from . import pretrain_Supervised as sup
from .replay import StepGraphs, parameter_addresses
from .step import backbone_latent

__all__ = ["Evaluator", "evaluator_for"]

KINDS = {"property": "regression", "pair": "bce"}
# use_graph of the entry points that are new with this module, by head kind ("property": eval_Supervised and
# SupervisedTrainer.evaluate; "pair": LEPTrainer.evaluate): decided by tools/bench_eval.py (profiles/eval_bench.json,
# DESIGN 5) - on where the replay beat the eager loop beyond the runs' spread at both measured batch sizes.  Measured:
# the slowest replayed pass was faster than the fastest eager one on every shape (1.7 - 3.3 x on QM9-sized molecules,
# 1.1 - 1.7 x on LEP's pairs), SchNet and PaiNN
USE_GRAPH_DEFAULT = {"property": True, "pair": True}


class Evaluator:
    """The forward-only graphs of (backbone, head) and the evaluation loop on them.  kind "property": the head of
    ``pretrain_Supervised.head_params`` and a target column (``task_id``) de-normalised by ``stats`` (a
    ``pretrain_Supervised._Stats``; its own (0, 1) when none is given); kind "pair": LEP's ``Linear(2F, 1)`` on pair
    batches.  ``captures`` counts captures.  Not copied or pickled with the backbone it is kept on."""

    def __init__(self, model, head, model_3d, kind, task_id=0, max_graphs=64, graph_mode="auto", stats=None):
        if kind not in KINDS:
            raise ValueError("kind is 'property' or 'pair', got %r" % (kind,))
        if model_3d not in ("schnet", "painn"):
            raise Exception("3D model {} not included.".format(model_3d))
        self.model, self.head, self.model_3d, self.kind, self.task_id = model, head, model_3d, kind, int(task_id)
        self.device = next(model.parameters()).device
        self.stats, self.own_stats = stats, stats is None
        if stats is None and kind == "property" and self.device.type == "cuda":
            self.stats = sup._Stats(self.device)
            self.stats.set(0.0, 1.0)
        self.graphs = StepGraphs(self._forward, model_3d, max_graphs, mode=graph_mode, modules=(model, head, None),
                                 noise_keys=("target",), views=1, pair_tuples=False)
        self.enabled = True
        self.bound = parameter_addresses(model, head)

    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())

    @property
    def captures(self):
        return self.graphs.captures

    def unchanged(self):
        return self.bound == parameter_addresses(self.model, self.head)

    # ---- the forward a graph holds
    @torch.no_grad()
    def _forward(self, sb, sn=None):
        if self.kind == "property":
            h, lay, dyn = backbone_latent(self.model_3d, sb, self.model, x=sup._x_of(self, sb), what="evaluation",
                                          layout=True)
            return ops.property_predict(h, sup.head_params(self.head), lay, sup.readout_of(self.model), self.stats.t,
                                        dyn=dyn)
        h, lay, dyn = backbone_latent(self.model_3d, sb, self.model, x=lep._x_of(self.model_3d, sb), what="evaluation",
                                      layout=True)
        w, b = lep.head_params(self.head)
        return ops.pair_predict(h, w, b, lay, sup.readout_of(self.model), dyn=dyn)

    # ---- what is served
    def modules_served(self):
        """Backbone and head run on the fused head of this kind (looked at once per pass)."""
        if self.kind == "pair":
            return lep.modules_ok(self.model, self.head)
        ps = sup.head_params(self.head)
        return ps is not None and sup.readout_of(self.model) is not None and sup.model_width(self.model) == ps[0].size(1)

    def batch_served(self, batch):
        """The batch goes through a graph (or the fused eager launches of a first sighting): a DeviceLoader handle with
        targets, or a collated CUDA batch with host sizes, of at least two structures / pairs."""
        if torch.cuda.is_current_stream_capturing():
            return False
        if self.kind == "pair":
            lep._check_handle(batch, self.model_3d)
            if not lep._fused_batch_ok(batch):
                return False
            return lep._is_handle(batch) or (getattr(batch, "_sizes_active", None) is not None
                                             and getattr(batch, "_sizes_inactive", None) is not None)
        if int(batch.num_graphs) < 2 or not sup._fused_batch_ok(batch, self.task_id):
            return False
        return getattr(batch, "_sizes", None) is not None

    def _one_pass(self, batch):
        return lep.fused_batch(batch) if self.kind == "pair" else batch

    def _capture_inputs(self, fb):
        return {"target": fb.y if self.kind == "pair" else sup.target_column(fb, self.task_id)}

    def _write(self, g, fb, inputs):
        if self.kind == "pair":
            lep.write_labels(g, fb)
        else:
            sup.write_targets(g, fb, self.task_id)

    def replay(self, batch):
        """The batch through its graph -> the graph's entry (``loss``: the static predictions, ``noise["target"]``: the
        static targets, both valid until the next replay), or None: no graph serves it now (a structure only its own
        graph can serve at its first sighting, a refused fill, a failed capture) - the caller launches eagerly."""
        if not self.enabled:
            return None
        fb = self._one_pass(batch)
        sg = self.graphs
        g, capture = sg.plan(fb)
        if g is None and not capture:
            return None
        g = sg.load(g, fb, self._capture_inputs(fb) if capture else None, self._write)
        if g is None:
            if not sg.enabled:
                self.enabled = False
            return None
        g["graph"].replay()
        _lib.poll_status(self.model)
        return g

    def predict(self, batch, eager=None):
        """The predictions of one batch: a clone of its graph's static output, or the eager result - the same forward
        as eager launches where no graph serves the batch now, ``eager(batch)`` for a batch the fused head refuses."""
        if self.modules_served() and self.batch_served(batch):
            g = self.replay(batch)
            return g["loss"].clone() if g is not None else self._forward(self._one_pass(batch))
        return self._refused(eager)(batch)

    @staticmethod
    def _refused(eager):
        if eager is None:
            raise ValueError("the fused head does not serve this batch and no eager route was given (eager=: the "
                             "predict_* call of the caller)")
        return eager

    # ---- the loop
    def run(self, loader, arrays=True, eager=None):
        """One pass over `loader` -> (sum a, sum s, rows, y_true, y_pred): the fp64 sums of csrc/eval_collect.hip over all
        rows (property: a = |pred - y|, s = (pred - y)^2 on the de-normalised predictions; pair: a = the BCE-with-logits
        term, s = 0), the row count, and - with ``arrays`` - the targets and predictions as float32 numpy arrays in loader
        order (else None, None).  eager(batch) -> the predictions of a batch the fused head refuses (``predict_*`` of the
        caller).  Batches are moved to the backbone's device.  One read of the accumulator and one of each array, behind
        the loop."""
        dev = self.device
        acc = ops.eval_buffer(dev)
        kind = KINDS[self.kind]
        try:
            M = len(loader.dataset)
        except (AttributeError, TypeError):
            M = 0
        out = None
        if arrays:
            out = [torch.empty(max(int(M), 64), dtype=torch.float32, device=dev) for _ in range(2)]
        served, offset = self.modules_served(), 0
        for batch in loader:
            if hasattr(batch, "to"):
                batch = batch.to(dev)
            fused = served and self.batch_served(batch)
            g = self.replay(batch) if fused else None
            if g is not None:
                pred = g["loss"]
                target = g["noise"]["target"][:pred.numel()]   # (a pair bucket's has a row per structure: B lead)
            else:
                # no graph serves it now: the same forward as eager launches; a refused batch: the caller's lines
                pred = (self._forward(self._one_pass(batch)) if fused
                        else self._refused(eager)(batch).detach().reshape(-1))
                y = batch.y
                target = (y.float() if self.kind == "pair" else sup.target_column(batch, self.task_id)).reshape(-1)
                if pred.dtype != torch.float32:
                    pred = pred.float()
                target = target.to(torch.float32).contiguous()
            B = pred.numel()
            if out is not None and offset + B > out[0].numel():   # (a loader without a length: doubled on the device)
                grown = [torch.empty(max(2 * o.numel(), offset + B), dtype=torch.float32, device=dev) for o in out]
                for n_, o in zip(grown, out):
                    n_[:offset].copy_(o[:offset])
                out = grown
            ops.eval_collect(pred, target, kind, offset, None if out is None else out[1], None if out is None else out[0],
                             acc)
            offset += B
        sum_a, sum_s, rows = ops.eval_read(acc)
        if out is None:
            return sum_a, sum_s, rows, None, None
        return sum_a, sum_s, rows, out[0][:offset].cpu().numpy(), out[1][:offset].cpu().numpy()


def evaluator_for(model, head, model_3d, kind, task_id=0, stats=None, max_graphs=64, graph_mode="auto"):
    """The evaluator of (backbone, head), kept on the backbone module; rebuilt when the head is another object, a
    parameter was replaced or moved since (the graphs bind parameter addresses), or it was made for another kind,
    backbone call or (mean, std) tensor.  The task column is data of a replay: it is set, not bound."""
    ev = model.__dict__.get("_geossl_evaluator")
    if (ev is None or ev.head is not head or ev.model_3d != model_3d or ev.kind != kind or not ev.unchanged()
            or (ev.stats is not stats if stats is not None else not ev.own_stats) or ev.graphs.mode != graph_mode):
        ev = model.__dict__["_geossl_evaluator"] = Evaluator(model, head, model_3d, kind, task_id, max_graphs, graph_mode,
                                                            stats)
    ev.task_id = int(task_id)
    return ev
