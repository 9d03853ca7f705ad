"""What every pretraining objective's step shares on the host: the descriptor BOTH owners of a ``replay.StepGraphs`` call
(``Objective``), the engine kept on the backbone module (``engine_for``: an ``autograd_step._AutogradStep``) with the
routing of the ``do_*`` functions to it (``run_graphed``), the backbone call (``backbone_latent`` /
``backbone_forward``) and the trainer base (``StepTrainer``).  The objective modules plug into this one; nothing here
knows an objective by name.
"""
import torch
import torch.nn as nn

from . import _lib
from .autograd_step import _AutogradStep
from .optim import FlatParams, FusedAdam
from .parallel import GradAllReduce
from .replay import StepGraphs, _OWN_CAPTURE, own_capture_open  # noqa: F401
from .switches import env as _env


class Args:
    """The fields do_DDM reads from the reference's argparse namespace, and what the reference passes beside it: the
    perturbation's (mu, sigma) and where a step draws (device_noise: on the GPU; else perturb's host draw)."""

    def __init__(self, model_3d="schnet", normalize=False, mu=0.0, sigma=0.3, device_noise=True):
        self.model_3d = model_3d
        self.normalize = normalize
        self.mu, self.sigma, self.device_noise = mu, sigma, device_noise


def stock_bce(criterion, or_none=False):
    """nn.BCEWithLogitsLoss() as the reference's scripts build it - mean, no weight, no pos_weight, not a subclass: what
    the fused BCE kernels (EBM-NCE, 3D InfoGraph, LEP) compute.  or_none: None stands for it too."""
    if criterion is None:
        return or_none
    return (type(criterion) is nn.BCEWithLogitsLoss and criterion.weight is None and criterion.pos_weight is None
            and criterion.reduction == "mean")


# ---- the objective, as both owners of its step graphs see it --------------------------------------------------------------
class Objective:
    """Everything that differs between objectives, stated ONCE for both owners of a ``replay.StepGraphs``: the engine of a
    caller that owns its optimizer (``autograd_step._AutogradStep``, behind the ``do_*`` functions) and the flat-buffer
    trainers (``StepTrainer``).  An instance is defined next to the objective's ``*_step_fused``.  The defaults are
    those of a step with one head, one view of the molecules and no per-step input beside the batch (Distance
    Prediction).

    ``owner``: whoever runs the step - anything with ``.model``, ``.n1``, ``.n2`` (backbone and up to two heads).
    ``args``: the objective's step-args object (``Args``, ``ContrastiveArgs``, ``RRArgs``, ``ChargeArgs``, a
    ``_StepArgs``): ``model_3d`` and whatever else the step reads - (mu, sigma, device_noise) of a step that draws.

    name            first entry of the default graph key
    views           views of the molecules the backbone sees in a capacity bucket (1 or 2)
    normalize       ``args.normalize`` keeps a batch off capacity buckets (DDM only: its row normalisation is over atoms)
    pair_tuples     the step reads the batch's pair tuples (``super_edge_index``); False (Supervised, LEP): a batch whose
                    layout is sparse - a structure above 255 atoms - may go through a sparse bucket (bucket.SPARSE), which
                    enumerates none
    head_params     head module -> the parameters the step reaches
    graph_key       args -> the key of the engine's StepGraphs (what a graph binds by value; fields it does not name
                    bind nothing)
    noise_keys      args -> names of the per-step static inputs of a graph (StepGraphs.noise_keys)
    forward         (owner, args, batch, noise) -> loss | (loss, extra static outputs); noise: the per-step inputs (a
                    graph's static ones, the caller's, or None: the step takes its own from the batch / draws them)
    capture_inputs  (owner, args, batch, noise) -> the tensors a first capture clones into its static inputs
    write_inputs    (owner, args, g, batch, noise): this step's inputs into the static inputs of graph ``g`` after
                    ``refresh``, before the replay (None: nothing).  A hook that draws asks ``draw_target`` where.
    result          (engine, out, g) -> what ``_AutogradStep.run`` returns
    """

    def __init__(self, name, forward, views=1, normalize=False, head_params=None, graph_key=None, noise_keys=None,
                 capture_inputs=None, write_inputs=None, result=None, pair_tuples=True):
        self.name, self.forward, self.views, self.normalize = name, forward, views, normalize
        self.pair_tuples = pair_tuples
        self.head_params = head_params or (lambda h: list(h.parameters()))
        self.graph_key = graph_key or (lambda args: (name, args.model_3d))
        self.noise_keys = noise_keys or (lambda args: ())
        self.capture_inputs = capture_inputs or (lambda owner, args, batch, noise: {})
        self.write_inputs = write_inputs
        self.result = result or (lambda engine, out, g: out)


def draw_target(owner, g, batch, noise):
    """Where a ``write_inputs`` hook puts this step's inputs -> (the batch that sizes a draw, the tensors to fill).  The
    one difference between the owners: the engine writes into the graph's static inputs at the real row counts of the
    caller's batch - its draws stay on torch's RNG stream, equal to the eager path's bit for bit - and so does whatever a
    caller gave; a trainer's OWN draws (``capacity_draws``, nothing given) are made on the graph's batch into the whole
    static inputs, so a bucket's draws cover its capacity."""
    if noise is None and owner.capacity_draws:
        return g["batch"], g["noise"]
    return batch, StepGraphs.noise_views(g)


def with_counts(engine, out, g):
    """``Objective.result`` of a step whose forward graph leaves accuracy counts beside the loss: read once the backward
    replay is queued, so the host waits for the forward only (the reference's own acc is a host value too)."""
    return out, g["extra"].tolist()


def engine_for(model, slot, objective, n1=None, n2=None):
    """The graph engine of (backbone, heads, objective), kept on the backbone module under ``slot``; rebuilt when a head
    is another object or a parameter was replaced, moved or frozen since (the graphs bind parameter addresses)."""
    eng = model.__dict__.get(slot)
    if eng is None or eng.n1 is not n1 or eng.n2 is not n2 or not eng.unchanged():
        eng = model.__dict__[slot] = _AutogradStep(model, n1, n2, objective=objective)
    return eng


def run_graphed(args, graph, model, slot, objective, step_args, batch, noise=None, n1=None, n2=None, prepare=None):
    """The routing every ``do_*`` shares, behind its own eligibility checks -> what the engine returns for this step
    (``objective.result``), or None: the caller runs its fused step as eager launches.
    args: the caller's namespace; graph: the ``graph=`` argument of the ``do_*`` - None: ``args.step_graph`` if present,
    else on unless GEOSSL_NO_STEP_GRAPH is set.  A step is replayed only when gradients are wanted and no capture of the
    caller's is open.  step_args: the objective's step-args object; ``args.step_graph_mode`` is handed over on it.
    prepare(engine): called before the run (Supervised keeps its (mean, std) tensor on the engine)."""
    if graph is None:
        graph = getattr(args, "step_graph", _env("GEOSSL_NO_STEP_GRAPH") is None)
    if not (graph and torch.is_grad_enabled() and not torch.cuda.is_current_stream_capturing()):
        return None
    step_args.step_graph_mode = getattr(args, "step_graph_mode", "auto")
    eng = engine_for(model, slot, objective, n1, n2)
    if prepare is not None:
        prepare(eng)
    return eng.run(step_args, batch, noise)


# ---- the backbone call ---------------------------------------------------------------------------------------------------
def latent(model, model_3d, x, positions, batch_vec, edges=None, **layouts):
    """The backbone's per-atom latent h [N, F]; the readout is dead compute in every step here and not evaluated.
    layouts: ``layout=`` / ``edge_layout=`` of a batch whose index structures the caller holds."""
    if model_3d == "schnet":
        return model(x, positions, batch_vec, return_latent=True, latent_only=True, **layouts)[1]
    if model_3d == "painn":
        return model(x, positions, edges, batch_vec, return_latent=True, latent_only=True, **layouts)[1]
    raise Exception("3D model {} not included.".format(model_3d))


def backbone_latent(model_3d, batch, model, x=None, what="", layout=False):
    """-> (h, layout, dyn) of a one-view step.  A plain batch: its own index tensors, ``get_layout(batch.batch)`` when
    ``layout`` is asked for, dyn None.  The static batch of a one-view capacity bucket (geossl_amd/bucket.py): tensors at
    the bucket's capacity, ``bucket.lay2`` (mol_ptr holds the B real offsets) and the real counts in ``bucket.dyn``.
    x: the atom types (default ``batch.x[:, 0]``); what: the step's name in the error of a bucket that is not its own."""
    if x is None:
        x = batch.x[:, 0]
    bucket = getattr(batch, "_bucket", None)
    if bucket is not None:
        if model_3d != bucket.kind or bucket.views != 1:
            raise _lib.GeosslHipError("the %s step needs a one-view bucket of its own backbone" % what)
        if bucket.kind == "schnet":
            h = latent(model, "schnet", x, batch.positions, bucket.b2, layout=bucket.lay2)
        else:
            h = latent(model, "painn", x, batch.positions, bucket.b2, bucket.e2, layout=bucket.lay2,
                       edge_layout=bucket.el)
        return h, bucket.lay2, bucket.dyn
    h = latent(model, model_3d, x, batch.positions, batch.batch, getattr(batch, "radius_edge_index", None))
    if layout:
        from .layout import get_layout
        return h, get_layout(batch.batch), None
    return h, None, None


def backbone_forward(args, batch, model, return_latent, x=None):
    """The three-way backbone branch of the reference's loops (``if args.model_3d == "schnet": ... elif "painn": ...
    else: raise``) with the readout evaluated: what the ATen restatements of the steps call.  return_latent False: the
    plain call of the reference (a stand-in backbone need not know the keyword)."""
    if x is None:
        x = batch.x[:, 0]
    kw = {"return_latent": True} if return_latent else {}
    if args.model_3d == "schnet":
        return model(x, batch.positions, batch.batch, **kw)
    elif args.model_3d == "painn":
        return model(x, batch.positions, batch.radius_edge_index, batch.batch, **kw)
    else:
        raise Exception("3D model {} not included.".format(args.model_3d))


# ---- the trainer ---------------------------------------------------------------------------------------------------------
class StepTrainer:
    """The body of a reference ``train()`` loop for one objective: forward, backward, gradient all-reduce, Adam - all
    parameters in one flat buffer (one fused Adam launch, one all-reduce), no host sync inside ``step``.
    ``use_graph=True``: forward + backward are captured into HIP graphs (StepGraphs) and replayed; the all-reduce and
    the Adam launch stay outside the graph.

    What the step computes and what a graph of it takes per step is the objective's ``Objective`` (forward,
    capture_inputs, write_inputs) with the trainer as the owner and ``args`` as the step-args object; a subclass overrides
    ``_forward`` / ``_capture_inputs`` / ``_write_inputs`` only where it differs from the engine of the ``do_*`` route."""

    with_extra = False      # a replayed step returns (loss, the graph's extra static outputs)
    capacity_draws = True   # a step's own draws cover the whole static inputs of its graph (draw_target)

    def __init__(self, modules, objective, args, lr, weight_decay, use_graph, max_graphs, graph_mode,
                 one_dtype=torch.float32):
        self.model, self.n1, self.n2 = (list(modules) + [None, None])[:3]
        self.objective, self.args = objective, args
        self.flat = FlatParams(modules)
        self.opt = FusedAdam(self.flat, lr=lr, weight_decay=weight_decay)
        self.reduce = GradAllReduce(self.flat.grad)
        self.use_graph = use_graph
        # graph_mode "auto": ragged batches share one capacity-bucket graph per batch size, equal-sized molecules one
        # graph per size, anything else one per structure from its second sighting on; "structure": one graph per
        # structure fingerprint, captured at first sight (StepGraphs).  An objective that reads no pair tuples
        # (Objective.pair_tuples False): its batches above 255 atoms per structure share a sparse bucket graph too
        self.step_graphs = StepGraphs(self._fwd_bwd, args.model_3d, max_graphs, mode=graph_mode,
                                      modules=(self.model, self.n1, self.n2), noise_keys=objective.noise_keys(args),
                                      views=objective.views, pair_tuples=objective.pair_tuples)
        self.step_graphs.zero_with_refresh = self.flat.grad
        self._one = torch.ones((), dtype=one_dtype, device=self.flat.grad.device)

    @property
    def lr(self):
        return self.opt.lr

    def set_lr(self, lr):
        """The learning rate of the following steps (an epoch-level scheduler: optim.cosine_annealing_lr)."""
        self.opt.lr = float(lr)

    def _forward(self, batch, noise):
        return self.objective.forward(self, self.args, batch, noise)

    def _backward(self, loss):
        with _lib.direct_grads():  # every p.grad is a view of self.flat.grad: kernels accumulate into it directly
            loss.backward(self._one)  # (a standing 1.0: backward() would fill a new one, a launch per step)
        self.flat.rebind_grads()
        return loss.detach()

    def _fwd_bwd(self, batch, noise=None):
        if not own_capture_open():
            self.flat.zero_grad()  # (a replayed step: cleared with the refresh of the graph's inputs, StepGraphs.refresh)
        out = self._forward(batch, noise)
        if isinstance(out, tuple):
            return (self._backward(out[0]),) + out[1:]
        return self._backward(out)

    def _eager(self, batch, noise=None):
        """The step as eager launches, as `step` returns it."""
        return self._fwd_bwd(batch, noise)

    def _capture_inputs(self, batch, noise):
        """The per-step inputs of a first capture, as tensors (the capture clones them)."""
        return self.objective.capture_inputs(self, self.args, batch, noise)

    def _write_inputs(self, g, batch, noise):
        """The per-step inputs into the graph's static inputs, after `refresh` and before the replay.  noise: the
        caller's, or what `_capture_inputs` gave for the capture that has just been made."""
        if self.objective.write_inputs is not None:
            self.objective.write_inputs(self, self.args, g, batch, noise)

    def _graph_fwd_bwd(self, batch, noise=None):
        sg = self.step_graphs
        g, capture = sg.plan(batch)
        if g is None and not capture:  # a structure only its own graph can serve, seen for the first time: eager
            return self._eager(batch, noise)
        if capture:
            noise = self._capture_inputs(batch, noise)
        g = sg.load(g, batch, noise, self._write_inputs)
        if g is None:  # (the bucket refused the batch's tensors: this step as eager launches)
            if not sg.enabled:  # capture failed: eager from now on
                self.use_graph = False
            return self._eager(batch, noise)
        g["graph"].replay()
        # (clones: the static outputs are overwritten by the next replay, and freed with their graph when that is dropped)
        if self.with_extra:
            return g["loss"].clone(), g["extra"].clone()
        return g["loss"].clone()

    def _finish(self, out):
        _lib.poll_status(self.model)
        scale = self.reduce()
        self.opt.step(grad_scale=scale)
        return out

    def step(self, batch, noise=None):
        """One training step -> what the objective's step returns, on the device.  noise: the step's draws, for an
        objective that has any.  A graph's static inputs take the caller's noise or the step's own device draws: a step
        that draws on the host (``args.device_noise`` off, nothing given) runs as eager launches."""
        if self.use_graph and (noise is not None or getattr(self.args, "device_noise", True)):
            return self._finish(self._graph_fwd_bwd(batch, noise))
        return self._finish(self._eager(batch, noise))
