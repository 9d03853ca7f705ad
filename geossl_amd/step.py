"""What every pretraining objective's step shares on the host: the descriptor the graph engine calls (``Objective``),
the engine kept on the backbone module (``engine_for``: an ``autograd_step._AutogradStep``), the backbone call
(``backbone_latent`` / ``backbone_forward``) and the trainer base (``StepTrainer``, on ``replay.StepGraphs``).  The
objective modules plug into this one; nothing here knows an objective by name.
"""
import torch

from . import _lib
from .autograd_step import _AutogradStep
from .optim import FlatParams, FusedAdam
from .parallel import GradAllReduce
from .replay import StepGraphs, _OWN_CAPTURE, own_capture_open  # noqa: F401


class Args:
    """The three fields do_DDM reads from the reference's argparse namespace."""

    def __init__(self, model_3d="schnet", normalize=False):
        self.model_3d = model_3d
        self.normalize = normalize


# ---- the objective, as the graph engine sees it --------------------------------------------------------------------------
def _no_inputs(engine, args, batch, mu, sigma, noise, device_noise):
    return {}


class Objective:
    """Everything ``autograd_step._AutogradStep`` needs to know about ONE objective; an instance is defined next to
    the objective's ``*_step_fused`` and passed to the engine.  The defaults are those of a step with one head, one view
    of the molecules and no per-step input beside the batch (Distance Prediction).

    name            first entry of the default graph key
    views           views of the molecules the backbone sees in a capacity bucket (1 or 2)
    normalize       ``args.normalize`` keeps a batch off capacity buckets (DDM only: its row normalisation is over atoms)
    pair_tuples     the step reads the batch's pair tuples (``super_edge_index``); False (Supervised, LEP): a batch whose
                    layout is sparse - a structure above 255 atoms - may go through a sparse bucket (bucket.SPARSE), which
                    enumerates none
    head_params     head module -> the parameters the step reaches
    graph_key       args -> the key of the engine's StepGraphs (what a graph binds by value)
    noise_keys      args -> names of the per-step static inputs of a graph (StepGraphs.noise_keys)
    step_args       args -> what ``forward`` is given as its args
    forward         (engine, step_args, mu, sigma, batch, noise) -> loss | (loss, extra static outputs)
    capture_inputs  (engine, args, batch, mu, sigma, noise, device_noise) -> the tensors a first capture clones
    write_inputs    (engine, args, sg, g, batch, mu, sigma, noise, device_noise): what a replay writes into the graph's
                    static inputs after ``refresh`` (None: nothing)
    result          (engine, out, g) -> what ``run`` returns
    """

    def __init__(self, name, forward, views=1, normalize=False, head_params=None, graph_key=None, noise_keys=None,
                 step_args=None, capture_inputs=_no_inputs, write_inputs=None, result=None, pair_tuples=True):
        self.name, self.forward, self.views, self.normalize = name, forward, views, normalize
        self.pair_tuples = pair_tuples
        self.head_params = head_params or (lambda h: list(h.parameters()))
        self.graph_key = graph_key or (lambda args: (name, args.model_3d))
        self.noise_keys = noise_keys or (lambda args: ())
        self.step_args = step_args or (lambda args: args)
        self.capture_inputs, self.write_inputs = capture_inputs, write_inputs
        self.result = result or (lambda engine, out, g: out)


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

    A subclass gives ``_forward(batch, noise) -> loss | (loss, extra)`` and, where its step has per-step inputs beside
    the batch, ``_capture_inputs`` and ``_write_inputs``."""

    with_extra = False   # a replayed step returns (loss, the graph's extra static outputs)

    def __init__(self, modules, model_3d, lr, weight_decay, use_graph, max_graphs, graph_mode, noise_keys=(), views=1,
                 one_dtype=torch.float32, pair_tuples=True):
        self.model = modules[0]
        self.flat = FlatParams(modules)
        self.opt = FusedAdam(self.flat, lr=lr, weight_decay=weight_decay)
        self.reduce = GradAllReduce(self.flat.grad)
        self.use_graph = use_graph
        # graph_mode "auto": ragged batches share one capacity-bucket graph per batch size, equal-sized molecules one
        # graph per size, anything else one per structure from its second sighting on; "structure": one graph per
        # structure fingerprint, captured at first sight (StepGraphs).  pair_tuples=False: the step reads no pair tuples
        # (Objective.pair_tuples) - its batches above 255 atoms per structure share a sparse bucket graph too
        self.step_graphs = StepGraphs(self._fwd_bwd, model_3d, max_graphs, mode=graph_mode,
                                      modules=tuple((list(modules) + [None, None])[:3]), noise_keys=noise_keys,
                                      views=views, pair_tuples=pair_tuples)
        self.step_graphs.zero_with_refresh = self.flat.grad
        self._one = torch.ones((), dtype=one_dtype, device=self.flat.grad.device)

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
        return {}

    def _write_inputs(self, g, batch, noise):
        """The per-step inputs into the graph's static inputs, after `refresh` and before the replay.  noise: the
        caller's, or what `_capture_inputs` gave for the capture that has just been made."""

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

    def step(self, batch):
        """One training step -> what the objective's step returns, on the device."""
        return self._finish(self._graph_fwd_bwd(batch) if self.use_graph else self._eager(batch))
