"""The graph engine of a caller that owns its optimizer (the reference's loop: ``loss, acc = do_X(...);
optimizer.zero_grad(); loss.backward(); optimizer.step()``): forward and backward replayed from two HIP graphs
(``replay.StepGraphs``), the loss behind an autograd node.  An objective comes in as a ``step.Objective``.
"""
import torch

from . import _lib
from .optim import ParamHome
from .replay import StepGraphs, _restore_backward_threads, _single_thread_backward, own_capture_open
from .switches import env as _env


class _ReplayedLoss(torch.autograd.Function):
    """The loss of a replayed step as a differentiable function of the parameters: forward returns the loss the forward
    graph computed, backward waits for the backward graph (replayed on the engine's side stream right behind the forward)
    and hands autograd its gradients, scaled by the upstream gradient - one launch; every parameter's gradient is a view
    of the product."""

    @staticmethod
    def forward(ctx, loss, engine, ticket, *params):
        ctx.engine, ctx.ticket = engine, ticket
        return loss.view_as(loss)

    @staticmethod
    def backward(ctx, gout):
        eng, ticket = ctx.engine, ctx.ticket
        src = eng.collect(ticket)
        pre = ticket.pop("views", None)
        if pre is not None:
            # the step's own output buffer and its per-parameter views were made in do_DDM, while the host was going to
            # wait for the forward anyway; handing them out once keeps them stealable (AccumulateGrad adopts a gradient
            # nobody else references - the list dies with this frame)
            buf, outs = pre
            torch.mul(src, gout, out=buf)
            return (None, None, None) + tuple(outs)
        g = src * gout
        # one split for all parameters, then a reshape each (two tensor operations per parameter were a third of this
        # backward's host time at 59 parameters - and the host is what bounds the loop at small batches)
        outs = [v if len(shape) == 1 else v.view(shape) for v, (shape, _) in zip(g.split_with_sizes(eng.numels), eng.shapes)]
        return (None, None, None) + tuple(outs)


class _StepLoss(torch.Tensor):
    """The loss do_DDM's graph path hands to a caller that owns its optimizer - an ordinary tensor attached to the autograd
    graph (``_ReplayedLoss`` with every parameter as an input: ``torch.autograd.grad``, scaled losses, sums with other
    terms all differentiate through it as before) whose plain ``loss.backward()`` (pretrain_GeoSSL.py:259) does not go
    through the autograd engine: the step's gradients are already in the engine's buffer, so backward() copies them into
    the step's own buffer (one launch) and points every parameter's ``.grad`` at its view - what the 59 AccumulateGrad
    nodes of the engine path do one queue round trip each (0.34 ms per step on the host, which is what bounds the loop at
    the reference's batch size).  Anything else - a gradient argument, retain_graph, create_graph, inputs=, a parameter
    that already holds a gradient (accumulation over several backward() calls) or carries a tensor hook, an arithmetic
    result (ops on this class return plain tensors) - takes the engine.  GEOSSL_NO_DIRECT_BACKWARD: always the engine."""

    __torch_function__ = torch._C._disabled_torch_function_impl

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        st = self.__dict__.pop("_geossl_step", None)
        if (st is not None and gradient is None and not retain_graph and not create_graph and inputs is None
                and st[0].direct_backward(st[1])):
            return None
        return torch.Tensor.backward(self, gradient, retain_graph, create_graph, inputs)


class _Ticket(dict):
    """The claim of one do_DDM step on the gradients its backward replay leaves in the engine's buffer ("serial",
    "event", "g", "used").  The replay runs on a side stream and READS the parameters: when a loss is dropped without
    backward() (a skipped non-finite step followed by an EMA update, load_state_dict, another loss's optimizer step) the
    caller's stream is made to wait for the replay here, so that no later parameter write can overtake it."""

    def __del__(self):
        try:
            _restore_backward_threads(self)
        except Exception:
            pass
        try:
            if (not self.get("used") and self.get("event") is not None and not torch.cuda.is_current_stream_capturing()
                    and not self["event"].query()):
                torch.cuda.current_stream().wait_event(self["event"])
        except Exception:  # interpreter shutdown, a destroyed context: nothing left to order
            pass


def _schnet_step_params(model):
    from .Geom3D.models.schnet import _core_params
    return _core_params(model)


class _AutogradStep:
    """do_DDM's graph path for a caller that owns its optimizer (the reference loop, pretrain_GeoSSL.py:249-260).

    Forward and backward of the step are captured as TWO graphs per index structure (one memory pool, one capture
    stream).  ``run`` draws the step's noise like the eager path (same generators, same order), refreshes the graph
    inputs, replays the forward on the caller's stream and the backward on a side stream right behind it, and returns
    the loss behind ``_ReplayedLoss``.  The reference's ``loss.detach().item()`` (:255) therefore waits for the forward
    only; ``optimizer.zero_grad()``, ``loss.backward()`` (one wait + one multiply; AccumulateGrad adopts the views) and
    the launches of ``optimizer.step()`` are issued by the host WHILE the backward graph runs.  The backward's gradients
    land in a flat static buffer (the parameters' .grad point into it only while a step is captured); a step whose
    backward() has not been called when the next step arrives keeps a snapshot of them."""

    capacity_draws = False   # draws land at the caller's real row counts: torch's RNG stream, as eager (step.draw_target)

    def __init__(self, model, n1, n2, objective):
        self.model, self.n1, self.n2 = model, n1, n2
        # the step.Objective of this engine says everything that differs between objectives: the heads'
        # parameters, the graphs' key and per-step static inputs, the forward, and what `run` returns.  The heads are
        # the objective's own: two NCSN heads (DDM), none (n1 = n2 = None: the contrastive steps), or one (n1).
        self.objective = objective
        heads = [m for m in (n1, n2) if m is not None]
        # the parameters the step reaches (a parameter outside it - an atomref table, PaiNN's output layers - gets no
        # gradient at all, like in the eager path, not a zero one)
        backbone = model._params() if hasattr(model, "_params") else _schnet_step_params(model)
        seen, self.params = set(), []
        for p in list(backbone) + [q for h in heads for q in objective.head_params(h)]:
            if id(p) not in seen and p.requires_grad:
                seen.add(id(p))
                self.params.append(p)
        dev = self.params[0].device
        # the parameters move into ONE flat buffer (values unchanged; they stay ordinary leaves): the gradients this
        # engine hands to autograd are views of one flat buffer at the same offsets, which lets a stock torch.optim.Adam
        # over these parameters run as one launch (optim.ParamHome and its step hook)
        self.home = ParamHome.of(self.params)
        self.gflat = torch.zeros(sum(p.numel() for p in self.params), dtype=torch.float32, device=dev)
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self.views, off = [], 0
        for p in self.params:
            self.views.append(self.gflat[off:off + p.numel()].view_as(p))
            off += p.numel()
        self.shapes = tuple((tuple(p.shape), p.numel()) for p in self.params)
        self.numels = [n for _, n in self.shapes]
        # where every parameter of the three modules hangs (submodule, name) with its object, address and grad flag:
        # `unchanged()` compares them per call without walking the module trees
        self._where = []
        for m in [self.model] + heads:
            seen_mod = set()
            for sub in m.modules():
                if id(sub) in seen_mod:
                    continue
                seen_mod.add(id(sub))
                for name, p in sub._parameters.items():
                    if p is not None:
                        self._where.append((sub._parameters, name, p, p.data_ptr(), p.requires_grad))
        self.graphs = {}   # objective.graph_key(args) -> StepGraphs
        self._cfg = None
        # static outputs of the graph `run` just replayed, for an objective whose `result` leaves them here (the caller
        # takes them at once and clears this)
        self.extra = None
        self._side = torch.cuda.Stream(device=dev)   # the backward graphs replay here
        self._bwd_done = None                        # event behind the last backward replay
        self._ticket = None                          # the step whose gradients are in gflat: {"serial", "event", "g"}
        self._serial = 0

    def unchanged(self):
        """No parameter of the three modules was replaced, moved or (un)frozen since the engine was built (its graphs bind
        the parameters' addresses)."""
        for d, name, p, addr, rg in self._where:
            if d.get(name) is not p or p.data_ptr() != addr or p.requires_grad != rg:
                return False
        return True

    # The engine hangs on the backbone module (model.__dict__) and holds graphs, streams and events: a copy or a pickle
    # of the model (copy.deepcopy for an EMA twin, torch.save(model)) carries None instead and builds its own on first use.
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())

    def _fwd(self, batch, noise):
        return self.objective.forward(self, self._cfg, batch, noise)

    def _bwd(self, loss):
        held = [p.grad for p in self.params]
        # tensor hooks of the caller (gradient clipping, logging, reducers) belong to ITS backward, which runs later on
        # the node `run` returns; the passes in here are internal - and in direct mode the nodes hand autograd no
        # gradients at all, so a hook would be called with None
        hooks = []
        for p in self.params:
            h = getattr(p, "_backward_hooks", None)
            if h:
                hooks.append((h, list(h.items())))
                h.clear()
        if not own_capture_open():
            self.gflat.zero_()  # (a replayed step: cleared by the launch that refreshes the graph's inputs, StepGraphs.refresh)
        for p, v in zip(self.params, self.views):
            p.grad = v
        try:
            with _lib.direct_grads():  # kernels accumulate straight into the static buffer
                loss.backward(self._one)  # (a standing 1.0: backward() would fill a new one, a launch per step)
            for p, v in zip(self.params, self.views):  # anything autograd replaced goes back into the buffer
                if p.grad is not None and p.grad.data_ptr() != v.data_ptr():
                    v.copy_(p.grad)
        finally:
            for p, h in zip(self.params, held):
                p.grad = h
            for h, items in hooks:
                h.update(items)

    def _fwd_bwd(self, batch, noise):
        loss = self._fwd(batch, noise)
        if isinstance(loss, tuple):
            self._bwd(loss[0])
            return loss[0].detach(), loss[1]
        self._bwd(loss)
        return loss.detach()

    def collect(self, ticket):
        """The gradients of the step `ticket` stands for (unscaled, read-only): the snapshot taken when a later step was
        about to overwrite them, else the static buffer itself once its backward replay is complete."""
        if ticket["g"] is not None:
            return ticket["g"]
        if ticket["serial"] != self._serial:
            raise RuntimeError("the gradients of this do_DDM step are gone (a later step replaced them after this step's "
                               "backward had already run once); call backward(retain_graph=...) before the next do_DDM")
        torch.cuda.current_stream().wait_event(ticket["event"])
        ticket["used"] = True
        return self.gflat

    def direct_backward(self, ticket):
        """loss.backward() of the step `ticket` stands for without the autograd engine (_StepLoss): True when done."""
        if _env("GEOSSL_NO_DIRECT_BACKWARD") or ticket.get("used") or "views" not in ticket:
            return False
        # hooks on the parameters' AccumulateGrad NODES (DistributedDataParallel's reducer) cannot be seen from here: with
        # more than one rank initialised the engine runs, whoever reduces the gradients
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return False
        for p in self.params:
            # (an existing gradient: accumulate like AccumulateGrad would; a tensor hook: call it like the engine would)
            if p.grad is not None or p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
                return False
        src = self.collect(ticket)   # (the caller's stream waits for the backward replay)
        buf, outs = ticket.pop("views")
        buf.copy_(src)               # d loss / d loss = 1: the engine path multiplies by it, same values
        for p, v in zip(self.params, outs):
            p.grad = v
        return True

    def run(self, args, batch, noise=None):
        """-> `objective.result` of the replayed step (the loss, or the loss and more), or None: run this step eagerly.
        args: the objective's step-args object; noise: the caller's per-step inputs, if any."""
        if getattr(batch, "_dataset", None) is None and (not batch.positions.is_cuda or batch.positions.requires_grad):
            return None
        obj = self.objective
        key = obj.graph_key(args)   # (whatever a graph binds by value is part of it)
        sg = self.graphs.get(key)
        if sg is None:
            sg = self.graphs[key] = StepGraphs(self._fwd_bwd, args.model_3d, split=(self._fwd, self._bwd),
                                               mode=getattr(args, "step_graph_mode", "auto"),
                                               normalize=obj.normalize and bool(getattr(args, "normalize", False)),
                                               modules=(self.model, self.n1, self.n2),
                                               noise_keys=obj.noise_keys(args), views=obj.views,
                                               pair_tuples=obj.pair_tuples)
            sg.zero_with_refresh = self.gflat
        if not sg.enabled:
            return None
        self._cfg = args
        g, capture = sg.plan(batch)
        if g is None and not capture:
            return None
        main = torch.cuda.current_stream()
        if self._bwd_done is not None:
            # the last backward replay reads the activations and writes the gradient buffer this step is about to reuse
            main.wait_event(self._bwd_done)
            t = self._ticket
            if t is not None and t["g"] is None and not t.get("used"):
                t["g"] = self.gflat.clone()  # a step still waiting for its backward() keeps its gradients
        if capture:   # (a failed capture has cleared sg.enabled: eager from now on)
            drawn = obj.capture_inputs(self, args, batch, noise)
            g = sg.load(None, batch, drawn, lambda g, _, drawn: sg.copy_noise(g, drawn))
        elif obj.write_inputs is None:
            g = sg.load(g, batch)
        else:
            g = sg.load(g, batch, write=lambda g, *_: obj.write_inputs(self, args, g, batch, noise))
        if g is None:
            return None  # (no graph, or the bucket refused the batch's tensors: this step as eager launches)
        g["graph"].replay()            # forward: the loss is on the device when this is done
        loss = g["loss"].clone()
        fwd_done = torch.cuda.Event()
        fwd_done.record(main)
        self._side.wait_event(fwd_done)
        with torch.cuda.stream(self._side):  # backward: behind the forward, beside whatever the host queues next
            g["graph_bwd"].replay()
            self._bwd_done = torch.cuda.Event()
            self._bwd_done.record(self._side)
        self._serial += 1
        prev = self._ticket
        if prev is not None:
            _restore_backward_threads(prev)  # (a loss that never saw its backward(): its switch goes back first)
        self._ticket = _Ticket(serial=self._serial, event=self._bwd_done, g=None)
        _single_thread_backward(self._ticket)
        buf = torch.empty_like(self.gflat)   # this step's (scaled) gradients as autograd will receive them
        # (a one-dimensional parameter's piece of the split already has its shape: no view for the biases - half the list)
        self._ticket["views"] = (buf, [v if len(shape) == 1 else v.view(shape)
                                       for v, (shape, _) in zip(buf.split_with_sizes(self.numels), self.shapes)])
        _lib.poll_status(self.model)   # (like StepTrainer._finish)
        out = _ReplayedLoss.apply(loss, self, self._ticket, *self.params).as_subclass(_StepLoss)
        out._geossl_step = (self, self._ticket)
        return obj.result(self, out, g)
